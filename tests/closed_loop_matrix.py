"""The closed-loop test matrix, stated once: which envs every closed-loop kernel family is compiled for, what kernel shape
each env brings, distinct start states for the two envs whose reset gives every lane the same state, and the network in NumPy
float64.  A plain helper module (no fixtures, no collection hooks): the family modules (test_gpu_ensemble.py,
test_gpu_safe_action_search.py, test_gpu_safety_gate.py, test_gpu_disturbance.py, test_gpu_safety_shield.py, test_gpu_projection.py,
test_gpu_mlp_bf16.py and the MFMA-actor test of test_gpu_parity.py) take their env lists from here, and test_closed_loop_matrix.py
holds the lists to the library's own registry and to what each entry point accepts.

The MFMA families (rollout_mlp, _safe, _ensemble, _disturbed, _search, _gated, _projected and the bf16 actor's rollout_mlp_bf16) exist
for the envs with an even state dim and at most 16 actions; rollout_policy_disturbed exists for all nine."""
import numpy as np

# (key, env id): head instruction and rows in use; critic layer-1 input width S + A, its chunks of four 4-wide k-tiles, parity
MFMA_ENVS = [
    ("cr", "ChemicalReactor-v0"),            # S 12, A 3: 4x4x1 head, 3 rows; critic width 15 (odd: a zero-padded k-step), one chunk
    ("pg", "PowerGrid-v0"),                  # S 32, A 8: 16x16x1 head, 8 rows (source lane groups 0 and 1); width 40, two chunks, 21 records
    ("ra", "RobotAssembly-v0"),              # S 24, A 7: 16x16x1 head, 7 rows; width 31 (odd), two chunks
    ("acr", "AdvancedChemicalReactor-v0"),   # S 20, A 6: 16x16x1 head, 6 rows; width 26 (even), one chunk; no draws: cloned lanes
    ("apg", "AdvancedPowerGrid-v0"),         # S 32, A 8: PowerGrid's shapes; no draws: cloned lanes; a[4], a[5] < 0.95 ends the episode
    ("hvac", "HVACControl-v0"),              # S 18, A 5: 16x16x1 head, 5 rows; width 23 (odd), one chunk
    ("steel", "SteelAnnealing-v0"),          # S 20, A 6: 16x16x1 head, 6 rows (two of lane group 1); width 26 (even), one chunk, no zero-padded k-step
    ("supply", "SupplyChain-v0"),            # S 28, A 10: 16x16x1 head, 10 rows: rows 8 and 9 come from source lane group 2 (r >> 2 == 2;
]                                            # no other env); width 38 (even), two chunks, 20 records, no padding record
# WaterTreatment-v0: S 15 (odd), A 4: no MFMA actor; the policy kernels only
POLICY_ENVS_ALL = MFMA_ENVS[:5] + [MFMA_ENVS[5], ("water", "WaterTreatment-v0")] + MFMA_ENVS[6:]      # the registry's order
NAMES = dict(POLICY_ENVS_ALL)
KEY_OF = {name: key for key, name in POLICY_ENVS_ALL}

# AdvancedChemicalReactor and AdvancedPowerGrid draw nothing (k_step == k_reset == 0): reset() gives every lane one state, and
# identical lanes stay identical.  A test of these two that starts from reset() compares clones -- a head read from the wrong
# source lane or a row stored to the wrong lane passes it.  Their cases start from start_states() instead.
CLONED = ("acr", "apg")

# Shapes of the cases the matrix adds: five full 128-env blocks and a partial one (two full 256-lane policy blocks and a
# partial one) and one partial wave; episodes of at most 5 steps end inside a launch of 7
B_BIG, B_SMALL, T_NEW, MAXS_NEW = 700, 5, 7, 5
# The oracle restates the device's summation order, so a routing error shared by the stream builder and the oracle passes bit
# equality.  The shapes only the matrix's cases reach are therefore also held to the network in NumPy float64 on step 0:
FLOAT64_KEYS = ("acr", "apg", "steel", "supply")
ACT_ATOL = 5e-6       # actions against a float64 network: test_gpu_parity.py's bar for the MFMA actor
PROB_ATOL = 1e-5       # critic probabilities against a float64 network: test_gpu_safety_shield.py's bar

_STARTS = {}


def start_states(ni, name, B, seed):
    """[B, S] float32: per-lane distinct, valid states for an env whose reset is the same for all lanes -- the states of a probe
    handle (no auto-reset) after reset() and one step on the bench workload's uniform actions of launch counter 1.  Lane i's row
    depends on i and the seed alone, so a smaller batch gets the first rows of a larger one.  At least 6 of 7 rows are distinct
    (AdvancedChemicalReactor clips half of some action ranges away: 622 distinct rows of 700; AdvancedPowerGrid: 700)."""
    import torch
    ck = (name, B, seed)
    if ck not in _STARTS:
        probe = ni.make_batched(name, B, autoreset=False, seed=seed)
        probe.reset()
        probe.step(probe.fill_actions(1)[:, :B], layout="soa")        # (fill_actions gives [A, ld]: the first B columns)
        torch.cuda.synchronize()
        s = probe.get_state().cpu().numpy().copy()
        probe.close()
        assert s.shape[0] == B and np.isfinite(s).all()
        distinct = len(np.unique(s, axis=0))
        assert distinct >= (6 * B) // 7, (name, B, distinct)
        assert B < 100 or (s.std(axis=0) > 0).sum() >= s.shape[1] // 2, "most state columns vary over the lanes"
        s.setflags(write=False)
        _STARTS[ck] = s
    return _STARTS[ck]


def install_start(ni, env, key, seed):
    """After env.reset(): give the lanes of a CLONED env their distinct start states (episode step 0, no violations, not done).
    Every other env keeps its reset states, which its own draws already spread."""
    if key in CLONED:
        env.set_state(np.array(start_states(ni, NAMES[key], env.batch, seed)), current_step=0, violation_count=0, done=False)


def random_actor(S, A, seed):
    """A random S -> 256 -> 256 -> A actor (the construction the family modules share)."""
    rng, f = np.random.default_rng(seed), np.float32
    return [(rng.normal(0, 1.0 / np.sqrt(S), (S, 256)).astype(f) * f(0.05), rng.normal(0, 0.05, 256).astype(f)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(f), rng.normal(0, 0.05, 256).astype(f)),
            (rng.normal(0, 1.0 / 8, (256, A)).astype(f), rng.normal(0, 0.1, A).astype(f))]


def random_critic(S, A, seed, n_out=1):
    """A random (S + A) -> 256 -> 256 -> n_out critic or safety-ensemble member."""
    rng, f, D = np.random.default_rng(seed), np.float32, S + A
    return [(rng.normal(0, 1.0 / np.sqrt(D), (D, 256)).astype(f) * f(0.05), rng.normal(0, 0.05, 256).astype(f)),
            (rng.normal(0, 1.0 / 16, (256, 256)).astype(f), rng.normal(0, 0.05, 256).astype(f)),
            (rng.normal(0, 1.0 / 2, (256, n_out)).astype(f), rng.normal(0, 0.1, n_out).astype(f))]


def continuing(key, ws):
    """The actor a matrix case installs.  An AdvancedPowerGrid episode ends whenever a voltage set-point action (a[4], a[5]) is
    below 0.95, which a random tanh head's output always is: every lane would finish on step 0, reset to the one reset state,
    and the later steps would compare clones.  Head biases of 5 for those two rows (the random part of their pre-activation is
    of order 1: tanh > 0.99) keep the actor's own episodes going; every other env keeps the weights it was given."""
    if key != "apg":
        return ws
    b3 = np.array(ws[2][1], dtype=np.float32)
    b3[4:6] = 5.0
    return [ws[0], ws[1], (ws[2][0], b3)]


_SCALE = {}


def state_scale(ni, key, seed):
    """1 / (1 + mean |s_i|) per state column over 700 lanes' start states (CLONED envs) or reset states."""
    import torch
    if key not in _SCALE:
        if key in CLONED:
            s = start_states(ni, NAMES[key], B_BIG, seed)
        else:
            probe = ni.make_batched(NAMES[key], B_BIG, seed=seed)
            probe.reset()
            torch.cuda.synchronize()
            s = probe.get_state().cpu().numpy()
            probe.close()
        _SCALE[key] = (1.0 / (1.0 + np.abs(s).mean(axis=0))).astype(np.float32)
    return _SCALE[key]


def matrix_actor(ni, key, ws, seed):
    """The actor a family module's own construction gives, made fit for the envs the matrix adds.  AdvancedChemicalReactor,
    SteelAnnealing and SupplyChain have state columns of 1e2 .. 1e5: unscaled they drive every tanh head to +-1 (five distinct
    action rows over 700 AdvancedChemicalReactor lanes) and float32 layer sums to errors far above the float64 bar, so their first
    layer is scaled by 20 / (1 + mean |s_i|) per state column (test_gpu_ensemble.py's construction).  AdvancedPowerGrid: continuing()."""
    if key in ("acr", "steel", "supply"):
        sc = state_scale(ni, key, seed)
        ws = [((ws[0][0] * np.float32(20.0) * sc[:, None]).astype(np.float32), ws[0][1]), ws[1], ws[2]]
    return continuing(key, ws)


def check_env_steps(oracle, L, key, o_obs, o_act, flags, seed, max_steps, env0=0, t0=0):
    """The plant behind a closed loop, teacher-forced: obs[k + 1] is the oracle's step of (obs[k], act[k]) with the lane's own
    draws, bit for bit, on the lanes that neither finished nor reset on step k and are live on both; and the TERMINATED bit of
    every live lane-step is the oracle's.  Returns the number of (lane, step) pairs whose next observation was compared."""
    T, B = flags.shape
    live = (flags & L.FLAG_INACTIVE) == 0
    k_step = oracle.spec(key).k_step
    checked = 0
    for k in range(T):
        fl = flags[k]
        step_after = (fl.astype(np.uint32) >> L.FLAG_STEP_SHIFT).astype(np.int32)
        nz = np.stack([oracle.gen_step_noise(key, seed, env0 + i, t0 + k + 1) for i in range(B)]) if k_step else None
        r = oracle.step(key, o_obs[k], o_act[k], nz, np.where(live[k], step_after - 1, 0), max_steps=max_steps, flavor=oracle.MATH_POLY)
        assert np.array_equal(((fl & L.FLAG_TERMINATED) != 0)[live[k]], (r["terminated"] != 0)[live[k]]), (k, "terminated")
        if k + 1 < T:
            cont = live[k] & live[k + 1] & ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED | L.FLAG_DID_RESET)) == 0)
            checked += int(cont.sum())
            assert np.array_equal(np.ascontiguousarray(o_obs[k + 1][cont]).view(np.uint32), r["state_next"][cont].view(np.uint32)), (k, "next obs")
    return checked


def distinct_rows(x):
    """The number of pairwise distinct rows of x [n, m] (compared as bit patterns)."""
    return len(np.unique(np.ascontiguousarray(x).view(np.uint32), axis=0))


def mlp64(layers, x):
    """The three-layer ReLU network's pre-activations of the last layer in NumPy float64: no tiles, no chunks, no lanes."""
    z = np.asarray(x, dtype=np.float64)
    for i, (W, b) in enumerate(layers):
        z = z @ np.asarray(W, dtype=np.float64) + np.asarray(b, dtype=np.float64).reshape(-1)
        if i < 2:
            z = np.maximum(z, 0)
    return z


def actor64(ws, obs):
    """tanh(actor(obs)) [..., A] in float64."""
    return np.tanh(mlp64(ws, obs))


def critic64(cw, obs, act):
    """sigmoid(critic([obs, act])) [...] in float64 (test_gpu_safety_shield.py's _critic64) for a one-column head."""
    z = mlp64(cw, np.concatenate([np.asarray(obs, dtype=np.float64), np.asarray(act, dtype=np.float64)], axis=-1))
    return 1.0 / (1.0 + np.exp(-z[..., 0]))


def worst(what, got, want, atol):
    """max |got - want| / atol, printed; the caller asserts it <= 1."""
    r = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)) / atol) if np.size(got) else 0.0
    print(f"{what}: worst error / bound ({atol:g}) = {r:.3g}")
    return r
