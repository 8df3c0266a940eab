"""gpu: the fused shield of shaped agents ("nig-mlp-shape-shield-v1", csrc/nig_mlp_shape_shield.hpp) -- nig_set_mlp_safety_dims and
nig_rollout_mlp_safe's dispatch on the actor slot and the critic slot.  The measuring stick is the restatement of "nig-mlp-shape-v1"
(tests/mlp_shape_ref.c, general in S, A and the widths) called with the critic's weights on [obs, raw action] and the oracle's
det_tanhf / det_sigmoidf (tests/mlp_shape_shield_ref.py): on the device's own obs_out, prob_out, the SHIELDED bit and act_out are that
restatement bit for bit, and the env stepped exactly as nig_step steps it on act_out.  Shapes: closed_loop_matrix's B_BIG (700: five
full 128-env blocks, one full wave and a ragged wave) and B_SMALL (5), T_NEW = 7 steps of episodes of at most MAXS_NEW = 5: the
largest launch is 6 blocks for 7 steps."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
import mlp_shape_ref as ref
import mlp_shape_shield_ref as sref
from footprint import Arena, Layout
from test_gpu_footprint import Rig, ceil4, clean, gap, pitch
from test_gpu_mlp_ln import _close, _dims, _stepped_as_nig_step
from test_gpu_mlp_shape import FILL, FLAGFILL, INVALID, SEED, UNSUPPORTED, Out, _actor, _bits, _code, _integer_net, _make, _play, _same

pytestmark = pytest.mark.gpu
f32 = np.float32
T = M.T_NEW
ALL = ("rew", "flags", "obs", "act", "pr", "state", "ctr", "tally")
CLASS_DIMS = ref.CLASSES


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _agent(ni, key, S, A, dims, cdims=None, seed=21, cseed=31, head=1.0):
    """test_gpu_mlp_shape._actor's actor with a critic from ref.random_actor(S + A, 1, cdims, cseed) under the same first-layer state
    scaling: what the law reads of a policy, its .weights and .safety_weights"""
    cw = sref.random_critic(S, A, dims if cdims is None else cdims, cseed, state_scale=M.state_scale(ni, key, SEED), head=head)
    return types.SimpleNamespace(weights=_actor(ni, key, S, A, dims, seed), safety_weights=cw)


def _padded(ni, pol, cls):
    """the policy zero-padded to the class's widths: the network the law states for it"""
    return types.SimpleNamespace(weights=ni.policies.pad_actor(pol.weights, CLASS_DIMS[cls]),
                                 safety_weights=ni.policies.pad_actor(pol.safety_weights, CLASS_DIMS[cls]))


class SOut(Out):
    """Out with prob_out rows, launched through nig_rollout_mlp_safe itself (rows [row0, row0 + n) of every output)"""
    def __init__(self, env, n):
        super().__init__(env, n)
        self.pr = torch.full((n, env.ld), FILL, dtype=torch.float32, device=env.device)

    def safe(self, row0=0, n=None):
        env, n = self.env, self.n - row0 if n is None else n
        P = lambda t: C.c_void_p(t[row0].data_ptr())
        with torch.cuda.device(env.device):
            return env._L.nig_rollout_mlp_safe(env._h, n, P(self.rw), P(self.fl), env.ld, P(self.obs_rows), self.ostep, P(self.act), env.ld,
                                               env.action_dim * env.ld, P(self.pr), env._stream())

    def numpy(self):
        d = super().numpy()
        d["pr_raw"] = self.pr.cpu().numpy()
        d["pr"] = d["pr_raw"][:, :self.env.batch]
        return d

    def untouched(self):
        return super().untouched() and bool((self.pr == FILL).all())


def _start(ni, key, env):
    env.reset()
    M.install_start(ni, env, key, SEED)
    torch.cuda.synchronize()
    return env.get_state().cpu().numpy().copy()


def _install(pol, thr):
    return lambda env: (env.set_mlp_policy_dims(pol.weights), env.set_mlp_safety_dims(pol.safety_weights, thr))


def _play_safe(ni, key, name, B, pol, threshold, n=T, autoreset=True, chunks=None, states=None, install=None):
    """One handle: actor and critic installed, `threshold` a number or a function of the start states; n steps in launches of `chunks`."""
    env = _make(ni, name, B, autoreset)
    s0 = _start(ni, key, env)
    if states is not None:
        env.set_state(states, current_step=0, violation_count=0, done=False)
        s0 = np.asarray(states, dtype=f32)
    thr = float(f32(threshold(s0) if callable(threshold) else threshold))
    (install or _install)(pol, thr)(env)
    out, t0, row = SOut(env, n), env.counter, 0
    for c in chunks or (n,):
        assert out.safe(row, c) == 0, env._L.nig_last_error()
        row += c
    assert row == n
    o = out.numpy()
    assert env.counter == t0 + n
    assert np.all(o["act_raw"][:, :, B:] == f32(FILL)) and np.all(o["rew"][:, B:] == f32(FILL)) and np.all(o["flags_raw"][:, B:] == FLAGFILL)
    assert np.all(o["pr_raw"][:, B:] == f32(FILL))
    o["state"], o["ctr"], o["tally"] = env.get_state().cpu().numpy().copy(), env.ctr.cpu().numpy().copy(), env.reduce_tally().cpu().numpy().copy()
    o["thr"], o["s0"], o["kind"], o["cdims"], o["adims"] = thr, s0, env.mlp_safety_kind, env.mlp_safety_dims, env.mlp_policy_dims
    env.close()
    return o


def _follows_the_law(ni, oracle, o, pol, live=None, steps=None):
    """on the device's own observations: prob_out, the SHIELDED bit and act_out of every live lane are the restatement, bit for bit
    (steps: the steps restated; default: all)"""
    SH = np.uint32(ni._lib.FLAG_SHIELDED)
    for k in range(o["obs"].shape[0]) if steps is None else steps:
        rows = slice(None) if live is None else live[k]
        raw, p, shield, act = sref.step(oracle, pol, o["obs"][k][rows], o["thr"])
        assert np.array_equal(_bits(o["pr"][k][rows]), _bits(p)), (k, "prob_out")
        assert np.array_equal((o["flags"][k][rows] & SH) != 0, shield), (k, "SHIELDED")
        assert np.array_equal(_bits(o["act"][k][rows]), _bits(act)), (k, "act_out")


def _median_p(oracle, pol, B):
    """the threshold: the median of the RESTATED p over the start states, before any launch -- and the condition that it divides them"""
    def threshold(s0):
        p = sref.prob(oracle, pol.safety_weights, s0, ref.act(oracle, pol.weights, s0))
        thr = f32(np.median(p))
        shielded = ~(p < thr)
        if B == M.B_BIG:
            assert 0.25 <= shielded.mean() <= 0.75, ("the threshold divides the lanes", shielded.mean())
        assert shielded.any() and not shielded.all(), "at least one lane of each kind"
        return thr
    return threshold


# ---- 1. the anchor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("cls", ref.SHIPPED)
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_probabilities_shield_and_actions_are_the_law_bit_for_bit(ni, oracle, key, name, cls, B):
    S, A = _dims(ni, name)
    pol = _agent(ni, key, S, A, CLASS_DIMS[cls])
    o = _play_safe(ni, key, name, B, pol, _median_p(oracle, pol, B))
    L = ni._lib
    assert o["kind"] == L.SAFETY_SIGMOID_SHAPED == 4 and o["cdims"] == o["adims"] == CLASS_DIMS[cls]
    assert not (o["flags"] & L.FLAG_INACTIVE).any() and np.isfinite(o["act"]).all() and np.isfinite(o["pr"]).all()
    assert np.array_equal(_bits(o["obs"][0]), _bits(o["s0"]))
    raw0 = ref.act(oracle, pol.weights, o["obs"][0])
    shielded = (o["flags"][0] & L.FLAG_SHIELDED) != 0
    assert np.array_equal(_bits(np.where(shielded[:, None], raw0 * f32(0.5), raw0)), _bits(o["act"][0])), "the raw action is mlp_shape_ref.act"
    _follows_the_law(ni, oracle, o, pol)
    unshielded = dict(o, flags=o["flags"] & ~np.uint32(L.FLAG_SHIELDED))          # nig_step knows no shield
    _stepped_as_nig_step(ni, key, name, B, unshielded)                           # state, reward, flags, counters and tally
    if B == M.B_BIG:
        print(f"{key} {cls}: {len(np.unique(o['pr'][0]))} distinct p on step 0 in [{o['pr'][0].min():.4f}, {o['pr'][0].max():.4f}], {shielded.mean():.3f} shielded")
        assert len(np.unique(o["pr"][0])) >= 4, "the critic is not saturated"
    # 5a. float64 on step 0: a routing error shared by builder and restatement would pass bit equality
    x = np.concatenate([o["obs"][0], raw0], axis=1)
    p64 = 1.0 / (1.0 + np.exp(-sref.pre64(pol.safety_weights, o["obs"][0], raw0)))
    err, bound = np.abs(o["pr"][0].astype(np.float64) - p64), sref.p_bound(pol.safety_weights, x)
    print(f"{key} {cls} B={B}: largest |p - p64| = {err.max():.3g}, largest error / bound = {np.max(err / bound):.3g}")
    assert np.all(err <= bound), float(np.max(err / bound))


# ---- 2. the raw action is the actor family's -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ref.SHIPPED)
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_the_raw_action_is_rollout_mlps_with_the_same_actor(ni, oracle, key, name, cls):
    S, A = _dims(ni, name)
    B = M.B_BIG
    pol = _agent(ni, key, S, A, CLASS_DIMS[cls])
    bare = _play(ni, key, name, B, lambda env: env.set_mlp_policy_dims(pol.weights), n=1)
    o = _play_safe(ni, key, name, B, pol, _median_p(oracle, pol, B), n=1)
    assert np.array_equal(_bits(o["obs"][0]), _bits(bare["obs"][0]))
    shielded = (o["flags"][0] & ni._lib.FLAG_SHIELDED) != 0
    assert shielded.any() and not shielded.all()
    assert np.array_equal(_bits(o["act"][0][~shielded]), _bits(bare["act"][0][~shielded]))
    assert np.array_equal(_bits(o["act"][0][shielded]), _bits(bare["act"][0][shielded] * f32(0.5)))


# ---- 4. threshold ends -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ref.SHIPPED)
@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])
def test_a_threshold_above_one_is_rollout_mlp_and_a_threshold_of_zero_halves_every_lane(ni, oracle, key, name, cls):
    S, A = _dims(ni, name)
    B = M.B_BIG
    pol = _agent(ni, key, S, A, CLASS_DIMS[cls])
    bare = _play(ni, key, name, B, lambda env: env.set_mlp_policy_dims(pol.weights), n=T)
    none = _play_safe(ni, key, name, B, pol, 2.0)
    _same(none, bare)                                          # rew, flags, obs, act, state, ctr, tally of all 7 steps: nothing is shielded
    ends = (0, T - 1)                                          # (the restatement is run on the first and the last step: the anchor holds every step)
    _follows_the_law(ni, oracle, none, pol, steps=ends)        # prob_out is written all the same
    assert not (none["flags"] & ni._lib.FLAG_SHIELDED).any() and np.all(none["pr"] != f32(FILL))
    every = _play_safe(ni, key, name, B, pol, 0.0)             # (the setter takes every threshold; no p is below 0)
    assert np.all((every["flags"] & ni._lib.FLAG_SHIELDED) != 0)
    _follows_the_law(ni, oracle, every, pol, steps=ends)
    for k in ends:
        assert np.array_equal(_bits(every["act"][k]), _bits(ref.act(oracle, pol.weights, every["obs"][k]) * f32(0.5))), k
    assert np.array_equal(_bits(every["act"][0]), _bits(bare["act"][0] * f32(0.5)))


# ---- 5b. the critic's layout on exact data, whatever the summation order ----------------------------------------------------------
@pytest.mark.parametrize("cls", ref.SHIPPED)
@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])          # ChemicalReactor: width 15 (a pad step); PowerGrid: 40, the critic's own layer-1 split
def test_critic_layout_on_integer_data_whatever_the_order(ni, oracle, key, name, cls):
    """Integer states in [-2, 2]; an actor whose action j is sign(s_j) exactly (hidden units relu(s_j) and relu(-s_j) passed through,
    head 16 (h+ - h-): tanh saturates to +-1 and tanh(0) = 0); a critic of small integers whose every partial sum in every order is
    an exact integer below 2^24: p is det_sigmoidf of the integer network's value, whatever order the device sums in."""
    S, A = _dims(ni, name)
    B, dims = M.B_BIG, CLASS_DIMS[cls]
    aw, K = [], S
    for H in dims:
        W = np.zeros((K, H), f32)
        if not aw:
            for j in range(A):
                W[j, 2 * j], W[j, 2 * j + 1] = 1, -1
        else:
            W[np.arange(2 * A), np.arange(2 * A)] = 1
        aw.append((W, np.zeros(H, f32)))
        K = H
    Wh = np.zeros((K, A), f32)
    for j in range(A):
        Wh[2 * j, j], Wh[2 * j + 1, j] = 16, -16
    aw.append((Wh, np.zeros(A, f32)))
    rng = np.random.default_rng(78)
    x = rng.integers(-2, 3, (B, S)).astype(np.int64)
    raw = np.sign(x[:, :A])
    assert np.array_equal(_bits(ref.act(oracle, aw, x.astype(f32))), _bits(raw.astype(f32))), "the actor's actions are exactly sign(s_j)"
    iw = _integer_net(S + A, 1, dims, seed=77)
    h = np.concatenate([x, raw], axis=1)
    mag = np.abs(h)
    for i, (W, b) in enumerate(iw):
        mag = mag @ np.abs(W) + np.abs(b)
        assert mag.max() < 2 ** 24, (i, mag.max())
        h = h @ W + b
        if i + 1 < len(iw):
            h = np.maximum(h, 0)
    assert np.abs(iw[0][0][S:]).sum() > 0, "the action rows reach the first layer"
    shift = int(np.ceil(np.log2(max(np.abs(h).max(), 1) / 4.0)))
    scale = 2.0 ** -max(shift, 0)
    cw = [(W.astype(f32), b.astype(f32)) for W, b in iw[:-1]] + [((iw[-1][0] * scale).astype(f32), (iw[-1][1] * scale).astype(f32))]
    pre = (h[:, 0] * scale).astype(f32)
    assert np.array_equal(pre.astype(np.float64), h[:, 0] * scale) and np.abs(pre).max() <= 4.0 and len(np.unique(pre)) > 8
    want = oracle.detmath_unary("sigmoidf", pre)
    pol = types.SimpleNamespace(weights=aw, safety_weights=cw)
    o = _play_safe(ni, key, name, B, pol, 2.0, n=1, states=x.astype(f32))
    assert np.array_equal(_bits(o["obs"][0]), _bits(x.astype(f32))) and np.array_equal(_bits(o["act"][0]), _bits(raw.astype(f32)))
    assert np.array_equal(_bits(o["pr"][0]), _bits(want))
    assert np.array_equal(_bits(sref.prob(oracle, cw, x.astype(f32), raw.astype(f32))), _bits(want)), "the restatement agrees on exact data"
    # two action rows of C1 trade places: another p, and the device follows
    C1 = cw[0][0].copy()
    C1[[S, S + A - 1]] = C1[[S + A - 1, S]]
    traded = types.SimpleNamespace(weights=aw, safety_weights=[(C1, cw[0][1])] + cw[1:])
    t = _play_safe(ni, key, name, B, traded, 2.0, n=1, states=x.astype(f32))
    assert np.array_equal(_bits(t["pr"][0]), _bits(sref.prob(oracle, traded.safety_weights, x.astype(f32), raw.astype(f32))))
    assert not np.array_equal(_bits(t["pr"][0]), _bits(o["pr"][0]))


# ---- 6. padded widths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(96, 64), (300, 200), (200, 150, 100)])
@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])          # ChemicalReactor: odd S + A; PowerGrid: the critic's layer-1 split differs from the actor's
def test_padded_networks_installed_by_hand_follow_the_law_of_their_padded_form(ni, oracle, key, name, dims):
    S, A = _dims(ni, name)
    B = M.B_BIG
    cls = ni.policies.actor_shape_class(dims)
    assert cls in CLASS_DIMS and CLASS_DIMS[cls] != dims
    pol = _agent(ni, key, S, A, dims)
    padded = _padded(ni, pol, cls)
    thr = _median_p(oracle, padded, B)
    o = _play_safe(ni, key, name, B, pol, thr)
    assert o["kind"] == 4 and o["cdims"] == dims and o["adims"] == dims          # the unpadded widths
    _follows_the_law(ni, oracle, o, padded)
    _same(o, _play_safe(ni, key, name, B, padded, thr), names=ALL)


@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])
def test_a_reference_class_critic_is_set_mlp_safety_of_the_padded_arrays(ni, key, name):
    """(200, 200): the reference class.  set_mlp_safety_dims beside the reference actor equals set_mlp_safety(pad_critic(..)) in every
    output; the slot's kind is the plain one and its widths the unpadded ones."""
    S, A = _dims(ni, name)
    B = M.B_BIG
    assert ni.policies.actor_shape_class((200, 200)) == "reference"
    actor = M.matrix_actor(ni, key, M.random_actor(S, A, 5), SEED)
    pol = types.SimpleNamespace(weights=actor, safety_weights=sref.random_critic(S, A, (200, 200), 31, state_scale=M.state_scale(ni, key, SEED)))
    by_dims = _play_safe(ni, key, name, B, pol, 0.5, install=lambda p, thr: lambda env: (env.set_mlp_policy(p.weights), env.set_mlp_safety_dims(p.safety_weights, thr)))
    by_hand = _play_safe(ni, key, name, B, pol, 0.5, install=lambda p, thr: lambda env: (env.set_mlp_policy(p.weights), env.set_mlp_safety(ni.policies.pad_critic(p.safety_weights), thr)))
    _same(by_dims, by_hand, names=ALL)
    assert by_dims["kind"] == by_hand["kind"] == ni._lib.SAFETY_SIGMOID == 1 and by_dims["cdims"] == (200, 200) and by_hand["cdims"] == (256, 256)
    sh = (by_dims["flags"] & ni._lib.FLAG_SHIELDED) != 0
    print(f"{key}: {sh.mean():.3f} shielded, p in [{by_dims['pr'].min():.4f}, {by_dims['pr'].max():.4f}]")


# ---- 7. launch splitting ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ref.SHIPPED)
def test_one_launch_equals_its_pieces(ni, oracle, cls):
    key, name, B = "pg", "PowerGrid-v0", M.B_BIG               # (the critic's layer 1 takes more chunks than the actor's: the chain restarts on the actor's)
    S, A = _dims(ni, name)
    pol = _agent(ni, key, S, A, CLASS_DIMS[cls])
    thr = _median_p(oracle, pol, B)
    whole = _play_safe(ni, key, name, B, pol, thr)
    _same(_play_safe(ni, key, name, B, pol, thr, chunks=(3, 4)), whole, names=ALL)
    _same(_play_safe(ni, key, name, B, pol, thr, chunks=(1, 1, 5)), whole, names=ALL)
    sh = (whole["flags"] & ni._lib.FLAG_SHIELDED) != 0
    assert sh.any() and not sh.all() and ((whole["flags"] & ni._lib.FLAG_DID_RESET) != 0).any()


# ---- 8. frozen lanes and auto-reset ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ref.SHIPPED)
def test_frozen_lanes_store_nothing_and_live_lanes_follow_the_law(ni, oracle, cls):
    """test_gpu_mlp_shape's scheme: no auto-reset, B = 5, 7 steps of episodes of at most 5, lanes 1 and 3 held from the start."""
    L = ni._lib
    key, name, B, n = "cr", "ChemicalReactor-v0", M.B_SMALL, T
    pol = _agent(ni, key, 12, 3, CLASS_DIMS[cls])
    env = _make(ni, name, B, autoreset=False)
    s0 = _start(ni, key, env)
    thr = float(f32(_median_p(oracle, pol, B)(s0)))
    _install(pol, thr)(env)
    held = np.array([1, 3])
    c = env.ctr.clone()
    c[torch.as_tensor(held, device=env.device)] |= L.CTR_DONE
    assert env._L.nig_set_state(env._h, None, B, C.c_void_p(c.data_ptr()), env._stream()) == 0
    torch.cuda.synchronize()
    state0, ctr0 = env.get_state().cpu().numpy().copy(), env.ctr.cpu().numpy().copy()
    out = SOut(env, n)
    assert out.safe() == 0, env._L.nig_last_error()
    o = out.numpy()
    o["thr"] = thr
    fl = o["flags"]
    live = (fl & L.FLAG_INACTIVE) == 0
    ended = live & ((fl & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0)
    is_held = np.isin(np.arange(B), held)
    assert np.array_equal(live[0], ~is_held) and np.array_equal(live[1:], live[:-1] & ~ended[:-1]) and not (fl & L.FLAG_DID_RESET).any()
    assert not live[M.MAXS_NEW:].any() and live[M.MAXS_NEW - 1].any()
    last_step = np.zeros(B, np.uint32)
    for k in range(n):
        fz = ~live[k]
        assert np.array_equal(fl[k][fz], (np.uint32(L.FLAG_INACTIVE) | (last_step << np.uint32(L.FLAG_STEP_SHIFT)))[fz]), k     # (no SHIELDED bit)
        last_step = np.where(live[k], (fl[k] & ~np.uint32(L.FLAG_SHIELDED)) >> np.uint32(L.FLAG_STEP_SHIFT), last_step)
        assert not _bits(o["rew"][k][:B])[fz].any(), k
        assert np.all(_bits(o["obs"][k])[fz] == _bits(f32(FILL))) and np.all(_bits(o["act"][k])[fz] == _bits(f32(FILL))), k
        assert np.all(_bits(o["pr"][k])[fz] == _bits(f32(FILL))) and np.all(o["pr"][k][live[k]] != f32(FILL)), k
    state1, ctr1 = env.get_state().cpu().numpy(), env.ctr.cpu().numpy()
    assert np.array_equal(_bits(state1)[held], _bits(state0)[held]) and np.array_equal(ctr1[held], ctr0[held])
    assert np.all((ctr1.view(np.uint32) & L.CTR_DONE) != 0), "every lane ends done"
    env.close()
    _follows_the_law(ni, oracle, o, pol, live=live)


@pytest.mark.parametrize("cls", ref.SHIPPED)
def test_episodes_end_and_restart_inside_the_launch_and_the_tally_counts_them(ni, oracle, cls):
    L = ni._lib
    key, name, B = "cr", "ChemicalReactor-v0", M.B_BIG
    pol = _agent(ni, key, 12, 3, CLASS_DIMS[cls])
    o = _play_safe(ni, key, name, B, pol, _median_p(oracle, pol, B))
    resets = (o["flags"] & L.FLAG_DID_RESET) != 0
    ended = (o["flags"] & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0
    assert np.array_equal(resets, ended) and resets.sum() >= B, "every lane finishes an episode of at most 5 steps within 7"
    assert int(round(float(o["tally"][L.T_EPISODES]))) == int(ended.sum())
    steps = (o["flags"] & ~np.uint32(L.FLAG_SHIELDED)) >> np.uint32(L.FLAG_STEP_SHIFT)
    assert np.all(steps[1:][resets[:-1]] == 1), "the step after a restart is the first of a new episode"
    assert int(round(float(o["tally"][L.T_LEN_SUM]))) == int(steps[ended].sum())


# ---- 9. the footprint ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ref.SHIPPED)
@pytest.mark.parametrize("key", ["cr", "pg"])                  # the 4 x 4 x 1 head; the 16 x 16 x 1 head
def test_footprint_at_pitches_beyond_ld(ni, key, cls):
    """One canary arena (tests/footprint.py): B_BIG lanes, every output -- prob_out included -- at a pitch beyond ld and a step stride
    with a gap; pads, stride gaps, the step beyond n_steps and the red zones keep the canary; every documented word is written."""
    B, mode = M.B_BIG, "wide"
    r = Rig(ni, key, B, autoreset=True, max_steps=M.MAXS_NEW)
    S, A, ld, L = r.S, r.A, r.ld, r.L
    pol = _agent(ni, key, S, A, CLASS_DIMS[cls])
    _install(pol, 0.5)(r.env)
    a = Arena("cuda")
    os_, lda = pitch(mode, B, ld, 1), pitch(mode, B, ld, 2)
    assert os_ > ld and lda > ld
    rew = a.add("reward_out", "f32", Layout(T, os_, 1, os_, B))
    fl = a.add("flags_out", "flags", Layout(T, os_, 1, os_, B))
    prob = a.add("prob_out", "f32", Layout(T, os_, 1, os_, B))
    obs = a.add("obs_out", "f32", Layout(T, ceil4(B * S) + gap(mode, 1, mult4=True), 1, B * S, B * S, lane_width=S), align=16)
    act = a.add("act_out", "f32", Layout(T, A * lda + gap(mode, 2), A, lda, B))
    a.build()
    r.reset()
    p = lambda b: C.c_void_p(b.ptr)
    rc = L.nig_rollout_mlp_safe(r.h, T, p(rew), p(fl), os_, p(obs), obs.layout.outer_stride, p(act), lda, act.layout.outer_stride, p(prob), r.st())
    assert rc == 0, L.nig_last_error()
    torch.cuda.synchronize()
    findings = [str(f) for f in a.check({b.name: dict(n_outer=T) for b in (rew, fl, prob, obs, act)})] + r.workspace_findings()
    r.close()
    clean(findings, f"nig_rollout_mlp_safe with a shaped actor and critic of class {cls}")


# ---- 10. slots and refusals ------------------------------------------------------------------------------------------------------
def _plain_safe(ni, name, B, install, n=T):
    """nig_rollout_mlp_safe on a fresh handle after install(env): the outputs, prob rows included"""
    env = _make(ni, name, B)
    install(env)
    env.reset()
    out = SOut(env, n)
    assert out.safe() == 0, env._L.nig_last_error()
    o = out.numpy()
    o["state"], o["ctr"], o["tally"] = env.get_state().cpu().numpy().copy(), env.ctr.cpu().numpy().copy(), env.reduce_tally().cpu().numpy().copy()
    env.close()
    return o


def test_the_four_critic_installs_replace_each_other_and_any_actor_keeps_the_critic(ni):
    import mlp_ln_shield_ref as lref
    from test_gpu_mlp_ln import _policy
    key, name, B = "cr", "ChemicalReactor-v0", M.B_BIG
    S, A = 12, 3
    pol, big = _agent(ni, key, S, A, (128, 128)), _agent(ni, key, S, A, (512, 512), cseed=77)
    actor, critic, cat = M.random_actor(S, A, 5), M.random_critic(S, A, 6), M.random_critic(S, A, 7, n_out=11)
    lnp = _policy(ni, key, S, A)
    lcw, lcn = lref.random_ln_critic(S, A, 31, state_scale=M.state_scale(ni, key, SEED), head=0.5)
    lnp = ni.LayerNormMLPPolicy(lnp.weights, lnp.norms, safety_weights=lcw, safety_norms=lcn)
    shp = lambda env: (env.set_mlp_policy_dims(pol.weights), env.set_mlp_safety_dims(pol.safety_weights, 0.45))
    shp_big = lambda env: (env.set_mlp_policy_dims(pol.weights), env.set_mlp_safety_dims(big.safety_weights, 0.9))     # (a larger class first: the slot's image is reused)
    sig = lambda env: (env.set_mlp_policy(actor), env.set_mlp_safety(critic, 0.5))
    ctg = lambda env: (env.set_mlp_policy(actor), env.set_mlp_safety_categorical(cat, 0.5))
    ln = lambda env: (env.set_mlp_policy_ln(lnp), env.set_mlp_safety_ln(lnp, 0.45))
    fresh = {k: _plain_safe(ni, name, B, f) for k, f in (("shp", shp), ("sig", sig), ("cat", ctg), ("ln", ln))}
    kinds, widths = [], []

    def chain(*installs):
        def run(env):
            assert env.mlp_safety_kind == 0 and env.mlp_safety_dims == ()
            for f in installs:
                f(env)
                kinds.append(env.mlp_safety_kind)
                widths.append(env.mlp_safety_dims)
        return run
    _same(_plain_safe(ni, name, B, chain(sig, ctg, ln, shp_big, shp)), fresh["shp"], names=ALL)
    _same(_plain_safe(ni, name, B, chain(shp, sig)), fresh["sig"], names=ALL)
    _same(_plain_safe(ni, name, B, chain(shp, ctg)), fresh["cat"], names=ALL)
    _same(_plain_safe(ni, name, B, chain(shp, ln)), fresh["ln"], names=ALL)
    assert kinds == [1, 2, 3, 4, 4, 4, 1, 4, 2, 4, 3]
    assert widths == [(256, 256)] * 3 + [(512, 512), (128, 128), (128, 128), (256, 256), (128, 128), (256, 256), (128, 128), (256, 256)]

    def actors_between(env):                                   # installing any actor keeps the critic
        env.set_mlp_safety_dims(pol.safety_weights, 0.45)
        env.set_mlp_policy(actor)
        env.set_mlp_policy_ln(lnp)
        env.set_mlp_policy_dims(big.weights)
        env.set_mlp_policy_dims(pol.weights)
        assert env.mlp_safety_kind == 4 and env.mlp_safety_dims == (128, 128)
    _same(_plain_safe(ni, name, B, actors_between), fresh["shp"], names=ALL)
    assert ni._lib.lib().nig_get_mlp_safety_dims(None, None) == -1


def test_a_refused_install_leaves_the_previous_critic_running(ni):
    key, name, B = "cr", "ChemicalReactor-v0", M.B_BIG
    S, A = 12, 3
    pol = _agent(ni, key, S, A, (128, 128))
    actor, critic = M.random_actor(S, A, 5), M.random_critic(S, A, 6)
    shp = lambda env: (env.set_mlp_policy_dims(pol.weights), env.set_mlp_safety_dims(pol.safety_weights, 0.45))
    sig = lambda env: (env.set_mlp_policy(actor), env.set_mlp_safety(critic, 0.5))
    ws = [(np.ascontiguousarray(W), np.ascontiguousarray(b)) for W, b in sref.random_critic(S, A, (64, 64), 4)]
    Wp = (C.c_void_p * 4)(*[W.ctypes.data for W, _ in ws], None)
    bp = (C.c_void_p * 4)(*[b.ctypes.data for _, b in ws], None)
    hid = lambda *d: (C.c_int32 * 3)(*d)

    def refused(first):
        def run(env):
            first(env)
            kind, widths = env.mlp_safety_kind, env.mlp_safety_dims
            for n_hidden, hidden, Wa, ba in ((1, hid(64, 0, 0), Wp, bp), (4, hid(64, 64, 64), Wp, bp), (2, hid(64, 513, 0), Wp, bp), (2, hid(0, 64, 0), Wp, bp),
                                             (2, None, Wp, bp), (2, hid(64, 64, 0), None, bp), (2, hid(64, 64, 0), Wp, None),
                                             (3, hid(64, 64, 64), Wp, bp), (3, hid(512, 512, 512), Wp, bp)):      # (the fourth layer's pointer is NULL; no class holds 512 x 3)
                assert env._L.nig_set_mlp_safety_dims(env._h, n_hidden, hidden, Wa, ba, C.c_float(0.5), env._stream()) == INVALID, (n_hidden, hidden)
                assert env.mlp_safety_kind == kind and env.mlp_safety_dims == widths
            assert env._L.nig_set_mlp_safety_dims(None, 2, hid(64, 64, 0), Wp, bp, C.c_float(0.5), None) == INVALID
        return run
    _same(_plain_safe(ni, name, B, refused(shp)), _plain_safe(ni, name, B, shp), names=ALL)
    _same(_plain_safe(ni, name, B, refused(sig)), _plain_safe(ni, name, B, sig), names=ALL)
    water = _make(ni, "WaterTreatment-v0", M.B_SMALL)          # odd state dim: no MFMA actor
    assert _code(lambda: water.set_mlp_safety_dims(sref.random_critic(water.state_dim, water.action_dim, (128, 128), 1), 0.5)) == UNSUPPORTED
    assert water.mlp_safety_kind == 0 and water.mlp_safety_dims == ()
    water.close()


def test_the_readers_of_the_slots_refuse_what_the_family_does_not_reach(ni):
    from test_gpu_mlp_ln import _policy
    name, B = "ChemicalReactor-v0", M.B_SMALL
    S, A = 12, 3
    pol, other = _agent(ni, "cr", S, A, (128, 128)), _agent(ni, "cr", S, A, (512, 256))
    env = _make(ni, name, B)
    env.reset()
    env.set_mlp_policy(M.random_actor(S, A, 5))
    env.set_mlp_safety_dims(pol.safety_weights, 0.5)
    o = SOut(env, 1)
    ch = torch.full((1, env.ld), FLAGFILL, dtype=torch.int32, device=env.device)
    rk = torch.full((1, env.ld), FILL, dtype=torch.float32, device=env.device)
    xf = torch.full((1, env.ld), FLAGFILL, dtype=torch.int32, device=env.device)
    vp = torch.full((env.ld,), FILL, dtype=torch.float32, device=env.device)
    vobs, vact = torch.zeros((S, env.ld), device=env.device), torch.zeros((A, env.ld), device=env.device)
    P = lambda t: C.c_void_p(t.data_ptr())
    state0, ctr0, t0 = env.get_state().clone(), env.ctr.clone(), env.counter

    def untouched():
        return (o.untouched() and bool((ch == FLAGFILL).all()) and bool((xf == FLAGFILL).all()) and bool((rk == FILL).all()) and bool((vp == FILL).all())
                and env.counter == t0 and torch.equal(env.get_state(), state0) and torch.equal(env.ctr, ctr0))
    readers = {"rollout_mlp_safe": lambda: env.rollout_mlp_safe(1, o.rw, o.fl, o.obs, o.act, o.pr),
               "rollout_mlp_search": lambda: env.rollout_mlp_search(1, 3, o.rw, o.fl, o.obs, o.act, o.pr, rk, ch),
               "rollout_mlp_safe_limited": lambda: env.rollout_mlp_safe_limited(1, o.rw, o.fl, o.obs, o.act, o.pr, xf),
               "rollout_mlp_search_limited": lambda: env.rollout_mlp_search_limited(1, 3, o.rw, o.fl, o.obs, o.act, o.pr, rk, ch, xf),
               "violation_prob": lambda: ni._lib.check(env._L.nig_mlp_violation_prob(env._h, B, P(vobs), env.ld, P(vact), env.ld, P(vp), None, 0, env._stream()))}
    for entry, call in readers.items():                        # the shaped critic beside the reference actor
        assert _code(call) == UNSUPPORTED, entry
        assert "shaped critic" in env._L.nig_last_error().decode(), (entry, env._L.nig_last_error())
        assert untouched() and env.mlp_safety_kind == 4, entry
    for what, install in (("a LayerNorm actor", lambda: env.set_mlp_policy_ln(_policy(ni, "cr", S, A))),
                          ("a bf16 actor beside the plain one", lambda: env.set_mlp_policy_bf16(M.random_actor(S, A, 5))),
                          ("a shaped actor of another class", lambda: env.set_mlp_policy_dims(other.weights))):
        install()
        assert _code(readers["rollout_mlp_safe"]) == UNSUPPORTED and untouched(), what
        assert "shaped critic" in env._L.nig_last_error().decode(), what
        env.set_mlp_policy(M.random_actor(S, A, 5))
    env.set_mlp_policy_dims(pol.weights)                       # shaped actor + shaped critic of its class: the family has no search and no twin
    for entry in ("rollout_mlp_search", "rollout_mlp_safe_limited", "rollout_mlp_search_limited", "violation_prob"):
        assert _code(readers[entry]) == UNSUPPORTED and untouched(), entry
    env.rollout_mlp_safe(1, o.rw, o.fl, o.obs, o.act, o.pr)    # positive control: the same buffers run
    assert not o.untouched() and not bool((o.pr[:, :B] == FILL).any()) and env.counter == t0 + 1
    env.close()
    for critic in ("none", "plain", "categorical"):            # a shaped actor beside any other critic: the shaped actor's refusal, as before
        bare = _make(ni, name, B)
        bare.reset()
        bare.set_mlp_policy_dims(pol.weights)
        if critic == "plain":
            bare.set_mlp_safety(M.random_critic(S, A, 6), 0.5)
        if critic == "categorical":
            bare.set_mlp_safety_categorical(M.random_critic(S, A, 7, n_out=11), 0.5)
        ob, tb = SOut(bare, 1), bare.counter
        assert _code(lambda: bare.rollout_mlp_safe(1, ob.rw, ob.fl, ob.obs, ob.act, ob.pr)) == UNSUPPORTED and ob.untouched() and bare.counter == tb, critic
        assert "shaped actor" in bare._L.nig_last_error().decode(), critic
        bare.close()


# ---- 11. routing -----------------------------------------------------------------------------------------------------------------
class _ShieldLawAgent:
    """The law's shielded actions computed on the host, observation by observation: the agent evaluate_with_safety can only play
    through its per-step host loop -- on exactly the actions the device computes."""
    is_trained = True

    def __init__(self, oracle, pol, thr):
        self.oracle, self.pol, self.thr = oracle, pol, thr

    def predict_device(self, obs):
        return torch.as_tensor(sref.step(self.oracle, self.pol, obs.cpu().numpy(), self.thr)[3], device=obs.device)


@pytest.mark.parametrize("cls", ref.SHIPPED)
def test_evaluate_plays_a_shielded_shaped_policy_with_rollout_mlp_safe_and_equals_the_host_loop(ni, oracle, cls):
    key, name, B = "cr", "ChemicalReactor-v0", 64
    net = _agent(ni, key, 12, 3, CLASS_DIMS[cls])
    make = lambda: ni.make_batched(name, B, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    probe = make()
    thr = float(f32(_median_p(oracle, net, B)(_start(ni, key, probe))))
    probe.close()
    pol = ni.MLPPolicy(net.weights, safety_weights=net.safety_weights)
    sh = pol.shielded(thr)
    assert sh.threshold == thr and sh.shape_shield_exact is True and sh.fusable is False and sh.base is pol
    benv = make()
    agent, rollout, disturbed = ni.utils._install_agent(sh, benv)
    routed = cls in ni.utils.SHAPE_SHIELD_ROUTED
    if not routed:                                             # a class the measurement left on the host route: its C entry point still runs
        assert rollout is None
        benv.set_mlp_policy_dims(sh.weights), benv.set_mlp_safety_dims(sh.safety_weights, sh.threshold)
        assert benv.mlp_safety_kind == 4
        benv.close()
        return
    assert agent is sh and disturbed is None and rollout is not None and rollout.__func__ is type(benv).rollout_mlp_safe
    assert benv.mlp_policy_dims == CLASS_DIMS[cls] == benv.mlp_safety_dims and benv.mlp_safety_kind == 4
    fused = ni.evaluate_with_safety(sh, benv, n_episodes=B)
    torch.cuda.synchronize()
    assert int(round(float(benv.reduce_tally()[ni._lib.T_EPISODES].item()))) == B
    henv = make()
    law = _ShieldLawAgent(oracle, net, thr)
    assert ni.utils._install_agent(law, henv)[1] is None
    host = ni.evaluate_with_safety(law, henv, n_episodes=B)
    assert henv.mlp_safety_kind == 0
    _close(fused, host)
    assert 1.0 <= fused["length_mean"] <= M.MAXS_NEW
    e1 = make()
    e_fused = ni.evaluate_episodes(sh, e1, n_episodes=B)
    assert e1.mlp_safety_kind == 4
    e1.close()
    assert e_fused["length_mean"] == fused["length_mean"] and e_fused["return_mean"] == pytest.approx(fused["return_mean"], rel=1e-12)
    benv.close(), henv.close()
    lim = make()                                               # added constraints: the policy's torch form plays
    lim.add_safety_constraint(ni.BoxConstraint("cap", {("state", 0): (-1e30, 1e30)}, penalty=0.0))
    assert ni.utils._install_agent(sh, lim)[1] is None
    res = ni.evaluate_with_safety(sh, lim, n_episodes=B)
    assert np.isfinite(res["return_mean"]) and 1.0 <= res["length_mean"] <= M.MAXS_NEW
    lim.close()
