"""gpu: the fused shield of LayerNorm agents ("nig-mlp-ln-shield-v1", csrc/nig_mlp_ln_shield.hpp) -- nig_set_mlp_safety_ln and
nig_rollout_mlp_safe's dispatch on the actor slot and the critic slot.  The measuring stick is the restatement of "nig-mlp-ln-v1"
(tests/mlp_ln_ref.c, general in IN / OUT) called with the critic's weights on [obs, raw action] and the oracle's det_tanhf /
det_sigmoidf (tests/mlp_ln_shield_ref.py): on the device's own obs_out, prob_out, the SHIELDED bit and act_out are that restatement bit
for bit, and the env stepped exactly as nig_step steps it on act_out.  Shapes: closed_loop_matrix's B_BIG (700: five full 128-env
blocks, one full wave and a ragged wave) and B_SMALL (5), T_NEW = 7 steps of episodes of at most MAXS_NEW = 5."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
import mlp_ln_ref as ref
import mlp_ln_shield_ref as sref
from footprint import Arena, Layout
from test_gpu_footprint import Rig, ceil4, clean, gap, pitch
from test_gpu_mlp_ln import _close, _dims, _policy, _stepped_as_nig_step, layout_policy
from test_gpu_mlp_shape import FILL, FLAGFILL, INVALID, SEED, UNSUPPORTED, Out, _bits, _code, _make, _play, _same

pytestmark = pytest.mark.gpu
f32 = np.float32
T = M.T_NEW
ALL = ("rew", "flags", "obs", "act", "pr", "state", "ctr", "tally")


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _agent(ni, key, S, A, seed=21, cseed=31, head=0.5):
    """test_gpu_mlp_ln._policy's actor with a critic from ref.random_ln_actor(S + A, 1, cseed) under the same first-layer state scaling"""
    actor = _policy(ni, key, S, A, seed)
    cw, cn = sref.random_ln_critic(S, A, cseed, state_scale=M.state_scale(ni, key, SEED), head=head)
    return ni.LayerNormMLPPolicy(actor.weights, actor.norms, safety_weights=cw, safety_norms=cn)


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


def _play_safe(ni, key, name, B, pol, threshold, n=T, autoreset=True, chunks=None, states=None):
    """One handle: actor and critic installed, `threshold` a number or a function of the start states; n steps in launches of `chunks`."""
    env = _make(ni, name, B, autoreset)
    env.set_mlp_policy_ln(pol)
    s0 = _start(ni, key, env)
    if states is not None:
        env.set_state(states, current_step=0, violation_count=0, done=False)
        s0 = np.asarray(states, dtype=f32)
    thr = float(f32(threshold(s0) if callable(threshold) else threshold))
    env.set_mlp_safety_ln(pol, thr)
    assert env.mlp_policy_norm is True and env.mlp_safety_kind == ni._lib.SAFETY_SIGMOID_LN == 3
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
    o["thr"], o["s0"] = thr, s0
    env.close()
    return o


def _follows_the_law(ni, oracle, o, pol, live=None):
    """on the device's own observations: prob_out, the SHIELDED bit and act_out of every live lane are the restatement, bit for bit"""
    SH = np.uint32(ni._lib.FLAG_SHIELDED)
    for k in range(o["obs"].shape[0]):
        rows = slice(None) if live is None else live[k]
        raw, p, shield, act = sref.step(oracle, pol, o["obs"][k][rows], o["thr"])
        assert np.array_equal(_bits(o["pr"][k][rows]), _bits(p)), (k, "prob_out")
        assert np.array_equal((o["flags"][k][rows] & SH) != 0, shield), (k, "SHIELDED")
        assert np.array_equal(_bits(o["act"][k][rows]), _bits(act)), (k, "act_out")


def _median_p(oracle, pol):
    def threshold(s0):
        raw = ref.act(oracle, pol.weights, pol.norms, s0, pol.eps)
        return np.median(sref.prob(oracle, pol.safety_weights, pol.safety_norms, s0, raw, pol.safety_eps))
    return threshold


# ---- 1. the anchor ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("key,name", M.MFMA_ENVS)
def test_probabilities_shield_and_actions_are_the_law_bit_for_bit(ni, oracle, key, name, B):
    S, A = _dims(ni, name)
    pol = _agent(ni, key, S, A)
    o = _play_safe(ni, key, name, B, pol, _median_p(oracle, pol))                # the threshold: from the RESTATED p, before the launch
    L = ni._lib
    assert not (o["flags"] & L.FLAG_INACTIVE).any() and np.isfinite(o["act"]).all() and np.isfinite(o["pr"]).all()
    assert np.array_equal(_bits(o["obs"][0]), _bits(o["s0"]))
    _follows_the_law(ni, oracle, o, pol)
    unshielded = dict(o, flags=o["flags"] & ~np.uint32(L.FLAG_SHIELDED))          # nig_step knows no shield
    _stepped_as_nig_step(ni, key, name, B, unshielded)
    if B == M.B_BIG:
        shielded = (o["flags"][0] & L.FLAG_SHIELDED) != 0
        print(f"{key}: {len(np.unique(o['pr'][0]))} distinct p on step 0 in [{o['pr'][0].min():.4f}, {o['pr'][0].max():.4f}], {shielded.mean():.3f} shielded")
        assert len(np.unique(o["pr"][0])) >= 4, "the critic is not saturated"
        assert 0.25 <= shielded.mean() <= 0.75, "the threshold divides the lanes"
    assert key == "apg" or ((o["flags"] & L.FLAG_DID_RESET) != 0).any(), "a restart falls inside the launch"
    if key in M.FLOAT64_KEYS:                                   # also held to the float64 formula (the bar of the plain shield's p)
        raw = ref.act(oracle, pol.weights, pol.norms, o["obs"][0], pol.eps)
        m = sref.model64(pol.safety_weights, pol.safety_norms, o["obs"][0], raw)
        assert M.worst(f"{key}: p against the float64 model", o["pr"][0], 1.0 / (1.0 + np.exp(-m["pre"][:, 0])), M.PROB_ATOL) <= 1.0


# ---- 2. edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])
def test_a_threshold_above_one_is_rollout_mlp_and_a_threshold_of_zero_halves_every_lane(ni, oracle, key, name):
    S, A = _dims(ni, name)
    B = M.B_BIG
    pol = _agent(ni, key, S, A)
    bare = _play(ni, key, name, B, lambda env: env.set_mlp_policy_ln(pol), n=T)
    none = _play_safe(ni, key, name, B, pol, 2.0)
    _same(none, bare)                                          # rew, flags, obs, act, state, ctr, tally: nothing is shielded
    _follows_the_law(ni, oracle, none, pol)                    # prob_out is written all the same
    assert not (none["flags"] & ni._lib.FLAG_SHIELDED).any()
    every = _play_safe(ni, key, name, B, pol, 0.0)
    assert np.all((every["flags"] & ni._lib.FLAG_SHIELDED) != 0)
    _follows_the_law(ni, oracle, every, pol)
    for k in range(T):
        raw = ref.act(oracle, pol.weights, pol.norms, every["obs"][k], pol.eps)
        assert np.array_equal(_bits(every["act"][k]), _bits(raw * f32(0.5))), k
    assert np.array_equal(_bits(every["act"][0]), _bits(bare["act"][0] * f32(0.5)))


def test_one_launch_equals_its_pieces(ni, oracle):
    key, name, B = "pg", "PowerGrid-v0", M.B_BIG
    S, A = _dims(ni, name)
    pol = _agent(ni, key, S, A)
    thr = _median_p(oracle, pol)
    whole = _play_safe(ni, key, name, B, pol, thr)
    _same(_play_safe(ni, key, name, B, pol, thr, chunks=(3, 4)), whole, names=ALL)
    _same(_play_safe(ni, key, name, B, pol, thr, chunks=(1,) * T), whole, names=ALL)
    assert ((whole["flags"] & ni._lib.FLAG_SHIELDED) != 0).any() and not ((whole["flags"] & ni._lib.FLAG_SHIELDED) != 0).all()


# ---- 3. the critic's layout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,name", M.MFMA_ENVS[:2])          # ChemicalReactor: critic width 15 (a pad step), one chunk; PowerGrid: 40, two chunks
def test_every_critic_unit_and_input_row_sits_where_the_law_says(ni, oracle, key, name):
    """The device's p equals the restatement on all 700 lanes.  Then two hidden units' gamma or beta trade places -- unit r with r ^ 4
    (the other lane half's row of the same register), r ^ 1 (the neighbouring register), r ^ 32 (the same place in the next tile) -- in
    either layer, and two rows of C1 trade places between a state column and an action column: for every unit, the restatement of the
    traded critic disagrees with the device's p of the original; and for one trade of each kind the traded critic, installed on the
    device, gives the traded restatement bit for bit."""
    S, A = _dims(ni, name)
    B, n = M.B_BIG, 8
    cws, cnorms = layout_policy(S + A, 1)
    cws = [cws[0], cws[1], ((cws[2][0] * f32(8)).astype(f32), cws[2][1])]      # (layout_policy's head / 32 is for a tanh; the sigmoid spreads p)
    aw, an = ref.random_ln_actor(S, A, 33)
    x = np.random.default_rng(34).normal(0, 1, (B, S)).astype(f32)

    def device_p(cw, cn):
        pol = ni.LayerNormMLPPolicy(aw, an, safety_weights=cw, safety_norms=cn)
        o = _play_safe(ni, key, name, B, pol, 0.5, n=1, states=x)
        assert np.array_equal(_bits(o["obs"][0]), _bits(x))
        return o["pr"][0], pol
    got, pol = device_p(cws, cnorms)
    raw = ref.act(oracle, aw, an, x, pol.eps)
    assert np.array_equal(_bits(got), _bits(sref.prob(oracle, cws, cnorms, x, raw)))
    assert len(np.unique(got)) > B // 2 and 0.001 < got.min() and got.max() < 0.999
    w, xp = sref.padded(cws, np.concatenate([x, raw], axis=1)[:n])
    _, h1, h2 = ref.pre(w, cnorms, xp, hidden=True)
    assert (h1 > 0).mean() > 0.99 and (h2 > 0).mean() > 0.99 and (h1 > 0).any(axis=0).all() and (h2 > 0).any(axis=0).all()
    survived, on_device = [], []
    for layer in range(2):
        for which in range(2):
            for flip in (4, 1, 32):
                for r in range(256):
                    if r & flip:
                        continue
                    norms = [list(nb) for nb in cnorms]
                    arr = norms[layer][which].copy()
                    arr[[r, r ^ flip]] = arr[[r ^ flip, r]]
                    norms[layer][which] = arr
                    if np.array_equal(_bits(sref.prob(oracle, cws, norms, x[:n], raw[:n])), _bits(got[:n])):
                        survived.append((layer, which, flip, r))
                    if r == 2 + 64 * layer + 8 * which:
                        on_device.append((cws, [tuple(nb) for nb in norms]))
    assert not survived, survived[:8]
    C1 = cws[0][0].copy()
    C1[[1, S + A - 1]] = C1[[S + A - 1, 1]]                    # state column 1 <-> the last action column
    on_device.append(([(C1, cws[0][1]), cws[1], cws[2]], cnorms))
    assert len(on_device) == 13
    for cw, cn in on_device:
        p, _ = device_p(cw, cn)
        assert np.array_equal(_bits(p), _bits(sref.prob(oracle, cw, cn, x, raw))) and not np.array_equal(_bits(p[:n]), _bits(got[:n]))


# ---- 4. slots and refusals -------------------------------------------------------------------------------------------------------
def _raw_install(env, pol, hidden=256, eps=1e-6, null=None, threshold=0.5):
    """nig_set_mlp_safety_ln itself: its return code; `null`: the index of a pointer argument passed as NULL"""
    (W1, b1), (W2, b2), (W3, b3) = [(np.ascontiguousarray(W, dtype=f32), np.ascontiguousarray(b, dtype=f32)) for W, b in pol.safety_weights]
    (g1, e1), (g2, e2) = [(np.ascontiguousarray(g, dtype=f32), np.ascontiguousarray(b, dtype=f32)) for g, b in pol.safety_norms]
    keep = [W1, b1, g1, e1, W2, b2, g2, e2, W3, b3]
    ptrs = [None if i == null else a.ctypes.data_as(C.c_void_p) for i, a in enumerate(keep)]
    with torch.cuda.device(env.device):
        return env._L.nig_set_mlp_safety_ln(env._h, hidden, *ptrs, C.c_float(eps), C.c_float(threshold), env._stream())


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


def test_the_three_critic_installs_replace_each_other(ni):
    key, name, B = "cr", "ChemicalReactor-v0", M.B_BIG
    S, A = 12, 3
    L = ni._lib
    pol, actor, critic = _agent(ni, key, S, A), M.random_actor(S, A, 5), M.random_critic(S, A, 6)
    cat = M.random_critic(S, A, 7, n_out=11)
    ln = lambda env: (env.set_mlp_policy_ln(pol), env.set_mlp_safety_ln(pol, 0.45))
    sig = lambda env: (env.set_mlp_policy(actor), env.set_mlp_safety(critic, 0.5))
    ctg = lambda env: (env.set_mlp_policy(actor), env.set_mlp_safety_categorical(cat, 0.5))
    fresh = {k: _plain_safe(ni, name, B, f) for k, f in (("ln", ln), ("sig", sig), ("cat", ctg))}
    kinds = []

    def chain(*installs):
        def run(env):
            assert env.mlp_safety_kind == L.SAFETY_NONE
            for f in installs:
                f(env)
                kinds.append(env.mlp_safety_kind)
        return run
    other = _agent(ni, key, S, A, cseed=77)
    ln_other = lambda env: (env.set_mlp_policy_ln(pol), env.set_mlp_safety_ln(other, 0.9))      # (another LayerNorm critic first: the slot's image is reused)
    _same(_plain_safe(ni, name, B, chain(sig, ctg, ln_other, ln)), fresh["ln"], names=ALL)
    _same(_plain_safe(ni, name, B, chain(ln, sig)), fresh["sig"], names=ALL)      # after a plain critic replaces it: a fresh handle's plain shield
    _same(_plain_safe(ni, name, B, chain(ln, ctg)), fresh["cat"], names=ALL)
    _same(_plain_safe(ni, name, B, chain(ctg, ln, sig, ln)), fresh["ln"], names=ALL)
    assert kinds == [1, 2, 3, 3, 3, 1, 3, 2, 2, 3, 1, 3]
    assert not np.array_equal(fresh["ln"]["pr"], fresh["sig"]["pr"])
    # installing any actor keeps the critic
    def actors_between(env):
        env.set_mlp_safety_ln(pol, 0.45)
        env.set_mlp_policy(actor)
        env.set_mlp_policy_ln(_policy(ni, key, S, A, seed=8))
        env.set_mlp_policy_ln(pol)
        assert env.mlp_safety_kind == 3
    _same(_plain_safe(ni, name, B, actors_between), fresh["ln"], names=ALL)
    assert ni._lib.lib().nig_get_mlp_safety_kind(None) == -1


def test_a_refused_install_leaves_the_previous_critic_running(ni):
    key, name, B = "cr", "ChemicalReactor-v0", M.B_BIG
    S, A = 12, 3
    pol, actor, critic = _agent(ni, key, S, A), M.random_actor(S, A, 5), M.random_critic(S, A, 6)
    other = _agent(ni, key, S, A, cseed=9)
    ln = lambda env: (env.set_mlp_policy_ln(pol), env.set_mlp_safety_ln(pol, 0.45))
    sig = lambda env: (env.set_mlp_policy(actor), env.set_mlp_safety(critic, 0.5))

    def refused(first):
        def run(env):
            first(env)
            kind = env.mlp_safety_kind
            for eps in (0.0, -1e-6, float("nan"), float("inf"), -float("inf")):
                assert _raw_install(env, other, eps=eps) == INVALID, eps
            for hidden in (128, 255, 512, 0, -256):
                assert _raw_install(env, other, hidden=hidden) == UNSUPPORTED, hidden
            for null in range(10):
                assert _raw_install(env, other, null=null) == INVALID, null
            assert env._L.nig_set_mlp_safety_ln(None, 256, *([None] * 10), C.c_float(1e-6), C.c_float(0.5), None) == INVALID
            assert env.mlp_safety_kind == kind
        return run
    _same(_plain_safe(ni, name, B, refused(ln)), _plain_safe(ni, name, B, ln), names=ALL)
    _same(_plain_safe(ni, name, B, refused(sig)), _plain_safe(ni, name, B, sig), names=ALL)
    water = _make(ni, "WaterTreatment-v0", M.B_SMALL)          # odd state dim: no MFMA actor
    wc = sref.random_ln_critic(water.state_dim, water.action_dim, 1)
    assert _code(lambda: water.set_mlp_safety_ln(wc, 0.5)) == UNSUPPORTED and water.mlp_safety_kind == 0
    water.close()
    # eps is part of the law: another eps, another p
    loose = ni.LayerNormMLPPolicy(pol.weights, pol.norms, safety_weights=pol.safety_weights, safety_norms=pol.safety_norms, safety_eps=1e-2)
    a, b = _plain_safe(ni, name, B, ln, n=1), _plain_safe(ni, name, B, lambda env: (env.set_mlp_policy_ln(loose), env.set_mlp_safety_ln(loose, 0.45)), n=1)
    assert not np.array_equal(a["pr"], b["pr"])


def test_the_readers_of_the_slots_refuse_what_the_family_does_not_reach(ni):
    name, B = "ChemicalReactor-v0", M.B_SMALL
    S, A = 12, 3
    pol = _agent(ni, "cr", S, A)
    env = _make(ni, name, B)
    env.reset()
    env.set_mlp_policy(M.random_actor(S, A, 5))
    env.set_mlp_safety_ln(pol, 0.5)
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
    for entry, call in readers.items():                        # the LayerNorm critic beside a plain actor
        assert _code(call) == UNSUPPORTED, entry
        assert "LayerNorm critic" in env._L.nig_last_error().decode(), (entry, env._L.nig_last_error())
        assert untouched() and env.mlp_safety_kind == 3, entry
    for install in (lambda: env.set_mlp_policy_dims(__import__("mlp_shape_ref").random_actor(S, A, (128, 128), 3)), lambda: env.set_mlp_policy_bf16(M.random_actor(S, A, 5))):
        install()                                              # a shaped actor in the slot; a bf16 actor beside the plain one
        assert _code(readers["rollout_mlp_safe"]) == UNSUPPORTED and untouched()
        env.set_mlp_policy(M.random_actor(S, A, 5))
    env.set_mlp_policy_ln(pol)                                 # LayerNorm actor + LayerNorm critic: the family has no search and no twin
    for entry in ("rollout_mlp_search", "rollout_mlp_safe_limited", "rollout_mlp_search_limited"):
        assert _code(readers[entry]) == UNSUPPORTED and untouched(), entry
    env.rollout_mlp_safe(1, o.rw, o.fl, o.obs, o.act, o.pr)    # positive control: the same buffers run
    assert not o.untouched() and not bool((o.pr[:, :B] == FILL).any()) and env.counter == t0 + 1
    env.close()
    bare = _make(ni, name, B)                                  # LayerNorm actor without a critic
    bare.reset()
    bare.set_mlp_policy_ln(pol)
    ob, tb = SOut(bare, 1), bare.counter
    assert _code(lambda: bare.rollout_mlp_safe(1, ob.rw, ob.fl, ob.obs, ob.act, ob.pr)) == INVALID and ob.untouched() and bare.counter == tb
    bare.close()


# ---- 5. frozen lanes -------------------------------------------------------------------------------------------------------------
def test_frozen_lanes_store_nothing_and_live_lanes_follow_the_law(ni, oracle):
    """test_gpu_mlp_ln's scheme: no auto-reset, B = 5, 7 steps of episodes of at most 5, lanes 1 and 3 held from the start."""
    L = ni._lib
    key, name, B, n = "cr", "ChemicalReactor-v0", M.B_SMALL, T
    pol = _agent(ni, key, 12, 3)
    env = _make(ni, name, B, autoreset=False)
    env.set_mlp_policy_ln(pol)
    s0 = _start(ni, key, env)
    thr = float(f32(_median_p(oracle, pol)(s0)))
    env.set_mlp_safety_ln(pol, thr)
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


# ---- 6. the footprint ------------------------------------------------------------------------------------------------------------
def test_footprint_at_pitches_beyond_ld(ni):
    """One canary arena (tests/footprint.py): B_BIG lanes, every output -- prob_out included -- at a pitch beyond ld and a step stride
    with a gap; pads, stride gaps, the step beyond n_steps and the red zones keep the canary; every documented word is written."""
    key, B, mode = "cr", M.B_BIG, "wide"
    r = Rig(ni, key, B, autoreset=True, max_steps=M.MAXS_NEW)
    S, A, ld, L = r.S, r.A, r.ld, r.L
    pol = _agent(ni, key, S, A)
    r.env.set_mlp_policy_ln(pol)
    r.env.set_mlp_safety_ln(pol, 0.5)
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
    clean(findings, "nig_rollout_mlp_safe with a LayerNorm actor and critic")


# ---- 7. routing ------------------------------------------------------------------------------------------------------------------
class _ShieldLawAgent:
    """The law's shielded actions computed on the host, observation by observation: the agent evaluate_with_safety can only play
    through its per-step host loop -- on exactly the actions the device computes."""
    is_trained = True

    def __init__(self, oracle, pol, thr):
        self.oracle, self.pol, self.thr = oracle, pol, thr

    def predict_device(self, obs):
        return torch.as_tensor(sref.step(self.oracle, self.pol, obs.cpu().numpy(), self.thr)[3], device=obs.device)


def test_evaluate_plays_a_shielded_ln_policy_with_rollout_mlp_safe_and_equals_the_host_loop(ni, oracle):
    key, name, B = "cr", "ChemicalReactor-v0", 64
    pol = _agent(ni, key, 12, 3)
    make = lambda: ni.make_batched(name, B, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    probe = make()
    thr = float(f32(_median_p(oracle, pol)(_start(ni, key, probe))))
    probe.close()
    sh = pol.shielded(thr)
    assert sh.threshold == thr and sh.normalization == "layer_norm" and sh.fusable is True and sh.base is pol
    benv = make()
    agent, rollout, disturbed = ni.utils._install_agent(sh, benv)
    assert agent is sh and disturbed is None and rollout is not None and rollout.__func__ is type(benv).rollout_mlp_safe
    assert benv.mlp_policy_norm is True and benv.mlp_safety_kind == 3
    fused = ni.evaluate_with_safety(sh, benv, n_episodes=B)
    torch.cuda.synchronize()
    assert int(round(float(benv.reduce_tally()[ni._lib.T_EPISODES].item()))) == B
    henv = make()
    law = _ShieldLawAgent(oracle, pol, thr)
    assert ni.utils._install_agent(law, henv)[1] is None
    host = ni.evaluate_with_safety(law, henv, n_episodes=B)
    assert henv.mlp_policy_norm is False and henv.mlp_safety_kind == 0
    _close(fused, host)
    assert 1.0 <= fused["length_mean"] <= M.MAXS_NEW
    bare = make()                                              # the shield is felt: the bare actor plays another round
    unshielded = ni.evaluate_with_safety(pol, bare, n_episodes=B)
    bare.close()
    assert unshielded["return_mean"] != fused["return_mean"]
    e1, e2 = make(), make()
    e_fused = ni.evaluate_episodes(sh, e1, n_episodes=B)
    e_host = ni.evaluate_episodes(law, e2, n_episodes=B)
    assert e1.mlp_safety_kind == 3 and e2.mlp_safety_kind == 0
    e1.close(), e2.close()
    for k in e_fused:
        if k != "launches" and isinstance(e_fused[k], (int, float, np.integer, np.floating)):
            assert e_fused[k] == pytest.approx(e_host[k], rel=1e-12, abs=1e-12), k
    assert e_fused["length_mean"] == fused["length_mean"] and e_fused["return_mean"] == pytest.approx(fused["return_mean"], rel=1e-12)
    benv.close(), henv.close()
    # where the kernel family does not reach -- added constraints, an env without the MFMA actor -- the policy's torch form plays
    lim = make()
    lim.add_safety_constraint(ni.BoxConstraint("cap", {("state", 0): (-1e30, 1e30)}, penalty=0.0))
    assert ni.utils._install_agent(sh, lim)[1] is None
    res = ni.evaluate_with_safety(sh, lim, n_episodes=B)
    assert np.isfinite(res["return_mean"]) and 1.0 <= res["length_mean"] <= M.MAXS_NEW
    lim.close()
    water = ni.make_batched("WaterTreatment-v0", B, tally=True, autoreset=False, max_episode_steps=M.MAXS_NEW, seed=SEED)
    ws, norms = ref.random_ln_actor(water.state_dim, water.action_dim, 1)
    cw, cn = sref.random_ln_critic(water.state_dim, water.action_dim, 2)
    wsh = ni.LayerNormMLPPolicy(ws, norms, safety_weights=cw, safety_norms=cn).shielded(0.5)
    assert ni.utils._install_agent(wsh, water)[1] is None
    res = ni.evaluate_with_safety(wsh, water, n_episodes=B)
    assert np.isfinite(res["return_mean"]) and 1.0 <= res["length_mean"] <= M.MAXS_NEW
    water.close()
