"""not-gpu: the fused shield of shaped agents ("nig-mlp-shape-shield-v1", csrc/nig_mlp_shape_shield.hpp) on the host -- the ABI's
declaration, the critic's operand image (the library's own put_shape_network with IN = S + A, OUT = 1, through
tests/mlp_shape_probe.hip) against an index formula written here, the restated p (tests/mlp_shape_shield_ref.py) against the float64
formula under the derived bound, and where utils._install_agent sends a shielded shaped policy."""
import os

import numpy as np
import pytest

import mlp_shape_ref as ref
import mlp_shape_shield_ref as sref
from conftest import ROOT
from test_mlp_shape_host import probe          # noqa: F401  (the module fixture that compiles and runs the library's builder)

f32 = np.float32
SA = [(12, 3), (32, 8), (28, 10)]


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    return ni


# ---- 1. the ABI --------------------------------------------------------------------------------------------------------------------
def test_the_abi_is_declared_bound_and_exported(ni):
    L = ni._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "nig.h")).read()
    assert "int nig_set_mlp_safety_dims(" in hdr and "int nig_get_mlp_safety_dims(" in hdr
    assert "#define NIG_SAFETY_SIGMOID_SHAPED 4" in hdr and '"nig-mlp-shape-shield-v1"' in hdr
    assert len(ni._lib.PROTOTYPES["nig_set_mlp_safety_dims"][1]) == 7 and len(ni._lib.PROTOTYPES["nig_get_mlp_safety_dims"][1]) == 2
    assert hasattr(L, "nig_set_mlp_safety_dims") and hasattr(L, "nig_get_mlp_safety_dims")
    assert ni._lib.SAFETY_SIGMOID_SHAPED == 4 and hasattr(ni.BatchedIndustrialEnv, "set_mlp_safety_dims")
    assert isinstance(ni.BatchedIndustrialEnv.mlp_safety_dims, property)
    assert L.nig_get_mlp_safety_dims(None, None) == -1
    assert ni.__version__ == "0.8.0" and L.nig_version().decode().startswith("nig 0.8.0")       # the version string stays


# ---- 2. the critic's image ---------------------------------------------------------------------------------------------------------
def _rho(t, hf):
    return (t & 3) + 8 * (t >> 2) + 4 * hf


def _plan(cls, IN):
    """(T, chrec, DP, R, tiles per layer-1 chunk, layer-1 chunks, kch) of class `cls` at IN inputs"""
    T = [d // 32 for d in ref.CLASSES[cls]]
    chrec = -(-(16 * min(8, max(T[:-1])) + 18) // 4) * 4
    DP = IN + (IN & 1)
    R = DP // 2 + 1
    per = T[0]
    while per > 1 and per * R > chrec:
        per //= 2
    return T, chrec, DP, R, per, T[0] // per, [0] + [-(-T[n - 1] // 8) for n in range(1, len(T))]


def _value_at(cls, IN, ws, ch, r, lane):
    """The index formula of the critic's image (OUT = 1): the float at record r, lane `lane` of chunk ch, or 0.0 -- looked up from
    the image's side, one word at a time"""
    T, chrec, DP, R, per, l1c, kch = _plan(cls, IN)
    nh = len(T)
    dims = [W.shape[1] for W, _ in ws[:-1]]
    i, hf = lane & 31, lane >> 5
    if ch < l1c:                                                # layer 1: tile mm of the chunk, record ks of the tile
        mm, ks = divmod(r, R)
        if mm >= per:
            return 0.0
        u = 32 * (ch * per + mm) + i
        if u >= dims[0]:
            return 0.0
        if ks == R - 1:
            return float(ws[0][1][u]) if hf == 0 else 0.0
        k = 2 * ks + hf
        return float(ws[0][0][k, u]) if k < IN else 0.0
    ch -= l1c
    for n in range(1, nh):
        if ch >= T[n] * kch[n]:
            ch -= T[n] * kch[n]
            continue
        m, j = divmod(ch, kch[n])
        kts = min(8, T[n - 1] - 8 * j)
        u = 32 * m + i
        if r < 16 * kts:
            k = 32 * (8 * j + r // 16) + _rho(r % 16, hf)
            return float(ws[n][0][k, u]) if k < dims[n - 1] and u < dims[n] else 0.0
        if j != kch[n] - 1:
            return 0.0
        r -= 16 * kts
        if r == 0:
            return float(ws[n][1][u]) if hf == 0 and u < dims[n] else 0.0
        if n != nh - 1 or (lane & 3) != 0:                      # the one head row sits on lane 4 b of every 4-lane block
            return 0.0
        if r <= 16:
            k = 32 * m + _rho(r - 1, hf)
            return float(ws[nh][0][k, 0]) if k < dims[n] else 0.0
        return float(ws[nh][1][0]) if r == 17 and m == T[n] - 1 else 0.0
    raise AssertionError("chunk beyond the image")


def _integer_critic(IN, dims, seed):
    """exact small-integer weights, every value nonzero: a word of the image is zero only where the law says so"""
    rng = np.random.default_rng(seed)
    ws, K = [], IN
    for H in list(dims) + [1]:
        ws.append((rng.choice(np.arange(1, 200), (K, H)).astype(f32) * rng.choice([-1, 1], (K, H)).astype(f32), rng.choice(np.arange(1, 200), H).astype(f32)))
        K = H
    return ws


def test_the_critics_image_is_put_shape_network_of_s_plus_a_inputs_and_one_output(probe):
    cases = [(cls, S + A, 1, _integer_critic(S + A, ref.CLASSES[cls], seed=S)) for cls in ref.SHIPPED for S, A in SA]
    cases += [("128x128", 15, 1, _integer_critic(15, (96, 64), 3)), ("512x512", 40, 1, _integer_critic(40, (300, 200), 4)),
              ("256x256x256", 38, 1, _integer_critic(38, (200, 150, 100), 5))]                        # padded critics
    res = probe["images"](cases)
    by = {}
    for (cls, IN, _, ws), r in zip(cases, res):
        T, chrec, DP, R, per, l1c, kch = _plan(cls, IN)
        case = (cls, IN, [W.shape for W, _ in ws])
        assert r["ok"], case
        chunks = l1c + sum(T[n] * kch[n] for n in range(1, len(T)))
        assert (r["chrec"], r["l1_rec"], r["l1_tiles"], r["l1_chunks"], r["chunks"], r["floats"]) == (chrec, R, per, l1c, chunks, chunks * chrec * 64), case
        got = r["image"].reshape(chunks, chrec, 64)
        want = np.array([[[_value_at(cls, IN, ws, ch, rr, l) for l in range(64)] for rr in range(chrec)] for ch in (0, l1c - 1, l1c, chunks - 1)], dtype=f32)
        # record by record on the first and last chunk of layer 1, the first chunk behind it and the last chunk (the head's bias) ...
        for n, ch in enumerate((0, l1c - 1, l1c, chunks - 1)):
            same = got[ch].view(np.uint32) == want[n].view(np.uint32)
            assert same.all(), (case, ch, np.argwhere(~same)[:4].tolist())
        # ... and on 4 000 words drawn over the whole image
        rng = np.random.default_rng(IN)
        for ch, rr, l in zip(rng.integers(0, chunks, 4000), rng.integers(0, chrec, 4000), rng.integers(0, 64, 4000)):
            assert got[ch, rr, l] == f32(_value_at(cls, IN, ws, int(ch), int(rr), int(l))), (case, ch, rr, l)
        # every weight of the network is in the image: the hidden layers once, a head weight on the 8 lane blocks of its half
        n_hidden = sum(W.size + b.size for W, b in ws[:-1])
        assert np.count_nonzero(got) == n_hidden + 8 * ws[-1][0].size + 16, case
        if [W.shape[1] for W, _ in ws[:-1]] == list(ref.CLASSES[cls]):
            by[(cls, IN)] = (r, got)
    # the cases the actor's image never met
    r, got = by[("128x128", 40)]
    assert (r["l1_rec"], r["l1_tiles"], r["l1_chunks"], r["chrec"]) == (21, 4, 1, 84) and np.count_nonzero(got[0][:, :32].any(axis=1)) == 84      # 84 of 84 slots
    r, got = by[("512x256", 40)]
    assert (r["l1_tiles"], r["l1_chunks"]) == (4, 4)            # the actor's plan at 32 inputs: 8 tiles in each of 2 chunks
    assert not got[0][84:].any() and got[3][83, :32].all() and not got[3][83, 32:].any()
    actor = probe["images"]([("512x256", 32, 8, _integer_critic(32, (512, 256), 1)[:-1] + [(np.ones((256, 8), f32), np.ones(8, f32))])])[0]
    assert (actor["l1_tiles"], actor["l1_chunks"]) == (8, 2) and actor["chunks"] - 2 == r["chunks"] - 4
    r, got = by[("256x256x256", 40)]
    assert (r["l1_tiles"], r["l1_chunks"]) == (4, 2)
    for cls in ref.SHIPPED:                                     # odd S + A = 15: the zero-padded k-step is record 7's lane half 1
        r, got = by[(cls, 15)]
        assert r["l1_rec"] == 9 and got[0][7, :32].all() and not got[0][7, 32:].any() and got[0][6].all()


# ---- 3. the restated p against the formula in float64 -----------------------------------------------------------------------------
HEAD = 8.0            # the critic's head scale: with it the restatement's p lies inside (0.02, 0.98) on N(0, 1) observations (checked below)


@pytest.mark.parametrize("S,A", SA)
@pytest.mark.parametrize("cls", ref.SHIPPED)
def test_the_restated_p_is_the_formula_within_the_derived_bound(oracle, cls, S, A):
    dims = ref.CLASSES[cls]
    ws = ref.random_actor(S, A, dims, seed=40 + S)
    cw = sref.random_critic(S, A, dims, seed=41 + S, head=HEAD)
    obs = np.random.default_rng(S).normal(0, 1, (4096, S)).astype(f32)
    raw = ref.act(oracle, ws, obs)
    x = np.concatenate([obs, raw], axis=1)
    pre, want = sref.critic_pre(cw, obs, raw), sref.pre64(cw, obs, raw)
    bound = sref.pre_bound(cw, x)
    err = np.abs(pre.astype(np.float64) - want)
    assert np.all(err <= bound), float(np.max(err / bound))
    p = sref.prob(oracle, cw, obs, raw)
    perr = np.abs(p.astype(np.float64) - 1.0 / (1.0 + np.exp(-want)))
    pbound = sref.p_bound(cw, x)
    print(f"{cls:12s} S={S} A={A}: pre error {err.max():.3g} (bound up to {bound.max():.3g}); p error {perr.max():.3g}, largest error / bound "
          f"{np.max(perr / pbound):.3g}; p in [{p.min():.4f}, {p.max():.4f}], {len(np.unique(p))} distinct")
    assert np.all(perr <= pbound), float(np.max(perr / pbound))
    assert len(np.unique(p)) > 2048 and 0.02 < p.min() and p.max() < 0.98, "p says something about its pre-activation"


# ---- 4. the policy's attributes and the routing -----------------------------------------------------------------------------------
def _tree(ws):
    return {"params": {"MLP_0": {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(ws)}}}


class _State:
    def __init__(self, params):
        self.params = params


class _Agent:
    constraint_threshold = 0.3

    def __init__(self, ws, cw):
        self.state = {"actor": _State(_tree(ws)), "safety": _State(_tree(cw))}


def test_install_agent_sends_a_shielded_shaped_policy_to_the_fused_shield(ni):
    import closed_loop_matrix as M
    from neorl_industrial_gym_amd.policies import MLPPolicy, ShieldedMLPPolicy
    from test_limits_families_host import _route
    S, A = 12, 3

    def names(route):
        return route[0], [c[0] for c in route[2]]
    HOST = (None, [])
    for cls, dims in ref.CLASSES.items():
        ws, cw = ref.random_actor(S, A, dims, seed=2), sref.random_critic(S, A, dims, seed=3)
        pol = MLPPolicy(ws, device="cpu", safety_weights=cw, constraint_threshold=0.3)
        sh = pol.shielded()
        assert type(sh) is ShieldedMLPPolicy and pol.shape_shield_exact is True and sh.shape_shield_exact is True
        assert pol.fusable is False and sh.fusable is False and pol.shape_class_exact       # `fusable` keeps its meaning: the 256 x 256 kernels
        route = _route(ni, sh, False)
        if cls in ni.utils.SHAPE_SHIELD_ROUTED:                # the classes whose measurement admits the fused route
            assert names(route) == ("rollout_mlp_safe", ["set_mlp_policy_dims", "set_mlp_safety_dims"]) and route[1] == (7,), (cls, route[:2])
            (_, (aw,)), (_, (sw, thr)) = route[2]
            assert aw is sh.weights and sw is sh.safety_weights and thr == 0.3
        else:                                                  # a class the routing leaves on the host: its C entry point still runs
            assert names(route) == HOST, cls
        assert names(_route(ni, pol, False)) == ("rollout_mlp", ["set_mlp_policy_dims"]), cls                # the bare policy
        assert names(_route(ni, MLPPolicy(ws, device="cpu"), False)) == ("rollout_mlp", ["set_mlp_policy_dims"]), cls
        assert names(_route(ni, sh, True)) == HOST, cls                                                      # added constraints
        assert names(_route(ni, sh, False, plain=False)) == HOST, cls                                        # recorded draws
        assert names(_route(ni, ni.Disturbed(sh, ni.Disturbance(action_noise=0.1), seed=1), False)) == HOST, cls
        # a raw reference agent with a shaped critic: today's route -- from_agent, the unshielded actor
        assert names(_route(ni, _Agent(ws, cw), False)) == ("rollout_mlp", ["set_mlp_policy_dims"]), cls
    # WaterTreatment's shape: no MFMA actor
    odd = MLPPolicy(ref.random_actor(15, 4, (128, 128), seed=2), device="cpu", safety_weights=sref.random_critic(15, 4, (128, 128), seed=3)).shielded()
    assert odd.shape_shield_exact and names(_route(ni, odd, False, state_dim=15, action_dim=4)) == HOST
    # pairs the routing leaves on the host: they run fused where the caller installs both by hand
    a128 = ref.random_actor(S, A, (128, 128), seed=2)
    for what, ws, cw in (("a 256-wide critic beside a (128, 128) actor", a128, M.random_critic(S, A, 6)),
                         ("a (64, 64) pair", ref.random_actor(S, A, (64, 64), seed=2), sref.random_critic(S, A, (64, 64), seed=3)),
                         ("a (512, 256) critic beside a (512, 512) actor", ref.random_actor(S, A, (512, 512), seed=2), sref.random_critic(S, A, (512, 256), seed=3)),
                         ("a (128, 128) critic beside a (256, 256, 256) actor", ref.random_actor(S, A, (256, 256, 256), seed=2), sref.random_critic(S, A, (128, 128), seed=3))):
        sh = MLPPolicy(ws, device="cpu", safety_weights=cw).shielded()
        assert sh.shape_shield_exact is False and sh.base.shape_shield_exact is False and sh.fusable is False, what
        assert names(_route(ni, sh, False)) == HOST, what
    cat = MLPPolicy(a128, device="cpu", safety_weights=ref.random_actor(S + A, 11, (128, 128), seed=4), safety_kind="categorical").shielded()
    assert cat.shape_shield_exact is False and cat.fusable is False and names(_route(ni, cat, False)) == HOST
    # the 256 x 256 routes are the ones they were
    two = MLPPolicy(M.random_actor(S, A, 1), device="cpu", safety_weights=M.random_critic(S, A, 2), constraint_threshold=0.3)
    assert two.fusable is True and two.shape_shield_exact is False and two.shielded().fusable is True and two.shielded().shape_shield_exact is False
    assert names(_route(ni, two.shielded(), False)) == ("rollout_mlp_safe", ["set_mlp_policy", "set_mlp_safety"])
    assert names(_route(ni, two.shielded(), True)) == ("rollout_mlp_safe_limited", ["set_mlp_policy", "set_mlp_safety"])
    assert MLPPolicy(M.random_actor(S, A, 1), device="cpu").shape_shield_exact is False
