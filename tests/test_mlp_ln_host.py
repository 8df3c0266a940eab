"""not-gpu: the LayerNorm MFMA actor ("nig-mlp-ln-v1", csrc/nig_mlp_ln.hpp) on the host -- the restatement of the law's arithmetic
(tests/mlp_ln_ref.c) against a float64 model of the formula under a derived bound, degenerate layers, det_rsqrtf over its whole domain
(tests/rsqrt_check.c), the operand image built by the library's own put_ln_network (tests/mlp_ln_probe.hip, host-only) against the
layout law restated here in NumPy, LayerNormMLPPolicy and its from_agent, and where utils._install_agent sends it.

The layout law (records of 64 floats, lane l = (i = l & 31, hf = l >> 5); chunks of 148 record slots; rho_hf(t) = (t & 3) + 8 (t >> 2)
+ 4 hf; everything not named is +0.0):
  layer 1   input width DP (even); tile m is DP/2 weight records + 1 bias record; eight tiles to one chunk where they fit the slot,
            else four to each of two.  Record ks of tile m, lane (i, hf): W1[2 ks + hf][32 m + i]; the bias record: b1[32 m + i] on half 0.
  layer 2   chunk L1 + m: record 16 kt + t, lane (i, hf): W2[32 kt + rho_hf(t)][32 m + i]; record 128: b2[32 m + i] on half 0.
  head      chunk L1 + 8: record 16 m + t: head row r of hidden row 32 m + rho_hf(t) on lane 4 b + r of every 4-lane block (OUT <= 4) or
            lane 16 b + r of every 16-lane block, r < OUT; record 128: b3[r] on the same lanes.
  table     behind the last chunk: entry (((layer 2 + which) 2 + hf) 8 + m) 16 + t = (which ? beta : gamma)_layer[32 m + rho_hf(t)]."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import closed_loop_matrix as M
import mlp_ln_ref as ref
from conftest import ROOT

f32 = np.float32


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    return ni


# ---- 1. the restatement against the formula in float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ref.fidelity_cases()), ids=lambda c: c[0].replace(" ", "_"))
def test_the_restatement_is_the_formula_within_the_derived_bound(oracle, case):
    label, S, A, ws, norms, obs = case
    m = ref.model64(ws, norms, obs)
    pre = ref.pre(ws, norms, obs)
    bound = ref.pre_bound(m, S)
    err = np.abs(pre.astype(np.float64) - m["pre"])
    print(f"{label}: head pre-activation error {err.max():.3g}, largest error / bound {np.max(err / bound):.3g}, bound up to {bound.max():.3g}")
    assert np.all(err <= bound), (label, float(np.max(err / bound)))
    act = oracle.detmath_unary("tanhf", pre)
    assert M.worst(f"{label}: actions", act, m["action"], M.ACT_ATOL) <= 1.0
    assert M.distinct_rows(act) == len(act) and (np.abs(act) < 0.999).mean() > 0.5, "the actions say something about their pre-activations"


# ---- 2. degenerate layers --------------------------------------------------------------------------------------------------------------
def test_with_zero_weights_every_unit_is_the_bias_constant_and_the_layer_is_relu_of_beta():
    """W = 0: z is the bias constant in every unit (a constant with a short significand, so that every partial sum of the mean is
    exact), d = 0 exactly, y = fma(0, rs gamma, beta) = beta, h = max(beta, 0) whatever gamma is."""
    S, A = 12, 3
    ws, norms = ref.random_ln_actor(S, A, 3)
    obs = np.random.default_rng(1).normal(0, 1, (64, S)).astype(f32)
    flat = [(np.zeros_like(ws[0][0]), np.full(256, 0.375, dtype=f32)), (np.zeros_like(ws[1][0]), np.full(256, -1.5, dtype=f32)), ws[2]]
    pre, h1, h2 = ref.pre(flat, norms, obs, hidden=True)
    assert np.array_equal(h1, np.broadcast_to(np.maximum(norms[0][1], f32(0)), h1.shape))
    assert np.array_equal(h2, np.broadcast_to(np.maximum(norms[1][1], f32(0)), h2.shape))
    assert (norms[1][1] > 0).sum() > 64 and len(np.unique(pre, axis=0)) == 1 and np.abs(pre).max() > 0


def test_on_an_observation_of_zeros_the_output_is_the_law_on_the_biases_alone():
    S, A = 32, 8
    ws, _ = ref.random_ln_actor(S, A, 4)
    plain = [(np.ones(256, dtype=f32), np.zeros(256, dtype=f32))] * 2
    biases_alone = [(np.zeros_like(ws[0][0]), ws[0][1]), ws[1], ws[2]]
    obs = np.random.default_rng(2).normal(0, 1, (8, S)).astype(f32)
    want = ref.pre(biases_alone, plain, obs)
    got = ref.pre(ws, plain, np.zeros((8, S), dtype=f32))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.abs(got).max() > 0
    m = ref.model64(ws, plain, np.zeros((1, S)))
    assert np.abs(got[0] - m["pre"][0]).max() <= ref.pre_bound(m, S).max()


# ---- 3. det_rsqrtf ---------------------------------------------------------------------------------------------------------------------
def test_rsqrtf_over_every_positive_normal_float(tmp_path):
    """tests/rsqrt_check.c: the restatement (IEEE sqrt, IEEE division; the device's bits: test_gpu_rsqrt.py) against 1 / sqrtl in long
    double on all 254 x 2^23 inputs.  Measured worst error 1.490349 ulp (at 0x1.019566p+2, just above a power of four, where the
    result lies just below a power of two): asserted at the next half ulp, the figure in DESIGN.md section 4."""
    exe = tmp_path / "rsqrt_check"
    subprocess.run(["gcc", "-O2", "-std=gnu11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-mfma", "-o", str(exe),
                    os.path.join(ROOT, "tests", "rsqrt_check.c"), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr
    name, worst, bad, n, at = out.stdout.split()
    print(out.stdout.strip())
    assert name == "rsqrtf.normal" and int(n) == 254 * 2 ** 23 and int(bad) == 0
    assert 1.0 < float(worst) <= 1.5, (worst, at)
    x = np.array([1.0, 4.0, 0.25, 16.0, 1e-6, 2.0 ** -126, 2.0 ** 127], dtype=f32)
    assert np.array_equal(ref.rsqrt(x), (f32(1) / np.sqrt(x)).astype(f32))          # (NumPy's sqrt and division are IEEE's as well)
    assert np.array_equal(ref.rsqrt(x[:4]), np.array([1.0, 0.5, 2.0, 0.25], dtype=f32))


# ---- 4. the operand image --------------------------------------------------------------------------------------------------------------
def _rho(t, hf):
    return (t & 3) + 8 * (t >> 2) + 4 * hf


def _law_image(IN, OUT, a):
    """The layout law of this module's docstring, in NumPy, from the ten arrays a = W1, b1, g1, be1, W2, b2, g2, be2, W3, b3."""
    W1, b1, g1, be1, W2, b2, g2, be2, W3, b3 = a
    DP = (IN + 1) & ~1
    records = DP // 2 + 1
    L1 = 1 if 8 * records <= 148 else 2
    tiles = 8 // L1
    chunks = L1 + 8 + 1
    img = np.zeros(chunks * 148 * 64 + 1024, dtype=f32)
    rec = lambda ch, r: img[(ch * 148 + r) * 64:(ch * 148 + r + 1) * 64]
    lanes = np.arange(64)
    i, hf = lanes & 31, lanes >> 5
    for m in range(8):
        ch, base = m // tiles, (m % tiles) * records
        for ks in range(DP // 2):
            k = 2 * ks + hf
            rec(ch, base + ks)[k < IN] = W1[k[k < IN], 32 * m + i[k < IN]]
        rec(ch, base + DP // 2)[:32] = b1[32 * m:32 * m + 32]
    for m in range(8):
        for kt in range(8):
            for t in range(16):
                rec(L1 + m, 16 * kt + t)[:] = W2[32 * kt + _rho(t, hf), 32 * m + i]
        rec(L1 + m, 128)[:32] = b2[32 * m:32 * m + 32]
    row = 3 if OUT <= 4 else 15
    on = (lanes & row) < OUT
    for m in range(8):
        for t in range(16):
            rec(L1 + 8, 16 * m + t)[on] = W3[32 * m + _rho(t, hf[on]), (lanes & row)[on]]
    rec(L1 + 8, 128)[on] = b3[(lanes & row)[on]]
    tab = img[chunks * 148 * 64:]
    for layer, (g, be) in enumerate(((g1, be1), (g2, be2))):
        for which, arr in enumerate((g, be)):
            for h in range(2):
                for m in range(8):
                    for t in range(16):
                        tab[(((layer * 2 + which) * 2 + h) * 8 + m) * 16 + t] = arr[32 * m + _rho(t, h)]
    return img, (L1, tiles, records, chunks, L1 + 8, chunks * 148 * 64)


def _tagged(IN, OUT):
    """Every weight, bias, gamma and beta a float32 integer of its own: array number x 2^20 + index (all below 2^24)."""
    shapes = [(IN, 256), (256,), (256,), (256,), (256, 256), (256,), (256,), (256,), (256, OUT), (OUT,)]
    out = [((n + 1) * 2 ** 20 + np.arange(int(np.prod(s)))).astype(f32).reshape(s) for n, s in enumerate(shapes)]
    assert len(np.unique(np.concatenate([x.ravel() for x in out]))) == sum(x.size for x in out)
    return out


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mlp_ln")
    hipcc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert hipcc, "hipcc not found: the probe is the library's own header, compiled for the host"
    exe = tmp / "mlp_ln_probe"
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc"),
                    "-o", str(exe), os.path.join(ROOT, "tests", "mlp_ln_probe.hip")], check=True)

    def image(IN, OUT, arrays):
        np.concatenate([x.ravel() for x in arrays]).astype(f32).tofile(tmp / "w.bin")
        out = subprocess.run([str(exe)], input=f"N {IN} {OUT} {tmp / 'w.bin'} {tmp / 'i.bin'}\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.returncode, out.stderr)
        vals = [int(x) for x in out.stdout.split()]
        return vals[0], tuple(vals[1:7]), vals[7], np.fromfile(tmp / "i.bin", dtype=f32)
    return image


@pytest.mark.parametrize("IN,OUT", [(12, 3), (32, 8), (28, 10), (18, 5), (36, 4), (24, 16)])
def test_the_image_holds_every_value_at_the_position_the_header_states(probe, IN, OUT):
    """Tagged values: the whole image, bit for bit, against the layout law -- every weight, bias, gamma and beta once (the head's rows
    once per lane block), zeros elsewhere.  (36, 4): a layer 1 of two chunks, which no env has and the builder supports."""
    arrays = _tagged(IN, OUT)
    want, plan = _law_image(IN, OUT, arrays)
    ok, got_plan, floats, img = probe(IN, OUT, arrays)
    assert ok == 1 and got_plan == plan and floats == want.size == img.size
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
    blocks = 16 if OUT <= 4 else 4                                   # lane blocks of a record: a head weight sits in those of its lane half
    for n, x in enumerate(arrays):
        times = {8: blocks // 2, 9: blocks}.get(n, 1)
        assert np.array_equal(np.sort(img[np.isin(img, x)]), np.sort(np.tile(x.ravel(), times))), n
    assert plan[0] == (2 if IN == 36 else 1)


# ---- 5. the policy class ---------------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self, params):
        self.params = params


class _Agent:
    def __init__(self, ws, norms):
        mlp = {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(ws)}
        mlp.update({f"LayerNorm_{i}": {"scale": g, "bias": b} for i, (g, b) in enumerate(norms) if g is not None})
        self.state = {"actor": _State({"params": {"MLP_0": mlp}})}


def test_from_agent_reads_both_layer_norms_and_refuses_anything_else(ni):
    S, A = 12, 3
    ws, norms = ref.random_ln_actor(S, A, 5)
    assert "LayerNormMLPPolicy" in ni.__all__ and ni.LayerNormMLPPolicy is ni.policies.LayerNormMLPPolicy
    pol = ni.LayerNormMLPPolicy.from_agent(_Agent(ws, norms), device="cpu")
    assert pol.fusable is True and pol.hidden_dims == (256, 256) and pol.eps == 1e-6 and (pol.state_dim, pol.action_dim) == (S, A)
    assert all(np.array_equal(W, V) and np.array_equal(b, c) for (W, b), (V, c) in zip(pol.weights, ws))
    assert all(np.array_equal(g, G) and np.array_equal(b, Bb) for (g, b), (G, Bb) in zip(pol.norms, norms))
    with pytest.raises(ValueError, match="LayerNorm"):                       # the plain class keeps refusing the same tree
        ni.MLPPolicy.from_agent(_Agent(ws, norms), device="cpu")
    for one_layer in ([norms[0], (None, None)], [(None, None), norms[1]], [(None, None), (None, None)]):
        with pytest.raises(ValueError):
            ni.LayerNormMLPPolicy.from_agent(_Agent(ws, one_layer), device="cpu")
    no_bias = _Agent(ws, norms)
    del no_bias.state["actor"].params["params"]["MLP_0"]["LayerNorm_1"]["bias"]
    with pytest.raises(ValueError):
        ni.LayerNormMLPPolicy.from_agent(no_bias, device="cpu")
    import mlp_shape_ref
    for dims in ((128, 128), (256, 128), (512, 256), (256, 256, 256)):
        wide = mlp_shape_ref.random_actor(S, A, dims, 2)
        wn = [(np.ones(d, dtype=f32), np.zeros(d, dtype=f32)) for d in dims]
        with pytest.raises(ValueError):
            ni.LayerNormMLPPolicy.from_agent(_Agent(wide, wn), device="cpu")
    for eps in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ni.LayerNormMLPPolicy(ws, norms, eps=eps, device="cpu")


def test_predict_is_the_formula(ni):
    S, A = 28, 10
    ws, norms = ref.random_ln_actor(S, A, 6)
    obs = np.random.default_rng(3).normal(0, 1, (256, S)).astype(f32)
    pol = ni.LayerNormMLPPolicy(ws, norms, device="cpu")
    got = pol.predict(obs)
    assert got.shape == (256, A) and got.dtype == f32 and pol.predict(obs[0]).shape == (A,)
    assert M.worst("torch host form against the float64 model", got, ref.model64(ws, norms, obs)["action"], 2e-5) <= 1.0


# ---- 6. the ABI and the routing ---------------------------------------------------------------------------------------------------------
def test_the_abi_is_declared_bound_and_exported(ni):
    L = ni._lib.lib()
    hdr = open(os.path.join(ROOT, "include", "nig.h")).read()
    for name, n_args in (("nig_set_mlp_policy_ln", 14), ("nig_get_mlp_policy_norm", 1)):
        assert ("int %s(" % name) in hdr and name in ni._lib.PROTOTYPES and hasattr(L, name), name
        assert len(ni._lib.PROTOTYPES[name][1]) == n_args
    assert hasattr(ni.BatchedIndustrialEnv, "set_mlp_policy_ln") and hasattr(ni.BatchedIndustrialEnv, "mlp_policy_norm")
    assert L.nig_get_mlp_policy_norm(None) == -1
    assert ni.__version__ == "0.8.0" and L.nig_version().decode().startswith("nig 0.8.0")


def test_install_agent_sends_only_the_explicit_policy_to_set_mlp_policy_ln(ni):
    from test_limits_families_host import _route
    S, A = 12, 3
    ws, norms = ref.random_ln_actor(S, A, 7)
    pol = ni.LayerNormMLPPolicy(ws, norms, device="cpu")

    def names(route):
        return route[0], [c[0] for c in route[2]]
    assert names(_route(ni, pol, False)) == ("rollout_mlp", ["set_mlp_policy_ln"])
    assert _route(ni, pol, False)[1] == (7,) and _route(ni, pol, False)[2][0][1] == (pol,)
    assert names(_route(ni, pol, True)) == (None, [])                                   # added constraints: the host loop
    assert names(_route(ni, _Agent(ws, norms), False)) == (None, [])                    # a raw LayerNorm agent: the host loop, as before
    assert names(_route(ni, _Agent(ws, norms), True)) == (None, [])
    assert names(_route(ni, pol, False, plain=False)) == (None, [])                     # recorded draws
    assert names(_route(ni, ni.Disturbed(pol, ni.Disturbance(action_noise=0.1), seed=1), False)) == (None, [])
    odd = ni.LayerNormMLPPolicy(*ref.random_ln_actor(15, 4, 8), device="cpu")
    assert names(_route(ni, odd, False, state_dim=15, action_dim=4)) == (None, [])      # WaterTreatment's shape: no MFMA actor
    plain = ni.MLPPolicy(ws, device="cpu")                                              # the 256 x 256 route is the one it was
    assert names(_route(ni, plain, False)) == ("rollout_mlp", ["set_mlp_policy"])
