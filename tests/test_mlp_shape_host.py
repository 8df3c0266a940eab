"""not-gpu: the shaped MFMA actor ("nig-mlp-shape-v1", include/nig.h) on the host -- the class table, the operand image built by the
library's own put_shape_network (tests/mlp_shape_probe.hip, host-only) against the layout law restated here in NumPy, the
restatement of the law's arithmetic (tests/mlp_shape_ref.c) against a float64 network under a derived bound, padding, and loading
a four-Dense actor tree.

The layout law (records of 64 floats, lane l = (i = l & 31, hf = l >> 5); chunks of `chrec` record slots, chrec = 84 for the class
128x128 and 148 elsewhere; everything not named is +0.0), T[n] = padded width of hidden layer n / 32:
  layer 1   input padded to the even width DP; tile m is DP/2 weight records + 1 bias record; tiles lie back to back, as many to a
            chunk (a power of two) as fit the slot.  Record ks of tile m, lane (i, hf): W1[2 ks + hf][32 m + i]; the bias record:
            b1[32 m + i] on lane half 0.
  layer n   output tile m takes 1 chunk where the layer below has at most 8 tiles and 2 where it has 16; chunk j of the tile:
            records 16 (kt - 8 j) + t for kt in [8 j, 8 j + 8), lane (i, hf): Wn[32 kt + rho_hf(t)][32 m + i], rho_hf(t) = (t & 3) +
            8 (t >> 2) + 4 hf; the tile's last chunk: the bias record behind them, bn[32 m + i] on lane half 0.
  head      behind the bias record of the LAST hidden layer's tile m: 16 records, record t: head row r of hidden row 32 m + rho_hf(t)
            on lane 4 b + r of every 4-lane block (OUT <= 4) or lane 16 b + r of every 16-lane block, r < OUT; the head's bias b[r]
            on the same lanes of the record behind the last chunk's head records.
One host-only compile of each probe and one run per module."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mlp_shape_ref as ref
from closed_loop_matrix import ACT_ATOL, mlp64
from conftest import ROOT

f32 = np.float32
KIND = {"reference": 1, "128x128": 2, "512x256": 3, "512x512": 4, "256x256x256": 5}
NAME = {v: k for k, v in KIND.items()}
PADDED = dict(ref.CLASSES, reference=(256, 256))
U = 2.0 ** -24                                     # float32 unit roundoff


def _indexed(IN, OUT, dims):
    """weights equal to their own flat index (from 1, all layers counted through): every value distinct, exact in float32"""
    ws, n, ins = [], 1, IN
    for out in list(dims) + [OUT]:
        W = np.arange(n, n + ins * out, dtype=np.float64).reshape(ins, out).astype(f32)
        n += ins * out
        b = np.arange(n, n + out, dtype=np.float64).astype(f32)
        n += out
        ws.append((W, b))
        ins = out
    assert n < 2 ** 24
    return ws


def _law(cls, IN, OUT, ws):
    """-> the image [chunks][chrec][64] of the network `ws` (unpadded) in class `cls`"""
    T = [d // 32 for d in PADDED[cls]]
    nh = len(T)
    dims = [W.shape[1] for W, _ in ws[:-1]]
    chrec = -(-(16 * min(8, max(T[:-1])) + 18) // 4) * 4
    DP = IN + (IN & 1)
    R = DP // 2 + 1
    per = T[0]
    while per > 1 and per * R > chrec:
        per //= 2
    kch = [0] + [-(-T[n - 1] // 8) for n in range(1, nh)]
    chunks = T[0] // per + sum(T[n] * kch[n] for n in range(1, nh))
    img = np.zeros((chunks, chrec, 64), dtype=f32)

    def padded(W, rows, cols):
        P = np.zeros((rows, cols), dtype=f32)
        P[:W.shape[0], :W.shape[1]] = W
        return P
    i = np.arange(32)
    W1, b1 = padded(ws[0][0], DP, 32 * T[0]), padded(ws[0][1][None, :], 1, 32 * T[0])[0]
    for m in range(T[0]):
        ch, base = divmod(m, per)
        base *= R
        for ks in range(DP // 2):
            for hf in (0, 1):
                img[ch, base + ks, 32 * hf + i] = W1[2 * ks + hf, 32 * m + i]
        img[ch, base + DP // 2, i] = b1[32 * m + i]
    ch = T[0] // per
    lane = np.arange(64)
    block = 4 if OUT <= 4 else 16
    row, hf_of = lane % block, lane // 32
    on = row < OUT
    for n in range(1, nh):
        Wn, bn = padded(ws[n][0], 32 * T[n - 1], 32 * T[n]), padded(ws[n][1][None, :], 1, 32 * T[n])[0]
        Wh = padded(ws[nh][0], 32 * T[nh - 1], OUT)
        for m in range(T[n]):
            for j in range(kch[n]):
                r = 0
                for kt in range(8 * j, min(8 * j + 8, T[n - 1])):
                    for t in range(16):
                        for hf in (0, 1):
                            img[ch, r, 32 * hf + i] = Wn[32 * kt + (t & 3) + 8 * (t >> 2) + 4 * hf, 32 * m + i]
                        r += 1
                if j == kch[n] - 1:
                    img[ch, r, i] = bn[32 * m + i]
                    r += 1
                    if n == nh - 1:
                        for t in range(16):
                            rho = (t & 3) + 8 * (t >> 2) + 4 * hf_of
                            img[ch, r, lane[on]] = Wh[32 * m + rho[on], row[on]]
                            r += 1
                        if m == T[n] - 1:
                            img[ch, r, lane[on]] = ws[nh][1][row[on]]
                ch += 1
    assert ch == chunks
    return img


def _hipcc():
    hipcc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert hipcc, "hipcc not found: the probe is the library's own header, compiled for the host"
    return hipcc


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mlp_shape")
    exes = {}
    for name in ("mlp_shape_probe", "mlp_stream_probe"):
        exes[name] = tmp / name
        subprocess.run([_hipcc(), "--cuda-host-only", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc"),
                        "-o", str(exes[name]), os.path.join(ROOT, "tests", name + ".hip")], check=True)

    def run(exe, lines):
        out = subprocess.run([str(exes[exe])], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.returncode, out.stderr)
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return got

    def classes(cases):
        """[(S, dims)] -> the library's class name or None for each"""
        lines = [f"C {S} {len(d)} " + " ".join(str(x) for x in (list(d) + [0, 0, 0])[:3]) for S, d in cases]
        return [NAME.get(int(x)) for x in run("mlp_shape_probe", lines)]

    def images(cases):
        """[(class name, IN, OUT, ws)] -> [dict(ok, chrec, ..., image)]"""
        lines = []
        for n, (cls, IN, OUT, ws) in enumerate(cases):
            np.concatenate([a.ravel() for pair in ws for a in pair]).astype(f32).tofile(tmp / f"w{n}.bin")
            d = [W.shape[1] for W, _ in ws[:-1]]
            lines.append(f"N {KIND[cls]} {IN} {OUT} {len(d)} " + " ".join(str(x) for x in (d + [0, 0, 0])[:3]) + f" {tmp / f'w{n}.bin'} {tmp / f'i{n}.bin'}")
        res = []
        for n, l in enumerate(run("mlp_shape_probe", lines)):
            ok, chrec, l1_rec, l1_tiles, l1_chunks, k2, k3, chunks, floats = (int(x) for x in l.split())
            res.append(dict(ok=bool(ok), chrec=chrec, l1_rec=l1_rec, l1_tiles=l1_tiles, l1_chunks=l1_chunks, kch=(k2, k3), chunks=chunks,
                            floats=floats, image=np.fromfile(tmp / f"i{n}.bin", dtype=f32)))
        return res

    def reference_image(IN, OUT, ws256):
        """put_network's image (MLP_STREAM_FLOATS floats) of the 256-wide network, by the existing probe"""
        floats = 9 * 148 * 64
        np.concatenate([a.ravel() for pair in ws256 for a in pair]).astype(f32).tofile(tmp / "wr.bin")
        got = run("mlp_stream_probe", [f"N {IN} {OUT} {floats} {tmp / 'wr.bin'} {tmp / 'ir.bin'}"])
        assert got[0].split()[0] == "1"
        return np.fromfile(tmp / "ir.bin", dtype=f32)
    return dict(classes=classes, images=images, reference_image=reference_image)


CLASS_TABLE = [((128, 128), "128x128"), ((256, 256), "reference"), ((512, 256), "512x256"), ((256, 256, 256), "256x256x256"),
               ((512, 512), "512x512"),                                      # the tuner's five
               ((64, 64), "128x128"), ((200, 200), "reference"), ((400, 300), "512x512"), ((256, 512), "512x512"), ((300, 256), "512x256"),
               ((128, 128, 64), "256x256x256"), ((129, 128), "reference"), ((128, 129), "reference"), ((257, 256), "512x256"),
               ((513, 256), None), ((256,), None), ((256,) * 4, None), ((512, 512, 512), None), ((0, 128), None)]


def test_class_table_python_and_library_agree(probe):
    import neorl_industrial_gym_amd as ni
    for dims, want in CLASS_TABLE:
        assert ni.policies.actor_shape_class(dims) == want, dims
    lib_cases = [(S, d) for d, _ in CLASS_TABLE if 1 <= len(d) <= 3 for S in (12, 32)]
    got = probe["classes"](lib_cases)
    for (S, d), g in zip(lib_cases, got):
        assert g == dict(CLASS_TABLE)[d], (S, d, g)


def test_image_is_the_law_bit_for_bit(probe):
    cases = []
    for cls in ref.SHIPPED:
        for S in (6, 12, 20):
            for A in (2, 8):
                cases.append((cls, S, A, _indexed(S, A, ref.CLASSES[cls])))
    cases += [("128x128", 32, 8, _indexed(32, 8, (96, 64))), ("512x512", 32, 8, _indexed(32, 8, (300, 200))),      # padded networks; S = 32:
              ("512x256", 24, 7, _indexed(24, 7, (300, 256))), ("256x256x256", 28, 10, _indexed(28, 10, (128, 128, 64)))]   # layer 1 in two chunks
    res = probe["images"](cases)
    assert {r["l1_chunks"] for r in res} == {1, 2} and {r["chrec"] for r in res} == {84, 148} and {r["kch"] for r in res} == {(1, 0), (2, 0), (1, 1)}
    for (cls, S, A, ws), r in zip(cases, res):
        case = (cls, S, A, [W.shape for W, _ in ws])
        assert r["ok"], case
        want = _law(cls, S, A, ws)
        assert r["chunks"] == want.shape[0] and r["chrec"] == want.shape[1] and r["floats"] == want.size, case
        got = r["image"].reshape(want.shape)
        same = got.view(np.uint32) == want.view(np.uint32)
        assert same.all(), (case, np.argwhere(~same)[:4].tolist())
        # every weight and bias of the hidden layers exactly once; a head weight once per lane block of its lane half, the head's bias
        # once per lane block of both halves (the kernel multiplies half 1's by 0); everything else zero
        vals, counts = np.unique(got[got != 0], return_counts=True)
        n_layers = sum(W.size + b.size for W, b in ws[:-1])
        blocks = 64 // (4 if A <= 4 else 16)
        assert len(vals) == n_layers + ws[-1][0].size + A and np.array_equal(vals, np.arange(1, len(vals) + 1, dtype=f32)), case
        assert (counts[:n_layers] == 1).all() and (counts[n_layers:-A] == blocks // 2).all() and (counts[-A:] == blocks).all(), case


def test_reference_class_image_is_put_networks_of_the_padded_arrays(probe):
    import neorl_industrial_gym_amd as ni
    for S, A, dims in ((12, 3, (200, 200)), (32, 8, (129, 7)), (20, 6, (256, 256))):
        ws = ref.random_actor(S, A, dims, seed=31)
        r = probe["images"]([("reference", S, A, ws)])[0]
        assert r["ok"]
        want = probe["reference_image"](S, A, ni.policies.pad_actor(ws, (256, 256)))
        assert r["image"].size == want.size and np.array_equal(r["image"].view(np.uint32), want.view(np.uint32)), (S, A, dims)


def _bound(ws, x):
    """The forward-error bound of the law's float32 evaluation against exact arithmetic, per sample and head row: a chain of n
    fused multiply-adds into one accumulator satisfies |fl - exact| <= gamma_n sum |w_k| |x_k|, gamma_n = n u / (1 - n u), u = 2^-24
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; one rounding per term).  A hidden unit is a chain of K + 1
    terms (the bias last); ReLU is 1-Lipschitz; an input error e_k enters the next layer as sum |w_k| e_k, and the computed
    activations are bounded by the exact ones plus e.  The head is two chains of at most K / 2 + 1 terms and one add: gamma_{K/2+2}."""
    g = lambda n: n * U / (1 - n * U)
    h = np.abs(np.asarray(x, dtype=np.float64))
    e = np.zeros_like(h)
    z = np.asarray(x, dtype=np.float64)
    for i, (W, b) in enumerate(ws):
        W, b = np.asarray(W, dtype=np.float64), np.asarray(b, dtype=np.float64).reshape(-1)
        K = W.shape[0]
        terms = K + 1 if i + 1 < len(ws) else K // 2 + 2
        mag = (np.abs(z) + e) @ np.abs(W) + np.abs(b)
        e = e @ np.abs(W) + g(terms) * mag
        z = z @ W + b
        if i + 1 < len(ws):
            z = np.maximum(z, 0)
    return e


FIDELITY_SHAPES = [("128x128", (128, 128)), ("reference", (256, 256)), ("512x256", (512, 256)), ("512x512", (512, 512)),
                   ("256x256x256", (256, 256, 256))]


def test_restatement_against_float64_under_the_derived_bound():
    import oracle.oracle as oracle
    rng = np.random.default_rng(5)
    for S, A in ((12, 3), (32, 8)):
        obs = rng.normal(0, 1, (64, S)).astype(f32)
        for cls, dims in FIDELITY_SHAPES:
            ws = ref.random_actor(S, A, dims, seed=17)
            got = ref.pre(ws, obs)
            want = ref.pre64(ws, obs)
            if len(dims) == 2:
                assert np.array_equal(want, mlp64(ws, obs))          # (the matrix's float64 network, where it has the depth)
            err, bound = np.abs(got.astype(np.float64) - want), _bound(ws, obs)
            print(f"{cls:12s} S {S:2d} A {A}: largest |pre - pre64| = {err.max():.3g}, derived bound at that element = "
                  f"{bound.flat[err.argmax()]:.3g}, largest bound = {bound.max():.3g}, worst error / bound = {(err / bound).max():.3g}")
            assert (err <= bound).all(), (cls, S)
            if cls == "reference":
                a_err = np.abs(oracle.detmath_unary("tanhf", got).astype(np.float64) - np.tanh(want)).max()
                print(f"{cls:12s} S {S:2d} A {A}: largest action error = {a_err:.3g} (ACT_ATOL {ACT_ATOL:g})")
                assert a_err <= ACT_ATOL


@pytest.mark.parametrize("dims", [(96, 64), (300, 200), (128, 128, 64)])
def test_padding_changes_no_value(dims):
    import neorl_industrial_gym_amd as ni
    cls = ni.policies.actor_shape_class(dims)
    assert cls in ref.CLASSES
    rng = np.random.default_rng(9)
    for S, A in ((12, 3), (28, 10)):
        ws = ref.random_actor(S, A, dims, seed=23)
        padded = ni.policies.pad_actor(ws, ref.CLASSES[cls])
        assert [W.shape[1] for W, _ in padded[:-1]] == list(ref.CLASSES[cls])
        obs = rng.normal(0, 1, (32, S)).astype(f32)
        assert (ref.pre(ws, obs) == ref.pre(padded, obs)).all()       # (==: the sign of a zero aside)
        assert np.abs(ref.pre(ws, obs)).min() > 0


def test_pad_actor_refuses_what_does_not_fit():
    import neorl_industrial_gym_amd as ni
    ws = ref.random_actor(12, 3, (96, 64), seed=1)
    with pytest.raises(ValueError):
        ni.policies.pad_actor(ws, (64, 64))
    with pytest.raises(ValueError):
        ni.policies.pad_actor(ws, (128, 128, 128))


def _tree(ws):
    return {"params": {"MLP_0": {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(ws)}}}


class _State:
    def __init__(self, params):
        self.params = params


class _Agent:
    def __init__(self, ws):
        self.state = {"actor": _State(_tree(ws))}


def test_from_agent_reads_a_four_dense_actor():
    import neorl_industrial_gym_amd as ni
    ws = ref.random_actor(12, 3, (256, 256, 256), seed=3)
    pol = ni.policies.MLPPolicy.from_agent(_Agent(ws), device="cpu")
    assert pol.hidden_dims == (256, 256, 256) and pol.fusable is False and pol.shape_class == "256x256x256"
    assert all(np.array_equal(W, V) and np.array_equal(b, c) for (W, b), (V, c) in zip(pol.weights, ws))
    two = ni.policies.MLPPolicy.from_agent(_Agent(ref.random_actor(12, 3, (256, 256), seed=3)), device="cpu")
    assert two.hidden_dims == (256, 256) and two.fusable is True and two.shape_class == "reference"
    tree = _tree(ws)
    tree["params"]["MLP_0"]["LayerNorm_0"] = {"scale": np.ones(256, dtype=f32), "bias": np.zeros(256, dtype=f32)}
    bad = _Agent(ws)
    bad.state = {"actor": _State(tree)}
    with pytest.raises(ValueError):
        ni.policies.MLPPolicy.from_agent(bad, device="cpu")


def test_install_agent_sends_a_shaped_actor_to_set_mlp_policy_dims():
    """utils._install_agent on a recording stand-in of the env (test_limits_families_host.StubEnv): a plain MLPPolicy whose hidden
    widths are a shaped class's own, and a reference agent MLPPolicy.from_agent reads into one, go to set_mlp_policy_dims +
    rollout_mlp on an MFMA env without added constraints; with constraints, wrapped, under bf16, on an env without the MFMA actor or
    with recorded draws they keep the host loop.  A network that needs padding keeps the host loop, as it did (it runs fused where the
    caller installs it with set_mlp_policy_dims), and the 256 x 256 routes are the ones they were."""
    import neorl_industrial_gym_amd as ni
    from neorl_industrial_gym_amd.policies import MLPPolicy
    from test_limits_families_host import _route
    S, A = 12, 3

    def names(route):
        return route[0], [c[0] for c in route[2]]
    for dims in ref.CLASSES.values():
        ws = ref.random_actor(S, A, dims, seed=2)
        pol = MLPPolicy(ws, device="cpu")
        assert pol.shape_class_exact and not pol.fusable, dims
        assert names(_route(ni, pol, False)) == ("rollout_mlp", ["set_mlp_policy_dims"]), dims
        assert names(_route(ni, _Agent(ws), False)) == ("rollout_mlp", ["set_mlp_policy_dims"]), dims
        assert names(_route(ni, pol, True)) == (None, []) and names(_route(ni, _Agent(ws), True)) == (None, []), dims
        assert _route(ni, pol, False, plain=False)[0] is None, dims
        assert _route(ni, ni.Disturbed(pol, ni.Disturbance(action_noise=0.1), seed=1), False)[0] is None, dims
        assert _route(ni, pol.bf16(), False)[0] is None, dims
    for dims in ((64, 64), (200, 200), (400, 300), (128, 128, 64), (600, 600)):
        ws = ref.random_actor(S, A, dims, seed=2)
        pol = MLPPolicy(ws, device="cpu")
        assert not pol.shape_class_exact
        assert names(_route(ni, pol, False)) == (None, []) and names(_route(ni, _Agent(ws), False)) == (None, []), dims
    odd = MLPPolicy(ref.random_actor(15, 4, (128, 128), seed=2), device="cpu")
    assert _route(ni, odd, False, state_dim=15, action_dim=4)[0] is None
    ws = ref.random_actor(S, A, (256, 256), seed=2)
    two = MLPPolicy(ws, device="cpu")
    assert two.fusable and not two.shape_class_exact
    assert names(_route(ni, two, False)) == ("rollout_mlp", ["set_mlp_policy"])
    assert _route(ni, _Agent(ws), False)[0] is None                  # (a raw reference agent of the reference shape: the host loop, as before)
