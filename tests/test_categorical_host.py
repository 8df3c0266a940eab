"""not-gpu: the distributional safety critic ("nig-categorical-v1", include/nig.h) as far as it can be held without a device --
the ABI's prototypes and host-side refusals, the default atom mask, MLPPolicy's reading of a RiskAwareCQLAgent, the operand
image of a head of up to 64 rows (csrc/nig_mlp_stream.hpp put_network_wide, built by the library's own header through
tests/categorical_stream_probe.hip), and the formula.

The reference's DistributionalSafetyCritic cannot run here (jax / flax are absent), so there is no golden fixture from it: the
softmax-mass formula is pinned against a float64 NumPy restatement of the reference's lines (agents/safety_critical.py:151-171,
tests/categorical_ref.py mass64) instead, within the radius derived in categorical_ref.radius."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import categorical_ref as R
from conftest import ROOT
from test_mlp_stream import CHREC, H, MT, SLOTS, _law, _weights

f32 = np.float32
NEW = ("nig_set_mlp_safety_categorical", "nig_get_mlp_safety_kind", "nig_get_mlp_safety_atoms", "nig_mlp_violation_prob")


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    return ni


def test_the_prototypes_are_bound_and_nothing_new_is_called_rollout(ni):
    L = ni._lib.lib()
    for s in NEW:
        assert s in ni._lib.PROTOTYPES and hasattr(L, s), s
    assert len(ni._lib.PROTOTYPES["nig_set_mlp_safety_categorical"][1]) == 12 and len(ni._lib.PROTOTYPES["nig_mlp_violation_prob"][1]) == 10
    assert ni.__version__ == "0.8.0" and b"0.8.0" in L.nig_version()
    assert ni._lib.MAX_ATOMS == 64 and (ni._lib.SAFETY_NONE, ni._lib.SAFETY_SIGMOID, ni._lib.SAFETY_CATEGORICAL) == (0, 1, 2)
    for name in ("set_mlp_safety_categorical", "violation_prob", "mlp_safety_kind"):
        assert hasattr(ni.BatchedIndustrialEnv, name), name
    assert {"categorical_below_mask", "categorical_mass"} <= set(ni.__all__)
    text = open(os.path.join(ROOT, "include", "nig.h")).read()
    assert '"nig-categorical-v1"' in text and all(s + "(" in text for s in NEW)


def test_the_setter_and_the_evaluator_refuse_on_the_host(ni):
    """What needs no device: the law's bounds are checked ahead of the handle, so atoms 1 and 65 and a mask bit at or above atoms
    are refused by name with a NULL handle; a NULL handle alone, a NULL buffer and a kind query on no handle likewise.  Nothing
    can have been launched or written: there is no device, and every pointer handed in is NULL or host memory that stays as it was."""
    L = ni._lib.lib()
    w = np.ones(4, dtype=f32)
    p = w.ctypes.data_as(C.c_void_p)
    before = w.copy()

    def setter(atoms, mask, h=None):
        rc = L.nig_set_mlp_safety_categorical(h, 256, atoms, p, p, p, p, p, p, mask, 0.5, None)
        return rc, L.nig_last_error().decode()
    for atoms in (1, 65, 0, -3):
        rc, msg = setter(atoms, 0)
        assert rc == 1 and "atoms outside" in msg, (atoms, rc, msg)
    for atoms, mask in ((2, 0b100), (51, 1 << 51), (63, 1 << 63), (16, 1 << 16)):
        rc, msg = setter(atoms, mask)
        assert rc == 1 and "below_mask" in msg, (atoms, mask, rc, msg)
    for atoms, mask in ((2, 0b11), (51, (1 << 25) - 1), (64, (1 << 64) - 1)):      # in bounds: the refusal is the NULL handle's
        rc, msg = setter(atoms, mask)
        assert rc == 1 and "NULL" in msg, (atoms, mask, rc, msg)
    assert L.nig_get_mlp_safety_kind(None) == -1 and L.nig_get_mlp_safety_atoms(None) == -1
    out = np.full(8, 7.5, dtype=f32)
    rc = L.nig_mlp_violation_prob(None, 4, p, 4, p, 4, out.ctypes.data_as(C.c_void_p), None, 0, None)
    assert rc == 1 and "NULL" in L.nig_last_error().decode()
    assert np.array_equal(out, np.full(8, 7.5, dtype=f32)) and np.array_equal(w, before)


def test_the_default_mask(ni):
    """The reference's atoms < 0 of linspace(-1, 1, 51): bits 0 .. 24.  Atom 25 is exactly 0.0 in float32, in float64 and in the
    lerp form of linspace, so it is not below the threshold in any of them."""
    assert ni.categorical_below_mask(51) == (1 << 25) - 1 == R.default_mask(51)
    for sup in (np.linspace(-1.0, 1.0, 51, dtype=f32), np.linspace(-1.0, 1.0, 51),
                np.array([-1.0 * (1 - i / 50) + 1.0 * (i / 50) for i in range(51)])):
        assert sup[25] == 0.0 and (sup[:25] < 0).all() and not (sup[25:] < 0).any()
    assert ni.categorical_below_mask(2) == 0b01 and ni.categorical_below_mask(64) == (1 << 32) - 1
    assert ni.categorical_below_mask(51, safety_threshold=2.0) == (1 << 51) - 1 and ni.categorical_below_mask(51, safety_threshold=-1.0) == 0
    assert ni.categorical_below_mask(5, 0.0, 4.0, 2.5) == 0b00111


def _tree(layers, names):
    return {"params": {n: {"kernel": W, "bias": b} for n, (W, b) in zip(names, layers)}}


def _duck_agent(S, A, atoms, seed=3):
    rng = np.random.default_rng(seed)
    actor = [(rng.normal(0, 0.1, (S, 256)).astype(f32), rng.normal(0, 0.1, 256).astype(f32)),
             (rng.normal(0, 0.1, (256, 256)).astype(f32), rng.normal(0, 0.1, 256).astype(f32)),
             (rng.normal(0, 0.1, (256, A)).astype(f32), rng.normal(0, 0.1, A).astype(f32))]
    dist = R.random_categorical_critic(S, A, atoms, seed + 1)
    risk = [(rng.normal(0, 0.1, (S + A, 128)).astype(f32), np.zeros(128, f32)), (rng.normal(0, 0.1, (128, 128)).astype(f32), np.zeros(128, f32)),
            (rng.normal(0, 0.1, (128, 1)).astype(f32), np.zeros(1, f32))]
    agent = types.SimpleNamespace(
        state={"actor": types.SimpleNamespace(params={"params": {"MLP_0": {f"Dense_{i}": {"kernel": W, "bias": b} for i, (W, b) in enumerate(actor)}}})},
        safety_state=types.SimpleNamespace(params=_tree(dist, ("layers_0", "layers_1", "value_head"))),
        risk_state=types.SimpleNamespace(params=_tree(risk, ("layers_0", "layers_1", "risk_head"))),
        distributional_atoms=atoms, uncertainty_threshold=0.37)
    return agent, actor, dist


def test_from_agent_reads_the_distributional_critic(ni):
    S, A, atoms = 12, 3, 51
    agent, actor, dist = _duck_agent(S, A, atoms)
    pol = ni.MLPPolicy.from_agent(agent, device="cpu", critic="distributional")
    assert pol.safety_kind == "categorical" and pol.below_mask == (1 << 25) - 1 and pol.constraint_threshold == 0.37
    for (W, b), (Wr, br) in zip(pol.weights, actor):
        assert np.array_equal(W, Wr) and np.array_equal(b, br)
    for (W, b), (Wr, br) in zip(pol.safety_weights, dist):
        assert np.array_equal(W, Wr) and np.array_equal(b, br)
    assert pol.safety_weights[2][0].shape == (256, atoms)
    assert ni.MLPPolicy.from_agent(agent, device="cpu", critic="distributional", below_mask=0b101).below_mask == 0b101
    assert ni.MLPPolicy.from_agent(agent, device="cpu", critic="risk").safety_kind == "sigmoid"       # the other trees stay where they were
    sh, se = pol.shielded(), pol.searching(3)
    assert sh.fusable and se.fusable and sh.safety_kind == se.safety_kind == "categorical" and se.below_mask == sh.below_mask == pol.below_mask
    assert se.safety_weights[2][0].shape == (256, atoms) and sh.threshold == se.threshold == 0.37
    with pytest.raises(ValueError):
        ni.MLPPolicy.from_agent(agent, device="cpu", critic="nope")
    agent.distributional_atoms = 31
    with pytest.raises(ValueError):
        ni.MLPPolicy.from_agent(agent, device="cpu", critic="distributional")
    agent.safety_state = None
    with pytest.raises(ValueError):
        ni.MLPPolicy.from_agent(agent, device="cpu", critic="distributional")
    with pytest.raises(ValueError):
        ni.MLPPolicy(actor, device="cpu", safety_weights=dist, safety_kind="categorical", below_mask=1 << atoms)
    with pytest.raises(ValueError):
        ni.MLPPolicy(actor, device="cpu", safety_weights=dist)                                         # 51 columns are no sigmoid critic


@pytest.mark.parametrize("atoms", [2, 16, 17, 51, 64])
def test_the_torch_form_is_the_float64_formula(ni, atoms):
    """MLPPolicy's host form of the law (categorical_mass on torch's own logits) against the reference's lines in float64 on the
    SAME logits, within categorical_ref.radius(atoms): torch.exp is at least as close as det_expf's 1.5 ulp and a float32 sum of N
    terms has at most N - 1 roundings in any order, so the derivation covers it.  And the law's own NumPy restatement within the
    same radius, on logits that include a wide spread (differences up to 120: atoms of no mass)."""
    import torch
    from oracle import oracle
    S, A, n = 12, 3, 400
    agent, actor, dist = _duck_agent(S, A, atoms, seed=10 + atoms)
    mask = R.default_mask(atoms)
    pol = ni.MLPPolicy(actor, device="cpu", safety_weights=dist, safety_kind="categorical")
    rng = np.random.default_rng(5)
    obs, act = rng.normal(0, 3, (n, S)).astype(f32), rng.uniform(-1, 1, (n, A)).astype(f32)
    x = torch.from_numpy(np.concatenate([obs, act], axis=1))
    for i, (W, b) in enumerate(pol.safety_layers):
        x = torch.addmm(b, x, W)
        x = torch.relu(x) if i < 2 else x
    z = x.numpy().T.copy()                                         # [atoms, n]: the logits both sides start from
    p = pol.safety_probs_device(torch.from_numpy(obs), torch.from_numpy(act)).numpy()
    want = R.mass64(z, mask)
    worst = np.abs(p.astype(np.float64) - want).max() / R.radius(atoms)
    print(f"atoms {atoms}: torch form against float64, worst error / radius = {worst:.3g}")
    assert worst <= 1.0 and 0.02 < want.min() and want.max() < 0.98 and len(np.unique(p)) > n // 2
    got = pol.compute_safety_violation_probability(obs, act)
    assert np.array_equal(got, p) and isinstance(pol.compute_safety_violation_probability(obs[0], act[0]), float)
    wide = (z * f32(150.0 / (z.max(axis=0) - z.min(axis=0)).max())).astype(f32)      # the widest column spreads over 150
    wide[0, :7] = -np.inf                                          # an atom of no mass
    pl = R.violation_prob(oracle, wide, mask)
    worst = np.abs(pl.astype(np.float64) - R.mass64(wide, mask)).max() / R.radius(atoms)
    print(f"atoms {atoms}: the law's restatement against float64 on wide logits, worst error / radius = {worst:.3g}")
    assert worst <= 1.0 and (wide.max(axis=0) - wide.min(axis=0))[7:].max() > 100
    bad = wide.copy()
    bad[1, 0], bad[1, 1] = np.nan, np.inf
    pb = R.violation_prob(oracle, bad, mask)
    assert np.isnan(pb[:2]).all() and R.same_bits(pb[2:], pl[2:])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    assert hipcc, "hipcc not found: the probe is the library's own header, compiled for the host"
    tmp = tmp_path_factory.mktemp("categorical_stream")
    exe = tmp / "categorical_stream_probe"
    subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc"),
                    "-o", str(exe), os.path.join(ROOT, "tests", "categorical_stream_probe.hip")], check=True)

    def run(IN, OUT, seed):
        w = _weights(IN, OUT, seed)
        np.concatenate([a.ravel() for a in w]).tofile(tmp / "w.bin")
        out = subprocess.run([str(exe), str(IN), str(OUT), str(tmp / "w.bin"), str(tmp / "i.bin"), str(tmp / "t.bin")], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, (out.returncode, out.stderr)
        ok, floats, tail_floats = (int(x) for x in out.stdout.split())
        return bool(ok), w, np.fromfile(tmp / "i.bin", dtype=f32), np.fromfile(tmp / "t.bin", dtype=f32), floats, tail_floats
    return run


@pytest.mark.parametrize("IN,OUT", [(15, 51), (40, 51), (15, 2), (40, 16), (15, 17), (40, 64), (26, 33)])
def test_the_wide_image_is_the_16_row_image_and_a_tail(probe, IN, OUT):
    """put_network_wide's image is, byte for byte, the image test_mlp_stream.py's law gives for the network whose head is columns
    0 .. 15 (zero-padded to 16: the 16 x 16 x 1 form whatever OUT is) -- so the chunks, and with them every existing network's
    image, are put_network's and stay what that module pins -- and the tail is the law stated here: entry 16 m2 + t, lane l,
    word P - 1 = W3[32 m2 + rho_{l >> 5}(t)][16 P + (l & 15)], entry 128 the bias, zero for rows >= OUT and in word 3."""
    ok, (W1, b1, W2, b2, W3, b3), image, tail, floats, tail_floats = probe(IN, OUT, 77 + OUT)
    assert ok and floats == SLOTS * CHREC * 64 and tail_floats == (MT * 16 + 1) * 64 * 4
    W16, b16 = np.zeros((H, 16), dtype=f32), np.zeros(16, dtype=f32)
    W16[:, :min(OUT, 16)], b16[:min(OUT, 16)] = W3[:, :16], b3[:16]
    want, _ = _law(IN, 16, W1, b1, W2, b2, W16, b16)
    assert np.array_equal(image.view(np.uint32), want.ravel().view(np.uint32))
    t_want = np.zeros((MT * 16 + 1, 64, 4), dtype=f32)
    lane = np.arange(64)
    for P in (1, 2, 3):
        row = 16 * P + (lane & 15)
        on = row < OUT
        for m2 in range(MT):
            for t in range(16):
                rho = (t & 3) + 8 * (t >> 2) + 4 * (lane >> 5)
                t_want[16 * m2 + t, lane[on], P - 1] = W3[32 * m2 + rho[on], row[on]]
        t_want[MT * 16, lane[on], P - 1] = b3[row[on]]
    assert np.array_equal(tail.view(np.uint32), t_want.ravel().view(np.uint32))
    assert (np.count_nonzero(tail) == 0) == (OUT <= 16)


def test_the_wide_builder_refuses_what_it_cannot_hold(probe):
    for IN, OUT in ((15, 1), (15, 65), (74, 51)):
        assert not probe(IN, OUT, 5)[0], (IN, OUT)
