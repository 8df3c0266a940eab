"""The guard of tests/handle_lifecycle.py (no GPU): its case table names every closed-loop entry point the library exports, on
exactly the envs whose translation units instantiate that entry point's launcher, so a new family or a new env cannot be added
without a lifecycle case; the held-lane sets are what part 1 of tests/test_gpu_handle_lifecycle.py promises; and that test is
parametrised over the whole table, both batch sizes and the three ways a lane becomes held."""
import glob
import importlib
import os

import numpy as np

import closed_loop_matrix as M
import handle_lifecycle as H
from conftest import KEYS, ROOT

CSRC = os.path.join(ROOT, "neorl-industrial-gym_amd", "csrc")


def test_the_table_names_every_closed_loop_entry_point():
    """Every nig_rollout* symbol of the ABI is a case's entry point or is listed, with its reason, as not one; every rollout*
    method of BatchedIndustrialEnv is such a symbol's wrapper; and each case's inputs have a setter."""
    import neorl_industrial_gym_amd as ni
    exported = {s for s in ni._lib.PROTOTYPES if s.startswith("nig_rollout")}
    assert all(hasattr(ni._lib.lib(), s) for s in exported)
    named = {sym for sym, _, _, _ in H.CASES.values()}
    assert named | set(H.NOT_A_CASE) == exported, sorted(exported ^ (named | set(H.NOT_A_CASE)))
    assert not named & set(H.NOT_A_CASE) and set(H.UNITS) == named
    methods = {"nig_" + m for m in dir(ni.batched.BatchedIndustrialEnv) if m.startswith("rollout")}
    assert methods <= exported and named <= methods, sorted(methods ^ named)
    for case, (sym, keys, block, inputs) in H.CASES.items():
        assert set(inputs) <= set(H.SETTERS) and block in (128, 256), case
        assert case.endswith("_limited") == sym.endswith("_limited"), case
        assert (block == 128) == ("_mlp" in sym), case
    # every twin has its parent, with the same inputs
    for case in H.TWINS:
        assert H.parent_of(case) in H.PARENTS and H.CASES[H.parent_of(case)][3] == H.CASES[case][3], case
        assert H.CASES[case][0] == H.CASES[H.parent_of(case)][0] + "_limited", case


def test_each_case_runs_on_the_envs_its_launcher_is_compiled_for():
    """The envs of a symbol: the keys <k> of the translation units csrc/<prefix><k>.hip that instantiate its launcher, for an
    MFMA family those with the MFMA actor (even state dim, at most 16 actions: closed_loop_matrix.MFMA_ENVS, which
    test_closed_loop_matrix.py holds to the registry), for nig_rollout_noise those the reference records draws for."""
    assert set(H.ALL) == {k for k, _ in M.POLICY_ENVS_ALL} and len(H.ALL) == 9
    mfma = {k for k, _ in M.MFMA_ENVS}
    by_symbol = {}
    for case, (sym, keys, _, _) in H.CASES.items():
        by_symbol.setdefault(sym, []).append(list(keys))
    for sym, (prefix, needs_mfma) in H.UNITS.items():
        units = {os.path.basename(p)[len(prefix):-len(".hip")] for p in glob.glob(os.path.join(CSRC, prefix + "*.hip"))}
        want = units & set(H.ALL)
        assert want, (sym, prefix)
        if needs_mfma:
            want &= mfma
        if sym == "nig_rollout_noise":
            want &= set(KEYS)
        for keys in by_symbol[sym]:
            assert len(keys) == len(set(keys)) and set(keys) == want, (sym, sorted(set(keys) ^ want))
    assert len(H.CELLS) == sum(len(v[1]) for v in H.CASES.values()) == len(set(H.CELLS))


def test_the_held_sets_are_what_part_one_promises():
    for block in (128, 256):
        for B in (M.B_BIG, M.B_SMALL):
            m = H.held_mask(B, block)
            assert m.shape == (B,) and 0.25 <= m.mean() <= 0.5, (B, block, m.mean())
        m = H.held_mask(M.B_BIG, block)
        first = m[:64]
        assert first.any() and (~first).any() and np.array_equal(np.where(first)[0], np.arange(0, 64, 3)), "held and live mixed in one wave"
        waves = m[:M.B_BIG // 64 * 64].reshape(-1, 64)
        assert waves.all(axis=1).sum() >= 1 + block // 64 and (~waves).all(axis=1).any(), "a whole wave held, whole waves live"
        blocks = m[:M.B_BIG // block * block].reshape(-1, block)
        assert blocks.all(axis=1).sum() == 1, "exactly one whole block held"
        assert M.B_BIG % block != 0 and m[-1] and not m[M.B_BIG // block * block:-1].any(), "the last lane of the partial block, alone"
    assert H.held_lanes(M.B_SMALL, 128).tolist() == H.held_lanes(M.B_SMALL, 256).tolist() == [1, 4]


def test_part_one_is_parametrised_over_the_whole_table():
    fn = importlib.import_module("test_gpu_handle_lifecycle").test_held_lanes_on_an_autoreset_handle
    marks = {tuple(n.strip() for n in m.args[0].split(",")): list(m.args[1]) for m in fn.pytestmark if m.name == "parametrize"}
    assert [tuple(c) for c in marks[("case", "key")]] == H.CELLS
    assert sorted(marks[("B",)]) == sorted([M.B_BIG, M.B_SMALL])
    assert marks[("how",)] == ["never_reset", "masked_reset", "set_state_done"]
    assert importlib.import_module("test_gpu_handle_lifecycle").pytestmark.name == "gpu"
