"""The guard of tests/closed_loop_matrix.py: the env lists are the library's own registry filtered by the documented condition
(not gpu), every anchor test of every family module is parametrised over the whole list at both matrix shapes (not gpu), and
each closed-loop entry point runs on exactly the envs of its list and refuses the others on the host (gpu).  The families with a
module of their own are held here too: the bf16 MFMA actor (rollout_mlp_bf16, tests/test_gpu_mlp_bf16.py) and the fused
constraint projection (rollout_mlp_projected, tests/test_gpu_projection.py)."""
import importlib
import re

import numpy as np
import pytest

import closed_loop_matrix as M

ENTRIES = ("rollout_mlp", "rollout_mlp_safe", "rollout_mlp_ensemble", "rollout_mlp_disturbed", "rollout_mlp_search",
           "rollout_mlp_gated", "rollout_policy_disturbed", "rollout_mlp_bf16", "rollout_mlp_projected")
UNSUPPORTED = 4            # NIG_ERR_UNSUPPORTED


def test_the_lists_are_the_registry(oracle):
    """MFMA_ENVS: the registered envs with an even state dim and at most 16 actions (has_mlp_actor), in the registry's order;
    POLICY_ENVS_ALL: every registered env.  The keys are the oracle's, with the same dimensions."""
    import neorl_industrial_gym_amd as ni
    ids = ni.batched.ENV_IDS
    assert [n for _, n in M.POLICY_ENVS_ALL] == sorted(ids, key=ids.get) and len(ids) == 9
    mfma = []
    for name in sorted(ids, key=ids.get):
        sp = ni._lib.env_spec(ids[name])
        if sp.state_dim % 2 == 0 and sp.action_dim <= 16:
            mfma.append(name)
    assert [n for _, n in M.MFMA_ENVS] == mfma and len(mfma) == 8
    assert set(M.MFMA_ENVS) < set(M.POLICY_ENVS_ALL) and len(set(k for k, _ in M.POLICY_ENVS_ALL)) == 9
    for key, name in M.POLICY_ENVS_ALL:
        sp, osp = ni._lib.env_spec(ids[name]), oracle.spec(key)
        assert (sp.state_dim, sp.action_dim) == (osp.state_dim, osp.action_dim) == (oracle.spec(name).state_dim, oracle.spec(name).action_dim)
        assert (key in M.CLONED) == (sp.k_step == 0 and sp.k_reset == 0), key


# (module, anchor test, the list it must cover)
MFMA, POLICY = "MFMA_ENVS", "POLICY_ENVS_ALL"
ANCHORS = [
    ("test_gpu_parity", "test_mfma_actor_matrix", MFMA),
    ("test_gpu_safety_shield", "test_shield_matrix", MFMA),
    ("test_gpu_ensemble", "test_members_action_and_uncertainty_matrix", MFMA),
    ("test_gpu_ensemble", "test_the_step_took_that_action_matrix", MFMA),
    ("test_gpu_ensemble", "test_one_voting_member_is_the_single_actor_matrix", MFMA),
    ("test_gpu_safe_action_search", "test_never_search_is_the_shield_kernel_at_the_same_threshold", MFMA),
    ("test_gpu_safe_action_search", "test_always_search_takes_the_first_least_risky_candidate", MFMA),
    ("test_gpu_safe_action_search", "test_mixed_lanes_keep_or_search_per_lane", MFMA),
    ("test_gpu_safety_gate", "test_one_member_is_the_oracles_critic_row_by_row", MFMA),
    ("test_gpu_safety_gate", "test_every_logit_is_the_oracles_critic_on_that_column", MFMA),
    ("test_gpu_safety_gate", "test_the_law_bit_for_bit_from_the_logits", MFMA),
    ("test_gpu_safety_gate", "test_prob_and_unc_against_the_references_formula", MFMA),
    ("test_gpu_disturbance", "test_zero_is_off_matrix", POLICY),
    ("test_gpu_disturbance", "test_the_draws_matrix", POLICY),
    ("test_gpu_disturbance", "test_the_action_matrix", POLICY),
    ("test_gpu_disturbance", "test_the_plant_received_it_matrix", POLICY),
    ("test_gpu_mlp_bf16", "test_layout_bit_for_bit_on_integer_data", MFMA),
    ("test_gpu_mlp_bf16", "test_each_layer_from_the_devices_own_previous_layer", MFMA),
    ("test_gpu_mlp_bf16", "test_the_step_took_that_action", MFMA),
    ("test_gpu_mlp_bf16", "test_frozen_lanes_store_nothing_and_live_lanes_follow_the_law", MFMA),
    ("test_gpu_projection", "test_the_law_bit_for_bit", MFMA),
]


def _cells(fn):
    """The (key, B) cells of a test function's parametrisation: the cross product of its parametrize marks, keys and batch
    sizes read from the arguments named `key` and `B` (B None where the test fixes its own)."""
    keys, Bs = set(), {None}
    joint = None
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [n.strip() for n in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        rows = [tuple(getattr(v, "values", v if isinstance(v, (tuple, list)) else (v,))) for v in mark.args[1]]
        if "key" in names and "B" in names:
            joint = {(r[names.index("key")], r[names.index("B")]) for r in rows}
        elif "key" in names:
            keys |= {r[names.index("key")] for r in rows}
        elif "B" in names:
            Bs = {r[names.index("B")] for r in rows}
    return joint if joint is not None else {(k, b) for k in keys for b in Bs}


@pytest.mark.parametrize("module,test,which", ANCHORS, ids=[f"{m}.{t}" for m, t, _ in ANCHORS])
def test_every_anchor_test_covers_its_whole_list(module, test, which):
    """Each anchor test -- one that pins a family's outputs to the oracle on the device's own obs_out -- names every env its
    family is compiled for, at B = 700 and at B = 5: an env dropped from a family's list, or from the matrix, fails here."""
    fn = getattr(importlib.import_module(module), test)
    cells = _cells(fn)
    want = {k for k, _ in getattr(M, which)}
    kinds = {None}
    if which == POLICY:                      # the disturbed loops: the MFMA actor on its envs, the policy kernel on all nine
        kinds = {"actor", "mpc", "pid"}
    for B in (M.B_BIG, M.B_SMALL):
        have = {k for k, b in cells if b == B or b is None}     # (None: the test fixes its own batch, 700 in these modules)
        if which == POLICY:
            by_kind = {}
            for mark in fn.pytestmark:
                if mark.name == "parametrize" and "kind" in str(mark.args[0]):
                    names = [n.strip() for n in mark.args[0].split(",")]
                    for r in mark.args[1]:
                        by_kind.setdefault(r[names.index("kind")], set()).add(r[names.index("key")])
            assert set(by_kind) >= kinds, (module, test, sorted(by_kind))
            assert by_kind["actor"] == {k for k, _ in M.MFMA_ENVS}, (module, test, "actor")
            for kind in ("mpc", "pid"):
                assert by_kind[kind] == want, (module, test, kind, sorted(want - by_kind[kind]))
        assert have == want, (module, test, B, "missing", sorted(want - have), "unknown", sorted(have - want))


def test_the_lifecycle_module_covers_every_entry_points_list():
    """tests/test_gpu_handle_lifecycle.py::test_held_lanes_on_an_autoreset_handle anchors every family at once: it is parametrised
    over (case, key) cells, not over `key` alone, so it is held here and not in ANCHORS.  For every entry point of ENTRIES the
    cells of the cases that launch it name exactly the envs of its list, at B = 700 and at B = 5.  (The whole table against the
    exported symbols: tests/test_handle_lifecycle_host.py.)"""
    import handle_lifecycle as H
    fn = importlib.import_module("test_gpu_handle_lifecycle").test_held_lanes_on_an_autoreset_handle
    marks = {m.args[0]: list(m.args[1]) for m in fn.pytestmark if m.name == "parametrize"}
    assert set(marks["B"]) == {M.B_BIG, M.B_SMALL}
    cells = [tuple(c) for c in marks["case,key"]]
    for entry in ENTRIES:
        cases = [c for c, v in H.CASES.items() if v[0] == "nig_" + entry]
        assert cases, entry
        want = {k for k, _ in (M.POLICY_ENVS_ALL if entry == "rollout_policy_disturbed" else M.MFMA_ENVS)}
        for case in cases:
            have = [k for c, k in cells if c == case]
            assert len(have) == len(set(have)) and set(have) == want, (entry, case, sorted(set(have) ^ want))


# ---- gpu: every entry point on every env ------------------------------------------------------------------------------------
def _code(call):
    """0, or the status code of the NigError the call raised."""
    import neorl_industrial_gym_amd as ni
    try:
        call()
    except ni._lib.NigError as e:
        return int(re.match(r"libnig error (\d+)", str(e)).group(1))
    return 0


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("key,name", M.POLICY_ENVS_ALL)
def test_each_entry_point_runs_on_exactly_its_envs(key, name, entry):
    """One step at B = 5 with the entry point's prerequisites installed.  On the envs of its list the launch succeeds and
    writes a flag word, a reward and an action row per lane (and nothing into the pad columns); on the others an installation
    or the launch returns NIG_ERR_UNSUPPORTED on the host, nothing is launched, and every output keeps its fill value."""
    import torch
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    supported = entry == "rollout_policy_disturbed" or key in {k for k, _ in M.MFMA_ENVS}
    B, FILL, FLAGFILL, HIDFILL = M.B_SMALL, -7.0, 0x5A5A5A5B, 0x7A7B
    env = ni.make_batched(name, B, seed=0x5EED, max_episode_steps=M.MAXS_NEW)
    S, A, ld, dev = env.state_dim, env.action_dim, env.ld, env.device
    env.reset()
    ws = M.random_actor(S, A, 5)
    installs = []
    if entry == "rollout_policy_disturbed":
        installs.append(lambda: env.set_policy(ni.mpc_agent(S, A)))
    elif entry == "rollout_mlp_bf16":
        installs.append(lambda: env.set_mlp_policy_bf16(ws))
    else:
        installs.append(lambda: env.set_mlp_policy(ws))
    if entry == "rollout_mlp_projected":
        installs.append(lambda: env.set_mlp_constraint(M.random_critic(S, A, 10, n_out=3), 0.5, 0.01))
    if entry in ("rollout_mlp_safe", "rollout_mlp_search"):
        installs.append(lambda: env.set_mlp_safety(M.random_critic(S, A, 6), 0.5))
    if entry == "rollout_mlp_ensemble":
        installs.append(lambda: env.set_mlp_ensemble([ws, M.random_actor(S, A, 7)], None, None, "voting", 0.2))
    if entry == "rollout_mlp_gated":
        installs.append(lambda: env.set_mlp_safety_ensemble([M.random_critic(S, A, 8, n_out=2), M.random_critic(S, A, 9, n_out=2)], 1.0, 0.5, 0.2))
    if entry.endswith("_disturbed"):
        installs.append(lambda: env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.1, clip=(-1, 1), hold="step")))
    codes = [_code(f) for f in installs]
    rw = torch.full((1, ld), FILL, dtype=torch.float32, device=dev)
    fl = torch.full((1, ld), FLAGFILL, dtype=torch.int32, device=dev)
    act = torch.full((1, A, ld), FILL, dtype=torch.float32, device=dev)
    rows = {n: torch.full((1, ld), FILL, dtype=torch.float32, device=dev) for n in ("pr", "rk", "un")}
    ch = torch.full((1, ld), FLAGFILL, dtype=torch.int32, device=dev)
    hid = torch.full((1, 512, ld), HIDFILL, dtype=torch.int16, device=dev)
    t0 = env.counter
    launch = {"rollout_mlp": lambda: env.rollout_mlp(1, rw, fl, None, act),
              "rollout_mlp_safe": lambda: env.rollout_mlp_safe(1, rw, fl, None, act, rows["pr"]),
              "rollout_mlp_ensemble": lambda: env.rollout_mlp_ensemble(1, rw, fl, None, act, rows["un"], None),
              "rollout_mlp_disturbed": lambda: env.rollout_mlp_disturbed(1, rw, fl, None, act, None),
              "rollout_mlp_search": lambda: env.rollout_mlp_search(1, 3, rw, fl, None, act, rows["pr"], rows["rk"], ch),
              "rollout_mlp_gated": lambda: env.rollout_mlp_gated(1, rw, fl, None, act),
              "rollout_policy_disturbed": lambda: env.rollout_policy_disturbed(1, rw, fl, None, act, None),
              "rollout_mlp_bf16": lambda: env.rollout_mlp_bf16(1, rw, fl, None, act, hid),
              "rollout_mlp_projected": lambda: env.rollout_mlp_projected(1, 3, 0.1, rw, fl, None, act, None, None, ch, None)}[entry]
    rc = _code(launch)
    torch.cuda.synchronize()
    used = {"rollout_mlp_safe": ("pr",), "rollout_mlp_search": ("pr", "rk"), "rollout_mlp_ensemble": ("un",)}.get(entry, ())
    if supported:
        assert codes == [0] * len(codes) and rc == 0, (codes, rc)
        assert env.counter == t0 + 1
        assert bool((fl[0, :B] != FLAGFILL).all()) and bool((rw[0, :B] != FILL).all())
        a = act[0, :, :B]
        assert bool(torch.isfinite(a).all()) and bool((a != FILL).all())
        for n in used:
            assert bool((rows[n][0, :B] != FILL).all()), n
        if entry in ("rollout_mlp_search", "rollout_mlp_projected"):
            assert bool((ch[0, :B] != FLAGFILL).all())
        if entry == "rollout_mlp_bf16":
            assert bool((hid[0, :, :B] != HIDFILL).all()) and bool((hid[0, :, B:] == HIDFILL).all())
        # pad columns keep their words
        assert bool((fl[0, B:] == FLAGFILL).all()) and bool((rw[0, B:] == FILL).all()) and bool((act[0, :, B:] == FILL).all())
    else:
        assert all(c in (0, UNSUPPORTED) for c in codes), codes
        assert codes[0] == UNSUPPORTED, "an env shape without the MFMA actor refuses the actor itself"
        # (nig_rollout_mlp itself reports the actor that could not be installed: NIG_ERR_INVALID, "no actor installed")
        assert rc == (1 if entry == "rollout_mlp" else UNSUPPORTED), rc
        assert env.counter == t0
        assert bool((fl == FLAGFILL).all()) and bool((rw == FILL).all()) and bool((act == FILL).all()) and bool((ch == FLAGFILL).all())
        assert all(bool((r == FILL).all()) for r in rows.values())
    if entry != "rollout_mlp_bf16" or not supported:
        assert bool((hid == HIDFILL).all()), "hid_out"
    if entry not in ("rollout_mlp_search", "rollout_mlp_projected") or not supported:
        assert bool((ch == FLAGFILL).all()), "choice / iters row"
    for n in rows:
        if n not in used or not supported:
            assert bool((rows[n] == FILL).all()), n
    env.close()
