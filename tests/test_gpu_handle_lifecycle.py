"""-m gpu: what a handle carries from one call to the next (struct nig_handle, csrc/nig_api.hip).  The family modules build a fresh
handle per case; callers keep one alive, replace its inputs, add and remove constraints, mix entry points and leave lanes done on
an auto-reset handle.  Every comparison here is against a LEAN TWIN (tests/handle_lifecycle.py): a second handle of the same env,
batch, seed and env_index0 that has only ever seen the one install and the one call under test, bit for bit -- every output
word, and everything the handle keeps (state rows, counter words, life_viol).
  1. held lanes on an auto-reset handle, in every closed loop: the freeze branch and the in-kernel restart meet in one wave;
  2. re-installation through every setter; installing one family's inputs leaves the others alone;
  3. one loaded handle (everything installed at once) against lean twins; limits added and removed; the constraint mask;
  4. the lazy side buffers (act32, act_soa, hst_*, a step plan) between closed-loop launches.
Shapes are the closed-loop matrix's: B = 700 and 5, T = 7, episodes of at most 5 steps, so every live lane finishes and restarts
inside a launch.

One law differs from a plain "a held lane's rows keep their canary": include/nig.h states that a frozen lane's xflags word is
written (0), and that nig_rollout's kernels (nig_rollout_sampled, nig_rollout_noise) write a frozen lane's obs_out row with the
state the lane holds; tests/test_gpu_limits*.py and test_gpu_footprint.py pin both.  Those words are held to that law here."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import closed_loop_matrix as M
import handle_lifecycle as H

pytestmark = pytest.mark.gpu

HOWS = ["never_reset", "masked_reset", "set_state_done"]
INVALID, UNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _code(ni, call):
    try:
        call()
    except ni._lib.NigError as e:
        return int(re.match(r"libnig error (\d+)", str(e)).group(1))
    return 0


# ---- 1. held lanes on an auto-reset handle -------------------------------------------------------------------------------------
def _prepare(ni, env, case, key, how, held):
    """The case's inputs and the start of the launch; `held` [B] bool: the lanes left done (None: the twin, nothing held).  Live
    lanes have the same history on both: every reset draws by global lane and launch counter."""
    B = env.batch
    H.install(ni, env, case, key)
    live = None if held is None else (~held).astype(np.uint8)
    if how == "never_reset":                             # held lanes were never reset: done since nig_create
        env.reset(mask=live)
    elif how == "masked_reset":                          # held lanes finished out of band and reset(mask) leaves them out
        env.reset()
        env.step(env.fill_actions(1)[:, :B], layout="soa")
        if held is not None:
            env.set_state(current_step=env.current_step, violation_count=env.violation_count, done=env.done | torch.from_numpy(held).to(env.device))
        env.reset(mask=live)
    else:                                                # held lanes are marked done by set_state
        env.reset()
        if held is not None:
            env.set_state(current_step=env.current_step, violation_count=env.violation_count, done=held)
    if key in M.CLONED:                                  # distinct start states; the held lanes stay done
        env.set_state(np.array(M.start_states(ni, M.NAMES[key], B, H.SEED)), current_step=0, violation_count=0,
                      done=False if held is None else held)
    torch.cuda.synchronize()


def _rows_beyond_the_head_are_clean(env, out, what):
    """The gate's and the projection's per-constraint rows beyond the installed head's width keep their canary."""
    base = H.parent_of(what[0])
    Cn = env._gate_shape[1] if base == "gated" else (env._constraint_outputs if base == "projected" else None)
    if Cn is None:
        return
    for name in ("prob", "unc", "viol", "logit"):
        if name in out:
            assert (H.bits(out[name][..., Cn:, :]) == H.canary_of(out[name])).all(), (what, name, "rows beyond n_outputs")


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("B", [M.B_BIG, M.B_SMALL])
@pytest.mark.parametrize("case,key", H.CELLS)
def test_held_lanes_on_an_autoreset_handle(ni, case, key, B, how):
    """Three handles with tallies: `a` holds lanes and plays T steps in one launch, `b` holds nothing, `c` holds a's lanes and
    plays 3 + 4 steps.  Held lanes: state, counter word, life_viol, episode return and tally rows untouched, still done, flag
    word FLAG_INACTIVE | step count, reward +0.0f, every other output word its canary (xflags 0, the open loop's obs row the held
    state).  Live lanes: every output word and everything kept equal b's.  c equals a in every byte.  After a full reset the
    whole batch equals the twin and no lane is done."""
    L = ni._lib
    block = H.CASES[case][2]
    held = H.held_mask(B, block)
    live = ~held
    assert 0.25 <= held.mean() <= 0.5 and live.any()
    cons = [H.band(ni, None)] if case.endswith("_limited") else []
    a, b, c = (H.make(ni, key, B, tally=True, cons=cons) for _ in range(3))
    _prepare(ni, a, case, key, how, held)
    _prepare(ni, b, case, key, how, None)
    _prepare(ni, c, case, key, how, held)
    before = H.kept(a)
    assert ((before["ctr"].view(np.uint32) & L.CTR_DONE) != 0).tolist() == held.tolist(), "exactly the held lanes are done"
    assert before["counter"] == H.kept(b)["counter"]
    oa, ob, oc = H.run(a, case), H.run(b, case), H.run_cut(c, case, (3, 4))
    ka, kb, kc = H.kept(a), H.kept(b), H.kept(c)
    what = (case, key, B, how)
    # held lanes
    for k in ("state", "ctr", "life", "ep_ret", "tally"):
        assert np.array_equal(H.bits(ka[k])[..., held], H.bits(before[k])[..., held]), (what, k, "held lanes")
    step = (before["ctr"].view(np.uint32) & L.CTR_STEP_MASK)[held]
    for name, arr in oa.items():
        h = H.bits(arr[..., :B][..., held])
        if name == "fl":
            assert np.array_equal(h, np.broadcast_to(L.FLAG_INACTIVE | (step << L.FLAG_STEP_SHIFT), h.shape)), (what, "flag words of held lanes")
        elif name in ("rew", "xf"):
            assert not h.any(), (what, name, "held lanes: +0.0f / 0")
        elif name.startswith("obs_held"):
            assert np.array_equal(h, np.broadcast_to(H.bits(before["state"])[:, held], h.shape)), (what, name, "held lanes: the state they hold")
        else:
            assert (h == H.canary_of(arr)).all(), (what, name, "held lanes keep the canary")
    # live lanes
    H.same(oa, ob, live, f"{what} outputs of live lanes")
    H.same(ka, kb, live, f"{what} kept of live lanes")
    H.pads_clean(oa, B, what)
    _rows_beyond_the_head_are_clean(a, oa, what)
    fl_live = oa["fl"][:, :B][:, live]
    assert not (fl_live & L.FLAG_INACTIVE).any(), (what, "live lanes stay live")
    assert (fl_live & L.FLAG_DID_RESET).any(), (what, "a live lane finishes and restarts inside the launch")
    # cutting the launch changes no byte.  (But the two float sums of the tally: a launch adds the returns of the episodes it
    # finished as ONE partial (LaneTally::merge, csrc/nig_episode.hpp), so where a lane finishes episodes on both sides of the cut
    # its return sum and square sum are added in another order; the other eleven rows, min and max included, are exact.)
    H.same(oc, oa, None, f"{what} 3 + 4 steps")
    exact = [r for r in range(L.T_ROWS) if r not in (L.T_RET_SUM, L.T_RET_SQ)]
    H.same(dict(kc, tally=kc["tally"][exact]), dict(ka, tally=ka["tally"][exact]), None, f"{what} kept after 3 + 4 steps")
    # a full reset clears the condition
    for e in (a, b):
        H.rewind(ni, e, key, t0=ka["counter"], case=case)
    oa, ob = H.run(a, case), H.run(b, case)
    ka, kb = H.kept(a), H.kept(b)
    H.same(oa, ob, None, f"{what} outputs after reset()")
    H.same({k: ka[k] for k in ("state", "ctr", "counter")}, {k: kb[k] for k in ("state", "ctr", "counter")}, None, f"{what} kept after reset()")
    H.same(ka, kb, live, f"{what} sums after reset()")           # (life_viol and the tally sums carry the first launch: live lanes)
    assert not (ka["ctr"].view(np.uint32) & L.CTR_DONE).any() and not (oa["fl"][:, :B] & L.FLAG_INACTIVE).any()
    for e in (a, b, c):
        e.close()


# ---- the lean twins of 2 and 3 ------------------------------------------------------------------------------------------------
_LEAN = {}


def _play(ni, env, case, key, reinstall_pid=False, spread=False):
    """Rewind, one launch.  life_viol is the one kept array a reset leaves alone (base.py:57,183: total_violations is never
    reset), so a used handle's carries its earlier plays: what the launch ADDED to it is compared (its twin starts from zero).
    spread: the launch starts from H.spread_start's states, outside the built-in constraints' boxes."""
    H.rewind(ni, env, key, t0=0, case=case if reinstall_pid else None)
    if spread:
        H.spread_start(env)
    life0 = H.kept(env)["life"]
    out = H.run(env, case)
    kept = H.kept(env)
    kept["life"] = kept["life"] - life0
    return dict(out=out, kept=kept)


def _lean(ni, case, key, B, tag, installer, floor=None, cmask=None, spread=False):
    """The lean twin's run: a fresh handle (with H.floor(*floor) as its one added constraint, where given), `installer(env)`, the
    one launch.  Computed once per key, left unchanged."""
    ck = (case, key, B, tag, floor, cmask, spread)
    if ck not in _LEAN:
        env = H.make(ni, key, B, cons=[] if floor is None else [H.floor(ni, *floor)])
        installer(env)
        if cmask is not None:
            env.set_constraint_mask(cmask)
        r = _play(ni, env, case, key, spread=spread)
        env.close()
        for d in (r["out"], r["kept"]):
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _LEAN[ck] = r
    return _LEAN[ck]


def _lean_v(ni, case, key, B, variants=None, **how):
    """The lean twin with the case's own inputs in the given variants (inputs of other families are not installed on it)."""
    mine = {i: (variants or {}).get(i, 0) for i in H.CASES[case][3]}
    return _lean(ni, case, key, B, tuple(sorted(mine.items())), lambda env: H.install(ni, env, case, key, mine), **how)


def _equal(got, lean, what):
    H.same(got["out"], lean["out"], None, f"{what} outputs")
    H.same(got["kept"], lean["kept"], None, f"{what} kept")


def _B(key):
    return M.B_BIG if key in ("cr", "supply") else M.B_SMALL          # the smallest and the widest head at B = 700


# ---- 2. re-installation --------------------------------------------------------------------------------------------------------
def _reinstall(ni, key, cases, stages, needs_actor=False, check=None):
    """One handle through `stages` = [(setter, variant, keyword arguments)]: each stage calls setter(ni, env, key, v=variant, ...)
    on the used handle (which got the float32 actor first, where the cases need one), then the handle rewinds and plays T steps
    of each case -- so every buffer has been read by a kernel before it is replaced.  From the second stage on each run equals
    the lean twin that only ever saw (the actor and) that stage's install."""
    B = _B(key)
    env = H.make(ni, key, B)
    if needs_actor:
        H.set_actor(ni, env, key)
    for i, (setter, v, kw) in enumerate(stages):
        setter(ni, env, key, v=v, **kw)

        def lean_install(e, setter=setter, v=v, kw=kw):
            if needs_actor:
                H.set_actor(ni, e, key)
            setter(ni, e, key, v=v, **kw)

        tag = (setter.__name__, v, tuple(sorted(kw.items())), needs_actor)
        for case in cases:
            got = _play(ni, env, case, key)
            if i:
                _equal(got, _lean(ni, case, key, B, tag, lean_install), (case, key, B, tag))
            if case in ("gated", "projected"):
                _rows_beyond_the_head_are_clean(env, got["out"], (case, key, tag))
            if check is not None:
                check(i, got["out"])
    env.close()


@pytest.mark.parametrize("key", H.MFMA)
def test_reinstalling_the_actor(ni, key):
    _reinstall(ni, key, ["mlp"], [(H.set_actor, v, {}) for v in range(3)])


@pytest.mark.parametrize("key", H.MFMA)
def test_reinstalling_the_bf16_actor(ni, key):
    _reinstall(ni, key, ["mlp_bf16"], [(H.set_bf16, v, {}) for v in range(3)])


@pytest.mark.parametrize("key", H.MFMA)
def test_reinstalling_the_critic(ni, key):
    """New weights and a new threshold; the shield and the search share the stream."""
    _reinstall(ni, key, ["safe", "search"], [(H.set_critic, v, {}) for v in range(3)], needs_actor=True)


@pytest.mark.parametrize("key", H.MFMA)
def test_reinstalling_the_constraint_predictor(ni, key):
    """Output count 4 -> 1 -> 3, new weights, threshold and tolerance: the forward and the backward stream are both replaced."""
    _reinstall(ni, key, ["projected"], [(H.set_predictor, v, dict(C=Cn)) for v, Cn in enumerate((4, 1, 3))], needs_actor=True)


@pytest.mark.parametrize("key", H.MFMA)
def test_reinstalling_the_ensemble(ni, key):
    """Members 5 -> 2 -> 8 -> 3: the capacity is reused, grows, is reused again; method mean -> voting -> mean -> mean with new
    weights, weight sum and threshold each time.  member_act_out is compared too: no row of an earlier install's member."""
    from neorl_industrial_gym_amd.policies import ensemble_action
    seq = [(5, "mean"), (2, "voting"), (8, "mean"), (3, "mean")]
    B = _B(key)

    def the_installed_rule(i, out):
        """A twin built by the same library shares a rule the launcher got wrong: the action row is also held to the documented
        law of the INSTALLED method on the launch's own member rows (policies.ensemble_action, bit for bit:
        tests/test_gpu_ensemble.py), rounded to float32 where it is float64."""
        K, method = seq[i]
        preds = np.ascontiguousarray(out["member"][..., :B].transpose(1, 0, 3, 2))            # [K, T, B, A]
        assert preds.shape[0] == K
        want = ensemble_action(preds, H.ensemble_weights(i, K), method).astype(np.float32)
        assert np.array_equal(H.bits(out["act"][..., :B].transpose(0, 2, 1)), H.bits(want)), (key, i, K, method, "the action is the installed rule's")

    _reinstall(ni, key, ["ens_mean"], [(H.set_ensemble, v, dict(method=m, K=K)) for v, (K, m) in enumerate(seq)], check=the_installed_rule)


@pytest.mark.parametrize("key", H.MFMA)
def test_reinstalling_the_safety_ensemble(ni, key):
    """K 3 -> 1 -> 8 -> 2 and n_outputs 4 -> 1 -> 3 -> 2 with a new temperature and new limits; prob / unc / logit rows beyond the
    new n_outputs keep their canary."""
    seq = [(3, 4), (1, 1), (8, 3), (2, 2)]
    _reinstall(ni, key, ["gated"], [(H.set_gate, v, dict(K=K, C=Cn)) for v, (K, Cn) in enumerate(seq)], needs_actor=True)


@pytest.mark.parametrize("key", H.ALL)
def test_reinstalling_the_policy(ni, key):
    """affine -> PID -> affine -> PID: the second PID law starts from zero memory (its lean twin's), although the first one's
    memory was written by a launch."""
    _reinstall(ni, key, ["policy_affine"], [(H.set_affine, 0, {}), (H.set_pid, 0, {}), (H.set_affine, 1, {}), (H.set_pid, 1, {})])


# One ensemble slot and one policy slot on a handle: a loaded handle holds the averaging ensemble and the affine law.
def _play_loaded(ni, env, case, key, spread=False):
    """One case on a handle that has everything installed: a case of the other ensemble method installs its members just before
    it plays, the PID case its law (afterwards the affine law goes back in)."""
    base = H.parent_of(case)
    if base.startswith("ens_"):
        H.SETTERS[base](ni, env, key, 0)
    got = _play(ni, env, case, key, reinstall_pid=True, spread=spread)
    if base == "policy_pid":
        H.set_affine(ni, env, key)
    return got


@pytest.mark.parametrize("key", H.ALL)
def test_reinstalling_the_disturbance(ni, key):
    """Kind A -> None -> kind B on a handle that has everything installed, every case of the table played in every stage.  After
    None the disturbed entry points refuse and launch nothing, and every other family -- sampled, noise, both policy laws, the
    MFMA actor, the bf16 actor, shield, search, both ensembles, gate, projection -- still equals its twin."""
    B = _B(key)
    env = H.make(ni, key, B)
    if key in H.MFMA:
        _load(ni, env, key)
    else:
        H.set_affine(ni, env, key)
        H.set_disturbance(ni, env, key, 0)
    parents = [c for c in H.PARENTS if key in H.CASES[c][1]]
    dist = [c for c in parents if "disturbance" in H.CASES[c][3]]
    others = [c for c in parents if c not in dist]
    assert dist and len(others) >= 3
    for case in dist + others:
        _equal(_play_loaded(ni, env, case, key), _lean_v(ni, case, key, B), (case, key, "disturbance A"))
    env.set_disturbance(None)
    H.rewind(ni, env, key)
    before = H.kept(env)
    for case in dist:
        assert _code(ni, lambda: H.run(env, case)) == INVALID and "no disturbance" in env._L.nig_last_error().decode(), case
    H.same(H.kept(env), before, None, "a refused launch leaves the handle alone")
    for case in others:
        _equal(_play_loaded(ni, env, case, key), _lean_v(ni, case, key, B), (case, key, "disturbance removed"))
    H.set_disturbance(ni, env, key, 1)
    for case in dist + others:
        _equal(_play_loaded(ni, env, case, key), _lean_v(ni, case, key, B, {"disturbance": 1}), (case, key, "disturbance B"))
    env.close()


def _load(ni, env, key, variants=None):
    """Everything at once: policy, actor, bf16 actor, critic, ensemble ("mean"), gate, predictor and disturbance."""
    for inp in ("affine", "actor", "bf16", "critic", "ens_mean", "gate", "predictor", "disturbance"):
        H.SETTERS[inp](ni, env, key, (variants or {}).get(inp, 0))


LOADED_CASES = ["policy_affine", "policy_disturbed", "mlp", "mlp_bf16", "safe", "search", "ens_mean", "gated", "projected", "disturbed"]


@pytest.mark.parametrize("key", H.MFMA)
def test_installing_one_familys_inputs_leaves_the_others_alone(ni, key):
    """A loaded handle; one input after the other is replaced by a variant.  After each replacement every family equals the lean
    twin with ITS inputs in their current variants: replacing the actor keeps the critic, ensemble, gate, predictor and bf16
    actor; replacing the critic moves the shield and the search (which share its stream) and nothing else; the bf16 and the
    float32 actor of different weights coexist, each rollout following its own."""
    B = _B(key)
    env = H.make(ni, key, B)
    _load(ni, env, key)
    now = {}
    for inp in (None, "actor", "critic", "bf16", "ens_voting", "gate", "predictor", "affine", "disturbance"):
        if inp is not None:
            now[inp] = 1
            H.SETTERS[inp](ni, env, key, 1)
        for case in LOADED_CASES:
            if case == "ens_mean" and "ens_voting" in now:
                case = "ens_voting"                      # (one ensemble slot: the voting ensemble replaced the averaging one)
            _equal(_play(ni, env, case, key), _lean_v(ni, case, key, B, now), (case, key, B, f"after replacing {inp}"))
    env.close()


# ---- 3. one loaded handle against lean twins --------------------------------------------------------------------------------------
def _violated(L, fl, B):
    """The built-in constraints (bit k) that some lane-step of a launch violates, from its flag words (every lane live)."""
    w = fl[:, :B].view(np.uint32)
    assert not (w & L.FLAG_INACTIVE).any()
    bits = ((w >> L.FLAG_VIOL_SHIFT) & 7) | (((w & L.FLAG_VIOL3) != 0).astype(np.uint32) << 3)
    return int(np.bitwise_or.reduce(bits, axis=None))


@pytest.mark.parametrize("key,B", [(k, M.B_SMALL) for k in H.MFMA] + [("cr", M.B_BIG), ("pg", M.B_BIG)])
def test_one_loaded_handle_against_lean_twins(ni, key, B):
    """Everything installed at once; every case of the table in turn, each from the same rewind, equals its lean twin.
    Then a box constraint is added: H.floor in the middle of the lanes' start values of a state row, so that on step 0 it
    fires on exactly the lanes below it, in every twin on every env at both batch sizes, and no twin's xflags are compared as
    zeros with zeros (a band on action row 0 does not do that: an averaging ensemble's stays inside it over 700 HVACControl
    lanes).  Every parent refuses, and every _limited twin equals a lean handle with the same limits, xflags included.  Then
    it is removed: every twin refuses and every parent equals its lean twin again.
    Then the built-in constraint mask goes to a proper subset and back, on launches that start from H.spread_start's states (from
    their reset states five of the eight envs violate no built-in constraint in seven steps, and a mask would move nothing):
    the constraint left out is the one that fires in the most cases of this env; both times the values are the lean twin's
    with that mask, and under the subset the flag words of every case in which that constraint fires differ from the full
    mask's and no longer show it."""
    L = ni._lib
    env = H.make(ni, key, B)
    _load(ni, env, key)
    parents = [c for c in H.PARENTS if key in H.CASES[c][1]]
    twins = [c for c in H.TWINS if key in H.CASES[c][1]]
    assert bool(twins) == (key in H.LIM_MFMA)
    for case in parents:
        _equal(_play_loaded(ni, env, case, key), _lean_v(ni, case, key, B), (case, key, B, "loaded"))
    if twins:
        H.rewind(ni, env, key)
        s0 = env.get_state().cpu().numpy()                   # [B, S]: every launch of this test starts here
        row = next(r for r in range(s0.shape[1]) if s0[:, r].min() < s0[:, r].max())
        lo = float(np.float32((float(s0[:, row].min()) + float(s0[:, row].max())) / 2))
        below = s0[:, row] < np.float32(lo)
        assert below.any() and not below.all(), (key, B, row, lo)
        env.add_safety_constraint(H.floor(ni, row, lo))
        before = H.kept(env)
        for case in parents:
            assert _code(ni, lambda: H.run(env, case)) == UNSUPPORTED, (case, "limits installed: the parent refuses")
        H.same(H.kept(env), before, None, "refused launches leave the handle alone")
        for case in twins:
            got = _play_loaded(ni, env, case, key)
            _equal(got, _lean_v(ni, case, key, B, floor=(row, lo)), (case, key, B, "loaded, limits"))
            assert ((got["out"]["xf"][0, :B] != 0) == below).all(), (case, key, B, "step 0: the floor fires on the lanes below it")
        env.remove_safety_constraint("floor")
        assert not env.has_limits
        for case in twins:
            assert _code(ni, lambda: H.run(env, case)) == INVALID and "no limits installed" in env._L.nig_last_error().decode(), case
        for case in parents:
            _equal(_play_loaded(ni, env, case, key), _lean_v(ni, case, key, B), (case, key, B, "limits removed"))
    # the mask
    n = int(env.spec.n_constraints)
    full = (1 << n) - 1
    wide = {case: _lean_v(ni, case, key, B, spread=True) for case in parents}
    fires = {case: _violated(L, wide[case]["out"]["fl"], B) for case in parents}
    count = [sum((f >> k) & 1 for f in fires.values()) for k in range(n)]
    k = int(np.argmax(count))                                # (the lowest of equals)
    sub = full & ~(1 << k)
    assert count[k] > 0 and 0 < sub < full, (key, B, "no built-in constraint fires in any case", fires)
    env.set_constraint_mask(sub)
    for case in parents:
        got = _play_loaded(ni, env, case, key, spread=True)
        _equal(got, _lean_v(ni, case, key, B, cmask=sub, spread=True), (case, key, B, "mask subset"))
        if (fires[case] >> k) & 1:                           # up to its first violation the run is the full mask's; there bit k is gone
            assert not np.array_equal(got["out"]["fl"], wide[case]["out"]["fl"]), (case, key, B, k, "the mask moved nothing")
            assert not (_violated(L, got["out"]["fl"], B) >> k) & 1, (case, key, B, k, "a masked constraint fired")
    env.set_constraint_mask(full)
    for case in parents:
        _equal(_play_loaded(ni, env, case, key, spread=True), wide[case], (case, key, B, "mask restored"))
    env.close()


# ---- 4. lazy buffers between closed loops -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["cr", "pg", "ra", "hvac"])
def test_lazy_buffers_between_closed_loops(ni, key):
    """On one handle, between rollout_mlp launches: nig_step64 on an env that takes float32 actions (the narrowed rows, act32:
    HVACControl -- ChemicalReactor, PowerGrid and RobotAssembly step on the float64 action itself), rollout() on a row-major
    [R, B, A] ring at R = 2 and then R = 9 (act_soa is freed and re-grown), nig_step_host (hst_*) and a step plan.  The twin makes
    the same env steps without the side buffers: step() on equal float32 actions, rollout() on [R, A, ld] rows.  After each
    detour the detour's own results, the next closed-loop launch and everything kept equal the twin's.
    Which env holds which buffer: act32 is reached only where the step takes float32 actions, so HVACControl stands beside
    cr, pg and ra (which step on the float64 action) and the nig_step64 detour is made on it alone.  act_soa is certain on cr, ra and hvac; PowerGrid's
    launcher reads a 16-byte aligned row-major ring in place where its kernel form allows (rows_native, csrc/nig_api.hip), and
    then this ring never reaches act_soa there -- the comparison holds that path instead."""
    B = M.B_BIG
    a, b = H.make(ni, key, B), H.make(ni, key, B)
    S, A, ld, dev = a.state_dim, a.action_dim, a.ld, a.device
    for e in (a, b):
        H.set_actor(ni, e, key)
        H.rewind(ni, e, key)

    def closed_loop(what):
        oa, ob = H.run(a, "mlp"), H.run(b, "mlp")
        H.same(oa, ob, None, f"{key} rollout_mlp after {what}")
        H.same(H.kept(a), H.kept(b), None, f"{key} kept after {what}")

    def actions(t):
        return a.fill_actions(t)[:, :B].clone()                            # float32 [A, B]

    def step_results(what):
        torch.cuda.synchronize()
        assert torch.equal(a.reward.view(torch.int32), b.reward.view(torch.int32)) and torch.equal(a.flags, b.flags), (key, what)

    closed_loop("nothing")
    if key not in H.ACT64:
        for t in (40, 41):
            act = actions(t)
            a.step(act.t().contiguous().to(torch.float64), layout="aos")   # nig_step64 -> the handle's narrowed float32 rows
            b.step(act, layout="soa")
            step_results("step64")
        closed_loop("nig_step64")
    for R, n in ((2, 3), (9, 9)):
        rows = torch.zeros(R, A, ld, dtype=torch.float32, device=dev)
        for s in range(R):
            a.fill_actions(50 + 10 * R + s, rows[s])
        ring = rows[:, :, :B].permute(0, 2, 1).contiguous()                # row-major [R, B, A]
        res = []
        for e, r in ((a, ring), (b, rows)):
            rew, fl = torch.full((n, ld), H.F_CAN, dtype=torch.float32, device=dev), torch.full((n, ld), H.I_CAN, dtype=torch.int32, device=dev)
            e.rollout(n, r, rew, fl)
            res.append((rew, fl))
        torch.cuda.synchronize()
        assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(res[0][1], res[1][1]), (key, R)
        closed_loop(f"rollout() on a row-major ring of {R}")
    # nig_step_host: host arrays in and out
    act = actions(70)
    host = dict(a=np.ascontiguousarray(act.cpu().numpy()), s=np.full((S, B), H.F_CAN, np.float32), r=np.full(B, float(H.F_CAN)), f=np.full(B, H.I_CAN, np.uint32))
    hp = lambda x: x.ctypes.data_as(C.c_void_p)
    with torch.cuda.device(a._dev_index):
        ni._lib.check(a._L.nig_step_host(a._h, hp(host["a"]), None, hp(host["s"]), hp(host["r"]), hp(host["f"]), a._stream()))
    b.step(act, layout="soa")
    torch.cuda.synchronize()
    assert np.array_equal(H.bits(host["s"]), H.bits(b.state_soa.cpu().numpy())), (key, "nig_step_host state_out")
    assert np.array_equal(H.bits(host["r"]), H.bits(b.reward64.cpu().numpy())) and np.array_equal(host["f"], b.flags.cpu().numpy().view(np.uint32))
    closed_loop("nig_step_host")
    # a step plan: three steps over a ring of two
    rows = torch.zeros(2, A, ld, dtype=torch.float32, device=dev)
    for s in range(2):
        a.fill_actions(80 + s, rows[s])
    rew, fl = torch.zeros(2, ld, dtype=torch.float32, device=dev), torch.zeros(2, ld, dtype=torch.int32, device=dev)
    plan = a.make_plan(3, rows, rew, fl)
    plan.launch()
    for k in range(3):
        b.step(rows[k % 2][:, :B], layout="soa")
    torch.cuda.synchronize()
    assert torch.equal(rew[0, :B].view(torch.int32), b.reward.view(torch.int32)) and torch.equal(fl[0, :B], b.flags), (key, "the plan's third step, slot 0")
    closed_loop("a step plan")
    plan.launch()                                                          # a replay after a closed loop moved the counter
    for k in range(3):
        b.step(rows[k % 2][:, :B], layout="soa")
    closed_loop("the plan's replay")
    plan.close()
    a.close(); b.close()
