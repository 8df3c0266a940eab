"""The refusal contract of the entry points test_gpu_closed_loop_refusals.py does not pin, by that module's rules (its Rig: return
code, the exact nig_last_error() text, the launch counter and canary-filled outputs untouched; expected strings as literals; no
rollout kernel launched except by the positive controls): the nine _limited twins of the closed loops, nig_step_limited and
nig_step64_limited, the parents nig_rollout_mlp_gated / _projected / _bf16 / nig_step / nig_step64, and every parent's refusal of
a handle with limits installed.

The order the library keeps:
  the seven later twins (_mlp_safe_, _search_, _gated_, _projected_, _ensemble_, _policy_disturbed_, _mlp_disturbed_limited):
    bad argument; no limits installed (code 1); no MFMA actor (code 4, the MFMA twins); the parent's refusals in the parent's order;
    out_stride, obs_out, the action pitch, the counter.  Their parents: the same with "limits are installed" (code 4) second.
  the early four pairs (nig_step, nig_step64, nig_rollout_policy, nig_rollout_mlp): the parent asks "limits are installed" before its
    own prerequisites (the step pair before the NULL-handle check); the twin asks its own prerequisites first and "no limits
    installed" after them.  nig_rollout_mlp and its twin answer an env without the MFMA actor with code 1, "no actor installed".
  the Advanced pair takes no limits, so every twin stops at "no limits installed".

Handles: 64 lanes, one step, auto-reset.  ChemicalReactor-v0 (MFMA actor, native float64 step), WaterTreatment-v0 (no MFMA actor,
float32 step: nig_step64 narrows the rows first), AdvancedChemicalReactor-v0 (takes no limits)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_closed_loop_refusals import (B, BAD_ACT, BAD_CANDIDATES, BAD_OBS, BAD_OUT_STRIDE, BAD_SEEN, BAD_SHAPE, CANARY_F, INVALID,
                                           MAX_CANDIDATES, NO_ACTOR, NO_CRITIC, NO_DISTURBANCE, NO_ENSEMBLE, NO_MFMA, NO_POLICY, OK,
                                           UNSUPPORTED, WRAP, Rig, _network, ni)  # noqa: F401  (ni: the module's fixture)

pytestmark = pytest.mark.gpu

LIMITS = ("limits are installed (nig_set_limits): this entry point does not know them -- use nig_step_limited / nig_step64_limited / "
          "nig_rollout_policy_limited / nig_rollout_mlp_limited, or remove them with nig_set_limits(h, 0, ...)")
NO_LIMITS = "no limits installed (nig_set_limits)"
NO_GATE = "no safety ensemble installed (nig_set_mlp_safety_ensemble)"
NO_PREDICTOR = "no constraint predictor installed (nig_set_mlp_constraint)"
NO_BF16 = "no bf16 actor installed (nig_set_mlp_policy_bf16)"
BAD_LD_C = "ld_c outside [batch, 2^26]"
BAD_C_STEP = "c_step_stride smaller than one [n_outputs][ld_c] block"
BAD_ITERS = "max_iters outside 1 .. NIG_MAX_PROJECT_ITERS"
BAD_STEP = "step must be finite"
BAD_GRAD = "bad action trajectory pitch (grad_out takes act_out's)"
BAD_HID = "bad hidden-activation pitch"
NULL_HANDLE = "NULL handle"
BAD_ACTIONS = "actions NULL or ld_act outside [batch, 2^26]"
NEEDS_STEP_NOISE = "parity mode needs step_noise"
NEEDS_RESET_NOISE = "parity mode with auto-reset needs reset_noise"
BAD_LD_NOISE = "ld_noise outside [batch, 2^26]"
BAD_LD_OBS = "ld_obs outside [batch, 2^26]"
NO_LIMITS_FOR_ADVANCED = "the Advanced envs override step() wholesale: no added constraints"
MAX_PROJECT_ITERS = 16
N_OUT = 2           # head columns of the installed safety ensemble and constraint predictor

STEPS = ["nig_step", "nig_step64"]
PINNED_PARENTS = ["nig_rollout_policy", "nig_rollout_mlp", "nig_rollout_mlp_safe", "nig_rollout_mlp_search", "nig_rollout_mlp_ensemble",
                  "nig_rollout_policy_disturbed", "nig_rollout_mlp_disturbed"]
TWINNED = PINNED_PARENTS + ["nig_rollout_mlp_gated", "nig_rollout_mlp_projected"]
PARENTS = TWINNED + ["nig_rollout_mlp_bf16"]
TWINS = [fn + "_limited" for fn in TWINNED]
EARLY_TWINS = ["nig_rollout_policy_limited", "nig_rollout_mlp_limited"]
LATER_TWINS = [fn for fn in TWINS if fn not in EARLY_TWINS]
MFMA_LATER_TWINS = [fn for fn in LATER_TWINS if "_mlp_" in fn]


def _bad_argument(fn):
    return "bad argument (handle, n_steps)" if "_ensemble" in fn else "bad argument"


def _base(fn):
    return fn[:-len("_limited")] if fn.endswith("_limited") else fn


class LimRig(Rig):
    """The module's Rig for every closed-loop family, twins and the step entry points included."""

    def __init__(self, ni, name, limits=False):
        super().__init__(ni, name)
        dev, A, S = self.env.device, self.A, self.S
        canary = lambda *shape: torch.full(shape, CANARY_F, device=dev)
        self.xf = canary(1, B)
        self.crows = [canary(1, N_OUT, B), canary(1, N_OUT, B)]                 # prob / unc (gate), prob / viol (projection)
        self.logit, self.iters, self.grad = canary(1, 2, N_OUT, B), canary(1, B), canary(1, A, B)
        self.hid, self.final = canary(1, 256, B), canary(S, B)                  # (hid_out: 512 rows of 16-bit words)
        self.canaries += [self.xf, self.logit, self.iters, self.grad, self.hid, self.final] + self.crows
        self.actions = torch.zeros(A, B, device=dev)
        self.actions64 = torch.zeros(A, B, dtype=torch.float64, device=dev)
        self.noise = torch.zeros(32, B, dtype=torch.float64, device=dev)
        if limits:
            self.env.add_safety_constraint(ni.BoxConstraint("trip", {("action", 0): (-0.6, 0.6)}, -5.0, critical=True))

    def install(self, *what):
        ni, env, S, A, rng = self.ni, self.env, self.S, self.A, np.random.default_rng(9)
        for w in what:
            {"policy": lambda: env.set_policy(ni.mpc_agent(S, A)),
             "actor": lambda: env.set_mlp_policy(_network(rng, S, A)),
             "bf16": lambda: env.set_mlp_policy_bf16(_network(rng, S, A)),
             "critic": lambda: env.set_mlp_safety(_network(rng, S + A, 1), 0.5),
             "ensemble": lambda: env.set_mlp_ensemble([_network(rng, S, A)], None, None, "voting", 0.2),
             "gate": lambda: env.set_mlp_safety_ensemble([_network(rng, S + A, N_OUT), _network(rng, S + A, N_OUT)], 1.0, 0.5, 0.2),
             "predictor": lambda: env.set_mlp_constraint(_network(rng, S + A, N_OUT), 0.1, 0.01),
             "disturbance": lambda: env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.2, clip=(-1, 1), hold="episode")),
             }[w]()

    def call(self, fn, h="own", n=1, n_candidates=4, bad=(), outputs=None, member_only=False):
        """Rig.call's `bad` and: "ld_c", "c_step" (gate, projection), "max_iters", "step", "grad" (projection), "hid" (bf16);
        for the step entry points "actions", "ld_act", "step_noise", "reset_noise", "ld_noise", "ld_obs"."""
        if fn.startswith("nig_step"):
            return self._step(fn, h, bad, outputs)
        S, A, base = self.S, self.A, _base(fn)
        rw, fl = outputs if outputs else (self.rw, self.fl)
        opt = lambda t, on=True: t.data_ptr() if bad and on else None      # an optional output: passed once something is to be got wrong
        shared = [rw.data_ptr(), fl.data_ptr(), B - 1 if "out_stride" in bad else B,
                  self.obs.data_ptr() + (4 if "obs" in bad else 0) if bad else None, B * S,
                  opt(self.act, not member_only), B - 1 if ("act" in bad or "grad" in bad) else B, A * B]
        rows = [None if outputs else r.data_ptr() for r in self.rows]
        pitch_c = [B - 1 if "ld_c" in bad else B, N_OUT * B - (1 if "c_step" in bad else 0)] if bad else [0, 0]
        head = [self.env._h if h == "own" else h, n]
        if base == "nig_rollout_mlp_search":
            head.append(n_candidates)
        if base == "nig_rollout_mlp_projected":
            head += [0 if "max_iters" in bad else 4, float("nan") if "step" in bad else 0.1]
        extra = {"nig_rollout_policy": lambda: [], "nig_rollout_mlp": lambda: [], "nig_rollout_mlp_safe": lambda: rows[:1],
                 "nig_rollout_mlp_search": lambda: rows,
                 "nig_rollout_mlp_ensemble": lambda: [rows[0], self.member.data_ptr() if member_only else None],
                 "nig_rollout_mlp_gated": lambda: [opt(self.crows[0]), opt(self.crows[1]), opt(self.logit)] + pitch_c,
                 "nig_rollout_mlp_projected": lambda: [opt(self.crows[0]), opt(self.crows[1]), opt(self.iters), opt(self.grad, "grad" in bad)] + pitch_c,
                 "nig_rollout_mlp_bf16": lambda: [opt(self.hid), B - 1 if "hid" in bad else B, 512 * B],
                 }.get(base, lambda: [self.seen.data_ptr() + (4 if "seen" in bad else 0) if bad else None, B * S])()
        if fn != base:
            extra.append(torch.zeros(1, B, dtype=torch.int32, device=self.env.device).data_ptr() if outputs else self.xf.data_ptr())
        if "wrap" in bad:
            assert self.lib.nig_set_counter(self.env._h, 0xFFFFFFFF) == OK
        return getattr(self.lib, fn)(*head, *shared, *extra, self.env._stream())

    def _step(self, fn, h, bad, outputs):
        rw, fl = outputs if outputs else (self.rw, self.fl)
        actions = self.actions64 if "64" in fn else self.actions
        noise = lambda name: self.noise.data_ptr() if name in bad else None     # "step_noise" / "reset_noise": that array alone is given
        args = [self.env._h if h == "own" else h, None if "actions" in bad else actions.data_ptr(), B - 1 if "ld_act" in bad else B,
                noise("step_noise"), noise("reset_noise"), B - 1 if "ld_noise" in bad else B, rw.data_ptr(), None, fl.data_ptr()]
        if fn.endswith("_limited"):
            args.append(torch.zeros(B, dtype=torch.int32, device=self.env.device).data_ptr() if outputs else self.xf.data_ptr())
        args += [self.final.data_ptr() if "ld_obs" in bad else None, B - 1 if "ld_obs" in bad else B]
        return getattr(self.lib, fn)(*args, self.env._stream())

    def argument_order(self, fn):
        """after the prerequisites: the family's own range checks, then out_stride, obs_out, the action pitch, the counter -- the
        first wrong one is named"""
        own = {"nig_rollout_policy_disturbed": [("seen", BAD_SEEN)], "nig_rollout_mlp_disturbed": [("seen", BAD_SEEN)],
               "nig_rollout_mlp_gated": [("ld_c", BAD_LD_C), ("c_step", BAD_C_STEP)],
               "nig_rollout_mlp_projected": [("max_iters", BAD_ITERS), ("step", BAD_STEP), ("ld_c", BAD_LD_C), ("c_step", BAD_C_STEP), ("grad", BAD_GRAD)],
               "nig_rollout_mlp_bf16": [("hid", BAD_HID)]}.get(_base(fn), [])
        checks = own + [("out_stride", BAD_OUT_STRIDE), ("obs", BAD_OBS), ("act", BAD_ACT), ("wrap", WRAP)]
        for k, (_, text) in enumerate(checks):
            self.refused(fn, INVALID, text, bad=tuple(name for name, _ in checks[k:]))

    def step_order(self, fn):
        """check_step's order on an auto-reset handle of an env with step noise"""
        self.refused(fn, INVALID, BAD_ACTIONS, bad=("actions", "step_noise", "ld_noise", "ld_obs"))
        self.refused(fn, INVALID, BAD_ACTIONS, bad=("ld_act", "reset_noise", "ld_noise", "ld_obs"))
        self.refused(fn, INVALID, NEEDS_STEP_NOISE, bad=("reset_noise", "ld_noise", "ld_obs"))
        self.refused(fn, INVALID, NEEDS_RESET_NOISE, bad=("step_noise", "ld_noise", "ld_obs"))
        self.refused(fn, INVALID, BAD_LD_NOISE, bad=("step_noise", "reset_noise", "ld_noise", "ld_obs"))
        self.refused(fn, INVALID, BAD_LD_OBS, bad=("step_noise", "reset_noise", "ld_obs"))
        self.refused(fn, INVALID, BAD_LD_OBS, bad=("ld_obs",))


EVERYTHING = ("policy", "actor", "bf16", "critic", "ensemble", "gate", "predictor", "disturbance")


@pytest.mark.parametrize("limits", [False, True])
def test_bad_argument_comes_first(ni, limits):
    """before the limits are asked about, whichever way: NULL handle and n_steps <= 0 (the step pair: see test_step_pair)"""
    rig = LimRig(ni, "ChemicalReactor-v0", limits=limits)
    for fn in TWINS + PARENTS:
        rig.refused(fn, INVALID, _bad_argument(fn), h=None)
        rig.refused(fn, INVALID, _bad_argument(fn), n=0)
        rig.refused(fn, INVALID, _bad_argument(fn), n=-1)


def test_parents_refuse_installed_limits(ni):
    """code 4 with the full text, before any prerequisite of the parent's own (nothing is installed, then everything), before the
    step pair's argument checks, and on the env without the MFMA actor before its shape is asked about"""
    rig = LimRig(ni, "ChemicalReactor-v0", limits=True)
    for installed in ((), EVERYTHING):
        rig.install(*installed)
        for fn in PARENTS + STEPS:
            rig.refused(fn, UNSUPPORTED, LIMITS)
        rig.refused("nig_rollout_mlp_search", UNSUPPORTED, LIMITS, n_candidates=0)
        for fn in STEPS:
            rig.refused(fn, UNSUPPORTED, LIMITS, bad=("actions", "ld_obs"))
    water = LimRig(ni, "WaterTreatment-v0", limits=True)
    for fn in PARENTS + STEPS:
        water.refused(fn, UNSUPPORTED, LIMITS)


def test_chain_without_limits(ni):
    """the three parents no order was pinned for, and where each twin stops on a handle without limits"""
    rig = LimRig(ni, "ChemicalReactor-v0")
    # nothing installed: the later twins ask for limits first, the early twins for their own prerequisite
    for fn in LATER_TWINS:
        rig.refused(fn, INVALID, NO_LIMITS)
    rig.refused("nig_rollout_mlp_search_limited", INVALID, NO_LIMITS, n_candidates=0)
    rig.refused("nig_rollout_policy_limited", INVALID, NO_POLICY)
    rig.refused("nig_rollout_mlp_limited", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_gated", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_projected", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_bf16", INVALID, NO_BF16)
    # the actor
    rig.install("actor")
    rig.refused("nig_rollout_mlp_bf16", INVALID, NO_BF16)             # (the float32 actor is not the bf16 one)
    rig.refused("nig_rollout_mlp_gated", INVALID, NO_GATE)
    rig.refused("nig_rollout_mlp_projected", INVALID, NO_PREDICTOR)
    rig.refused("nig_rollout_mlp_projected", INVALID, NO_PREDICTOR, bad=("max_iters", "step"))       # the predictor before the ranges
    rig.refused("nig_rollout_mlp_limited", INVALID, NO_LIMITS)
    # everything
    rig.install(*EVERYTHING)
    for fn in TWINS:
        rig.refused(fn, INVALID, NO_LIMITS)
    for fn in ("nig_rollout_mlp_gated", "nig_rollout_mlp_projected", "nig_rollout_mlp_bf16"):
        rig.accepted(fn)
        rig.argument_order(fn)
    rig.refused("nig_rollout_mlp_projected", INVALID, BAD_ITERS, bad=("max_iters",))


def test_twin_chain_under_limits(ni):
    """nothing installed -> policy, actor -> critic -> ensemble, gate, predictor -> disturbance; then every twin accepts, and names
    its first wrong argument"""
    rig = LimRig(ni, "ChemicalReactor-v0", limits=True)
    rig.refused("nig_rollout_policy_limited", INVALID, NO_POLICY)
    rig.refused("nig_rollout_policy_disturbed_limited", INVALID, NO_POLICY)
    rig.refused("nig_rollout_mlp_limited", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_safe_limited", INVALID, NO_ACTOR)
    for n_candidates in (0, MAX_CANDIDATES + 1):                    # checked before the actor
        rig.refused("nig_rollout_mlp_search_limited", INVALID, BAD_CANDIDATES, n_candidates=n_candidates)
    rig.refused("nig_rollout_mlp_search_limited", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_gated_limited", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_projected_limited", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_ensemble_limited", INVALID, NO_ENSEMBLE)
    rig.refused("nig_rollout_mlp_disturbed_limited", INVALID, NO_ACTOR)
    rig.install("policy", "actor")
    rig.refused("nig_rollout_policy_disturbed_limited", INVALID, NO_DISTURBANCE)
    rig.refused("nig_rollout_mlp_safe_limited", INVALID, NO_CRITIC)
    rig.refused("nig_rollout_mlp_search_limited", INVALID, BAD_CANDIDATES, n_candidates=0)
    rig.refused("nig_rollout_mlp_search_limited", INVALID, NO_CRITIC)
    rig.refused("nig_rollout_mlp_gated_limited", INVALID, NO_GATE)
    rig.refused("nig_rollout_mlp_projected_limited", INVALID, NO_PREDICTOR)
    rig.refused("nig_rollout_mlp_projected_limited", INVALID, NO_PREDICTOR, bad=("max_iters", "step"))
    rig.refused("nig_rollout_mlp_ensemble_limited", INVALID, NO_ENSEMBLE)
    rig.refused("nig_rollout_mlp_disturbed_limited", INVALID, NO_DISTURBANCE)
    rig.accepted("nig_rollout_policy_limited")
    rig.accepted("nig_rollout_mlp_limited")
    rig.install("critic")
    rig.refused("nig_rollout_mlp_search_limited", INVALID, BAD_CANDIDATES, n_candidates=MAX_CANDIDATES + 1)
    rig.accepted("nig_rollout_mlp_safe_limited")
    rig.accepted("nig_rollout_mlp_search_limited")
    rig.install("ensemble", "gate", "predictor", "disturbance")
    for fn in TWINS:
        rig.accepted(fn)
        rig.argument_order(fn)
    rig.refused("nig_rollout_mlp_projected_limited", INVALID, BAD_ITERS, bad=("max_iters",))
    # member_act_out is checked through act_out's pitches where act_out is absent
    rig.refused("nig_rollout_mlp_ensemble_limited", INVALID, BAD_ACT, bad=("act",), member_only=True)
    # the limits removed: the twins stop there again, the parents run
    rig.env.remove_safety_constraint("trip")
    for fn in TWINS:
        rig.refused(fn, INVALID, NO_LIMITS)
    rig.accepted("nig_rollout_mlp_gated")


def test_env_without_mfma_actor(ni):
    """WaterTreatment-v0 takes limits and has no MFMA actor"""
    rig = LimRig(ni, "WaterTreatment-v0")
    rig.refused("nig_rollout_mlp_gated", UNSUPPORTED, NO_MFMA)
    rig.refused("nig_rollout_mlp_projected", UNSUPPORTED, NO_MFMA)
    rig.refused("nig_rollout_mlp_projected", UNSUPPORTED, NO_MFMA, bad=("max_iters",))
    rig.refused("nig_rollout_mlp_bf16", UNSUPPORTED, BAD_SHAPE)
    for fn in LATER_TWINS:                                          # the limits before the shape
        rig.refused(fn, INVALID, NO_LIMITS)
    rig.refused("nig_rollout_mlp_limited", INVALID, NO_ACTOR)
    rig = LimRig(ni, "WaterTreatment-v0", limits=True)
    for fn in MFMA_LATER_TWINS:
        rig.refused(fn, UNSUPPORTED, NO_MFMA)
    rig.refused("nig_rollout_mlp_search_limited", UNSUPPORTED, NO_MFMA, n_candidates=0)      # the shape before n_candidates
    rig.refused("nig_rollout_mlp_limited", INVALID, NO_ACTOR)        # (no actor can be installed: the pair says so, code 1)
    rig.refused("nig_rollout_policy_limited", INVALID, NO_POLICY)
    rig.refused("nig_rollout_policy_disturbed_limited", INVALID, NO_POLICY)
    rig.install("policy")
    rig.refused("nig_rollout_policy_disturbed_limited", INVALID, NO_DISTURBANCE)
    rig.install("disturbance")
    for fn in ("nig_rollout_policy_limited", "nig_rollout_policy_disturbed_limited"):
        rig.accepted(fn)
        rig.argument_order(fn)
    rig.refused("nig_rollout_mlp_disturbed_limited", UNSUPPORTED, NO_MFMA)


def test_advanced_env_takes_no_limits(ni):
    """AdvancedChemicalReactor-v0: nig_set_limits refuses, so every twin stops at "no limits installed" (the early twins after their
    own prerequisite), and every parent runs its own chain"""
    rig = LimRig(ni, "AdvancedChemicalReactor-v0")
    with pytest.raises(ni._lib.NigError) as e:
        rig.env.add_safety_constraint(ni.BoxConstraint("trip", {("action", 0): (-0.6, 0.6)}, -5.0))
    assert str(e.value) == f"libnig error {UNSUPPORTED}: nig_set_limits: {NO_LIMITS_FOR_ADVANCED}"
    assert rig.lib.nig_get_limit_count(rig.env._h) == 0
    for fn in LATER_TWINS + ["nig_step_limited", "nig_step64_limited"]:
        rig.refused(fn, INVALID, NO_LIMITS)
    rig.refused("nig_rollout_policy_limited", INVALID, NO_POLICY)
    rig.refused("nig_rollout_mlp_limited", INVALID, NO_ACTOR)
    rig.refused("nig_step_limited", INVALID, BAD_ACTIONS, bad=("actions",))
    rig.install(*EVERYTHING)
    for fn in TWINS:
        rig.refused(fn, INVALID, NO_LIMITS)
    for fn in ("nig_rollout_mlp_gated", "nig_rollout_mlp_projected", "nig_rollout_mlp_bf16", "nig_step", "nig_step64"):
        rig.accepted(fn)


@pytest.mark.parametrize("name", ["ChemicalReactor-v0", "WaterTreatment-v0"])
def test_step_pair(ni, name):
    """nig_step / nig_step64 and their twins: the argument checks in check_step's order; the parent asks about limits before them
    (even before the NULL handle, which that question tolerates), the twin after them.  A call counts one step, on the env
    whose float64 rows are narrowed first as on the one that takes them."""
    rig = LimRig(ni, name)
    for fn in STEPS:
        rig.refused(fn, INVALID, NULL_HANDLE, h=None)
        rig.step_order(fn)
        rig.accepted(fn)
    for fn in ("nig_step_limited", "nig_step64_limited"):
        rig.refused(fn, INVALID, NULL_HANDLE, h=None)
        rig.step_order(fn)
        rig.refused(fn, INVALID, NO_LIMITS)
    rig = LimRig(ni, name, limits=True)
    for fn in STEPS:
        rig.refused(fn, INVALID, NULL_HANDLE, h=None)               # (no handle, no limits to refuse for)
        rig.refused(fn, UNSUPPORTED, LIMITS)
        rig.refused(fn, UNSUPPORTED, LIMITS, bad=("actions", "step_noise", "ld_noise", "ld_obs"))
    for fn in ("nig_step_limited", "nig_step64_limited"):
        rig.refused(fn, INVALID, NULL_HANDLE, h=None)
        rig.step_order(fn)
        rig.accepted(fn)
