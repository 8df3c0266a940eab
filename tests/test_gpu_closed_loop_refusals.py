"""The refusal contract of the seven closed-loop entry points and the three weight uploads, pinned call by call through ctypes:
return code, the exact nig_last_error() text, the launch counter and canary-filled outputs untouched.  The expected strings are
literals (the text csrc/nig_api.hip has carried since each entry point was added), so the test pins the library's behaviour
and not the way the host layer is arranged.  Every call but the positive controls is refused: no rollout kernel is launched.

Handles: 64 lanes, one step.  ChemicalReactor-v0 has the MFMA actor; WaterTreatment-v0 (15 states) is the one env without it."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, SEED = 64, 0x5EED
OK, INVALID, UNSUPPORTED = 0, 1, 4
CANARY_F, CANARY_I = -7.0, 77
MAX_CANDIDATES = 128

NO_POLICY = "no policy installed (nig_set_policy)"
NO_ACTOR = "no actor installed (nig_set_mlp_policy)"
NO_CRITIC = "no safety critic installed (nig_set_mlp_safety)"
NO_ENSEMBLE = "no ensemble installed (nig_set_mlp_ensemble)"
NO_DISTURBANCE = "no disturbance installed (nig_set_disturbance)"
NO_MFMA = "env shape has no MFMA actor"
BAD_CANDIDATES = "n_candidates outside 1 .. NIG_MAX_CANDIDATES"
BAD_HIDDEN = "hidden must be 256 (agents/networks.py default)"
BAD_SHAPE = "env shape not supported (even state dim, at most 16 actions)"
BAD_OUT_STRIDE = "out_stride outside {0} U [batch, 2^26]"
BAD_OBS = "obs_out needs 16-byte alignment and obs_step_stride >= S*batch (multiple of 4)"
BAD_SEEN = "seen_out needs 16-byte alignment and seen_step_stride >= S*batch (multiple of 4)"
BAD_ACT = "bad action trajectory pitch"
WRAP = "launch counter would wrap"

ROLLOUTS = ["nig_rollout_policy", "nig_rollout_mlp", "nig_rollout_mlp_safe", "nig_rollout_mlp_search", "nig_rollout_mlp_ensemble",
            "nig_rollout_policy_disturbed", "nig_rollout_mlp_disturbed"]
BAD_ARGUMENT = {fn: "bad argument" for fn in ROLLOUTS}
BAD_ARGUMENT["nig_rollout_mlp_ensemble"] = "bad argument (handle, n_steps)"


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return ni


def _network(rng, n_in, n_out):
    """[(W1, b1), (W2, b2), (W3, b3)] of a small-weight n_in -> 256 -> 256 -> n_out network, [in, out] as set_mlp_policy takes it"""
    shapes = [(n_in, 256), (256, 256), (256, n_out)]
    return [((rng.standard_normal(s) * 0.05).astype(np.float32), np.zeros(s[1], dtype=np.float32)) for s in shapes]


class Rig:
    """One handle with canary-filled outputs; call() makes one ctypes call of a closed-loop entry point."""

    def __init__(self, ni, name):
        self.ni, self.lib = ni, ni._lib.lib()
        self.env = ni.make_batched(name, B, seed=SEED)
        self.env.reset()
        self.S, self.A, dev = self.env.state_dim, self.env.action_dim, self.env.device
        self.rw = torch.full((1, B), CANARY_F, device=dev)
        self.fl = torch.full((1, B), CANARY_I, dtype=torch.int32, device=dev)
        self.rows = [torch.full((1, B), CANARY_F, device=dev) for _ in range(3)]        # prob / unc, risk, choice (refused: never read)
        self.obs = torch.full((1, B, self.S), CANARY_F, device=dev)
        self.seen = torch.full((1, B, self.S), CANARY_F, device=dev)
        self.act = torch.full((1, self.A, B), CANARY_F, device=dev)
        self.member = torch.full((1, 1, self.A, B), CANARY_F, device=dev)
        self.canaries = [self.rw, self.obs, self.seen, self.act, self.member] + self.rows

    def counter(self):
        t = C.c_uint32(0)
        assert self.lib.nig_get_counter(self.env._h, C.byref(t)) == OK
        return t.value

    def call(self, fn, h="own", n=1, n_candidates=4, bad=(), outputs=None, member_only=False):
        """bad: which of "seen", "out_stride", "obs", "act", "wrap" to get wrong, all at once.  outputs: the reward / flags rows
        of an accepted call (the canaries otherwise)."""
        S, A = self.S, self.A
        rw, fl = outputs if outputs else (self.rw, self.fl)
        shared = [rw.data_ptr(), fl.data_ptr(), B - 1 if "out_stride" in bad else B,
                  self.obs.data_ptr() + (4 if "obs" in bad else 0) if bad else None, B * S,
                  self.act.data_ptr() if bad and not member_only else None, B - 1 if "act" in bad else B, A * B]
        rows = [None if outputs else r.data_ptr() for r in self.rows]
        extra = {"nig_rollout_policy": [], "nig_rollout_mlp": [], "nig_rollout_mlp_safe": rows[:1], "nig_rollout_mlp_search": rows,
                 "nig_rollout_mlp_ensemble": [rows[0], self.member.data_ptr() if member_only else None],
                 "nig_rollout_policy_disturbed": None, "nig_rollout_mlp_disturbed": None}[fn]
        if extra is None:
            extra = [self.seen.data_ptr() + (4 if "seen" in bad else 0) if bad else None, B * S]
        head = [self.env._h if h == "own" else h, n] + ([n_candidates] if fn == "nig_rollout_mlp_search" else [])
        if "wrap" in bad:
            assert self.lib.nig_set_counter(self.env._h, 0xFFFFFFFF) == OK
        rc = getattr(self.lib, fn)(*head, *shared, *extra, self.env._stream())
        return rc

    def refused(self, fn, code, text, **kw):
        t0 = self.counter()
        rc = self.call(fn, **kw)
        t1 = self.counter() if "wrap" not in kw.get("bad", ()) else self._unwrap(t0)
        assert (rc, self.lib.nig_last_error().decode()) == (code, f"{fn}: {text}"), (fn, kw)
        assert t1 == t0, (fn, kw, "a refused call moved the launch counter")
        torch.cuda.synchronize()
        assert all(bool((c == CANARY_F).all()) for c in self.canaries) and bool((self.fl == CANARY_I).all()), (fn, kw, "a refused call wrote")

    def _unwrap(self, t0):
        """after a call made at counter 2^32 - 1: it is still there; put the handle's own count back"""
        assert self.counter() == 0xFFFFFFFF, "a refused call moved the launch counter"
        assert self.lib.nig_set_counter(self.env._h, t0) == OK
        return t0

    def accepted(self, fn):
        dev = self.env.device
        out = (torch.zeros(1, B, device=dev), torch.zeros(1, B, dtype=torch.int32, device=dev))
        t0 = self.counter()
        rc = self.call(fn, outputs=out)
        assert rc == OK, (fn, self.lib.nig_last_error())
        assert self.counter() == t0 + 1, fn
        torch.cuda.synchronize()

    def argument_order(self, fn):
        """after the prerequisites: [seen_out,] out_stride, obs_out, the action pitch, the counter -- the first wrong one is named"""
        checks = [("out_stride", BAD_OUT_STRIDE), ("obs", BAD_OBS), ("act", BAD_ACT), ("wrap", WRAP)]
        if fn.endswith("_disturbed"):
            checks.insert(0, ("seen", BAD_SEEN))
        for k, (_, text) in enumerate(checks):
            self.refused(fn, INVALID, text, bad=tuple(name for name, _ in checks[k:]))

    def set_weights(self, fn, hidden, net):
        """nig_set_mlp_policy / _safety / _ensemble (one member, voting) with the six arrays of `net`"""
        arrays = [np.ascontiguousarray(x) for pair in net for x in pair]
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in arrays]
        h, st = self.env._h, self.env._stream()
        if fn == "nig_set_mlp_policy":
            return self.lib.nig_set_mlp_policy(h, hidden, *ptrs, st)
        if fn == "nig_set_mlp_safety":
            return self.lib.nig_set_mlp_safety(h, hidden, *ptrs, 0.5, st)
        cols = [(C.c_void_p * 1)(a.ctypes.data) for a in arrays]
        return self.lib.nig_set_mlp_ensemble(h, 1, hidden, *cols, self.ni._lib.ENSEMBLE_VOTING, None, 0.0, 0.2, st)

    def weights_refused(self, fn, hidden, net, text):
        assert self.set_weights(fn, hidden, net) == UNSUPPORTED
        assert self.lib.nig_last_error().decode() == f"{fn}: {text}"


def test_null_handle_and_step_count(ni):
    rig = Rig(ni, "ChemicalReactor-v0")
    for fn in ROLLOUTS:
        rig.refused(fn, INVALID, BAD_ARGUMENT[fn], h=None)
        rig.refused(fn, INVALID, BAD_ARGUMENT[fn], n=0)
        rig.refused(fn, INVALID, BAD_ARGUMENT[fn], n=-1)


def test_actor_chain(ni):
    """nothing installed -> actor only -> actor and critic (-> ensemble and disturbance for the positive controls)"""
    rig = Rig(ni, "ChemicalReactor-v0")
    S, A, rng = rig.S, rig.A, np.random.default_rng(7)
    actor, critic = _network(rng, S, A), _network(rng, S + A, 1)
    # nothing installed
    rig.refused("nig_rollout_mlp", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_safe", INVALID, NO_ACTOR)
    for n_candidates in (0, MAX_CANDIDATES + 1):                    # checked before the actor
        rig.refused("nig_rollout_mlp_search", INVALID, BAD_CANDIDATES, n_candidates=n_candidates)
    rig.refused("nig_rollout_mlp_search", INVALID, NO_ACTOR)
    rig.refused("nig_rollout_mlp_ensemble", INVALID, NO_ENSEMBLE)
    rig.refused("nig_rollout_mlp_disturbed", INVALID, NO_ACTOR)
    for fn, net in (("nig_set_mlp_policy", actor), ("nig_set_mlp_safety", critic), ("nig_set_mlp_ensemble", actor)):
        rig.weights_refused(fn, 128, net, BAD_HIDDEN)
    rig.refused("nig_rollout_mlp", INVALID, NO_ACTOR)                # the refused uploads installed nothing
    rig.refused("nig_rollout_mlp_ensemble", INVALID, NO_ENSEMBLE)
    # actor only
    assert rig.set_weights("nig_set_mlp_policy", 256, actor) == OK, rig.lib.nig_last_error()
    rig.refused("nig_rollout_mlp_safe", INVALID, NO_CRITIC)
    rig.refused("nig_rollout_mlp_search", INVALID, BAD_CANDIDATES, n_candidates=0)
    rig.refused("nig_rollout_mlp_search", INVALID, NO_CRITIC)
    rig.refused("nig_rollout_mlp_ensemble", INVALID, NO_ENSEMBLE)
    rig.refused("nig_rollout_mlp_disturbed", INVALID, NO_DISTURBANCE)
    rig.accepted("nig_rollout_mlp")
    # actor and critic
    assert rig.set_weights("nig_set_mlp_safety", 256, critic) == OK, rig.lib.nig_last_error()
    rig.refused("nig_rollout_mlp_search", INVALID, BAD_CANDIDATES, n_candidates=MAX_CANDIDATES + 1)
    rig.refused("nig_rollout_mlp_ensemble", INVALID, NO_ENSEMBLE)
    rig.accepted("nig_rollout_mlp_safe")
    rig.accepted("nig_rollout_mlp_search")
    # the ensemble and a disturbance beside them: every MFMA entry point accepts, and names its first wrong argument
    assert rig.set_weights("nig_set_mlp_ensemble", 256, actor) == OK, rig.lib.nig_last_error()
    rig.env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.2, clip=(-1, 1), hold="episode"))
    rig.accepted("nig_rollout_mlp_ensemble")
    rig.accepted("nig_rollout_mlp_disturbed")
    for fn in ROLLOUTS:
        if "_mlp" in fn:
            rig.argument_order(fn)
    # member_act_out is checked through act_out's pitches where act_out is absent
    rig.refused("nig_rollout_mlp_ensemble", INVALID, BAD_ACT, bad=("act",), member_only=True)


@pytest.mark.parametrize("name", ["ChemicalReactor-v0", "WaterTreatment-v0"])
def test_policy_chain(ni, name):
    """nothing installed -> policy only -> policy and disturbance; the policy kernels exist for every env shape"""
    rig = Rig(ni, name)
    rig.refused("nig_rollout_policy", INVALID, NO_POLICY)
    rig.refused("nig_rollout_policy_disturbed", INVALID, NO_POLICY)
    rig.env.set_policy(ni.mpc_agent(rig.S, rig.A))
    rig.refused("nig_rollout_policy_disturbed", INVALID, NO_DISTURBANCE)
    rig.accepted("nig_rollout_policy")
    rig.env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.2, clip=(-1, 1), hold="episode"))
    rig.accepted("nig_rollout_policy_disturbed")
    rig.argument_order("nig_rollout_policy")
    rig.argument_order("nig_rollout_policy_disturbed")
    rig.env.set_disturbance(None)
    rig.refused("nig_rollout_policy_disturbed", INVALID, NO_DISTURBANCE)


def test_env_without_mfma_actor(ni):
    """WaterTreatment-v0: the shape is refused before anything else is asked, by the uploads and by the rollouts"""
    rig = Rig(ni, "WaterTreatment-v0")
    S, A, rng = rig.S, rig.A, np.random.default_rng(8)
    actor, critic = _network(rng, S, A), _network(rng, S + A, 1)
    for fn, net in (("nig_set_mlp_policy", actor), ("nig_set_mlp_safety", critic), ("nig_set_mlp_ensemble", actor)):
        rig.weights_refused(fn, 128, net, BAD_HIDDEN)               # the hidden width is asked first
        rig.weights_refused(fn, 256, net, BAD_SHAPE)
    rig.refused("nig_rollout_mlp", INVALID, NO_ACTOR)                # (no actor can be installed: the entry point says so)
    for fn in ("nig_rollout_mlp_safe", "nig_rollout_mlp_search", "nig_rollout_mlp_ensemble", "nig_rollout_mlp_disturbed"):
        rig.refused(fn, UNSUPPORTED, NO_MFMA)
    rig.refused("nig_rollout_mlp_search", UNSUPPORTED, NO_MFMA, n_candidates=0)      # the shape before n_candidates
    rig.env.set_disturbance(ni.Disturbance(obs_noise=0.1, action_noise=0.2, clip=(-1, 1), hold="episode"))
    rig.refused("nig_rollout_mlp_disturbed", UNSUPPORTED, NO_MFMA)
