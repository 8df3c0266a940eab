"""ctypes binding of include/nig.h (libnig.so).  No torch types cross this boundary:
device pointers are plain integers (tensor.data_ptr()), streams are hipStream_t handles.

The extension is mandatory: importing this module without a built libnig.so raises.
"""
import ctypes as C
import os

# torch ships its own HIP runtime (libamdhip64).  It must be in the process BEFORE libnig.so is
# loaded so that libnig.so binds to that same runtime: with the opposite order the loader pulls the
# system ROCm copy for libnig.so, two runtimes coexist, and the second one to initialise reports
# "no ROCm-capable device is detected".
import torch  # noqa: F401,E402

from . import _build

NIG_OK = 0
F_AUTORESET, F_TALLY = 0x1, 0x2
FLAG_TERMINATED, FLAG_TRUNCATED = 0x1, 0x2
FLAG_VIOL_SHIFT, FLAG_NVIOL_SHIFT, FLAG_NCRIT_SHIFT = 2, 5, 7
FLAG_SHUTDOWN, FLAG_DID_RESET, FLAG_INACTIVE, FLAG_STEP_SHIFT = 0x200, 0x400, 0x800, 16
FLAG_VIOL3, FLAG_NVIOL_HI = 0x1000, 0x2000
FLAG_SHIELDED = 0x4000          # nig_rollout_mlp_safe: the safety critic halved the action (_search: replaced it; _gated: by zero; _projected: the lane was projected)
FLAG_UNCERTAIN = 0x8000         # nig_rollout_mlp_ensemble: uncertainty > threshold on this live step (_gated: some sd[c] not below the limit)
MAX_ENSEMBLE = 8
MAX_PROJECT_ITERS = 16          # nig_rollout_mlp_projected: max_iters 1 .. NIG_MAX_PROJECT_ITERS
MAX_ATOMS = 64                  # nig_set_mlp_safety_categorical: atoms 2 .. NIG_MAX_ATOMS ("nig-categorical-v1")
SAFETY_NONE, SAFETY_SIGMOID, SAFETY_CATEGORICAL, SAFETY_SIGMOID_LN, SAFETY_SIGMOID_SHAPED = 0, 1, 2, 3, 4       # nig_get_mlp_safety_kind
MAX_CANDIDATES = 128            # nig_rollout_mlp_search: n_candidates 1 .. NIG_MAX_CANDIDATES
ENSEMBLE_AVERAGE, ENSEMBLE_VOTING = 0, 1
CTR_STEP_MASK, CTR_DONE, CTR_VIOL_SHIFT = 0x7FFF, 0x8000, 16
MAX_EPISODE_STEPS = 21845
(T_EPISODES, T_RET_SUM, T_RET_SQ, T_RET_MIN, T_RET_MAX, T_LEN_SUM, T_LEN_SQ, T_VIOL, T_CRIT,
 T_SHUTDOWN, T_SUCCESS, T_SATISFIED, T_CONSTRAINTS, T_ROWS) = range(14)

TUNE_SPLIT_BLOCKS = 0
TUNE_WIDE_MIN_BLOCKS = 1
TUNE_DIAG_RING_FAULT = 2

class EnvSpec(C.Structure):
    _fields_ = [("state_dim", C.c_int32), ("action_dim", C.c_int32), ("n_constraints", C.c_int32),
                ("max_episode_steps", C.c_int32), ("k_step", C.c_int32), ("k_reset", C.c_int32),
                ("dt", C.c_double), ("penalty", C.c_double * 3), ("critical", C.c_int32 * 3),
                ("reward_is_f32", C.c_int32)]


class Layout(C.Structure):
    _fields_ = [("batch", C.c_int64), ("ld", C.c_int64), ("bytes", C.c_int64), ("off_state", C.c_int64),
                ("off_ctr", C.c_int64), ("off_life_viol", C.c_int64), ("off_ep_return", C.c_int64),
                ("off_tally", C.c_int64)]


class EpisodeLogLayout(C.Structure):
    """nig_episode_log_layout (include/nig.h): byte offsets of an episode log's arrays."""
    _fields_ = [("batch", C.c_int64), ("capacity", C.c_int64), ("ld", C.c_int64), ("bytes", C.c_int64),
                ("off_ret", C.c_int64), ("off_w", C.c_int64 * 5), ("off_count", C.c_int64), ("off_carry_ret", C.c_int64),
                ("off_carry_w", C.c_int64), ("off_tally", C.c_int64), ("off_scratch", C.c_int64)]


class Policy(C.Structure):
    """nig_policy (include/nig.h, "nig-policy-v1")."""
    _fields_ = [("kind", C.c_int32), ("colmask", C.c_uint32), ("Wt", (C.c_float * 10) * 32), ("b", C.c_float * 10),
                ("sigma", C.c_float * 10), ("half_range", C.c_float * 10), ("p_uniform", C.c_float),
                ("uniform_range", C.c_float), ("clip_lo", C.c_float), ("clip_hi", C.c_float),
                ("kp", C.c_float), ("ki", C.c_float), ("kd", C.c_float), ("setpoint", C.c_float * 10)]


POLICY_AFFINE, POLICY_PID = 1, 2
HOLD_STEP, HOLD_EPISODE = 0, 1


class DisturbanceStruct(C.Structure):
    """nig_disturbance (include/nig.h, "nig-disturb-v1")."""
    _fields_ = [("sigma_obs", C.c_float * 32), ("sigma_act", C.c_float * 10), ("clip_lo", C.c_float), ("clip_hi", C.c_float),
                ("hold", C.c_int32)]


MAX_LIMITS, LIMIT_ROWS = 4, 48        # nig_set_limits: added box constraints per handle, row capacity of their bounds
XFLAG_NVIOL_SHIFT, XFLAG_NCRIT_SHIFT = 4, 8


class LimitStruct(C.Structure):
    """nig_limit (include/nig.h, "nig-limits-v1")."""
    _fields_ = [("mask", C.c_uint64), ("lo", C.c_float * LIMIT_ROWS), ("hi", C.c_float * LIMIT_ROWS), ("penalty", C.c_double),
                ("critical", C.c_int32), ("reserved", C.c_int32)]


MIXED_MAX_SEGMENTS = 12


class MixedInfo(C.Structure):
    """nig_mixed_info (include/nig.h)."""
    _fields_ = [("n_segments", C.c_int32), ("state_dim_max", C.c_int32), ("action_dim_max", C.c_int32),
                ("reserved", C.c_int32), ("lanes", C.c_int64), ("ld", C.c_int64),
                ("env", C.c_int32 * MIXED_MAX_SEGMENTS), ("offset", C.c_int64 * MIXED_MAX_SEGMENTS),
                ("count", C.c_int64 * MIXED_MAX_SEGMENTS)]


# The C ABI as ctypes sees it: symbol -> (restype, argtypes).
cp, vp, ci, i32, i64, u32, u64, f32, f64, P = (C.c_char_p, C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64,
                                               C.c_float, C.c_double, C.POINTER)
# what the closed-loop rollouts share: handle, n_steps, reward_out, flags_out, out_stride, obs_out, obs_step_stride, act_out, ld_act,
# act_step_stride; each adds its own outputs and the stream (nig_rollout_mlp_search: n_candidates after n_steps)
CLOSED_LOOP = [vp, i32, vp, vp, i64, vp, i64, vp, i64, i64]
PROTOTYPES = {
    "nig_version": (cp, []),
    "nig_last_error": (cp, []),
    "nig_tune": (ci, [i32, i64]),
    "nig_tune_get": (i64, [i32]),
    "nig_handle_tune_get": (i64, [vp, i32]),
    "nig_clock_stamp": (ci, [vp, vp]),
    "nig_env_id": (ci, [cp]),
    "nig_env_name": (cp, [ci]),
    "nig_env_spec_get": (ci, [ci, P(EnvSpec)]),
    "nig_layout_query": (ci, [ci, i64, u32, P(Layout)]),
    "nig_create": (ci, [ci, i64, ci, u64, u64, i32, f64, u32, vp, P(vp)]),
    "nig_destroy": (ci, [vp]),
    "nig_get_layout": (ci, [vp, P(Layout)]),
    "nig_workspace": (vp, [vp]),
    "nig_get_counter": (ci, [vp, P(u32)]),
    "nig_set_counter": (ci, [vp, u32]),
    "nig_set_constraint_mask": (ci, [vp, u32]),
    "nig_set_limits": (ci, [vp, i32, P(LimitStruct), vp]),
    "nig_get_limit_count": (ci, [vp]),
    "nig_step_limited": (ci, [vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]),
    "nig_step64_limited": (ci, [vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]),
    "nig_reset": (ci, [vp, vp, vp, i64, vp]),
    "nig_step": (ci, [vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp]),
    "nig_fill_actions": (ci, [vp, u32, vp, i64, vp]),
    "nig_set_state": (ci, [vp, vp, i64, vp, vp]),
    "nig_get_state": (ci, [vp, vp, i64, vp, vp]),
    "nig_get_safety_metrics": (ci, [vp, vp, vp, i64, vp]),
    "nig_reduce_tally": (ci, [vp, vp, vp]),
    "nig_plan_create": (ci, [vp, i32, vp, i64, i64, i32, vp, vp, i64, P(vp)]),
    "nig_plan_launch": (ci, [vp, vp]),
    "nig_plan_destroy": (ci, [vp]),
    "nig_bind_state": (ci, [vp, vp, i64]),
    "nig_set_policy": (ci, [vp, P(Policy), vp]),
    "nig_rollout_policy": (ci, CLOSED_LOOP + [vp]),
    "nig_set_mlp_policy": (ci, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "nig_rollout_mlp": (ci, CLOSED_LOOP + [vp]),
    "nig_set_mlp_policy_dims": (ci, [vp, i32, vp, vp, vp, vp]),
    "nig_get_mlp_policy_dims": (ci, [vp, vp]),
    "nig_set_mlp_policy_ln": (ci, [vp, i32] + [vp] * 10 + [f32, vp]),
    "nig_get_mlp_policy_norm": (ci, [vp]),
    "nig_set_mlp_policy_bf16": (ci, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "nig_rollout_mlp_bf16": (ci, CLOSED_LOOP + [vp, i64, i64, vp]),
    "nig_bf16_from_f32": (ci, [vp, vp, i64]),
    "nig_set_mlp_safety": (ci, [vp, i32, vp, vp, vp, vp, vp, vp, f32, vp]),
    "nig_set_mlp_safety_categorical": (ci, [vp, i32, i32, vp, vp, vp, vp, vp, vp, u64, f32, vp]),
    "nig_get_mlp_safety_kind": (ci, [vp]),
    "nig_set_mlp_safety_dims": (ci, [vp, i32, vp, vp, vp, f32, vp]),
    "nig_get_mlp_safety_dims": (ci, [vp, vp]),
    "nig_set_mlp_safety_ln": (ci, [vp, i32] + [vp] * 10 + [f32, f32, vp]),
    "nig_get_mlp_safety_atoms": (ci, [vp]),
    "nig_mlp_violation_prob": (ci, [vp, i64, vp, i64, vp, i64, vp, vp, i64, vp]),
    "nig_rollout_mlp_safe": (ci, CLOSED_LOOP + [vp, vp]),
    "nig_rollout_mlp_search": (ci, CLOSED_LOOP[:2] + [i32] + CLOSED_LOOP[2:] + [vp, vp, vp, vp]),
    "nig_set_mlp_safety_ensemble": (ci, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, f32, f32, vp]),
    "nig_rollout_mlp_gated": (ci, CLOSED_LOOP + [vp, vp, vp, i64, i64, vp]),
    "nig_set_mlp_constraint": (ci, [vp, i32, i32, vp, vp, vp, vp, vp, vp, f32, f32, vp]),
    "nig_rollout_mlp_projected": (ci, CLOSED_LOOP[:2] + [i32, f32] + CLOSED_LOOP[2:] + [vp, vp, vp, vp, i64, i64, vp]),
    "nig_set_mlp_ensemble": (ci, [vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, f64, f32, vp]),
    "nig_rollout_mlp_ensemble": (ci, CLOSED_LOOP + [vp, vp, vp]),
    "nig_set_disturbance": (ci, [vp, P(DisturbanceStruct), vp]),
    "nig_rollout_policy_disturbed": (ci, CLOSED_LOOP + [vp, i64, vp]),
    "nig_rollout_mlp_disturbed": (ci, CLOSED_LOOP + [vp, i64, vp]),
    "nig_reset_host": (ci, [vp, vp, vp, vp]),
    "nig_step_host": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "nig_step_host64": (ci, [vp, vp, vp, vp, vp, vp, vp]),
    "nig_reduce_metrics": (ci, [P(vp), i32, vp, vp, i64, vp, vp]),
    "nig_step64": (ci, [vp, vp, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp]),
    "nig_rollout": (ci, [vp, i32, vp, i64, i64, i32, vp, vp, i64, vp, i64, i64, vp]),
    "nig_rollout_sampled": (ci, [vp, i32, vp, vp, i64, vp, i64, i64, vp]),
    "nig_rollout_noise": (ci, [vp, i32, vp, i64, i64, i32, vp, i64, vp, i64, i64, vp, vp, i64, vp, i64, vp]),
    "nig_create_mixed": (ci, [i32, P(i32), P(i64), ci, u64, u64, u32, P(vp)]),
    "nig_mixed_destroy": (ci, [vp]),
    "nig_mixed_get_info": (ci, [vp, P(MixedInfo)]),
    "nig_mixed_state": (vp, [vp]),
    "nig_mixed_segment": (vp, [vp, i32]),
    "nig_mixed_reset": (ci, [vp, vp]),
    "nig_mixed_fill_actions": (ci, [vp, u32, vp, vp]),
    "nig_mixed_rollout": (ci, [vp, i32, vp, i64, i32, vp, vp, i64, vp]),
    "nig_mixed_step": (ci, [vp, vp, vp, vp, vp]),
    "nig_rollout_mixed": (ci, [P(vp), P(i64), i32, i32, vp, i64, i64, i32, vp, vp, i64, vp]),
    "nig_rollout_mixed_obs": (ci, [P(vp), P(i64), i32, i32, vp, i64, i64, i32, vp, vp, i64, vp, i64, i64, vp]),
    "nig_mixed_rollout_obs": (ci, [vp, i32, vp, i64, i32, vp, vp, i64, vp, i64, vp]),
    "nig_episode_log_query": (ci, [i64, i64, i64, P(EpisodeLogLayout)]),
    "nig_episode_log_init": (ci, [vp, vp, i64, i64, vp]),
    "nig_collect_episodes": (ci, [vp, i32, vp, vp, i64, vp, i64, i64, vp]),
    "nig_reduce_episodes": (ci, [vp, vp, i64, i64, i64, vp, vp]),
}
# a closed loop's twin under the added constraints: the parent's arguments, xflags_out, the stream
for _parent in ("nig_rollout_policy", "nig_rollout_mlp", "nig_rollout_mlp_safe", "nig_rollout_mlp_search", "nig_rollout_mlp_gated",
                "nig_rollout_mlp_projected", "nig_rollout_mlp_ensemble", "nig_rollout_policy_disturbed", "nig_rollout_mlp_disturbed"):
    _restype, _argtypes = PROTOTYPES[_parent]
    PROTOTYPES[_parent + "_limited"] = (_restype, _argtypes[:-1] + [vp, _argtypes[-1]])
SYMBOLS = list(PROTOTYPES)


class NigError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libnig.so.  A stale or missing library is rebuilt first (content hash of csrc/), except
    inside a profiled process or with NIG_NO_AUTOBUILD set, where that is an ImportError (_build.ensure)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    override = os.environ.get("NIG_LIB_PATH")
    if override:
        # an experiment's library variant (profiles/mkvariant.sh) for same-box A/B runs: loaded in place of libnig.so,
        # which is never overwritten (an interrupted A/B script used to leave a variant behind as "current")
        path = override
    else:
        _build.ensure()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  This package has no CPU fallback.")
    L = C.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        getattr(L, name).restype, getattr(L, name).argtypes = restype, argtypes
    _lib = L
    return L


def check(status):
    if status != NIG_OK:
        raise NigError(f"libnig error {status}: {lib().nig_last_error().decode()}")


def env_spec(env_id: int) -> EnvSpec:
    s = EnvSpec()
    check(lib().nig_env_spec_get(env_id, C.byref(s)))
    return s


def layout_query(env_id: int, batch: int, flags: int) -> Layout:
    lay = Layout()
    check(lib().nig_layout_query(env_id, batch, flags, C.byref(lay)))
    return lay


def episode_log_query(batch: int, capacity: int, ld: int = 0) -> EpisodeLogLayout:
    lay = EpisodeLogLayout()
    check(lib().nig_episode_log_query(batch, capacity, ld, C.byref(lay)))
    return lay
