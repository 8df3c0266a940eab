"""BatchedIndustrialEnv: B independent env instances of one type stepped by ONE HIP kernel.

This is the batched form of IndustrialEnv (reference environments/base.py:19-228): the
same reset/step semantics per lane, with every per-step Python object of the reference
(`SafetyMetrics`, the `info` dict) replaced by a packed flag word per lane that can be
decoded lazily.  torch is used only for device memory and the stream handle; all compute
happens in libnig.so through the C ABI (include/nig.h).
"""
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .core import BoxConstraint, SafetyConstraint, SafetyMetrics, make_box

# the built-in constraints' names (the reference envs' own; remove_safety_constraint(name) clears the matching mask bit)
BUILTIN_CONSTRAINTS = {
    "ChemicalReactor-v0": ("temperature_limit", "pressure_limit", "level_safety"),
    "PowerGrid-v0": ("frequency_stability", "voltage_limits", "generation_limits"),
    "RobotAssembly-v0": ("force_limits", "collision_avoidance", "velocity_limits"),
}


def _builtin_names(env_id, n):
    if env_id in BUILTIN_CONSTRAINTS:
        return list(BUILTIN_CONSTRAINTS[env_id])
    from . import spec_plants
    plant = {"HVACControl-v0": "HVAC", "WaterTreatment-v0": "WATER", "SteelAnnealing-v0": "STEEL", "SupplyChain-v0": "SUPPLY"}.get(env_id)
    if plant:
        return [c[0] for c in getattr(spec_plants, plant)["constraints"]]
    return [f"constraint_{k}" for k in range(n)]

ENV_IDS = {"ChemicalReactor-v0": 0, "PowerGrid-v0": 1, "RobotAssembly-v0": 2,
           # candidate rows: registered upstream (utils.py:30-31) but not instantiable there
           "AdvancedChemicalReactor-v0": 3, "AdvancedPowerGrid-v0": 4,
           # README-only upstream (README.md:28-32): build-specified plants, spec_plants.py
           "HVACControl-v0": 5, "WaterTreatment-v0": 6, "SteelAnnealing-v0": 7, "SupplyChain-v0": 8}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rows(t: Optional[torch.Tensor], dtype, n_steps: Optional[int] = None):
    """(pointer, row stride) of an optional per-step output: [rows, >=B] (stride of its rows; at least n_steps rows when
    n_steps is given) or [B] (stride 0: every step overwrites it)."""
    if t is None:
        return None, 0
    assert t.dtype == dtype and t.stride(-1) == 1
    if t.dim() == 2:
        assert n_steps is None or t.shape[0] >= n_steps
        return C.c_void_p(t.data_ptr()), t.stride(0)
    return C.c_void_p(t.data_ptr()), 0


def _mlp_weights(weights, shapes):
    """[(W, b), ...] -> the six contiguous float32 host arrays W1, b1, W2, b2, W3, b3, shapes asserted."""
    W = [np.ascontiguousarray(np.asarray(x), dtype=np.float32) for pair in weights for x in pair]
    if W[4].ndim == 1 and shapes[4][1:] == (1,):
        W[4] = W[4].reshape(-1, 1)                     # a critic's head given as a vector
    assert [w.shape for w in W] == shapes, [w.shape for w in W]
    return W


def categorical_below_mask(atoms: int, v_min: float = -1.0, v_max: float = 1.0, safety_threshold: float = 0.0) -> int:
    """The atoms of a distributional critic that count as a violation, as "nig-categorical-v1"'s mask: bit j where
    np.linspace(v_min, v_max, atoms, dtype=float32)[j] < safety_threshold (agents/safety_critical.py:163-168; the reference's
    51 atoms on [-1, 1] against 0: bits 0 .. 24, atom 25 is exactly 0.0)."""
    below = np.linspace(v_min, v_max, int(atoms), dtype=np.float32) < np.float32(safety_threshold)
    return sum(1 << j for j in range(int(atoms)) if below[j])


class StepInfo:
    """Lazy view of the per-lane flag words of one step (the batched `info`).

    Fields are torch tensors on the env's device, decoded on first use:
      terminated, truncated, done, violation_count, critical_violations, critical_shutdown,
      constraint_violated [3,B], did_reset, inactive, step.
    With added box constraints on the env (add_safety_constraint) `xflags` is the step's second word per lane and the counts,
    constraint_violated ([3 + n_added, B], the added ones behind the built-ins) and safety_metrics() cover all constraints.
    """

    def __init__(self, flags: torch.Tensor, n_constraints: int = 3, xflags: Optional[torch.Tensor] = None, n_added: int = 0,
                 n_enabled: Optional[int] = None):
        self.flags = flags
        self.n_constraints = n_constraints
        self.xflags = xflags
        self.n_added = int(n_added) if xflags is not None else 0
        self.n_enabled = n_constraints if n_enabled is None else int(n_enabled)      # built-ins still enabled (set_constraint_mask)

    @property
    def terminated(self):
        return (self.flags & _lib.FLAG_TERMINATED) != 0

    @property
    def truncated(self):
        return (self.flags & _lib.FLAG_TRUNCATED) != 0

    @property
    def done(self):
        return (self.flags & (_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED)) != 0

    @property
    def violation_count(self):
        n = ((self.flags >> _lib.FLAG_NVIOL_SHIFT) & 3) + ((self.flags >> 13) & 1) * 4
        return n if self.xflags is None else n + ((self.xflags >> _lib.XFLAG_NVIOL_SHIFT) & 7)

    @property
    def critical_violations(self):
        n = (self.flags >> _lib.FLAG_NCRIT_SHIFT) & 3
        return n if self.xflags is None else n + ((self.xflags >> _lib.XFLAG_NCRIT_SHIFT) & 7)

    @property
    def critical_shutdown(self):
        return (self.flags & _lib.FLAG_SHUTDOWN) != 0

    @property
    def constraint_violated(self):
        builtin = torch.stack([((self.flags >> (_lib.FLAG_VIOL_SHIFT + k)) & 1) != 0 for k in range(3)]
                              + [((self.flags >> 12) & 1) != 0])[:self.n_constraints]
        if self.xflags is None:
            return builtin
        return torch.cat([builtin, torch.stack([((self.xflags >> c) & 1) != 0 for c in range(self.n_added)])])

    @property
    def did_reset(self):
        return (self.flags & _lib.FLAG_DID_RESET) != 0

    @property
    def inactive(self):
        return (self.flags & _lib.FLAG_INACTIVE) != 0

    @property
    def step(self):
        return (self.flags >> _lib.FLAG_STEP_SHIFT) & 0xFFFF

    def safety_metrics(self, lane: int) -> SafetyMetrics:
        """The reference's per-step SafetyMetrics object for one lane (base.py:118-124)."""
        f = int(self.flags[lane].item())
        nv = ((f >> _lib.FLAG_NVIOL_SHIFT) & 3) + ((f >> 13) & 1) * 4
        nc = (f >> _lib.FLAG_NCRIT_SHIFT) & 3
        n = self.n_constraints
        if self.xflags is not None:
            x = int(self.xflags[lane].item())
            nv += (x >> _lib.XFLAG_NVIOL_SHIFT) & 7
            nc += (x >> _lib.XFLAG_NCRIT_SHIFT) & 7
            n = self.n_enabled + self.n_added
        return SafetyMetrics(constraints_satisfied=n - nv, total_constraints=n, violation_count=nv,
                             critical_violations=nc, safety_score=(n - nv) / n if n else 1.0)


class BatchedIndustrialEnv:
    """B lanes of `env_id` on one GPU.

    Args mirror IndustrialEnv.__init__ (base.py:22-29) plus the batch controls:
      batch            number of env instances (lanes)
      device           torch device ("cuda:0")
      seed             key of the counter-based generator used in fast mode
      env_index0       global index of lane 0 (sharding-invariant RNG streams)
      autoreset        finished lanes start their next episode inside the step kernel
      tally            keep per-lane episode tallies for evaluate_with_safety
      workspace        optional caller-owned uint8 tensor on `device` that holds the handle's arrays (nig_create's
                       `workspace`: at least nig_layout.bytes, 256-byte aligned); default: the env allocates its own
    Layouts: `state` / `obs` is the library-owned SoA array viewed as [B, S] with strides
    (1, ld) -- a zero-copy view a policy network can consume directly; actions are
    accepted as [A, B] (native SoA, no copy) or [B, A] (transposed on the way in).
    """

    def __init__(self, env_id: str, batch: int, device="cuda:0", seed: int = 0x5EED, env_index0: int = 0,
                 max_episode_steps: Optional[int] = None, dt: Optional[float] = None, autoreset: bool = True,
                 tally: bool = False, bind_state: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None):
        if env_id not in ENV_IDS:
            available = ", ".join(ENV_IDS.keys())
            raise ValueError(f"Unknown environment '{env_id}'. Available: {available}")
        self.env_id = env_id
        self.seed, self.env_index0 = int(seed), int(env_index0)
        self._eid = ENV_IDS[env_id]
        self._L = _lib.lib()
        self.spec = _lib.env_spec(self._eid)
        self.state_dim, self.action_dim = int(self.spec.state_dim), int(self.spec.action_dim)
        self.batch = int(batch)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BatchedIndustrialEnv needs a HIP device (torch device type 'cuda'); "
                               "there is no CPU fallback")
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible to torch; BatchedIndustrialEnv has no CPU fallback")
        self.max_episode_steps = int(max_episode_steps) if max_episode_steps else int(self.spec.max_episode_steps)
        self.dt = float(dt) if dt else float(self.spec.dt)
        self.autoreset, self.tally_enabled = bool(autoreset), bool(tally)
        self._flags = (_lib.F_AUTORESET if autoreset else 0) | (_lib.F_TALLY if tally else 0)
        lay = _lib.layout_query(self._eid, self.batch, self._flags)
        self.ld = int(lay.ld)
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(dev_index):
            if workspace is None:
                self._ws = torch.empty(int(lay.bytes), dtype=torch.uint8, device=self.device)
            else:
                assert workspace.dtype == torch.uint8 and workspace.is_contiguous()
                assert workspace.device.type == "cuda" and workspace.device.index == dev_index, "workspace on another device"
                assert workspace.numel() >= int(lay.bytes), "workspace smaller than nig_layout.bytes"
                self._ws = workspace[:int(lay.bytes)]
            assert self._ws.data_ptr() % 256 == 0, "workspace must be 256-byte aligned"
            h = C.c_void_p()
            _lib.check(self._L.nig_create(self._eid, self.batch, dev_index, C.c_uint64(seed), C.c_uint64(env_index0),
                                          self.max_episode_steps if max_episode_steps else 0,
                                          C.c_double(self.dt if dt else 0.0), self._flags,
                                          C.c_void_p(self._ws.data_ptr()), C.byref(h)))
        self._h = h
        self._dev_index = dev_index
        B, ld, S = self.batch, self.ld, self.state_dim

        def view(off, nbytes, dtype):
            return self._ws[off:off + nbytes].view(dtype)

        if bind_state is None:
            self.state_soa = view(lay.off_state, S * ld * 4, torch.float32).view(S, ld)[:, :B]   # [S, B]
        else:
            # caller-owned padded SoA array (mixed batches): a [>=S, B] float32 view with unit column stride
            assert bind_state.dtype == torch.float32 and bind_state.device == self.device
            assert bind_state.shape[0] >= S and bind_state.shape[1] == B and bind_state.stride(1) == 1
            _lib.check(self._L.nig_bind_state(self._h, C.c_void_p(bind_state.data_ptr()), bind_state.stride(0)))
            self._bound = bind_state
            self.state_soa = bind_state[:S]
        self.obs = self.state_soa.t()                                                       # [B, S] strided view
        self.ctr = view(lay.off_ctr, ld * 4, torch.int32)[:B]
        self.life_viol = view(lay.off_life_viol, ld * 8, torch.int64)[:B]
        if tally:
            self.ep_return = view(lay.off_ep_return, ld * 8, torch.float64)[:B]
            self.tally = view(lay.off_tally, _lib.T_ROWS * ld * 8, torch.float64).view(_lib.T_ROWS, ld)[:, :B]
        else:
            self.ep_return = self.tally = None
        self.reward = torch.zeros(B, dtype=torch.float32, device=self.device)
        self.reward64 = torch.zeros(B, dtype=torch.float64, device=self.device)
        self.flags = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.xflags = torch.zeros(B, dtype=torch.int32, device=self.device)      # the added constraints' word of the last step
        self._cmask = (1 << int(self.spec.n_constraints)) - 1
        self._builtin_names = _builtin_names(env_id, int(self.spec.n_constraints))
        self._added = []                # BoxConstraints installed on the handle, in installation order
        self._act_soa = torch.zeros(self.action_dim, ld, dtype=torch.float32, device=self.device)
        self.observation_space = make_box(-np.inf, np.inf, (self.state_dim,), np.float32)
        self.action_space = make_box(-1.0, 1.0, (self.action_dim,), np.float32)

    # ------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.nig_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _noise(self, x, rows):
        """numpy/torch [rows, B] (or [B, rows]) fp64 -> contiguous device [rows, B]."""
        if x is None:
            return None
        t = torch.as_tensor(x, dtype=torch.float64, device=self.device)
        if t.shape == (self.batch, rows) and rows != self.batch:
            t = t.t()
        if t.shape != (rows, self.batch):
            raise ValueError(f"noise must have shape ({rows}, {self.batch}), got {tuple(t.shape)}")
        return t.contiguous()

    # ------------------------------------------------------------------
    @property
    def counter(self) -> int:
        t = C.c_uint32()
        _lib.check(self._L.nig_get_counter(self._h, C.byref(t)))
        return int(t.value)

    @counter.setter
    def counter(self, t: int):
        _lib.check(self._L.nig_set_counter(self._h, C.c_uint32(t)))

    def set_constraint_mask(self, mask: int):
        _lib.check(self._L.nig_set_constraint_mask(self._h, C.c_uint32(mask)))
        self._cmask = int(mask) & ((1 << int(self.spec.n_constraints)) - 1)

    # ---- added safety constraints (base.py:220-228; include/nig.h "nig-limits-v1") --------------------------------------------
    @property
    def safety_constraints(self):
        """The constraints in force, the reference's list (base.py:51): the enabled built-ins as names-only SafetyConstraint
        records (their check runs in the kernel), then the added BoxConstraints in installation order."""
        builtin = [SafetyConstraint(name=n, check_fn=None, penalty=float(self.spec.penalty[k]) if k < 3 else 0.0,
                                    critical=bool(self.spec.critical[k]) if k < 3 else False, description="built-in (device)")
                   for k, n in enumerate(self._builtin_names) if (self._cmask >> k) & 1]
        return builtin + list(self._added)

    @property
    def has_limits(self) -> bool:
        return bool(self._added)

    def _install_limits(self, added):
        n = len(added)
        arr = (_lib.LimitStruct * max(n, 1))()
        for c, box in enumerate(added):
            mask, rows = box.limit_rows(self.state_dim, self.action_dim)
            arr[c].mask = mask
            for bit, (lo, hi) in rows.items():
                arr[c].lo[bit], arr[c].hi[bit] = float(lo), float(hi)
            arr[c].penalty, arr[c].critical = float(box.penalty), int(bool(box.critical))
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_limits(self._h, n, arr, self._stream()))
        self._added = list(added)

    def add_safety_constraint(self, constraint):
        """env.add_safety_constraint (base.py:220-222) for a BoxConstraint: from the next step on it is checked, penalised and
        counted on the device beside the built-ins (at most MAX_LIMITS added ones).  step() and the rollout_*_limited() methods
        know the added constraints; every other stepping entry point refuses while any is installed."""
        if not isinstance(constraint, BoxConstraint):
            raise TypeError("BatchedIndustrialEnv evaluates added constraints on the device and takes BoxConstraint only (declarative "
                            "bounds on state / action rows); an arbitrary check_fn callable runs on the single env: make(env_id)"
                            ".add_safety_constraint(c)")
        if len(self._added) >= _lib.MAX_LIMITS:
            raise ValueError(f"at most {_lib.MAX_LIMITS} added constraints per batched env")
        self._install_limits(self._added + [constraint])

    def remove_safety_constraint(self, name: str):
        """env.remove_safety_constraint (base.py:224-228): every constraint of that name goes -- an added one from the device
        table, a built-in one by clearing its bit of the constraint mask."""
        kept = [c for c in self._added if c.name != name]
        if len(kept) != len(self._added):
            self._install_limits(kept)
        for k, n in enumerate(self._builtin_names):
            if n == name and (self._cmask >> k) & 1:
                self.set_constraint_mask(self._cmask & ~(1 << k))

    def _refuse_limits(self, what: str):
        if self._added:
            raise RuntimeError(f"{what} does not know the added safety constraints ({', '.join(c.name for c in self._added)}): "
                               "remove them first (remove_safety_constraint), or use evaluate_with_safety / step / "
                               "rollout_policy_limited / rollout_mlp_limited")

    @property
    def current_step(self):
        return self.ctr & _lib.CTR_STEP_MASK

    @property
    def done(self):
        return (self.ctr & _lib.CTR_DONE) != 0

    @property
    def violation_count(self):
        return (self.ctr >> _lib.CTR_VIOL_SHIFT) & 0xFFFF

    @property
    def total_violations(self):
        """base.py:57,183: lifetime count = finished episodes + the running one."""
        running = torch.where(self.done, torch.zeros_like(self.ctr), self.violation_count)
        return self.life_viol + running.to(torch.int64)

    # ------------------------------------------------------------------
    def reset(self, mask=None, init_noise=None):
        """IndustrialEnv.reset (base.py:133-155) for all lanes or those where mask != 0.
        init_noise: optional [k_reset, B] fp64 draws (parity mode).  Returns the obs view."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        nz = self._noise(init_noise, int(self.spec.k_reset))
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_reset(self._h, _ptr(m), _ptr(nz), self.batch, self._stream()))
        return self.obs

    def step(self, actions, step_noise=None, reset_noise=None, final_obs: Optional[torch.Tensor] = None,
             layout: Optional[str] = None):
        """IndustrialEnv.step (base.py:157-213) for every lane: one kernel launch.

        actions: [A, B] (SoA, zero-copy) or [B, A] tensor/array on any device; float32, or float64 --
        upstream clips without casting (base.py:167), so a float64 action vector makes NumPy evaluate
        the action-dependent arithmetic in float64: float64 input goes through nig_step64, which
        follows that (CR / PG / RA; the other envs take float32).  Other dtypes are cast to float32.
        `layout` ("soa"/"aos") disambiguates when A == B (default then: [B, A]).
        Returns (obs [B,S] view, reward f32 [B], terminated [B], truncated [B], StepInfo).
        """
        A, B = self.action_dim, self.batch
        a = torch.as_tensor(actions, device=self.device)
        act64 = a.dtype == torch.float64
        if not act64 and a.dtype != torch.float32:
            a = a.to(torch.float32)
        if layout in ("soa", "aos"):
            soa = layout == "soa"
        else:
            soa = (a.shape == (A, B)) and (A != B)
        if soa and a.shape != (A, B):
            raise ValueError(f"actions must have shape ({A}, {B}) for layout='soa', got {tuple(a.shape)}")
        if not soa and a.shape != (B, A):
            raise ValueError(f"actions must have shape ({A}, {B}) or ({B}, {A}), got {tuple(a.shape)}")
        if soa and a.stride(1) == 1 and a.stride(0) >= B:
            act, ld_act = a, a.stride(0)                      # native SoA, zero-copy
        elif (not soa) and a.stride(0) == 1 and a.stride(1) >= B:
            act, ld_act = a, a.stride(1)                      # [B,A] view of an SoA buffer, zero-copy
        elif act64:
            if getattr(self, "_act64_soa", None) is None:
                self._act64_soa = torch.zeros(self.action_dim, self.ld, dtype=torch.float64, device=self.device)
            self._act64_soa[:, :B].copy_(a if soa else a.t())
            act, ld_act = self._act64_soa, self.ld
        else:
            self._act_soa[:, :B].copy_(a if soa else a.t())   # one transposing copy
            act, ld_act = self._act_soa, self.ld
        sn = self._noise(step_noise, int(self.spec.k_step)) if int(self.spec.k_step) else None
        rn = self._noise(reset_noise, int(self.spec.k_reset))
        ld_obs = 0
        if final_obs is not None:
            assert final_obs.dtype == torch.float32 and final_obs.shape[0] == self.state_dim and final_obs.stride(1) == 1
            ld_obs = final_obs.stride(0)
        with torch.cuda.device(self._dev_index):
            if self._added:         # the added constraints are part of the step law: nig_step_limited, a second word per lane
                _lib.check((self._L.nig_step64_limited if act64 else self._L.nig_step_limited)(
                    self._h, _ptr(act), ld_act, _ptr(sn), _ptr(rn), B, _ptr(self.reward), _ptr(self.reward64),
                    _ptr(self.flags), _ptr(self.xflags), _ptr(final_obs), ld_obs, self._stream()))
            else:
                _lib.check((self._L.nig_step64 if act64 else self._L.nig_step)(
                    self._h, _ptr(act), ld_act, _ptr(sn), _ptr(rn), B, _ptr(self.reward), _ptr(self.reward64),
                    _ptr(self.flags), _ptr(final_obs), ld_obs, self._stream()))
        info = self._step_info()
        return self.obs, self.reward, info.terminated, info.truncated, info

    def _step_info(self) -> StepInfo:
        if self._added:
            return StepInfo(self.flags, int(self.spec.n_constraints), self.xflags, len(self._added), bin(self._cmask).count("1"))
        return StepInfo(self.flags, int(self.spec.n_constraints))

    def step_raw(self, act_soa: torch.Tensor, ld_act: int, reward=True, reward64=False, flags=True):
        """Hot-loop form: no tensor conversions, no decoding; `act_soa` is float32 [A, >=B]."""
        _lib.check(self._L.nig_step(self._h, C.c_void_p(act_soa.data_ptr()), ld_act, None, None, 0,
                                    _ptr(self.reward) if reward else None,
                                    _ptr(self.reward64) if reward64 else None,
                                    _ptr(self.flags) if flags else None, None, 0, self._stream()))

    def make_plan(self, n_steps: int, action_ring: torch.Tensor, reward_ring: Optional[torch.Tensor] = None,
                  flags_ring: Optional[torch.Tensor] = None) -> "StepPlan":
        """Record n_steps fast-mode steps as one hipGraph.  action_ring: float32 [R, A, ld>=B];
        step k of every replay reads slot k % R.  Optional reward/flags rings [R, B] (or [B])."""
        return StepPlan(self, n_steps, action_ring, reward_ring, flags_ring)

    def rollout(self, n_steps: int, action_ring: torch.Tensor, reward_out: Optional[torch.Tensor] = None,
                flags_out: Optional[torch.Tensor] = None, obs_out: Optional[torch.Tensor] = None):
        """n_steps fused steps in ONE kernel launch (state stays in registers; fast mode).
        action_ring: float32 [R, A, ld>=B] (rows), or contiguous [R, B, A] (row-major: what a policy network's batched output
        looks like; read natively by PowerGrid's wide form, transposed into rows by the library for every other kernel form --
        include/nig.h nig_rollout, ld_act == 0); step k reads slot k % R.
        reward_out float32 / flags_out int32: [n_steps, >=B] (per-step rows) or [B] (overwritten).
        obs_out: float32 trajectory of returned observations, [n_steps, S, >=B] (SoA rows) or
        contiguous [n_steps, B, S] (row-major transitions, D4RL layout; fastest to write)."""
        assert action_ring.dtype == torch.float32 and action_ring.dim() == 3 and action_ring.stride(2) == 1
        R = action_ring.shape[0]
        if action_ring.shape[1] == self.action_dim and action_ring.shape[2] >= self.batch:
            A, ld = action_ring.shape[1], action_ring.stride(1)                          # rows [R, A, ld]
        else:
            assert action_ring.shape[1:] == (self.batch, self.action_dim) and action_ring.stride(1) == self.action_dim, \
                "action_ring is [R, A, ld >= batch] or contiguous [R, batch, A]"
            A, ld = self.action_dim, 0                                                   # row-major [R, B, A]
        rp, fp, os_, op, ldo, so = self._rollout_outputs(n_steps, reward_out, flags_out, obs_out)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_rollout(self._h, int(n_steps), C.c_void_p(action_ring.data_ptr()), ld,
                                           action_ring.stride(0), R, rp, fp, os_, op, ldo, so, self._stream()))

    def _rollout_outputs(self, n_steps, reward_out, flags_out, obs_out):
        """The output arguments of nig_rollout / nig_rollout_sampled from the optional tensors, validated:
        (reward ptr, flags ptr, out_stride, obs ptr, ld_obs, obs_step_stride)."""
        rp, rs = _rows(reward_out, torch.float32, n_steps)
        fp, fs = _rows(flags_out, torch.int32, n_steps)
        assert (rp is None) == (fp is None), "reward_out and flags_out go together (both or neither)"
        assert rp is None or rs == fs, "reward/flags outputs must share their row stride"
        assert obs_out is None or rp is not None, "an observation trajectory needs reward_out and flags_out too"
        op, ldo, so = None, 0, 0
        if obs_out is not None:
            assert obs_out.dtype == torch.float32 and obs_out.dim() == 3 and obs_out.stride(2) == 1
            assert obs_out.shape[0] >= n_steps
            if obs_out.shape[1:] == (self.batch, self.state_dim) and obs_out.stride(1) == self.state_dim \
                    and self.batch != self.state_dim:
                op, ldo, so = C.c_void_p(obs_out.data_ptr()), 0, obs_out.stride(0)          # row-major [T,B,S]
            else:
                assert obs_out.shape[1] == self.state_dim and obs_out.shape[2] >= self.batch
                op, ldo, so = C.c_void_p(obs_out.data_ptr()), obs_out.stride(1), obs_out.stride(0)
        return rp, fp, rs or fs, op, ldo, so

    def rollout_sampled(self, n_steps: int, reward_out: Optional[torch.Tensor] = None,
                        flags_out: Optional[torch.Tensor] = None, obs_out: Optional[torch.Tensor] = None):
        """rollout() without an action ring (nig_rollout_sampled): every step draws its own uniform action of the env's
        action Box in the kernel -- the reference's measurement loop (performance_benchmark.py:106-133).  The step with launch
        counter t takes the action fill_actions(t) writes, so the call is bit-identical to rollout() on a ring of n_steps slots
        filled that way; to record the actions, regenerate them with fill_actions.  Outputs as rollout()."""
        rp, fp, os_, op, ldo, so = self._rollout_outputs(n_steps, reward_out, flags_out, obs_out)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_rollout_sampled(self._h, int(n_steps), rp, fp, os_, op, ldo, so, self._stream()))

    def rollout_noise(self, n_steps: int, action_ring: torch.Tensor, step_noise: Optional[torch.Tensor],
                      reset_noise: Optional[torch.Tensor], reward_out: torch.Tensor, flags_out: torch.Tensor,
                      obs_out: torch.Tensor):
        """rollout() on the reference's RECORDED draws (nig_rollout_noise): the same kernel form the batch would
        take, with np.random's values injected.  action_ring float32 [n_steps, A, ld]; step_noise float64
        [n_steps, k_step, ld] (None for an env without step noise); reset_noise float64 [n_steps, k_reset, ld]
        (auto-reset handles: the initial-state draws of a lane that finishes in that step); reward_out /
        flags_out [n_steps, >=B]; obs_out float32 contiguous [n_steps, B, S]."""
        assert action_ring.dtype == torch.float32 and action_ring.dim() == 3 and action_ring.stride(2) == 1
        assert action_ring.shape[0] >= n_steps and action_ring.shape[1] == self.action_dim
        ldn = 0

        def nz(t):
            nonlocal ldn
            if t is None:
                return None, 0
            assert t.dtype == torch.float64 and t.dim() == 3 and t.stride(2) == 1 and t.shape[0] >= n_steps
            assert ldn in (0, t.stride(1)), "step_noise and reset_noise share their row pitch"
            ldn = t.stride(1)
            return C.c_void_p(t.data_ptr()), t.stride(0)

        sp, ss = nz(step_noise)
        rp, rs = nz(reset_noise)
        assert reward_out.dtype == torch.float32 and flags_out.dtype == torch.int32 and reward_out.dim() == 2
        assert reward_out.stride(0) == flags_out.stride(0) and reward_out.shape[0] >= n_steps
        assert obs_out.dtype == torch.float32 and obs_out.is_contiguous() and obs_out.shape[1:] == (self.batch, self.state_dim)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_rollout_noise(
                self._h, int(n_steps), C.c_void_p(action_ring.data_ptr()), action_ring.stride(1), action_ring.stride(0),
                action_ring.shape[0], sp, ss, rp, rs, ldn, C.c_void_p(reward_out.data_ptr()),
                C.c_void_p(flags_out.data_ptr()), reward_out.stride(0), C.c_void_p(obs_out.data_ptr()), obs_out.stride(0),
                self._stream()))

    # ------------------------------------------------------------------
    def set_policy(self, policy):
        """Install an on-device policy (policies.DevicePolicy) for rollout_policy()."""
        P = policy.to_struct() if hasattr(policy, "to_struct") else policy
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_policy(self._h, C.byref(P), self._stream()))
        self._policy = policy

    def _actor_shapes(self):
        S, A, Hd = self.state_dim, self.action_dim, 256
        return [(S, Hd), (Hd,), (Hd, Hd), (Hd,), (Hd, A), (A,)]

    def set_mlp_policy(self, weights):
        """Install the reference agents' actor (S->256->256->A, ReLU, tanh) for rollout_mlp():
        weights = [(W1 [S,256], b1), (W2 [256,256], b2), (W3 [256,A], b3)], host arrays, [in, out]."""
        Hd = 256
        W = _mlp_weights(weights, self._actor_shapes())
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_policy(self._h, Hd, *[w.ctypes.data_as(C.c_void_p) for w in W], self._stream()))

    def set_mlp_policy_dims(self, weights):
        """Install an actor of any hidden shape a shape class holds ("nig-mlp-shape-v1", include/nig.h: two or three ReLU hidden
        layers of 1 .. 512 units, tanh head) for rollout_mlp(): weights = [(W1 [S,h1], b1), .., (W_head [h_last,A], b_head)], host
        arrays, [in, out], unpadded -- the library pads to the class.  Fills the ONE actor slot set_mlp_policy() fills: either
        call replaces the other's actor.  While a class other than the reference's is installed, every other closed loop that
        reads the actor (safe, search, gated, projected, disturbed, the _limited twins) refuses with code 4."""
        ws = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(np.asarray(b, dtype=np.float32).reshape(-1))) for W, b in weights]
        n_hidden = len(ws) - 1
        ins = [self.state_dim] + [W.shape[1] for W, _ in ws[:-1]]
        outs = [W.shape[1] for W, _ in ws[:-1]] + [self.action_dim]
        if n_hidden < 1 or any(W.shape != (i, o) or b.shape != (o,) for (W, b), i, o in zip(ws, ins, outs)):
            raise ValueError(f"actor layers must chain {self.state_dim} -> .. -> {self.action_dim}, got {[W.shape for W, _ in ws]}")
        hidden = (C.c_int32 * max(n_hidden, 1))(*outs[:-1])
        Wp = (C.c_void_p * len(ws))(*[W.ctypes.data for W, _ in ws])
        bp = (C.c_void_p * len(ws))(*[b.ctypes.data for _, b in ws])
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_policy_dims(self._h, n_hidden, hidden, Wp, bp, self._stream()))

    @property
    def mlp_policy_dims(self):
        """The hidden widths of the installed actor (set_mlp_policy: (256, 256)), () without one."""
        hidden = (C.c_int32 * 3)()
        n = self._L.nig_get_mlp_policy_dims(self._h, hidden)
        return tuple(int(hidden[i]) for i in range(max(n, 0)))

    def set_mlp_policy_ln(self, policy):
        """Install a LayerNorm actor (policies.LayerNormMLPPolicy: S->256->LayerNorm->ReLU->256->LayerNorm->ReLU->A, tanh; the law
        "nig-mlp-ln-v1", csrc/nig_mlp_ln.hpp) for rollout_mlp().  Fills the ONE actor slot set_mlp_policy() and set_mlp_policy_dims()
        fill: each call replaces the others' actor.  While it is installed, every other closed loop that reads the actor (safe,
        search, gated, projected, disturbed, the _limited twins) refuses with code 4."""
        W = _mlp_weights(policy.weights, self._actor_shapes())
        G = [np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1)) for pair in policy.norms for x in pair]
        assert len(G) == 4 and all(g.shape == (256,) for g in G), [g.shape for g in G]
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_policy_ln(self._h, 256, P(W[0]), P(W[1]), P(G[0]), P(G[1]), P(W[2]), P(W[3]), P(G[2]), P(G[3]),
                                                     P(W[4]), P(W[5]), float(policy.eps), self._stream()))

    @property
    def mlp_policy_norm(self):
        """True while the actor slot holds a LayerNorm actor (set_mlp_policy_ln)."""
        return self._L.nig_get_mlp_policy_norm(self._h) == 1

    def rollout_mlp(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None):
        """Closed loop with the installed MLP actor evaluated by f32 MFMA inside the env kernel
        (same outputs as rollout_policy)."""
        self._closed_loop(self._L.nig_rollout_mlp, n_steps, reward_out, flags_out, obs_out, act_out)

    def set_mlp_policy_bf16(self, weights):
        """Install the same actor for rollout_mlp_bf16(): set_mlp_policy()'s weights, rounded to bfloat16 by the library
        ("nig-mlp-bf16-v1"; the biases stay float32).  Kept beside the float32 actor: neither install disturbs the other."""
        W = _mlp_weights(weights, self._actor_shapes())
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_policy_bf16(self._h, 256, *[w.ctypes.data_as(C.c_void_p) for w in W], self._stream()))

    def rollout_mlp_bf16(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, hid_out=None):
        """rollout_mlp() with the actor on the bf16 matrix unit, for throughput-only sweeps (its own arithmetic, "nig-mlp-bf16-v1":
        outside rollout_mlp()'s parity bar).  hid_out (debug; int16 or uint16 [n_steps, 512, >=B]): the lane's h1 (rows 0-255)
        and h2 (rows 256-511) as bf16 words."""
        hp, ldh, sh = None, 0, 0
        if hid_out is not None:
            assert hid_out.dtype in (torch.int16, getattr(torch, "uint16", torch.int16)) and hid_out.dim() == 3 and hid_out.stride(2) == 1
            assert hid_out.shape[0] >= n_steps and hid_out.shape[1] == 512 and hid_out.shape[2] >= self.batch
            hp, ldh, sh = C.c_void_p(hid_out.data_ptr()), hid_out.stride(1), hid_out.stride(0)
        self._closed_loop(self._L.nig_rollout_mlp_bf16, n_steps, reward_out, flags_out, obs_out, act_out, tail=(hp, ldh, sh))

    def set_mlp_safety(self, weights, threshold: float):
        """Install the reference agents' safety critic ((S+A)->256->256->1, ReLU, sigmoid) for rollout_mlp_safe():
        weights = [(C1 [S+A,256], c1), (C2 [256,256], c2), (C3 [256,1], c3)], host arrays, [in, out].  The action
        is halved unless p < threshold (the threshold is used as given).  Replacing the actor keeps the critic."""
        D, Hd = self.state_dim + self.action_dim, 256
        W = _mlp_weights(weights, [(D, Hd), (Hd,), (Hd, Hd), (Hd,), (Hd, 1), (1,)])
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_safety(self._h, Hd, *[w.ctypes.data_as(C.c_void_p) for w in W],
                                                  float(threshold), self._stream()))

    def set_mlp_safety_categorical(self, weights, threshold: float, below_mask=None, v_min: float = -1.0, v_max: float = 1.0,
                                   safety_threshold: float = 0.0):
        """Install the distributional safety critic of RiskAwareCQLAgent ((S+A)->256->256->atoms, ReLU, softmax;
        agents/safety_critical.py DistributionalSafetyCritic) in the handle's ONE critic slot, in place of set_mlp_safety()'s:
        weights = [(C1 [S+A,256], c1), (C2 [256,256], c2), (C3 [256,atoms], c3 [atoms])], 2 <= atoms <= 64.  p is the softmax
        mass on the atoms of `below_mask` (an int, bit j = atom j; default: the atoms of linspace(v_min, v_max, atoms) below
        safety_threshold -- bits 0 .. 24 for the reference's 51 atoms), the law "nig-categorical-v1" (include/nig.h).
        rollout_mlp_safe() / rollout_mlp_search() and their _limited twins then act on this p (risky unless p < threshold);
        violation_prob() evaluates it on any batch."""
        D, Hd = self.state_dim + self.action_dim, 256
        atoms = int(np.shape(weights[2][0])[-1])
        W = _mlp_weights(weights, [(D, Hd), (Hd,), (Hd, Hd), (Hd,), (Hd, atoms), (atoms,)])
        if below_mask is None:
            below_mask = categorical_below_mask(atoms, v_min, v_max, safety_threshold)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_safety_categorical(self._h, Hd, atoms, *[w.ctypes.data_as(C.c_void_p) for w in W],
                                                              int(below_mask), float(threshold), self._stream()))

    def set_mlp_safety_ln(self, critic, threshold: float, eps=None):
        """Install a LayerNorm safety critic ((S+A)->256->LayerNorm->ReLU->256->LayerNorm->ReLU->1, sigmoid: agents/networks.py
        SafetyCritic with use_layer_norm=True) in the handle's ONE critic slot, in place of set_mlp_safety()'s and
        set_mlp_safety_categorical()'s.  `critic`: a policies.LayerNormMLPPolicy with a safety critic (its safety_weights,
        safety_norms and safety_eps), or a pair (weights, norms) laid out as the actor's of set_mlp_policy_ln(); eps: flax's epsilon
        (default: the policy's, 1e-6 for a pair).  Beside a LayerNorm actor rollout_mlp_safe() then runs the law
        "nig-mlp-ln-shield-v1" (csrc/nig_mlp_ln_shield.hpp): the action is halved unless p < threshold.  While it is installed,
        every other reader of the critic slot (search, violation_prob, the _limited twins) refuses with code 4."""
        if hasattr(critic, "safety_weights"):
            if critic.safety_weights is None:
                raise RuntimeError("Safety critic must be trained")
            weights, norms = critic.safety_weights, critic.safety_norms
            eps = critic.safety_eps if eps is None else eps
        else:
            weights, norms = critic
        eps = 1e-6 if eps is None else eps
        D, Hd = self.state_dim + self.action_dim, 256
        W = _mlp_weights(weights, [(D, Hd), (Hd,), (Hd, Hd), (Hd,), (Hd, 1), (1,)])
        G = [np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1)) for pair in norms for x in pair]
        assert len(G) == 4 and all(g.shape == (256,) for g in G), [g.shape for g in G]
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_safety_ln(self._h, Hd, P(W[0]), P(W[1]), P(G[0]), P(G[1]), P(W[2]), P(W[3]), P(G[2]), P(G[3]),
                                                     P(W[4]), P(W[5]), float(eps), float(threshold), self._stream()))

    def set_mlp_safety_dims(self, weights, threshold: float):
        """Install a sigmoid safety critic of any hidden shape a shape class holds ("nig-mlp-shape-shield-v1", include/nig.h: two or
        three ReLU hidden layers of 1 .. 512 units, one output) in the handle's ONE critic slot, in place of the other three critic
        installs: weights = [(C1 [S+A,h1], c1), .., (C_head [h_last,1], c_head)], host arrays, [in, out], unpadded -- the library
        pads to the class.  Beside a shaped actor of the same class (set_mlp_policy_dims) rollout_mlp_safe() then runs the fused
        shield: the action is halved unless p < threshold.  Widths of the reference class fill the slot as set_mlp_safety() does on
        the zero-padded arrays.  While a shaped critic is installed, every other reader of the critic slot (search, violation_prob,
        the _limited twins) refuses with code 4."""
        ws = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(np.asarray(b, dtype=np.float32).reshape(-1))) for W, b in weights]
        n_hidden = len(ws) - 1
        D = self.state_dim + self.action_dim
        ins = [D] + [W.shape[1] for W, _ in ws[:-1]]
        outs = [W.shape[1] for W, _ in ws[:-1]] + [1]
        if n_hidden < 1 or any(W.shape != (i, o) or b.shape != (o,) for (W, b), i, o in zip(ws, ins, outs)):
            raise ValueError(f"critic layers must chain {D} -> .. -> 1, got {[W.shape for W, _ in ws]}")
        hidden = (C.c_int32 * max(n_hidden, 1))(*outs[:-1])
        Wp = (C.c_void_p * len(ws))(*[W.ctypes.data for W, _ in ws])
        bp = (C.c_void_p * len(ws))(*[b.ctypes.data for _, b in ws])
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_safety_dims(self._h, n_hidden, hidden, Wp, bp, float(threshold), self._stream()))

    @property
    def mlp_safety_dims(self):
        """The hidden widths of the installed critic (set_mlp_safety, _categorical, _ln: (256, 256)), () without one."""
        hidden = (C.c_int32 * 3)()
        n = self._L.nig_get_mlp_safety_dims(self._h, hidden)
        return tuple(int(hidden[i]) for i in range(max(n, 0)))

    @property
    def mlp_safety_kind(self) -> int:
        """What the critic slot holds: 0 none, 1 the sigmoid critic (set_mlp_safety), 2 the categorical one, 3 the LayerNorm
        critic (set_mlp_safety_ln), 4 a shaped sigmoid critic (set_mlp_safety_dims)."""
        return int(self._L.nig_get_mlp_safety_kind(self._h))

    def violation_prob(self, obs, act, prob_out=None, logits_out=None, layout: str = "rows"):
        """compute_safety_violation_probability of the installed categorical critic over a batch, on the device: p of
        "nig-categorical-v1" for n (state, action) pairs; the action is used as given.  layout "rows": obs [n, S], act [n, A]
        (transposed on the device first); "soa": obs [S, >=n], act [A, >=n] with unit column stride, read in place, n = the
        pitch-free width obs.shape[1].  prob_out float32 [>=n], logits_out float32 [atoms, >=n] (optional; words past column
        n - 1 keep their values).  A kernel of its own: no env state is read or written.  Returns p [n]."""
        obs, act = (torch.as_tensor(x, dtype=torch.float32, device=self.device) for x in (obs, act))
        if layout == "rows":
            obs, act = obs.reshape(-1, self.state_dim).t().contiguous(), act.reshape(-1, self.action_dim).t().contiguous()
        elif layout != "soa":
            raise ValueError(f"layout is 'rows' or 'soa', not {layout!r}")
        if obs.dim() != 2 or act.dim() != 2 or obs.shape[0] != self.state_dim or act.shape[0] != self.action_dim:
            raise ValueError(f"obs / act must be [{self.state_dim}, n] / [{self.action_dim}, n] (layout 'soa'), got {tuple(obs.shape)} / {tuple(act.shape)}")
        n = int(obs.shape[1])
        if n < 1 or act.shape[1] < n or (n > 1 and (obs.stride(1) != 1 or act.stride(1) != 1)):     # (one column has no column stride)
            raise ValueError("obs / act need n >= 1 columns of unit stride, act at least as many as obs")
        atoms = int(self._L.nig_get_mlp_safety_atoms(self._h))          # (the handle's own: the critic may have been installed through the C ABI)
        if prob_out is None:
            prob_out = torch.empty(n, dtype=torch.float32, device=self.device)

        def on_device(t, what):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != obs.device.type
                    or t.device.index != obs.device.index):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
        on_device(prob_out, "prob_out")
        if prob_out.dim() != 1 or prob_out.shape[0] < n or (prob_out.shape[0] > 1 and prob_out.stride(0) != 1):
            raise ValueError(f"prob_out must be a contiguous vector of at least {n} words")
        zp, ldz = None, 0
        if logits_out is not None:
            on_device(logits_out, "logits_out")
            if logits_out.dim() != 2 or logits_out.shape[0] < atoms or logits_out.shape[1] < n or (logits_out.shape[1] > 1 and logits_out.stride(1) != 1):
                raise ValueError(f"logits_out must be [>= {atoms} atoms, >= {n}] with unit column stride, got {tuple(logits_out.shape)}")
            zp, ldz = C.c_void_p(logits_out.data_ptr()), max(int(logits_out.stride(0)), n)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_mlp_violation_prob(self._h, n, _ptr(obs), obs.stride(0), _ptr(act), act.stride(0), _ptr(prob_out),
                                                      zp, ldz, self._stream()))
        return prob_out[:n]

    def rollout_mlp_safe(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, prob_out=None):
        """rollout_mlp() with the safety-critic shield (predict_with_safety on the device): act_out holds the action the
        env received; prob_out float32 [n_steps, >=B] the critic's p of the unshielded action (same row stride as
        reward_out / flags_out); flags carry FLAG_SHIELDED where the action was halved."""
        self._closed_loop(self._L.nig_rollout_mlp_safe, n_steps, reward_out, flags_out, obs_out, act_out,
                          rows=[("prob_out", prob_out, torch.float32)])

    def rollout_mlp_safe_limited(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, prob_out=None,
                                 xflags_out=None):
        """rollout_mlp_safe() under the added safety constraints (add_safety_constraint; "nig-limits-v1"), checked on the action
        the env received; xflags_out as rollout_policy_limited()'s."""
        self._closed_loop(self._L.nig_rollout_mlp_safe_limited, n_steps, reward_out, flags_out, obs_out, act_out,
                          rows=[("prob_out", prob_out, torch.float32)], xflags=(xflags_out,))

    def rollout_mlp_search(self, n_steps: int, n_candidates: int, reward_out=None, flags_out=None, obs_out=None, act_out=None,
                           prob_out=None, risk_out=None, choice_out=None):
        """rollout_mlp_safe() with the safety-critical agents' get_safe_action in place of the halving ("nig-search-v1",
        include/nig.h): where the installed critic's p of the actor's action is not below the installed threshold, the env
        receives the first of least p among n_candidates (1 .. MAX_CANDIDATES) uniform actions of [-1, 1)
        (policies.search_candidates restates the draws).  act_out holds the action the env received; prob_out float32 the
        actor's action's p, risk_out float32 the received action's p, choice_out int32 the candidate's number (-1: the actor's
        action was kept), each [n_steps, >=B] with the row stride of reward_out / flags_out; flags carry FLAG_SHIELDED where
        a candidate was taken."""
        self._closed_loop(self._L.nig_rollout_mlp_search, n_steps, reward_out, flags_out, obs_out, act_out, head=(int(n_candidates),),
                          rows=[("prob_out", prob_out, torch.float32), ("risk_out", risk_out, torch.float32), ("choice_out", choice_out, torch.int32)])

    def rollout_mlp_search_limited(self, n_steps: int, n_candidates: int, reward_out=None, flags_out=None, obs_out=None, act_out=None,
                                   prob_out=None, risk_out=None, choice_out=None, xflags_out=None):
        """rollout_mlp_search() under the added safety constraints, checked on the action the env received; xflags_out as
        rollout_policy_limited()'s."""
        self._closed_loop(self._L.nig_rollout_mlp_search_limited, n_steps, reward_out, flags_out, obs_out, act_out, head=(int(n_candidates),),
                          rows=[("prob_out", prob_out, torch.float32), ("risk_out", risk_out, torch.float32), ("choice_out", choice_out, torch.int32)],
                          xflags=(xflags_out,))

    def set_mlp_safety_ensemble(self, members, temperature: float = 1.0, threshold: float = 0.1, max_uncertainty: float = 0.2):
        """Install the safety ensemble of SafeEnsembleAgent (agents/safety_critical.py) for rollout_mlp_gated(): `members` = a
        list of 1 .. MAX_ENSEMBLE set_mlp_safety() weight lists whose heads have the same 1 .. 4 columns, one per constraint
        (C3 [256, C], c3 [C]).  The law "nig-gate-v1" (include/nig.h) takes the temperature and the two limits as given.
        The actor, the single critic and the actor ensemble stay as they are."""
        K, Hd, D = len(members), 256, self.state_dim + self.action_dim
        n_out = int(np.asarray(members[0][2][1]).size) if K else 0
        W = [_mlp_weights(m, [(D, Hd), (Hd,), (Hd, Hd), (Hd,), (Hd, n_out), (n_out,)]) for m in members]
        cols = [(C.c_void_p * K)(*[w[j].ctypes.data for w in W]) for j in range(6)] if K else [None] * 6
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_safety_ensemble(self._h, K, Hd, n_out, *cols, float(temperature), float(threshold),
                                                           float(max_uncertainty), self._stream()))
        self._gate_shape = (K, n_out)

    def rollout_mlp_gated(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, prob_out=None,
                          unc_out=None, logit_out=None):
        """rollout_mlp() with the installed safety ensemble's gate (SafeEnsembleAgent.get_safe_action on the device): the env
        receives the actor's action where every constraint's violation probability is below the threshold and every spread
        below the limit, the zero action elsewhere.  act_out holds the action the env received; prob_out / unc_out float32
        [n_steps, C, >=B] p and sd per constraint; logit_out float32 [n_steps, K, C, >=B] every member's logits (the three
        share their pitches); flags carry FLAG_SHIELDED where the action was replaced and FLAG_UNCERTAIN where a spread is not
        below the limit."""
        self._gated(self._L.nig_rollout_mlp_gated, (), n_steps, reward_out, flags_out, obs_out, act_out, prob_out, unc_out, logit_out)

    def rollout_mlp_gated_limited(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, prob_out=None,
                                  unc_out=None, logit_out=None, xflags_out=None):
        """rollout_mlp_gated() under the added safety constraints, checked on the action the env received; xflags_out as
        rollout_policy_limited()'s."""
        self._gated(self._L.nig_rollout_mlp_gated_limited, (xflags_out,), n_steps, reward_out, flags_out, obs_out, act_out, prob_out, unc_out,
                    logit_out)

    def _gated(self, fn, xflags, n_steps, reward_out, flags_out, obs_out, act_out, prob_out, unc_out, logit_out):
        K, Cn = getattr(self, "_gate_shape", (0, 0))
        ptrs, pitches = [], set()
        for name, t, lead in (("prob_out", prob_out, ()), ("unc_out", unc_out, ()), ("logit_out", logit_out, (K,))):
            if t is None:
                ptrs.append(None)
                continue
            assert t.dtype == torch.float32 and t.dim() == 3 + len(lead) and t.stride(-1) == 1, name
            assert t.shape[0] >= n_steps and tuple(t.shape[1:-1]) == lead + (Cn,) and t.shape[-1] >= self.batch, name
            assert not lead or t.stride(0) == K * t.stride(1), name
            ptrs.append(C.c_void_p(t.data_ptr()))
            pitches.add((t.stride(-2), t.stride(-3)))
        assert len(pitches) <= 1, "prob_out, unc_out and logit_out share their pitches"
        ld_c, c_step = pitches.pop() if pitches else (0, 0)
        self._closed_loop(fn, n_steps, reward_out, flags_out, obs_out, act_out, tail=(*ptrs, ld_c, c_step), xflags=xflags)

    def set_mlp_constraint(self, predictor, threshold: float = 0.1, tolerance: float = 0.01):
        """Install the constraint predictor of ConstrainedIQLAgent (agents/safety_critical.py) for rollout_mlp_projected():
        `predictor` = a set_mlp_safety() weight list whose head has 1 .. 4 columns, one per constraint (C3 [256, C], c3 [C]).  The
        law "nig-project-v1" (include/nig.h) takes the acceptance threshold and the tolerance as given.  The actor, the critic,
        the gate and the actor ensemble stay as they are."""
        Hd, D = 256, self.state_dim + self.action_dim
        n_out = int(np.asarray(predictor[2][1]).size)
        W = _mlp_weights(predictor, [(D, Hd), (Hd,), (Hd, Hd), (Hd,), (Hd, n_out), (n_out,)])
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_constraint(self._h, Hd, n_out, *[C.c_void_p(w.ctypes.data) for w in W], float(threshold),
                                                      float(tolerance), self._stream()))
        self._constraint_outputs = n_out

    def rollout_mlp_projected(self, n_steps: int, max_iters: int = 10, step: float = 0.1, reward_out=None, flags_out=None, obs_out=None,
                              act_out=None, prob_out=None, viol_out=None, iters_out=None, grad_out=None):
        """rollout_mlp() with the installed constraint predictor's projection (ConstrainedIQLAgent.get_safe_action on the
        device): the env receives the actor's action where every constraint's violation probability is below the threshold;
        elsewhere the action after up to max_iters (1 .. MAX_PROJECT_ITERS) gradient steps of size `step` towards logits below the
        tolerance.  act_out holds the action the env received; prob_out / viol_out float32 [n_steps, C, >=B] the probabilities of
        the actor's action / of the action the env received (they share their pitches); iters_out int32 [n_steps, >=B] the
        gradient steps taken, -1 where the actor's action was kept; grad_out float32 [n_steps, A, >=B] (act_out's pitches) the
        first gradient, written where iters >= 1; flags carry FLAG_SHIELDED on projected lanes."""
        self._projected(self._L.nig_rollout_mlp_projected, (), n_steps, max_iters, step, reward_out, flags_out, obs_out, act_out,
                        prob_out, viol_out, iters_out, grad_out)

    def rollout_mlp_projected_limited(self, n_steps: int, max_iters: int = 10, step: float = 0.1, reward_out=None, flags_out=None,
                                      obs_out=None, act_out=None, prob_out=None, viol_out=None, iters_out=None, grad_out=None,
                                      xflags_out=None):
        """rollout_mlp_projected() under the added safety constraints, checked on the action the env received; xflags_out as
        rollout_policy_limited()'s."""
        self._projected(self._L.nig_rollout_mlp_projected_limited, (xflags_out,), n_steps, max_iters, step, reward_out, flags_out,
                        obs_out, act_out, prob_out, viol_out, iters_out, grad_out)

    def _projected(self, fn, xflags, n_steps, max_iters, step, reward_out, flags_out, obs_out, act_out, prob_out, viol_out, iters_out,
                   grad_out):
        Cn = getattr(self, "_constraint_outputs", 0)
        ptrs, pitches = [], set()
        for name, t in (("prob_out", prob_out), ("viol_out", viol_out)):
            if t is None:
                ptrs.append(None)
                continue
            assert t.dtype == torch.float32 and t.dim() == 3 and t.stride(-1) == 1, name
            assert t.shape[0] >= n_steps and t.shape[1] == Cn and t.shape[-1] >= self.batch, name
            ptrs.append(C.c_void_p(t.data_ptr()))
            pitches.add((t.stride(1), t.stride(0)))
        assert len(pitches) <= 1, "prob_out and viol_out share their pitches"
        ld_c, c_step = pitches.pop() if pitches else (0, 0)
        gp, grad_pitches = None, None
        if grad_out is not None:
            assert grad_out.dtype == torch.float32 and grad_out.dim() == 3 and grad_out.stride(2) == 1, "grad_out"
            assert grad_out.shape[0] >= n_steps and grad_out.shape[1] == self.action_dim and grad_out.shape[2] >= self.batch, "grad_out"
            gp, grad_pitches = C.c_void_p(grad_out.data_ptr()), (grad_out.stride(1), grad_out.stride(0))
        self._closed_loop(fn, n_steps, reward_out, flags_out, obs_out, act_out, head=(int(max_iters), float(step)), front=ptrs,
                          rows=[("iters_out", iters_out, torch.int32)], tail=(gp, ld_c, c_step), act_pitches=("grad_out", grad_pitches),
                          xflags=xflags, sharing="iters_out (and xflags_out) share")

    def set_mlp_ensemble(self, members, weights=None, weight_sum=None, method: str = "mean", uncertainty_threshold: float = 0.2):
        """Install an ensemble of actors (agents/ensemble.py EnsembleAgent) for rollout_mlp_ensemble(): `members` = a list of
        set_mlp_policy() weight lists.  method "mean" / "weighted": `weights` = the ACTIVE float64 weights of np.average (for
        "mean" already divided by their sum, as the reference does) and `weight_sum` = np.sum(weights) (computed here with
        NumPy when None); "voting": both ignored.  policies.EnsemblePolicy.install() derives all of it from an agent."""
        if method not in ("mean", "weighted", "voting"):
            raise ValueError(f"Unknown ensemble method: {method}")
        K, Hd = len(members), 256
        W = [_mlp_weights(m, self._actor_shapes()) for m in members]
        cols = [(C.c_void_p * K)(*[w[j].ctypes.data for w in W]) for j in range(6)] if K else [None] * 6
        wp, ws = None, 0.0
        if method != "voting":
            aw = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
            assert aw.shape == (K,), aw.shape
            wp, ws = aw.ctypes.data_as(C.c_void_p), float(np.sum(aw) if weight_sum is None else weight_sum)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_mlp_ensemble(self._h, K, Hd, *cols, _lib.ENSEMBLE_VOTING if method == "voting" else _lib.ENSEMBLE_AVERAGE,
                                                    wp, ws, float(uncertainty_threshold), self._stream()))
        self._ensemble_members = K

    def rollout_mlp_ensemble(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, unc_out=None,
                             member_act_out=None):
        """rollout_mlp() with the installed ensemble: act_out holds the action the env received (the float64 average rounded
        to float32 for "mean" / "weighted"); unc_out float32 [n_steps, >=B] the members' disagreement (same row stride as
        reward_out / flags_out); member_act_out float32 [n_steps, K, A, >=B] every member's action (same pitches as act_out);
        flags carry FLAG_UNCERTAIN where the uncertainty exceeds the installed threshold."""
        self._ensemble(self._L.nig_rollout_mlp_ensemble, (), n_steps, reward_out, flags_out, obs_out, act_out, unc_out, member_act_out)

    def rollout_mlp_ensemble_limited(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, unc_out=None,
                                     member_act_out=None, xflags_out=None):
        """rollout_mlp_ensemble() under the added safety constraints, checked on the action the env received (the float64 average
        where the env steps on it); xflags_out as rollout_policy_limited()'s."""
        self._ensemble(self._L.nig_rollout_mlp_ensemble_limited, (xflags_out,), n_steps, reward_out, flags_out, obs_out, act_out, unc_out,
                       member_act_out)

    def _ensemble(self, fn, xflags, n_steps, reward_out, flags_out, obs_out, act_out, unc_out, member_act_out):
        mp, pitches = None, None
        if member_act_out is not None:
            K, m = getattr(self, "_ensemble_members", 0), member_act_out
            assert m.dtype == torch.float32 and m.dim() == 4 and m.stride(3) == 1 and m.stride(0) == K * m.stride(1)
            assert m.shape[0] >= n_steps and m.shape[1] == K and m.shape[2] == self.action_dim and m.shape[3] >= self.batch
            mp, pitches = C.c_void_p(m.data_ptr()), (m.stride(2), m.stride(1))
        self._closed_loop(fn, n_steps, reward_out, flags_out, obs_out, act_out,
                          rows=[("unc_out", unc_out, torch.float32)], tail=(mp,), act_pitches=("member_act_out", pitches), xflags=xflags)

    def _closed_loop(self, fn, n_steps, reward_out, flags_out, obs_out, act_out, head=(), front=(), rows=(), tail=(), act_pitches=(None, None),
                     xflags=(), sharing=None):
        """One closed-loop call of the C ABI: fn(handle, n_steps, *head, <the eight output arguments the closed loops share: reward
        ptr, flags ptr, out_stride, obs ptr, obs_step_stride, act ptr, ld_act, act_step_stride>, *front, <a pointer per entry of
        `rows`>, *tail, <a _limited twin's xflags_out>, stream), the four optional output tensors validated.  rows: (name, tensor or
        None, dtype) of the variant's extra per-step rows [n_steps, >=B], which share the row stride of reward_out / flags_out.
        xflags: () for a parent, (xflags_out,) for a _limited twin -- such a row, the last argument before the stream.  act_pitches:
        (name, (ld_act, act_step_stride) or None) of an output that shares act_out's pitches and states them where act_out is
        absent (the ensemble's member_act_out, the projection's grad_out).  sharing: the subject of the row-stride message where
        it is not made of the rows' names."""
        rp, fp, os_, op, so, ap, lda, sa = self._closed_loop_outputs(n_steps, reward_out, flags_out, obs_out, act_out)
        rows = [*rows, *(("xflags_out", t, torch.int32) for t in xflags)]
        extra = [_rows(t, dtype, n_steps) for _, t, dtype in rows]
        strides = {st for ptr, st in extra if ptr is not None} | ({os_} if (rp is not None or fp is not None) else set())
        names = [name for name, _, _ in rows]
        assert len(strides) <= 1, (sharing or (f"{', '.join(names[:-1])} and {names[-1]} share" if len(names) > 1 else f"{names[0]} shares")) \
            + " the reward/flags row stride"
        name, pitches = act_pitches
        if pitches is not None:
            assert ap is None or pitches == (lda, sa), f"{name} shares act_out's pitches"
            lda, sa = pitches
        ptrs = [ptr for ptr, _ in extra]
        with torch.cuda.device(self._dev_index):
            _lib.check(fn(self._h, int(n_steps), *head, rp, fp, strides.pop() if strides else 0, op, so, ap, lda, sa, *front,
                          *ptrs[:len(ptrs) - len(xflags)], *tail, *ptrs[len(ptrs) - len(xflags):], self._stream()))

    def _closed_loop_outputs(self, n_steps, reward_out, flags_out, obs_out, act_out):
        """The output arguments the closed-loop rollouts share, from the optional tensors, validated:
        (reward ptr, flags ptr, out_stride, obs ptr, obs_step_stride, act ptr, ld_act, act_step_stride)."""
        rp, rs = _rows(reward_out, torch.float32, n_steps)
        fp, fs = _rows(flags_out, torch.int32, n_steps)
        assert rp is None or fp is None or rs == fs
        op, so = None, 0
        if obs_out is not None:
            assert obs_out.dtype == torch.float32 and obs_out.is_contiguous()
            assert obs_out.shape[0] >= n_steps and obs_out.shape[1:] == (self.batch, self.state_dim)
            op, so = C.c_void_p(obs_out.data_ptr()), obs_out.stride(0)
        ap, lda, sa = None, 0, 0
        if act_out is not None:
            assert act_out.dtype == torch.float32 and act_out.dim() == 3 and act_out.stride(2) == 1
            assert act_out.shape[0] >= n_steps and act_out.shape[1] == self.action_dim and act_out.shape[2] >= self.batch
            ap, lda, sa = C.c_void_p(act_out.data_ptr()), act_out.stride(1), act_out.stride(0)
        return rp, fp, rs or fs, op, so, ap, lda, sa

    def rollout_policy(self, n_steps: int, reward_out: Optional[torch.Tensor] = None,
                       flags_out: Optional[torch.Tensor] = None, obs_out: Optional[torch.Tensor] = None,
                       act_out: Optional[torch.Tensor] = None):
        """n_steps closed-loop steps (action = installed policy(observation)) in ONE launch.
        obs_out: float32 contiguous [n_steps, B, S] (observation the policy acted on);
        act_out: float32 [n_steps, A, >=B]; reward_out / flags_out: [n_steps, >=B] or [B]."""
        self._closed_loop(self._L.nig_rollout_policy, n_steps, reward_out, flags_out, obs_out, act_out)

    def rollout_policy_limited(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, xflags_out=None):
        """rollout_policy() under the added safety constraints (add_safety_constraint; "nig-limits-v1"): xflags_out int32
        [n_steps, >=B] (the row stride of reward_out / flags_out) is the added constraints' word of every step -- bit c: added
        constraint c violated, bits 4-6 how many, bits 8-10 how many critical ones."""
        self._closed_loop(self._L.nig_rollout_policy_limited, n_steps, reward_out, flags_out, obs_out, act_out, xflags=(xflags_out,))

    def rollout_mlp_limited(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, xflags_out=None):
        """rollout_mlp() under the added safety constraints; outputs as rollout_policy_limited()."""
        self._closed_loop(self._L.nig_rollout_mlp_limited, n_steps, reward_out, flags_out, obs_out, act_out, xflags=(xflags_out,))

    # ------------------------------------------------------------------
    def set_disturbance(self, disturbance):
        """Install the sensor / actuator noise (disturbance.Disturbance) the _disturbed rollouts apply; None removes it.
        The other rollouts ignore it."""
        with torch.cuda.device(self._dev_index):
            if disturbance is None:
                _lib.check(self._L.nig_set_disturbance(self._h, None, self._stream()))
            else:
                D = disturbance.to_struct(self.state_dim, self.action_dim) if hasattr(disturbance, "to_struct") else disturbance
                _lib.check(self._L.nig_set_disturbance(self._h, C.byref(D), self._stream()))
        self._disturbance = disturbance

    def _seen_rows(self, n_steps, seen_out):
        if seen_out is None:
            return None, 0
        assert seen_out.dtype == torch.float32 and seen_out.is_contiguous()
        assert seen_out.shape[0] >= n_steps and seen_out.shape[1:] == (self.batch, self.state_dim)
        return C.c_void_p(seen_out.data_ptr()), seen_out.stride(0)

    def rollout_policy_disturbed(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, seen_out=None):
        """rollout_policy() under the installed disturbance ("nig-disturb-v1"): obs_out holds the TRUE state, seen_out
        (float32 contiguous [n_steps, B, S]) the noisy observation the policy acted on, act_out the action the env received."""
        self._closed_loop(self._L.nig_rollout_policy_disturbed, n_steps, reward_out, flags_out, obs_out, act_out,
                          tail=self._seen_rows(n_steps, seen_out))

    def rollout_mlp_disturbed(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, seen_out=None):
        """rollout_mlp() under the installed disturbance; outputs as rollout_policy_disturbed()."""
        self._closed_loop(self._L.nig_rollout_mlp_disturbed, n_steps, reward_out, flags_out, obs_out, act_out,
                          tail=self._seen_rows(n_steps, seen_out))

    def rollout_policy_disturbed_limited(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, seen_out=None,
                                         xflags_out=None):
        """rollout_policy_disturbed() under the added safety constraints, checked on the true state and the action the env received;
        xflags_out as rollout_policy_limited()'s."""
        self._closed_loop(self._L.nig_rollout_policy_disturbed_limited, n_steps, reward_out, flags_out, obs_out, act_out,
                          tail=self._seen_rows(n_steps, seen_out), xflags=(xflags_out,))

    def rollout_mlp_disturbed_limited(self, n_steps: int, reward_out=None, flags_out=None, obs_out=None, act_out=None, seen_out=None,
                                      xflags_out=None):
        """rollout_mlp_disturbed() under the added safety constraints; outputs as rollout_policy_disturbed_limited()."""
        self._closed_loop(self._L.nig_rollout_mlp_disturbed_limited, n_steps, reward_out, flags_out, obs_out, act_out,
                          tail=self._seen_rows(n_steps, seen_out), xflags=(xflags_out,))

    def get_dataset(self, quality: str = "mixed", scale: int = 1, chunk: int = 100):
        """Batched env.get_dataset(quality): every lane is one episode of the reference's
        data-collection loop (chemical_reactor.py:324-420, power_grid.py:194-249,
        robot_assembly.py:246-308) driven by the on-device behaviour policy; `scale` multiplies
        the upstream episode count.  Needs batch >= episodes*scale and autoreset=False.
        Returns the D4RL-style dict as torch tensors on the device (episode-major order)."""
        from .policies import DATASET_SHAPE, behaviour_policy
        self._refuse_limits("get_dataset")
        assert not self.autoreset, "dataset generation needs autoreset=False (one episode per lane)"
        n_eps, cap = DATASET_SHAPE[self.env_id][quality]
        n_eps *= int(scale)
        if n_eps > self.batch:
            raise ValueError(f"batch {self.batch} < {n_eps} episodes")
        B, S, A = self.batch, self.state_dim, self.action_dim
        self.set_policy(behaviour_policy(self.env_id, quality))
        mask = torch.zeros(B, dtype=torch.uint8, device=self.device)
        mask[:n_eps] = 1
        self.ctr.fill_(_lib.CTR_DONE)                 # lanes beyond n_eps stay idle
        self.reset(mask=mask)
        obs_c, act_c, rew_c, live_c, term_c = [], [], [], [], []
        done_steps = 0
        while done_steps < cap:
            T = min(chunk, cap - done_steps)
            obs = torch.empty(T, B, S, dtype=torch.float32, device=self.device)
            act = torch.empty(T, A, self.ld, dtype=torch.float32, device=self.device)
            rew = torch.empty(T, self.ld, dtype=torch.float32, device=self.device)
            fl = torch.empty(T, self.ld, dtype=torch.int32, device=self.device)
            self.rollout_policy(T, rew, fl, obs, act)
            live = (fl[:, :n_eps] & _lib.FLAG_INACTIVE) == 0
            obs_c.append(obs[:, :n_eps]); act_c.append(act[:, :, :n_eps]); rew_c.append(rew[:, :n_eps])
            live_c.append(live)
            both = (fl[:, :n_eps] & (_lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED)) != 0
            term_c.append(both if self.env_id == "ChemicalReactor-v0" else (fl[:, :n_eps] & _lib.FLAG_TERMINATED) != 0)
            done_steps += T
            if not bool(live[-1].any().item()):
                break
        live = torch.cat(live_c).t()                                  # [episodes, steps] -> episode-major
        sel = live.reshape(-1)
        obs = torch.cat(obs_c).permute(1, 0, 2).reshape(-1, S)[sel]
        act = torch.cat(act_c).permute(2, 0, 1).reshape(-1, A)[sel]
        rew = torch.cat(rew_c).t().reshape(-1)[sel]
        term = torch.cat(term_c).t().reshape(-1)[sel]
        out = {"observations": obs, "actions": act, "rewards": rew, "terminals": term}
        if self.env_id == "ChemicalReactor-v0":
            out["timeouts"] = torch.zeros_like(term)
        return out

    def fill_actions(self, t: int, out: Optional[torch.Tensor] = None):
        """Synthetic uniform [-1,1) actions of the bench workload for launch counter t -> [A, B]."""
        if out is None:
            out = torch.empty(self.action_dim, self.ld, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_fill_actions(self._h, C.c_uint32(t), _ptr(out), out.stride(0), self._stream()))
        return out

    # ------------------------------------------------------------------
    def set_state(self, state=None, current_step=None, violation_count=None, done=None):
        """Teacher forcing: state [B,S] or [S,B]; counters optional (per-lane arrays)."""
        B, S = self.batch, self.state_dim
        st = None
        if state is not None:
            t = torch.as_tensor(state, dtype=torch.float32, device=self.device)
            st = (t.t() if t.shape == (B, S) else t).contiguous()    # [B,S] wins when B == S
            assert st.shape == (S, B)
        c = None
        if current_step is not None or violation_count is not None or done is not None:
            cs = torch.as_tensor(0 if current_step is None else current_step, device=self.device).to(torch.int64)
            vc = torch.as_tensor(0 if violation_count is None else violation_count, device=self.device).to(torch.int64)
            dn = torch.as_tensor(False if done is None else done, device=self.device).to(torch.int64)
            word = (cs & _lib.CTR_STEP_MASK) | (dn * _lib.CTR_DONE) | ((vc & 0xFFFF) << _lib.CTR_VIOL_SHIFT)
            word = torch.broadcast_to(word, (B,))
            c = torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32).contiguous()
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_set_state(self._h, _ptr(st), B, _ptr(c), self._stream()))

    def get_state(self) -> torch.Tensor:
        """A contiguous [B, S] copy of the current state."""
        return self.obs.contiguous()

    def get_safety_metrics(self):
        """Per-lane SafetyMetrics fields of the last step as an int32 tensor [5, B]
        (rows: constraints_satisfied, total_constraints, violation_count, critical_violations,
        satisfied = safety_score * total)."""
        out = torch.empty(5, self.batch, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_get_safety_metrics(self._h, _ptr(self.flags), _ptr(out), self.batch, self._stream()))
        if self._added:             # the added constraints of the last step: counted in, satisfied where they did not fire
            live = (self.flags & _lib.FLAG_INACTIVE) == 0
            nv = torch.where(live, (self.xflags >> _lib.XFLAG_NVIOL_SHIFT) & 7, torch.zeros_like(self.xflags))
            nc = torch.where(live, (self.xflags >> _lib.XFLAG_NCRIT_SHIFT) & 7, torch.zeros_like(self.xflags))
            n = torch.where(live, torch.full_like(nv, len(self._added)), torch.zeros_like(nv))
            out[0] += n - nv
            out[1] += n
            out[2] += nv
            out[3] += nc
            out[4] += n - nv
        return out

    def episode_log(self, capacity: int, ld: Optional[int] = None):
        """A log of `capacity` per-episode records per lane (episodes.EpisodeLog; include/nig.h nig_episode_log_*), cleared."""
        from .episodes import EpisodeLog
        return EpisodeLog(self, capacity, ld)

    def collect_episodes(self, log, n_steps: int, reward_rows: torch.Tensor, flag_rows: torch.Tensor):
        """nig_collect_episodes: the n_steps reward / flag rows a rollout (or step) of this env wrote go into `log` -- finished
        episodes become records, the running ones stay in the log's carry for the next call."""
        log.collect(n_steps, reward_rows, flag_rows)

    def reduce_tally(self) -> torch.Tensor:
        """Device reduction of the per-lane tallies -> float64 [T_ROWS] partial vector."""
        out = torch.empty(_lib.T_ROWS, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self._dev_index):
            _lib.check(self._L.nig_reduce_tally(self._h, _ptr(out), self._stream()))
        return out


class StepPlan:
    """n consecutive env.step() launches replayed as one hipGraph (include/nig.h nig_plan_*)."""

    def __init__(self, env: BatchedIndustrialEnv, n_steps: int, action_ring: torch.Tensor,
                 reward_ring: Optional[torch.Tensor], flags_ring: Optional[torch.Tensor]):
        assert action_ring.dtype == torch.float32 and action_ring.dim() == 3 and action_ring.stride(2) == 1
        R, A, ld = action_ring.shape[0], action_ring.shape[1], action_ring.stride(1)
        assert A == env.action_dim and ld >= env.batch
        self.env, self.n_steps = env, int(n_steps)
        self._keep = (action_ring, reward_ring, flags_ring)

        rp, rs = _rows(reward_ring, torch.float32)            # (a ring: no lower bound on its slots)
        fp, fs = _rows(flags_ring, torch.int32)
        assert rs == fs or rp is None or fp is None, "reward/flags rings must share their slot stride"
        p = C.c_void_p()
        with torch.cuda.device(env._dev_index):
            _lib.check(env._L.nig_plan_create(env._h, self.n_steps, C.c_void_p(action_ring.data_ptr()), ld,
                                              action_ring.stride(0), R, rp, fp, rs or fs, C.byref(p)))
        self._p = p

    def launch(self):
        _lib.check(self.env._L.nig_plan_launch(self._p, self.env._stream()))

    def close(self):
        if getattr(self, "_p", None):
            self.env._L.nig_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MixedBatchedEnv:
    """Several env types in one padded batch (BASELINE config "all envs mixed-batch, heterogeneous
    state dims, padded SoA").  Lanes are grouped in contiguous, 256-aligned segments, one env type
    each (every wavefront is homogeneous); all segments share ONE observation matrix
    `state_soa` [S_max, LD] (rows >= S of a segment stay zero) and one action matrix layout
    [A_max, LD].  Each segment is a BatchedIndustrialEnv bound to its columns; a step or rollout
    launches one kernel per segment, each on its own HIP stream.  max_episode_steps (optional) replaces every segment's
    own episode limit."""

    def __init__(self, segments, device="cuda:0", seed: int = 0x5EED, autoreset: bool = True, tally: bool = False,
                 env_index0: int = 0, fused: bool = True, max_episode_steps: Optional[int] = None):
        self.device = torch.device(device)
        segs = list(segments.items()) if isinstance(segments, dict) else list(segments)
        self.S_max = max(int(_lib.env_spec(ENV_IDS[e]).state_dim) for e, _ in segs)
        self.A_max = max(int(_lib.env_spec(ENV_IDS[e]).action_dim) for e, _ in segs)
        offs, off = [], 0
        for _, n in segs:
            offs.append(off)
            off += (int(n) + 255) // 256 * 256
        self.ld = off
        self.batch = sum(int(n) for _, n in segs)
        self.state_soa = torch.zeros(self.S_max, self.ld, dtype=torch.float32, device=self.device)
        self.obs = self.state_soa.t()
        self.reward = torch.zeros(self.ld, dtype=torch.float32, device=self.device)
        self.flags = torch.zeros(self.ld, dtype=torch.int32, device=self.device)
        self.offsets = offs
        self.envs = []
        for (e, n), o in zip(segs, offs):
            self.envs.append(BatchedIndustrialEnv(e, int(n), device=device, seed=seed, env_index0=env_index0 + o,
                                                  autoreset=autoreset, tally=tally, max_episode_steps=max_episode_steps,
                                                  bind_state=self.state_soa[:, o:o + int(n)]))
        self._streams = [torch.cuda.Stream(device=self.device) for _ in self.envs]
        self.fused = bool(fused)
        n = len(self.envs)
        self._hs = (C.c_void_p * n)(*[e._h for e in self.envs])
        self._offs = (C.c_int64 * n)(*offs)

    def _fan(self, fn):
        cur = torch.cuda.current_stream(self.device)
        ev = torch.cuda.Event(); ev.record(cur)
        for env, st, o in zip(self.envs, self._streams, self.offsets):
            st.wait_event(ev)
            with torch.cuda.stream(st):
                fn(env, o)
            done = torch.cuda.Event(); done.record(st)
            cur.wait_event(done)

    def reset(self):
        self._fan(lambda env, o: env.reset())
        return self.obs

    def step(self, actions_soa: torch.Tensor):
        """actions_soa: float32 [A_max, LD] (rows >= A of a segment ignored).  Returns the padded
        (obs view [LD, S_max], reward [LD], flags [LD])."""
        assert actions_soa.shape == (self.A_max, self.ld) and actions_soa.stride(1) == 1

        def f(env, o):
            env.step(actions_soa[:env.action_dim, o:o + env.batch], layout="soa")
            self.reward[o:o + env.batch].copy_(env.reward)
            self.flags[o:o + env.batch].copy_(env.flags)
        self._fan(f)
        return self.obs, self.reward, self.flags

    def rollout(self, n_steps: int, action_ring: torch.Tensor, reward_out=None, flags_out=None, obs_out=None):
        """action_ring: float32 [R, A_max, LD]; optional reward/flags outputs [n_steps, LD]; optional obs_out float32
        [n_steps, S_max, LD]: the observation every env.step returns, in the padded SoA layout of the state matrix
        (rows >= S of a segment are left as they are)."""
        assert action_ring.shape[1:] == (self.A_max, self.ld)
        if obs_out is not None:
            assert reward_out is not None and obs_out.dtype == torch.float32 and obs_out.dim() == 3
            assert obs_out.shape[0] >= n_steps and obs_out.shape[1] >= self.S_max and obs_out.shape[2] == self.ld
            assert obs_out.stride(2) == 1 and obs_out.stride(1) == self.ld
        if self.fused:
            assert action_ring.dtype == torch.float32 and action_ring.stride(2) == 1 and action_ring.stride(1) == self.ld
            assert (reward_out is None) == (flags_out is None)
            os_ = 0
            if reward_out is not None:
                assert reward_out.dtype == torch.float32 and flags_out.dtype == torch.int32
                assert reward_out.shape[-1] == self.ld and flags_out.shape[-1] == self.ld
                os_ = reward_out.stride(0) if reward_out.dim() == 2 else 0
                assert (flags_out.stride(0) if flags_out.dim() == 2 else 0) == os_
            L = self.envs[0]._L
            with torch.cuda.device(self.envs[0]._dev_index):
                _lib.check(L.nig_rollout_mixed_obs(self._hs, self._offs, len(self.envs), int(n_steps),
                                                   C.c_void_p(action_ring.data_ptr()), self.ld, action_ring.stride(0),
                                                   action_ring.shape[0], _ptr(reward_out), _ptr(flags_out), os_,
                                                   _ptr(obs_out), self.ld, 0 if obs_out is None else obs_out.stride(0),
                                                   self.envs[0]._stream()))
            return

        def f(env, o):
            env.rollout(n_steps, action_ring[:, :env.action_dim, o:o + env.batch],
                        None if reward_out is None else reward_out[:, o:o + env.batch],
                        None if flags_out is None else flags_out[:, o:o + env.batch],
                        None if obs_out is None else obs_out[:, :env.state_dim, o:o + env.batch])
        self._fan(f)

    def fill_actions(self, t: int, out: torch.Tensor):
        self._fan(lambda env, o: env.fill_actions(t, out[:env.action_dim, o:o + env.batch]))
        return out

    def reduce_tally(self):
        return [env.reduce_tally() for env in self.envs]

    def close(self):
        for e in self.envs:
            e.close()
