"""Policies that run ON the device inside the fused closed-loop rollout ("nig-policy-v1",
include/nig.h), with a host `predict()` of the same float32 arithmetic so the very same
object also works with the single-env classes and the reference-shaped evaluation loop.

Families (all the reference's non-neural agents):
  * baseline agents of benchmarks/baseline_agents.py:28-114: constant_agent, mpc_agent
    ("MPC" = proportional pull to the origin), pid_agent, random_agent;
  * behaviour policies of get_dataset: behaviour_policy(env_id, quality)
    (chemical_reactor.py:364-393, power_grid.py:216-233, robot_assembly.py:266-290).
The neural actors (agents/networks.py) stay outside: pass any object with
`predict_device(obs_tensor)` / `predict(obs)` to evaluate_with_safety for those.
"""
from typing import Optional, Sequence

import numpy as np

from . import _lib

f32 = np.float32
_DIMS = {"ChemicalReactor-v0": (12, 3), "PowerGrid-v0": (32, 8), "RobotAssembly-v0": (24, 7)}


class DevicePolicy:
    """a = clip(b + W @ obs (+ noise, + epsilon-uniform mixture), lo, hi)  or a PID law."""
    is_trained = True          # evaluate_with_safety's gate (utils.py:69-70)

    def __init__(self, state_dim: int, action_dim: int, kind: int = _lib.POLICY_AFFINE, W=None, b=None, sigma=None,
                 half_range=None, p_uniform: float = 0.0, uniform_range: float = 1.0, clip=(-np.inf, np.inf),
                 kp: float = 0.0, ki: float = 0.0, kd: float = 0.0, setpoint=None):
        assert state_dim <= 32 and action_dim <= 10      # NIG_MAX_STATE_DIM / NIG_MAX_ACTION_DIM (include/nig.h)
        self.state_dim, self.action_dim, self.kind = state_dim, action_dim, kind
        z = lambda: np.zeros(action_dim, dtype=f32)     # noqa: E731
        self.W = np.zeros((action_dim, state_dim), dtype=f32) if W is None else np.asarray(W, dtype=f32)
        self.b = z() if b is None else np.asarray(b, dtype=f32)
        self.sigma = z() if sigma is None else np.asarray(sigma, dtype=f32)
        self.half_range = z() if half_range is None else np.asarray(half_range, dtype=f32)
        self.p_uniform, self.uniform_range = f32(p_uniform), f32(uniform_range)
        self.clip = (f32(clip[0]), f32(clip[1]))
        self.kp, self.ki, self.kd = f32(kp), f32(ki), f32(kd)
        self.setpoint = z() if setpoint is None else np.asarray(setpoint, dtype=f32)
        self._integ, self._eprev = z(), z()
        assert self.W.shape == (action_dim, state_dim)

    @property
    def stochastic(self) -> bool:
        return bool(np.any(self.sigma != 0) or np.any(self.half_range != 0) or self.p_uniform > 0)

    def to_struct(self) -> _lib.Policy:
        P = _lib.Policy()
        P.kind = self.kind
        for j in range(self.action_dim):
            for k in range(self.state_dim):
                P.Wt[k][j] = float(self.W[j, k])
            P.b[j], P.sigma[j], P.half_range[j] = float(self.b[j]), float(self.sigma[j]), float(self.half_range[j])
            P.setpoint[j] = float(self.setpoint[j])
        P.p_uniform, P.uniform_range = float(self.p_uniform), float(self.uniform_range)
        P.clip_lo, P.clip_hi = float(self.clip[0]), float(self.clip[1])
        P.kp, P.ki, P.kd = float(self.kp), float(self.ki), float(self.kd)
        return P

    def predict(self, observations, deterministic: bool = True):
        """Host evaluation of the deterministic part in the device's float32 term order
        (agent.predict contract, agents/base.py:106-141: [n,S] -> [n,A])."""
        obs = np.asarray(observations, dtype=f32)
        single = obs.ndim == 1
        obs = np.atleast_2d(obs)
        out = np.zeros((obs.shape[0], self.action_dim), dtype=f32)
        for i, o in enumerate(obs):
            if self.kind == _lib.POLICY_PID:
                e = self.setpoint - o[:self.action_dim]
                self._integ = (self._integ + e).astype(f32)
                u = ((self.kp * e + self.ki * self._integ) + self.kd * (e - self._eprev)).astype(f32)
                self._eprev = e
            else:
                u = self.b.copy()
                for k in range(self.state_dim):
                    if np.any(self.W[:, k] != 0):
                        u = (u + self.W[:, k] * o[k]).astype(f32)
            out[i] = np.minimum(np.maximum(u, self.clip[0]), self.clip[1])
        return out[0] if single else out


def constant_agent(state_dim: int, action_dim: int, constant_action: Optional[Sequence[float]] = None) -> DevicePolicy:
    """ConstantAgent, baseline_agents.py:102-113"""
    return DevicePolicy(state_dim, action_dim, b=np.zeros(action_dim) if constant_action is None else constant_action)


def mpc_agent(state_dim: int, action_dim: int) -> DevicePolicy:
    """MPC_Agent, baseline_agents.py:83-99: 0.5 * (0 - state[:A]) clipped to [-1, 1]."""
    W = np.zeros((action_dim, state_dim), dtype=f32)
    for j in range(action_dim):
        W[j, j] = -0.5
    return DevicePolicy(state_dim, action_dim, W=W, clip=(-1.0, 1.0))


def pid_agent(state_dim: int, action_dim: int, kp=1.0, ki=0.1, kd=0.01, setpoint=None) -> DevicePolicy:
    """PIDControllerAgent, baseline_agents.py:44-80 (integral never reset, as upstream)."""
    return DevicePolicy(state_dim, action_dim, kind=_lib.POLICY_PID, kp=kp, ki=ki, kd=kd, setpoint=setpoint,
                        clip=(-1.0, 1.0))


def random_agent(state_dim: int, action_dim: int, action_low: float = -1.0, action_high: float = 1.0) -> DevicePolicy:
    """RandomAgent, baseline_agents.py:28-41 (symmetric range)."""
    assert action_low == -action_high, "the device mixture draws from U(-r, r)"
    return DevicePolicy(state_dim, action_dim, p_uniform=1.0, uniform_range=action_high)


# (episodes, step cap) of each get_dataset quality
from .spec_plants import PLANTS as _PLANT_LIST  # noqa: E402

_SPEC_PLANTS = {p["name"]: p for p in _PLANT_LIST}
for _p in _PLANT_LIST:
    _DIMS[_p["name"]] = (len(_p["y"]) + len(_p["act"]) + 3, len(_p["act"]))

DATASET_SHAPE = {
    "ChemicalReactor-v0": {"expert": (100, 400), "medium": (200, 350), "mixed": (300, 300), "random": (500, 200)},
    "PowerGrid-v0": {"expert": (100, 1000), "medium": (150, 1000), "mixed": (200, 1000), "random": (80, 1000)},
    "RobotAssembly-v0": {"expert": (120, 1000), "medium": (180, 1000), "mixed": (250, 1000), "random": (100, 1000)},
}
# README-only envs: (episodes, step cap) chosen here, nothing upstream to follow
for _p in _PLANT_LIST:
    DATASET_SHAPE[_p["name"]] = {"expert": (100, 500), "medium": (150, 500), "mixed": (200, 500), "random": (100, 500)}


def behaviour_policy(env_id: str, quality: str) -> DevicePolicy:
    """The data-collection policy of env.get_dataset(quality) as a device policy."""
    S, A = _DIMS[env_id]
    W = np.zeros((A, S), dtype=np.float64)
    b = np.zeros(A)
    if env_id == "ChemicalReactor-v0":                       # chemical_reactor.py:333-393
        nl = {"expert": 0.1, "medium": 0.3, "mixed": 0.5}.get(quality, 1.0)
        if quality == "expert":
            W[0, 0], b[0] = -0.5 / 50, 0.5 * 320.0 / 50      # -temp_error*0.5, temp_error=(T-320)/50
            W[1, 0], b[1] = 0.3 / 50, -0.3 * 320.0 / 50      #  temp_error*0.3
            W[2, 10], b[2] = -0.2 / 50, 0.2 * 55.0 / 50      # -level_error*0.2
            return DevicePolicy(S, A, W=W, b=b, sigma=[nl * 0.1] * 3, clip=(-1.0, 1.0))
        if nl >= 1.0:
            # "random": np.random.random() < (1 - 1.0) never holds (:380), so every action is uniform(-1, 1, 3) (:389):
            # no feedback term at all (found by tests/golden/behaviour_laws.npz: the reference's law with its draws
            # patched to zero is identically 0 here)
            return DevicePolicy(S, A, p_uniform=1.0, uniform_range=1.0, clip=(-1.0, 1.0))
        W[0, 0], b[0] = -0.2 / 50, 0.2 * 320.0 / 50
        return DevicePolicy(S, A, W=W, b=b, sigma=[nl * 0.3, nl * 0.5, nl * 0.3], p_uniform=nl, uniform_range=1.0,
                            clip=(-1.0, 1.0))
    if env_id == "PowerGrid-v0":                             # power_grid.py:216-233 (no policy-side clip)
        if quality == "expert":
            W[:, 0] = -0.5
            W[:, 17:25] = 0.1 / A
            W[:, 9:17] = -0.1 / A
            return DevicePolicy(S, A, W=W)
        if quality == "random":
            return DevicePolicy(S, A, p_uniform=1.0, uniform_range=5.0)
        W[:, 0] = -0.3
        return DevicePolicy(S, A, W=W, p_uniform=0.4, uniform_range=3.0)
    if env_id == "RobotAssembly-v0":                         # robot_assembly.py:266-292, np.clip(action, -2, 2)
        tgt = [0.3, 0.0, 0.4]
        if quality == "expert":
            for j in range(3):
                W[j, j], b[j] = -2.0, 2.0 * tgt[j]
            for i in range(4):
                W[3 + i, 10 + i] = -0.1
            return DevicePolicy(S, A, W=W, b=b, clip=(-2.0, 2.0))
        if quality == "random":
            return DevicePolicy(S, A, p_uniform=1.0, uniform_range=1.0, clip=(-2.0, 2.0))
        for j in range(3):
            W[j, j], b[j] = -1.0, tgt[j]
        return DevicePolicy(S, A, W=W, b=b, half_range=[0, 0, 0, 0.5, 0.5, 0.5, 0.5], p_uniform=0.3,
                            uniform_range=0.8, clip=(-2.0, 2.0))
    if env_id in _SPEC_PLANTS:                               # build-specified plants: proportional control on the table
        return _spec_behaviour(_SPEC_PLANTS[env_id], quality)
    raise ValueError(env_id)


def _spec_behaviour(P, quality: str) -> DevicePolicy:
    """Data-collection policies of the four README-only envs (no upstream get_dataset exists for them):
    a proportional controller read off the plant table -- actuator j is driven against the weighted
    setpoint errors of the variables it acts on, u_j = -kp * sum_i w_i sign(G_ij) (y_i - sp_i) / span_i --
    plus Gaussian exploration noise (expert), a weaker gain with an epsilon-uniform mixture (medium,
    mixed), or uniform actions (random)."""
    ys, acts = P["y"], P["act"]
    NP_, A = len(ys), len(acts)
    S = NP_ + A + 3
    if quality == "random":
        return DevicePolicy(S, A, p_uniform=1.0, uniform_range=1.0, clip=(-1.0, 1.0))
    kp, sigma, eps = {"expert": (2.0, 0.05, 0.0), "medium": (1.0, 0.15, 0.1)}.get(quality, (0.5, 0.3, 0.3))
    W = np.zeros((A, S))
    b = np.zeros(A)
    aidx = {a["name"]: j for j, a in enumerate(acts)}
    for i, y in enumerate(ys):
        if y["w"] == 0.0:
            continue
        span = max(abs(y["hi"] - y["lo"]), 1e-6)
        for name, g in y["gains"].items():
            c = -kp * np.sign(g) * min(1.0, y["w"] * 10.0) / span * 10.0
            W[aidx[name], i] += c
            b[aidx[name]] -= c * y["sp"]
    return DevicePolicy(S, A, W=W, b=b, sigma=[sigma] * A, p_uniform=eps, uniform_range=1.0, clip=(-1.0, 1.0))


_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
STREAM_POLICY, SEARCH_BLOCK0 = 0xC0000000, 0x100     # csrc/nig_detmath.hpp, csrc/nig_mlp.hpp


def philox4x32_7(ctr, key):
    """Philox4x32 with seven rounds (the library's generator, csrc/nig_detmath.hpp) of counters ctr [n, 4] under keys
    key [n, 2] (or one key [2]) -> uint32 [n, 4]."""
    c = np.asarray(ctr, dtype=np.uint64).reshape(-1, 4) & np.uint64(0xFFFFFFFF)
    k = np.broadcast_to(np.asarray(key, dtype=np.uint64).reshape(-1, 2), (c.shape[0], 2)) & np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    lo32, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(7):
        p0, p1 = np.uint64(_PHILOX_M0) * c0, np.uint64(_PHILOX_M1) * c2         # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & lo32, (p0 >> sh) ^ c3 ^ k1, p0 & lo32
        k0, k1 = (k0 + np.uint64(_PHILOX_W0)) & lo32, (k1 + np.uint64(_PHILOX_W1)) & lo32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def search_candidates(seed: int, env_index: int, t: int, n_candidates: int, action_dim: int):
    """The candidate actions nig_rollout_mlp_search draws for lane `env_index` (its global index) on the step whose launch
    counter is t: float32 [n_candidates, action_dim], the one host statement of "nig-search-v1"'s draws (include/nig.h).
    Action j of candidate c is fmaf(w >> 8, 2^-23, -1) -- uniform on [-1, 1), a multiple of 2^-23, so the float32 arithmetic
    below rounds nothing -- of word j & 3 of the policy stream's block 0x100 + 4 c + (j >> 2) under the key (env_index, t, seed)."""
    N, A = int(n_candidates), int(action_dim)
    nb = (A + 3) // 4
    assert N >= 1 and 1 <= nb <= 4
    blocks = STREAM_POLICY + SEARCH_BLOCK0 + 4 * np.arange(N, dtype=np.uint64)[:, None] + np.arange(nb, dtype=np.uint64)[None, :]
    ctr = np.empty((N * nb, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = int(env_index) & 0xFFFFFFFF, (int(env_index) >> 32) & 0xFFFFFFFF, int(t) & 0xFFFFFFFF
    ctr[:, 3] = blocks.reshape(-1)
    w = philox4x32_7(ctr, [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]).reshape(N, 4 * nb)[:, :A]
    return ((w >> np.uint32(8)).astype(f32) * f32(2.0 ** -23) - f32(1.0)).astype(f32)


def categorical_mass(logits, below):
    """The softmax mass of logits [n, N] on the atoms of the bool mask `below` [N], in torch: exp(z - max z) summed over the
    mask / over all atoms -- "nig-categorical-v1"'s formula (include/nig.h) without its summation order or its det_expf."""
    import torch
    e = torch.exp(logits - logits.max(dim=1, keepdim=True).values)
    return (e * below.to(e.dtype)).sum(dim=1) / e.sum(dim=1)


def pad_critic(weights, hidden: int = 256):
    """A critic [(C1 [D,h], c1 [h]), (C2 [h,h], c2 [h]), (C3 [h,1], c3 [1])] with h <= hidden (the reference's RiskEstimator:
    128) as the `hidden`-wide network set_mlp_safety() takes: C1's columns, C2's rows and columns, C3's rows and the biases
    padded with zeros.  The added units are exactly 0 after ReLU and every added term is an exact zero, so the padded
    network computes the h-wide one's number.  hidden-wide weights come back as float32 copies; anything else is refused."""
    if len(weights) != 3:
        raise ValueError(f"a critic has three layers, got {len(weights)}")
    (C1, c1), (C2, c2), (C3, c3) = [(np.asarray(W, dtype=f32), np.asarray(b, dtype=f32).reshape(-1)) for W, b in weights]
    C3 = C3.reshape(C3.shape[0], -1)
    h = C1.shape[1]
    if not (1 <= h <= hidden and C2.shape == (h, h) and C3.shape == (h, 1) and c1.shape == (h,) and c2.shape == (h,) and c3.shape == (1,)):
        raise ValueError(f"cannot pad a critic of shapes {[np.shape(W) for W, _ in weights]} to hidden width {hidden}")
    P1, p1 = np.zeros((C1.shape[0], hidden), dtype=f32), np.zeros(hidden, dtype=f32)
    P2, p2 = np.zeros((hidden, hidden), dtype=f32), np.zeros(hidden, dtype=f32)
    P3 = np.zeros((hidden, 1), dtype=f32)
    P1[:, :h], p1[:h], P2[:h, :h], p2[:h], P3[:h] = C1, c1, C2, c2, C3
    return [(P1, p1), (P2, p2), (P3, c3.copy())]


# The shape classes of the float32 MFMA actor ("nig-mlp-shape-v1", include/nig.h), cheapest first among those of equal depth:
# name -> the widths a network is zero-padded to.  "reference" is the 256 x 256 kernel of set_mlp_policy.
ACTOR_SHAPE_CLASSES = (("128x128", (128, 128)), ("reference", (256, 256)), ("512x256", (512, 256)), ("512x512", (512, 512)),
                       ("256x256x256", (256, 256, 256)))


def actor_shape_class(hidden_dims):
    """The name of the cheapest shape class (fewest MFMAs per step) that holds an actor with these hidden widths -- "128x128",
    "reference", "512x256", "512x512", "256x256x256" -- or None where no class does: one or more than three hidden layers, a
    width outside 1 .. 512.  The library's own choice (nig_set_mlp_policy_dims) is the same function."""
    dims = tuple(int(d) for d in hidden_dims)
    for name, cls in ACTOR_SHAPE_CLASSES:
        if len(cls) == len(dims) and all(1 <= d <= c for d, c in zip(dims, cls)):
            return name
    return None


def pad_actor(weights, dims):
    """An actor [(W1 [S,h1], b1), .., (W_head [h_last,A], b_head)] zero-padded to the hidden widths `dims` (one per hidden layer,
    each at least the network's own): the columns and biases of a hidden layer and the rows of the layer above it.  The added
    units are exactly relu(0) = 0 and every added term is fma(w, 0, c) == c, so the padded network computes the same numbers (the
    sign of a zero aside).  Float32 copies come back; anything that does not fit is refused."""
    dims = tuple(int(d) for d in dims)
    ws = [(np.asarray(W, dtype=f32), np.asarray(b, dtype=f32).reshape(-1)) for W, b in weights]
    own = tuple(W.shape[1] for W, _ in ws[:-1])
    if len(ws) != len(dims) + 1 or any(o > d for o, d in zip(own, dims)) or any(W.shape[1] != b.shape[0] for W, b in ws) \
            or any(ws[i + 1][0].shape[0] != own[i] for i in range(len(own))):
        raise ValueError(f"cannot pad an actor of shapes {[np.shape(W) for W, _ in weights]} to hidden widths {dims}")
    out, rows = [], ws[0][0].shape[0]
    for i, (W, b) in enumerate(ws):
        cols = dims[i] if i < len(dims) else W.shape[1]
        P, q = np.zeros((rows, cols), dtype=f32), np.zeros(cols, dtype=f32)
        P[:W.shape[0], :W.shape[1]], q[:b.shape[0]] = W, b
        out.append((P, q))
        rows = cols
    return out


def pad_safety_member(weights, hidden: int = 256):
    """pad_critic for a head of 1 .. 4 columns: a safety-ensemble member [(C1 [D,h], c1 [h]), (C2 [h,h], c2 [h]), (C3 [h,C], c3 [C])]
    with h <= hidden (the reference's SafetyEnsembleMember: 128) as the `hidden`-wide network set_mlp_safety_ensemble() takes.
    The added units are exactly 0 after ReLU and every added term is an exact zero, so each padded row computes the h-wide
    one's number.  hidden-wide weights come back as float32 copies; anything else is refused."""
    if len(weights) != 3:
        raise ValueError(f"a safety-ensemble member has three layers, got {len(weights)}")
    (C1, c1), (C2, c2), (C3, c3) = [(np.asarray(W, dtype=f32), np.asarray(b, dtype=f32).reshape(-1)) for W, b in weights]
    C3 = C3.reshape(C3.shape[0], -1)
    h, n = C1.shape[1], c3.shape[0]
    if not (1 <= h <= hidden and 1 <= n <= 4 and C2.shape == (h, h) and C3.shape == (h, n) and c1.shape == (h,) and c2.shape == (h,)):
        raise ValueError(f"cannot pad a member of shapes {[np.shape(W) for W, _ in weights]} to hidden width {hidden} and a head of 1 .. 4 columns")
    P1, p1 = np.zeros((C1.shape[0], hidden), dtype=f32), np.zeros(hidden, dtype=f32)
    P2, p2 = np.zeros((hidden, hidden), dtype=f32), np.zeros(hidden, dtype=f32)
    P3 = np.zeros((hidden, n), dtype=f32)
    P1[:, :h], p1[:h], P2[:h, :h], p2[:h], P3[:h] = C1, c1, C2, c2, C3
    return [(P1, p1), (P2, p2), (P3, c3.copy())]


def bf16_round(x):
    """bf(x) of "nig-mlp-bf16-v1" (include/nig.h): float32 -> bfloat16, round to nearest even, returned as float32 (the low 16
    bits of every word are zero; `.view(np.uint32) >> 16` are the bf16 words).  A NaN stays a (quiet) NaN.  NumPy only."""
    u = np.ascontiguousarray(np.asarray(x, dtype=f32)).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = (u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))).astype(np.uint32) & np.uint32(0xFFFF0000)
    r = np.where(nan, (u & np.uint32(0xFFFF0000)) | np.uint32(0x00400000), r).astype(np.uint32)
    return r.view(f32).reshape(np.shape(x))


def bf16_split(x):
    """The law's input split: (hi, lo) float32 with hi = bf(x), lo = bf(x - hi) (the subtraction is exact in float32), lo = 0
    where hi is not finite."""
    x = np.asarray(x, dtype=f32)
    hi = bf16_round(x)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = bf16_round((x - hi).astype(f32))
    return hi, np.where(np.isfinite(hi), lo, f32(0)).astype(f32)


def mlp_bf16_reference(weights, obs, h1=None, h2=None):
    """ "nig-mlp-bf16-v1" with float64 sums, for obs [n, S] float32 and weights [(W1, b1), (W2, b2), (W3, b3)]: a dict of
    z1, h1, z2, h2, z3 (pre-activations float64; h1, h2 float32 holding bf16 values), action = tanh(z3) (float64), and abs1, abs2,
    abs3 = sum |term| including |bias| of every pre-activation (what an accumulation-error radius scales with).  h1 / h2 given:
    the layers behind them are computed from these activations instead (a device's own intermediates)."""
    f64 = np.float64
    (W1, b1), (W2, b2), (W3, b3) = [(bf16_round(W).astype(f64), np.asarray(b, dtype=f32).astype(f64).reshape(-1)) for W, b in weights]
    hi, lo = bf16_split(np.asarray(obs, dtype=f32).reshape(-1, W1.shape[0]))
    x = np.concatenate([hi, lo], axis=1).astype(f64)
    W1x = np.concatenate([W1, W1], axis=0)
    out = {}

    def layer(k, x, W, b):
        out[f"z{k}"] = x @ W + b
        out[f"abs{k}"] = np.abs(x) @ np.abs(W) + np.abs(b)
        return out[f"z{k}"]

    z1 = layer(1, x, W1x, b1)
    out["h1"] = bf16_round(np.maximum(z1, 0).astype(f32)) if h1 is None else np.asarray(h1, dtype=f32)
    z2 = layer(2, out["h1"].astype(f64), W2, b2)
    out["h2"] = bf16_round(np.maximum(z2, 0).astype(f32)) if h2 is None else np.asarray(h2, dtype=f32)
    z3 = layer(3, out["h2"].astype(f64), W3, b3)
    out["action"] = np.tanh(z3)
    return out


class Bf16MLPPolicy:
    """MLPPolicy.bf16(): the same actor under "nig-mlp-bf16-v1" (include/nig.h) -- weights and activations rounded to bfloat16,
    the observation split into two bf16 parts, float32 sums -- for throughput-only sweeps: evaluate_with_safety and
    evaluate_episodes play it with rollout_mlp_bf16 (the actor on the bf16 matrix unit) where the env has the MFMA actor and no
    added constraints, and with this class's torch emulation of the law on the host loop elsewhere.  The emulation agrees with
    the kernel up to accumulation order."""
    is_trained = True
    precision = "bf16"

    def __init__(self, parent):
        import torch
        self.device, self.weights, self.fusable = parent.device, parent.weights, parent.fusable
        self.state_dim, self.action_dim = parent.state_dim, parent.action_dim
        bf = lambda W: W.to(torch.bfloat16).to(torch.float32)
        self.layers = [(bf(W), b) for W, b in parent.layers]
        self.layers[0] = (torch.cat([self.layers[0][0], self.layers[0][0]], dim=0).contiguous(), self.layers[0][1])

    def predict_device(self, obs):
        import torch
        bf = lambda v: v.to(torch.bfloat16).to(torch.float32)
        hi = bf(obs)
        lo = torch.where(torch.isfinite(hi), bf(obs - hi), torch.zeros_like(hi))
        x = torch.cat([hi, lo], dim=1)
        for i, (W, b) in enumerate(self.layers):
            x = torch.addmm(b, x, W)
            x = bf(torch.relu(x)) if i + 1 < len(self.layers) else torch.tanh(x)
        return x

    def predict(self, observations, deterministic: bool = True):
        import torch
        o = torch.as_tensor(np.asarray(observations, dtype=f32), device=self.device)
        single = o.dim() == 1
        out = self.predict_device(o.reshape(-1, self.state_dim)).cpu().numpy()
        return out[0] if single else out


class MLPPolicy:
    """The deterministic actor of the reference's agents -- (S -> 256 -> 256 -> A) ReLU MLP with a
    tanh head (agents/networks.py:47-70,125-144; cql.py:339-343) -- kept on the GPU.

    `weights` = [(W1 [S,H], b1 [H]), (W2 [H,H], b2 [H]), (W3 [H,A], b3 [A])] as exported from the
    agent (Flax Dense kernels are [in, out]).  evaluate_with_safety() calls `predict_device`, so
    observations and actions never leave the device; `predict` is the host form of the same net
    (agent.predict contract, agents/base.py:106-141).

    `safety_weights` (optional) = the agents' SafetyCritic, [(C1 [S+A,H], c1), (C2 [H,H], c2), (C3 [H,1], c3)]
    (networks.py:147-169), with `constraint_threshold` (base.py: 0.1): predict_with_safety() follows
    cql.py:354-394, and shielded() is the policy that acts with it (fused into the env kernel by
    evaluate_with_safety when both nets have the reference shape).

    safety_kind="categorical": `safety_weights` is the DistributionalSafetyCritic of RiskAwareCQLAgent instead
    (agents/safety_critical.py:92-110), [(C1 [S+A,H], c1), (C2 [H,H], c2), (C3 [H,N], c3 [N])] with 2 <= N <= 64 atoms, and p is
    its softmax mass on the atoms of `below_mask` (an int, bit j = atom j; default: linspace(-1, 1, N) < 0, the reference's
    compute_safety_violation_probability) -- the law "nig-categorical-v1" (include/nig.h).  Every method that scores with p
    (predict_with_safety, get_safe_action, shielded(), searching()) then scores with that p."""
    is_trained = True

    def __init__(self, weights, device="cuda:0", safety_weights=None, constraint_threshold: float = 0.1, safety_kind: str = "sigmoid",
                 below_mask=None):
        import torch
        self.device = torch.device(device)
        self.layers = [(torch.as_tensor(np.asarray(W), dtype=torch.float32, device=self.device).contiguous(),
                        torch.as_tensor(np.asarray(b), dtype=torch.float32, device=self.device).contiguous())
                       for W, b in weights]
        self.state_dim = self.layers[0][0].shape[0]
        self.action_dim = self.layers[-1][0].shape[1]
        self.weights = [(np.asarray(W, dtype=f32), np.asarray(b, dtype=f32)) for W, b in weights]
        # the fused MFMA kernel covers the reference actor shape; anything else goes through torch GEMMs
        self.fusable = (len(self.weights) == 3 and self.weights[0][0].shape[1] == 256
                        and self.weights[1][0].shape == (256, 256))
        # every hidden shape: the widths, and the shape class of the MFMA actor that holds them ("nig-mlp-shape-v1"; None: the host path)
        self.hidden_dims = tuple(int(W.shape[1]) for W, _ in self.weights[:-1])
        self.shape_class = actor_shape_class(self.hidden_dims)
        # the widths are a shaped class's own, no padding needed: what evaluate_with_safety sends to the shaped kernel by itself
        self.shape_class_exact = self.shape_class not in (None, "reference") and dict(ACTOR_SHAPE_CLASSES)[self.shape_class] == self.hidden_dims
        self.constraint_threshold = float(constraint_threshold)
        self.safety_weights = None
        self.safety_layers = None
        if safety_kind not in ("sigmoid", "categorical"):
            raise ValueError(f"safety_kind is 'sigmoid' or 'categorical', not {safety_kind!r}")
        self.safety_kind, self.below_mask = safety_kind, None
        if safety_weights is not None:
            self.safety_weights = [(np.asarray(W, dtype=f32).reshape(np.shape(W)[0], -1), np.asarray(b, dtype=f32).reshape(-1))
                                   for W, b in safety_weights]
            n_out = self.safety_weights[-1][0].shape[1]
            if safety_kind == "categorical":
                from .batched import categorical_below_mask
                if self.safety_weights[0][0].shape[0] != self.state_dim + self.action_dim or not 2 <= n_out <= _lib.MAX_ATOMS:
                    raise ValueError(f"distributional safety critic must map S+A={self.state_dim + self.action_dim} inputs to 2 .. "
                                     f"{_lib.MAX_ATOMS} atoms, got {[w.shape for w, _ in self.safety_weights]}")
                self.below_mask = categorical_below_mask(n_out) if below_mask is None else int(below_mask)
                if self.below_mask >> n_out:
                    raise ValueError(f"below_mask {self.below_mask:#x} has a bit at or above the {n_out} atoms")
                self._below = torch.as_tensor([(self.below_mask >> j) & 1 for j in range(n_out)], dtype=torch.bool, device=self.device)
            elif self.safety_weights[0][0].shape[0] != self.state_dim + self.action_dim or n_out != 1:
                raise ValueError(f"safety critic must map S+A={self.state_dim + self.action_dim} inputs to 1 output, got "
                                 f"{[w.shape for w, _ in self.safety_weights]}")
            self.safety_layers = [(torch.as_tensor(W, device=self.device).contiguous(), torch.as_tensor(b, device=self.device).contiguous())
                                  for W, b in self.safety_weights]
        # the shaped shield ("nig-mlp-shape-shield-v1"): the actor's widths are a shaped class's own and the sigmoid critic has the
        # same hidden widths, as the reference builds it (SafetyCritic(hidden_dims=self.hidden_dims)) -- what evaluate_with_safety
        # sends to set_mlp_policy_dims + set_mlp_safety_dims + rollout_mlp_safe by itself
        self.shape_shield_exact = bool(self.shape_class_exact and self.safety_weights is not None and safety_kind == "sigmoid"
                                       and tuple(int(W.shape[1]) for W, _ in self.safety_weights[:-1]) == self.hidden_dims)

    @classmethod
    def from_agent(cls, agent, device="cuda:0", critic: str = "safety", below_mask=None):
        """The actor (and, when the agent has one, the safety critic with the agent's constraint_threshold) of a
        reference agent: agent.state["actor"].params / agent.state["safety"].params, Flax trees
        {"params": {"MLP_0": {"Dense_0|1|2": {"kernel", "bias"}}}} (any nested mapping of array-likes).  LayerNorm
        networks are refused (ValueError); Dropout has no parameters and is inert at training=False.
        critic="risk": the critic is the RiskEstimator of the safety-critical agents (agents/safety_critical.py:113-149),
        agent.risk_state.params = {"params": {"layers_0", "layers_1", "risk_head"}} (modules built in setup), with
        agent.uncertainty_threshold as the threshold -- what get_safe_action / searching() score with.
        critic="distributional": the critic is the same agents' DistributionalSafetyCritic (safety_critical.py:92-110),
        agent.safety_state.params = {"params": {"layers_0", "layers_1", "value_head"}} with agent.distributional_atoms atoms
        (checked against the head), scored by compute_safety_violation_probability's softmax mass ("nig-categorical-v1";
        below_mask: the atoms that count, default the reference's linspace(-1, 1, atoms) < 0), agent.uncertainty_threshold
        as the threshold."""
        if critic not in ("safety", "risk", "distributional"):
            raise ValueError(f"critic is 'safety', 'risk' or 'distributional', not {critic!r}")
        state = agent.state
        actor = _dense_layers(state["actor"].params, "actor")
        if critic == "distributional":
            ss = getattr(agent, "safety_state", None)
            if ss is None or getattr(ss, "params", None) is None:
                raise ValueError("critic='distributional' needs agent.safety_state.params (a RiskAwareCQLAgent's DistributionalSafetyCritic)")
            layers = _named_layers(ss.params, ("layers_0", "layers_1", "value_head"), "distributional safety critic")
            atoms = getattr(agent, "distributional_atoms", None)
            if atoms is not None and int(atoms) != np.shape(layers[-1][0])[-1]:
                raise ValueError(f"agent.distributional_atoms = {atoms}, but the value head has {np.shape(layers[-1][0])[-1]} columns")
            return cls(actor, device=device, safety_weights=layers, constraint_threshold=getattr(agent, "uncertainty_threshold", 0.1),
                       safety_kind="categorical", below_mask=below_mask)
        if critic == "risk":
            rs = getattr(agent, "risk_state", None)
            if rs is None or getattr(rs, "params", None) is None:
                raise ValueError("critic='risk' needs agent.risk_state.params (a safety-critical agent's RiskEstimator)")
            return cls(actor, device=device, safety_weights=_named_layers(rs.params, ("layers_0", "layers_1", "risk_head"), "risk"),
                       constraint_threshold=getattr(agent, "uncertainty_threshold", 0.1))
        safety = state.get("safety") if hasattr(state, "get") else None
        critic = None if safety is None or getattr(safety, "params", None) is None else _dense_layers(safety.params, "safety")
        return cls(actor, device=device, safety_weights=critic,
                   constraint_threshold=getattr(agent, "constraint_threshold", 0.1))

    def predict_device(self, obs):
        import torch
        x = obs
        for i, (W, b) in enumerate(self.layers):
            x = torch.addmm(b, x, W)
            x = torch.relu(x) if i + 1 < len(self.layers) else torch.tanh(x)
        return x

    def predict(self, observations, deterministic: bool = True):
        import torch
        o = torch.as_tensor(np.asarray(observations, dtype=f32), device=self.device)
        single = o.dim() == 1
        out = self.predict_device(o.reshape(-1, self.state_dim)).cpu().numpy()
        return out[0] if single else out

    def bf16(self):
        """This actor under "nig-mlp-bf16-v1" (Bf16MLPPolicy): the bf16 matrix unit's kernel family, for throughput-only sweeps."""
        return Bf16MLPPolicy(self)

    def exploring(self, sigma: float = 0.1):
        """The reference agents' predict(obs, deterministic=False), clip(actor + sigma N(0,1), -1, 1) (agents/cql.py:345-350),
        as a policy of its own (for evaluate_with_safety: fused into the env kernel when the actor is fusable)."""
        from .disturbance import Disturbance, Disturbed
        return Disturbed(self, Disturbance(action_noise=sigma, clip=(-1.0, 1.0)))

    def _threshold(self, safety_threshold):
        return safety_threshold or self.constraint_threshold           # cql.py:384 (0.0 / None fall back)

    def safety_probs_device(self, obs, actions):
        """p = sigmoid(critic([obs, actions])), [n] (networks.py:147-169); with the categorical critic the softmax mass on the
        atoms of below_mask (safety_critical.py:151-171): "nig-categorical-v1"'s formula in torch's arithmetic -- max-shifted
        exponentials, V / T -- not its bits."""
        import torch
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        x = torch.cat([obs, actions], dim=1)
        for i, (W, b) in enumerate(self.safety_layers):
            x = torch.addmm(b, x, W)
            if i + 1 < len(self.safety_layers):
                x = torch.relu(x)
        if self.safety_kind == "categorical":
            return categorical_mass(x, self._below)
        return torch.sigmoid(x[:, 0])

    def compute_safety_violation_probability(self, state, action, env=None):
        """RiskAwareCQLAgent.compute_safety_violation_probability over a batch (the categorical critic; with the sigmoid critic,
        its p).  With `env` a BatchedIndustrialEnv whose shape has the MFMA actor and a critic of the reference's width, the
        critic is installed there and evaluated by the device kernel (env.violation_prob, "nig-categorical-v1" bit for bit);
        otherwise by the torch form.  state [n, S] / [S], action [n, A] / [A]; returns a NumPy array [n] (a float for one pair)."""
        import torch
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        o = torch.as_tensor(np.asarray(state, dtype=f32), device=self.device)
        single = o.dim() == 1
        o = o.reshape(-1, self.state_dim)
        a = torch.as_tensor(np.asarray(action, dtype=f32), device=self.device).reshape(-1, self.action_dim)
        sw = self.safety_weights
        on_device = (env is not None and self.safety_kind == "categorical" and env.state_dim % 2 == 0 and env.action_dim <= 16
                     and len(sw) == 3 and sw[0][0].shape[1] == 256 and sw[1][0].shape == (256, 256))
        if on_device:
            env.set_mlp_safety_categorical(sw, self.constraint_threshold, self.below_mask)
            p = env.violation_prob(o, a)
        else:
            p = self.safety_probs_device(o, a)
        p = p.cpu().numpy()
        return float(p[0]) if single else p

    def predict_with_safety_device(self, obs, safety_threshold=None):
        """predict_with_safety on device tensors: (actions [n, A], probs [n])."""
        import torch
        a = self.predict_device(obs)
        p = self.safety_probs_device(obs, a)
        return torch.where((p < self._threshold(safety_threshold))[:, None], a, a * 0.5), p

    def predict_with_safety(self, observations, safety_threshold=None):
        """cql.py:354-394: actions of the deterministic actor, halved where the safety critic's p is not below
        `safety_threshold or constraint_threshold`; returns (actions, safety_probs) as NumPy arrays."""
        import torch
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        o = torch.as_tensor(np.asarray(observations, dtype=f32), device=self.device)
        single = o.dim() == 1
        a, p = self.predict_with_safety_device(o.reshape(-1, self.state_dim), safety_threshold)
        a, p = a.cpu().numpy(), p.cpu().numpy()
        return (a[0], p[0]) if single else (a, p)

    def shielded(self, safety_threshold=None):
        """The policy that acts with predict_with_safety's actions (for evaluate_with_safety)."""
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        return ShieldedMLPPolicy(self, self._threshold(safety_threshold))


    # ---- get_safe_action of the safety-critical agents (agents/safety_critical.py:173-208) ----
    def _search_threshold(self, safety_threshold):
        return self.constraint_threshold if safety_threshold is None else float(safety_threshold)   # (0.0 is a threshold here)

    def get_safe_action_device(self, obs, preferred=None, n_candidates: int = 100, safety_threshold=None, generator=None):
        """RiskAwareCQLAgent.get_safe_action on device tensors, a batch of states at once: the critic scores `preferred`
        (default: the actor's action); rows whose risk is not below the threshold (default: constraint_threshold) get the
        first of least risk among n_candidates uniform actions, even where that risk is above the preferred action's (as the
        reference).  The law of nig_rollout_mlp_search with torch's draws, u = torch.rand((n, n_candidates, A), generator=
        generator) * 2 - 1 in one call, and torch's GEMMs: it agrees with the kernel in distribution, not draw for draw.
        Returns (actions [n, A], {"risk" [n]: of the returned action, "corrected" [n] bool, "choice" [n]: the candidate's
        number, -1 where the preferred action was kept})."""
        import torch
        a = self.predict_device(obs) if preferred is None else preferred
        p0 = self.safety_probs_device(obs, a)
        corrected = ~(p0 < self._search_threshold(safety_threshold))
        n, N = obs.shape[0], int(n_candidates)
        u = torch.rand((n, N, self.action_dim), generator=generator, dtype=torch.float32, device=obs.device) * 2.0 - 1.0
        best = torch.zeros(n, dtype=torch.int64, device=obs.device)
        p_best = self.safety_probs_device(obs, u[:, 0])
        for c in range(1, N):                                  # the running first minimum: memory does not grow with N
            pc = self.safety_probs_device(obs, u[:, c])
            take = (pc < p_best) | (torch.isnan(p_best) & ~torch.isnan(pc))
            p_best = torch.where(take, pc, p_best)
            best = torch.where(take, torch.full_like(best, c), best)
        u_best = u[torch.arange(n, device=obs.device), best]
        info = {"risk": torch.where(corrected, p_best, p0), "corrected": corrected,
                "choice": torch.where(corrected, best, torch.full_like(best, -1))}
        return torch.where(corrected[:, None], u_best, a), info

    def get_safe_action(self, observations, preferred=None, n_candidates: int = 100, safety_threshold=None, generator=None):
        """get_safe_action_device on host arrays: (actions, {"risk", "corrected", "choice"}) as NumPy arrays (scalars in the
        dict for a single observation, the reference's form)."""
        import torch
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        o = torch.as_tensor(np.asarray(observations, dtype=f32), device=self.device)
        single = o.dim() == 1
        pa = None if preferred is None else torch.as_tensor(np.asarray(preferred, dtype=f32), device=self.device).reshape(-1, self.action_dim)
        a, info = self.get_safe_action_device(o.reshape(-1, self.state_dim), pa, n_candidates, safety_threshold, generator)
        a, info = a.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}
        if single:
            return a[0], {"risk": float(info["risk"][0]), "corrected": bool(info["corrected"][0]), "choice": int(info["choice"][0])}
        return a, info

    def searching(self, n_candidates: int = 100, safety_threshold=None):
        """The policy that acts with get_safe_action's actions (for evaluate_with_safety / evaluate_episodes)."""
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        return SearchShieldPolicy(self, n_candidates, self._search_threshold(safety_threshold))


class LayerNormMLPPolicy:
    """The deterministic actor of a reference agent built with use_layer_norm=True (agents/networks.py MLP.__call__: Dense ->
    LayerNorm -> ReLU per hidden layer, tanh head), hidden widths exactly (256, 256), kept on the GPU.

    `weights` = [(W1 [S,256], b1), (W2 [256,256], b2), (W3 [256,A], b3)] (Flax Dense kernels are [in, out]); `norms` =
    [(scale1 [256], bias1 [256]), (scale2, bias2)], the two LayerNorms; `eps` flax's epsilon (1e-6).  On an env with the MFMA actor,
    without added constraints and without recorded draws, evaluate_with_safety / evaluate_episodes install it with
    env.set_mlp_policy_ln and play it inside the env kernel (rollout_mlp, the law "nig-mlp-ln-v1": csrc/nig_mlp_ln.hpp).
    `predict` / `predict_device` are the torch host form of the same formula -- two-pass variance, 1 / sqrt(var + eps) -- in torch's
    arithmetic, not the law's bits: the route on WaterTreatment and under added constraints.

    With `safety_weights` = [(C1 [S+A,256], c1), (C2 [256,256], c2), (C3 [256,1], c3)] and `safety_norms` (the critic's two
    LayerNorms; `safety_eps`: its epsilon, default `eps`) the policy also carries the agent's LayerNorm safety critic
    (agents/networks.py SafetyCritic with use_layer_norm=True) and `constraint_threshold` (base.py: 0.1): predict_with_safety()
    follows agents/cql.py:354-394, and shielded() is the policy evaluate_with_safety / evaluate_episodes play inside the env kernel
    (set_mlp_policy_ln + set_mlp_safety_ln + rollout_mlp_safe, the law "nig-mlp-ln-shield-v1": csrc/nig_mlp_ln_shield.hpp)."""
    is_trained = True
    normalization = "layer_norm"

    def __init__(self, weights, norms, eps: float = 1e-6, device="cuda:0", safety_weights=None, safety_norms=None, safety_eps=None,
                 constraint_threshold: float = 0.1):
        import torch
        self.device = torch.device(device)
        self.weights = [(np.asarray(W, dtype=f32), np.asarray(b, dtype=f32).reshape(-1)) for W, b in weights]
        self.norms = [(np.asarray(g, dtype=f32).reshape(-1), np.asarray(b, dtype=f32).reshape(-1)) for g, b in norms]
        if len(self.weights) != 3 or len(self.norms) != 2:
            raise ValueError(f"a LayerNorm actor has three Dense layers and two LayerNorms, got {len(self.weights)} and {len(self.norms)}")
        self.weights[2] = (self.weights[2][0].reshape(self.weights[1][0].shape[-1], -1), self.weights[2][1])
        (W1, b1), (W2, b2), (W3, b3) = self.weights
        self.hidden_dims = (int(W1.shape[1]), int(W2.shape[1]))
        if self.hidden_dims != (256, 256):
            raise ValueError(f"a LayerNorm actor has hidden widths (256, 256), got {self.hidden_dims}")
        if W2.shape != (256, 256) or W3.shape[0] != 256 or b1.shape != (256,) or b2.shape != (256,) or b3.shape != (W3.shape[1],) \
                or any(g.shape != (256,) or b.shape != (256,) for g, b in self.norms):
            raise ValueError(f"LayerNorm actor layers do not chain: {[W.shape for W, _ in self.weights]}, norms {[g.shape for g, _ in self.norms]}")
        self.eps = float(eps)
        if not (np.isfinite(self.eps) and self.eps > 0):
            raise ValueError(f"eps must be finite and positive, got {eps}")
        self.state_dim, self.action_dim = int(W1.shape[0]), int(W3.shape[1])
        T = lambda a: torch.as_tensor(a, dtype=torch.float32, device=self.device).contiguous()
        self.layers = [(T(W), T(b)) for W, b in self.weights]
        self.norm_layers = [(T(g), T(b)) for g, b in self.norms]
        self.fusable = True          # the shape "nig-mlp-ln-v1" covers: the constructor refuses every other
        self.constraint_threshold = float(constraint_threshold)
        self.safety_weights = self.safety_norms = self.safety_layers = self.safety_norm_layers = None
        self.safety_eps = self.eps if safety_eps is None else float(safety_eps)
        if (safety_weights is None) != (safety_norms is None):
            raise ValueError("a LayerNorm safety critic needs both safety_weights and safety_norms")
        if safety_weights is not None:
            sw = [(np.asarray(W, dtype=f32), np.asarray(b, dtype=f32).reshape(-1)) for W, b in safety_weights]
            sn = [(np.asarray(g, dtype=f32).reshape(-1), np.asarray(b, dtype=f32).reshape(-1)) for g, b in safety_norms]
            if len(sw) != 3 or len(sn) != 2:
                raise ValueError(f"a LayerNorm safety critic has three Dense layers and two LayerNorms, got {len(sw)} and {len(sn)}")
            sw[2] = (sw[2][0].reshape(sw[1][0].shape[-1], -1), sw[2][1])
            (C1, c1), (C2, c2), (C3, c3) = sw
            D = self.state_dim + self.action_dim
            if C1.shape != (D, 256) or C2.shape != (256, 256) or C3.shape != (256, 1) or c1.shape != (256,) or c2.shape != (256,) \
                    or c3.shape != (1,) or any(g.shape != (256,) or b.shape != (256,) for g, b in sn):
                raise ValueError(f"a LayerNorm safety critic is ({D}, 256), (256, 256), (256, 1) with two LayerNorms of 256, got "
                                 f"{[W.shape for W, _ in sw]}, norms {[g.shape for g, _ in sn]}")
            if not (np.isfinite(self.safety_eps) and self.safety_eps > 0):
                raise ValueError(f"safety_eps must be finite and positive, got {safety_eps}")
            self.safety_weights, self.safety_norms = sw, sn
            self.safety_layers = [(T(W), T(b)) for W, b in sw]
            self.safety_norm_layers = [(T(g), T(b)) for g, b in sn]

    @classmethod
    def from_agent(cls, agent, device="cuda:0", eps: float = 1e-6):
        """The actor of a reference agent trained with use_layer_norm=True: agent.state["actor"].params, a Flax tree
        {"params": {"MLP_0": {"Dense_0|1|2": {"kernel", "bias"}, "LayerNorm_0|1": {"scale", "bias"}}}} (any nested mapping of
        array-likes).  Both hidden layers must carry a LayerNorm with scale and bias; anything else is refused (ValueError).
        When agent.state has a "safety" entry that is not None, its params -- the same Dense_0..2 / LayerNorm_0..1 tree -- become the
        policy's safety critic, with agent.constraint_threshold; a safety tree without LayerNorm is a ValueError."""
        def read(t, what):
            while hasattr(t, "items") and not any(str(k).startswith("Dense_") for k in t.keys()):
                subs = [v for v in t.values() if hasattr(v, "items")]
                if len(subs) != 1:
                    raise ValueError(f"{what}: cannot find the Dense layers of the parameter tree (keys {list(t.keys())})")
                t = subs[0]
            if not hasattr(t, "items"):
                raise ValueError(f"{what}: cannot find the Dense layers of the parameter tree")
            dense = sorted((k for k in t.keys() if str(k).startswith("Dense_")), key=lambda k: int(str(k)[6:]))
            norm = sorted((k for k in t.keys() if str(k).startswith("LayerNorm_")), key=lambda k: int(str(k)[10:]))
            if [str(k) for k in dense] != ["Dense_0", "Dense_1", "Dense_2"] or [str(k) for k in norm] != ["LayerNorm_0", "LayerNorm_1"]:
                raise ValueError(f"{what}: a LayerNorm network is Dense_0..2 with LayerNorm_0 and LayerNorm_1, got {[str(k) for k in dense + norm]}")
            for k in norm:
                if not (hasattr(t[k], "keys") and "scale" in t[k].keys() and "bias" in t[k].keys()):
                    raise ValueError(f"{what}: {k} needs both scale and bias (use_scale / use_bias)")
            return ([(np.asarray(t[k]["kernel"], dtype=f32), np.asarray(t[k]["bias"], dtype=f32)) for k in dense],
                    [(np.asarray(t[k]["scale"], dtype=f32), np.asarray(t[k]["bias"], dtype=f32)) for k in norm])
        weights, norms = read(agent.state["actor"].params, "actor")
        safety = agent.state["safety"] if "safety" in agent.state else None
        if safety is None:
            return cls(weights, norms, eps=eps, device=device)
        sw, sn = read(safety.params, "safety")
        return cls(weights, norms, eps=eps, device=device, safety_weights=sw, safety_norms=sn,
                   constraint_threshold=getattr(agent, "constraint_threshold", 0.1))

    @staticmethod
    def _hidden(x, layers, norm_layers, eps):
        import torch
        for (W, b), (g, be) in zip(layers[:2], norm_layers):
            z = torch.addmm(b, x, W)
            d = z - z.mean(dim=1, keepdim=True)
            rs = torch.rsqrt((d * d).mean(dim=1, keepdim=True) + eps)
            x = torch.relu(d * (rs * g) + be)
        W, b = layers[2]
        return torch.addmm(b, x, W)

    def predict_device(self, obs):
        import torch
        return torch.tanh(self._hidden(obs, self.layers, self.norm_layers, self.eps))

    def _threshold(self, safety_threshold):
        return safety_threshold or self.constraint_threshold           # cql.py:384 (0.0 / None fall back)

    def safety_probs_device(self, obs, actions):
        """p = sigmoid(critic([obs, actions])), [n]: the LayerNorm critic in torch's arithmetic ("nig-mlp-ln-shield-v1"'s formula,
        not its bits)."""
        import torch
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        return torch.sigmoid(self._hidden(torch.cat([obs, actions], dim=1), self.safety_layers, self.safety_norm_layers, self.safety_eps)[:, 0])

    def predict_with_safety_device(self, obs, safety_threshold=None):
        """predict_with_safety on device tensors: (actions [n, A], probs [n])."""
        import torch
        a = self.predict_device(obs)
        p = self.safety_probs_device(obs, a)
        return torch.where((p < self._threshold(safety_threshold))[:, None], a, a * 0.5), p

    def predict_with_safety(self, observations, safety_threshold=None):
        """cql.py:354-394: actions of the deterministic actor, halved where the safety critic's p is not below
        `safety_threshold or constraint_threshold`; returns (actions, safety_probs) as NumPy arrays."""
        import torch
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        o = torch.as_tensor(np.asarray(observations, dtype=f32), device=self.device)
        single = o.dim() == 1
        a, p = self.predict_with_safety_device(o.reshape(-1, self.state_dim), safety_threshold)
        a, p = a.cpu().numpy(), p.cpu().numpy()
        return (a[0], p[0]) if single else (a, p)

    def shielded(self, safety_threshold=None):
        """The policy that acts with predict_with_safety's actions (for evaluate_with_safety / evaluate_episodes)."""
        if self.safety_layers is None:
            raise RuntimeError("Safety critic must be trained")
        return ShieldedLayerNormPolicy(self, self._threshold(safety_threshold))

    def predict(self, observations, deterministic: bool = True):
        import torch
        o = torch.as_tensor(np.asarray(observations, dtype=f32), device=self.device)
        single = o.dim() == 1
        out = self.predict_device(o.reshape(-1, self.state_dim)).cpu().numpy()
        return out[0] if single else out


class ShieldedLayerNormPolicy:
    """LayerNormMLPPolicy.shielded(): predict / predict_device give predict_with_safety's actions.  On an env with the MFMA actor,
    without added constraints and without recorded draws, evaluate_with_safety / evaluate_episodes run it fused into the env kernel
    (set_mlp_policy_ln + set_mlp_safety_ln + rollout_mlp_safe, "nig-mlp-ln-shield-v1"); otherwise through torch GEMMs."""
    is_trained = True
    normalization = "layer_norm"

    def __init__(self, base: LayerNormMLPPolicy, threshold: float):
        self.base = base
        self.threshold = float(threshold)
        self.state_dim, self.action_dim = base.state_dim, base.action_dim
        self.fusable = bool(base.fusable) and base.safety_weights is not None

    def predict_device(self, obs):
        return self.base.predict_with_safety_device(obs, self.threshold)[0]

    def predict(self, observations, deterministic: bool = True):
        return self.base.predict_with_safety(observations, self.threshold)[0]


class SearchShieldPolicy:
    """MLPPolicy.searching(): predict / predict_device give get_safe_action's actions.  When the actor has the reference shape
    and the critic three layers of hidden width <= 256 (padded to 256 by pad_critic: the reference's RiskEstimator is 128 wide),
    evaluate_with_safety runs it fused into the env kernel (BatchedIndustrialEnv.rollout_mlp_search); otherwise, and under a
    disturbance.Disturbed wrapper, through torch GEMMs with torch's draws."""
    is_trained = True

    def __init__(self, base: MLPPolicy, n_candidates: int, threshold: float):
        if not 1 <= int(n_candidates) <= _lib.MAX_CANDIDATES:
            raise ValueError(f"n_candidates must lie in 1 .. {_lib.MAX_CANDIDATES}, got {n_candidates}")
        self.base = base
        self.n_candidates, self.threshold = int(n_candidates), float(threshold)
        self.state_dim, self.action_dim = base.state_dim, base.action_dim
        self.weights = base.weights
        sw = base.safety_weights
        h = sw[0][0].shape[1]
        self.safety_kind, self.below_mask = base.safety_kind, base.below_mask
        if self.safety_kind == "categorical":      # the reference's DistributionalSafetyCritic is 256 wide: no padding
            self.fusable = base.fusable and len(sw) == 3 and h == 256 and sw[1][0].shape == (h, h)
            self.safety_weights = sw                                        # what set_mlp_safety_categorical takes
        else:
            self.fusable = base.fusable and len(sw) == 3 and h <= 256 and sw[1][0].shape == (h, h)
            self.safety_weights = pad_critic(sw) if self.fusable else sw    # what set_mlp_safety takes

    def predict_device(self, obs):
        return self.base.get_safe_action_device(obs, None, self.n_candidates, self.threshold)[0]

    def predict(self, observations, deterministic: bool = True):
        return self.base.get_safe_action(observations, None, self.n_candidates, self.threshold)[0]


class ShieldedMLPPolicy:
    """MLPPolicy.shielded(): predict / predict_device give predict_with_safety's actions.  When actor and critic
    have the reference shape (hidden 256), evaluate_with_safety runs it fused into the env kernel
    (BatchedIndustrialEnv.rollout_mlp_safe), and so it does when both have the widths of one shaped class (`shape_shield_exact`:
    set_mlp_policy_dims + set_mlp_safety_dims, "nig-mlp-shape-shield-v1"); otherwise through torch GEMMs."""
    is_trained = True

    def __init__(self, base: MLPPolicy, threshold: float):
        self.base = base
        self.threshold = float(threshold)
        self.state_dim, self.action_dim = base.state_dim, base.action_dim
        self.weights, self.safety_weights = base.weights, base.safety_weights
        self.safety_kind, self.below_mask = base.safety_kind, base.below_mask
        sw = base.safety_weights
        self.fusable = base.fusable and len(sw) == 3 and sw[0][0].shape[1] == 256 and sw[1][0].shape == (256, 256)
        # actor and critic of the same shaped class, unpadded: the fused shaped shield ("nig-mlp-shape-shield-v1")
        self.shape_shield_exact = type(base) is MLPPolicy and bool(getattr(base, "shape_shield_exact", False))

    def predict_device(self, obs):
        return self.base.predict_with_safety_device(obs, self.threshold)[0]

    def predict(self, observations, deterministic: bool = True):
        return self.base.predict_with_safety(observations, self.threshold)[0]


class SafetyEnsemblePolicy:
    """The reference's SafeEnsembleAgent.get_safe_action (agents/safety_critical.py:391-532) over an actor and K safety
    predictors with one head column per constraint, kept on the GPU: the actor's action is accepted where every constraint's
    violation probability p = clip(sigmoid(mean / T) + 0.5 min(sd, 1), 0, 1) is below `threshold` and every spread sd of the
    members' logits below `max_uncertainty`; the zero action is commanded elsewhere.  The arithmetic is the law "nig-gate-v1"
    of include/nig.h in torch (float32, the shifted variance about member 0, the clamp that keeps a NaN).

    `actor`: an MLPPolicy or a weight list; `members`: weight lists [(C1 [S+A,h], c1), (C2 [h,h], c2), (C3 [h,C], c3)] with the
    same C in 1 .. 4.  When the actor has the reference shape and every member three layers of hidden width <= 256 (padded to 256
    by pad_safety_member: the reference's members are 128 wide) and there are at most 8 members (`fusable`),
    evaluate_with_safety / evaluate_episodes run the gate fused into the env kernel (BatchedIndustrialEnv.rollout_mlp_gated);
    otherwise through torch GEMMs."""
    is_trained = True

    def __init__(self, actor, members, temperature: float = 1.0, threshold: float = 0.1, max_uncertainty: float = 0.2, device="cuda:0"):
        import torch
        self.actor = actor if hasattr(actor, "predict_device") else MLPPolicy(actor, device=device)
        self.device = torch.device(getattr(self.actor, "device", device))
        self.state_dim, self.action_dim = self.actor.state_dim, self.actor.action_dim
        self.weights = self.actor.weights
        self.members = [[(np.asarray(W, dtype=f32).reshape(np.shape(W)[0], -1), np.asarray(b, dtype=f32).reshape(-1)) for W, b in m]
                        for m in members]
        if not self.members:
            raise RuntimeError("No members in the safety ensemble")
        self.n_outputs = self.members[0][-1][0].shape[1]
        for m in self.members:
            if m[0][0].shape[0] != self.state_dim + self.action_dim or m[-1][0].shape[1] != self.n_outputs or m[-1][1].shape != (self.n_outputs,):
                raise ValueError(f"safety-ensemble members must map S+A={self.state_dim + self.action_dim} inputs to the same number of "
                                 f"constraints, got {[w.shape for w, _ in m]}")
        self.temperature, self.threshold, self.max_uncertainty = float(temperature), float(threshold), float(max_uncertainty)
        if not (np.isfinite(self.temperature) and self.temperature > 0):
            raise ValueError(f"temperature must be finite and > 0, got {temperature}")
        if np.isnan(self.threshold) or np.isnan(self.max_uncertainty):
            raise ValueError("a NaN threshold")
        self.member_layers = [[(torch.as_tensor(W, device=self.device).contiguous(), torch.as_tensor(b, device=self.device).contiguous())
                               for W, b in m] for m in self.members]

        def paddable(m):
            h = m[0][0].shape[1]
            return len(m) == 3 and h <= 256 and m[1][0].shape == (h, h) and m[2][0].shape[0] == h
        self.fusable = (bool(getattr(self.actor, "fusable", False)) and len(self.members) <= _lib.MAX_ENSEMBLE
                        and 1 <= self.n_outputs <= 4 and all(paddable(m) for m in self.members))

    @classmethod
    def from_agent(cls, actor_agent, safe_agent, device="cuda:0", max_uncertainty: float = 0.2):
        """From a reference agent with an actor (MLPPolicy.from_agent) and a SafeEnsembleAgent: the members
        safe_agent.ensemble_states[i].params = {"params": {"layers_0", "layers_1", "safety_head"}} in list order,
        safe_agent.temperature, and safe_agent.uncertainty_threshold as the probability limit (safety_critical.py:512; the
        spread limit is the reference's constant 0.2)."""
        members = [_named_layers(st.params, ("layers_0", "layers_1", "safety_head"), "safety ensemble member") for st in safe_agent.ensemble_states]
        return cls(MLPPolicy.from_agent(actor_agent, device=device), members, temperature=getattr(safe_agent, "temperature", 1.0),
                   threshold=safe_agent.uncertainty_threshold, max_uncertainty=max_uncertainty, device=device)

    def install(self, env):
        """Install actor and members on a BatchedIndustrialEnv for rollout_mlp_gated()."""
        env.set_mlp_policy(self.weights)
        env.set_mlp_safety_ensemble([pad_safety_member(m) for m in self.members], self.temperature, self.threshold, self.max_uncertainty)

    # ---- device (torch) forms of the law ----
    def member_logits_device(self, obs, actions):
        """z [K, n, C]: every member's head on [obs, actions]."""
        import torch
        x0 = torch.cat([obs, actions], dim=1)
        out = []
        for layers in self.member_layers:
            x = x0
            for i, (W, b) in enumerate(layers):
                x = torch.addmm(b, x, W)
                if i + 1 < len(layers):
                    x = torch.relu(x)
            out.append(x)
        return torch.stack(out)

    def _law_device(self, z):
        """(p [n, C], sd [n, C]) of the members' logits z [K, n, C]: "nig-gate-v1"."""
        import torch
        K = z.shape[0]
        kf = torch.tensor(K, dtype=torch.float32, device=z.device)
        acc, s1, s2 = z[0], torch.zeros_like(z[0]), torch.zeros_like(z[0])
        for m in range(1, K):
            acc = acc + z[m]
            d = z[m] - z[0]
            s1 = s1 + d
            s2 = s2 + d * d
        v = s2 - (s1 * s1) / kf
        v = torch.where(v < 0, torch.zeros_like(v), v)              # (a NaN stays a NaN)
        sd = torch.sqrt(v / kf)
        pen = torch.where(sd > 1, torch.ones_like(sd), sd)
        p = torch.sigmoid((acc / kf) / self.temperature) + 0.5 * pen
        p = torch.where(p < 0, torch.zeros_like(p), torch.where(p > 1, torch.ones_like(p), p))
        return p, sd

    def violation_probs_device(self, obs, actions):
        """compute_safety_violation_probability on device tensors: (p [n, C], sd [n, C])."""
        return self._law_device(self.member_logits_device(obs, actions))

    def get_safe_action_device(self, obs, preferred=None):
        """get_safe_action on device tensors, a batch of states at once: (actions [n, A], {"violation_prob" [n, C],
        "uncertainty" [n, C], "accept" [n] bool, "certain" [n] bool})."""
        import torch
        a = self.actor.predict_device(obs) if preferred is None else preferred
        p, sd = self.violation_probs_device(obs, a)
        safe, certain = (p < self.threshold).all(dim=1), (sd < self.max_uncertainty).all(dim=1)
        accept = safe & certain
        return torch.where(accept[:, None], a, torch.zeros_like(a)), {"violation_prob": p, "uncertainty": sd, "accept": accept, "certain": certain}

    def predict_device(self, obs):
        return self.get_safe_action_device(obs)[0]

    # ---- host forms (the reference's contract) ----
    def _host(self, x, width):
        import torch
        t = torch.as_tensor(np.asarray(x, dtype=f32), device=self.device)
        return t.reshape(-1, width), t.dim() == 1

    def violation_probs(self, observations, actions):
        """(violation_prob, uncertainty) as NumPy arrays, [C] for a single observation."""
        o, single = self._host(observations, self.state_dim)
        p, sd = self.violation_probs_device(o, self._host(actions, self.action_dim)[0])
        p, sd = p.cpu().numpy(), sd.cpu().numpy()
        return (p[0], sd[0]) if single else (p, sd)

    def get_safe_action(self, observations, preferred=None):
        """SafeEnsembleAgent.get_safe_action on host arrays, `preferred` defaulting to the actor's action: (action,
        {"violation_prob", "uncertainty", "decision"}), decision "accept" or "reject_conservative" (an array of them for a
        batch of observations, whose rows are decided one by one)."""
        o, single = self._host(observations, self.state_dim)
        pa = None if preferred is None else self._host(preferred, self.action_dim)[0]
        a, info = self.get_safe_action_device(o, pa)
        decision = np.where(info["accept"].cpu().numpy(), "accept", "reject_conservative")
        a, p, sd = a.cpu().numpy(), info["violation_prob"].cpu().numpy(), info["uncertainty"].cpu().numpy()
        if single:
            return a[0], {"violation_prob": p[0], "uncertainty": sd[0], "decision": str(decision[0])}
        return a, {"violation_prob": p, "uncertainty": sd, "decision": decision}

    def predict(self, observations, deterministic: bool = True):
        return self.get_safe_action(observations)[0]


class ConstraintProjectionPolicy:
    """The reference's ConstrainedIQLAgent.get_safe_action (agents/safety_critical.py:240-370) over an actor and a constraint
    predictor f(s, a) with one head column per constraint, kept on the GPU: the actor's action is kept where every
    sigmoid(f_c) is below `threshold`; elsewhere it walks a <- clip(a - step * dG/da, -1, 1), G = sum_c relu(f_c), until every
    logit is below `tolerance` or `max_iters` steps are taken (the reference: 10 steps of 0.1).  The arithmetic is the law
    "nig-project-v1" of include/nig.h in torch (float32); the gradient is the analytic backward pass -- the transposed network
    with a select on the forward pass's ReLU masks, derivative 0 at 0 -- not autograd.

    `actor`: an MLPPolicy or a weight list; `predictor`: [(C1 [S+A,h], c1), (C2 [h,h], c2), (C3 [h,C], c3)], C in 1 .. 4.  When the
    actor has the reference shape and the predictor three layers of hidden width <= 256 (padded to 256 by pad_safety_member:
    the reference's ConstraintPredictor is 128 wide) and max_iters is at most 16 (`fusable`), evaluate_with_safety /
    evaluate_episodes / evaluate_robustness run the projection fused into the env kernel
    (BatchedIndustrialEnv.rollout_mlp_projected); otherwise through torch GEMMs."""
    is_trained = True

    def __init__(self, actor, predictor, threshold: float = 0.1, tolerance: float = 0.01, max_iters: int = 10, step: float = 0.1,
                 device="cuda:0"):
        import torch
        self.actor = actor if hasattr(actor, "predict_device") else MLPPolicy(actor, device=device)
        self.device = torch.device(getattr(self.actor, "device", device))
        self.state_dim, self.action_dim = self.actor.state_dim, self.actor.action_dim
        self.weights = self.actor.weights
        self.predictor = [(np.asarray(W, dtype=f32).reshape(np.shape(W)[0], -1), np.asarray(b, dtype=f32).reshape(-1)) for W, b in predictor]
        self.n_outputs = self.predictor[-1][0].shape[1]
        if self.predictor[0][0].shape[0] != self.state_dim + self.action_dim or self.predictor[-1][1].shape != (self.n_outputs,):
            raise ValueError(f"the constraint predictor must map S+A={self.state_dim + self.action_dim} inputs to its constraints, got "
                             f"{[w.shape for w, _ in self.predictor]}")
        self.threshold, self.tolerance, self.max_iters, self.step = float(threshold), float(tolerance), int(max_iters), float(step)
        if not (np.isfinite(self.threshold) and np.isfinite(self.tolerance) and np.isfinite(self.step)):
            raise ValueError("threshold, tolerance and step must be finite")
        if self.max_iters < 1:
            raise ValueError(f"max_iters must be at least 1, got {max_iters}")
        self.predictor_layers = [(torch.as_tensor(W, device=self.device).contiguous(), torch.as_tensor(b, device=self.device).contiguous())
                                 for W, b in self.predictor]
        p = self.predictor
        h = p[0][0].shape[1]
        self.fusable = (bool(getattr(self.actor, "fusable", False)) and len(p) == 3 and h <= 256 and p[1][0].shape == (h, h)
                        and p[2][0].shape[0] == h and 1 <= self.n_outputs <= 4 and self.max_iters <= _lib.MAX_PROJECT_ITERS)

    @classmethod
    def from_agent(cls, actor_agent, ciql_agent, device="cuda:0", max_iters: int = 10, step: float = 0.1):
        """From a reference agent with an actor (MLPPolicy.from_agent) and a ConstrainedIQLAgent: the predictor
        ciql_agent.constraint_state.params = {"params": {"layers_0", "layers_1", "constraint_head"}},
        ciql_agent.uncertainty_threshold as the acceptance threshold and ciql_agent.constraint_tolerance as the tolerance
        (safety_critical.py:330, 352; the step count and size are the reference's constants 10 and 0.1)."""
        predictor = _named_layers(ciql_agent.constraint_state.params, ("layers_0", "layers_1", "constraint_head"), "constraint predictor")
        return cls(MLPPolicy.from_agent(actor_agent, device=device), predictor, threshold=ciql_agent.uncertainty_threshold,
                   tolerance=ciql_agent.constraint_tolerance, max_iters=max_iters, step=step, device=device)

    def install(self, env):
        """Install actor and predictor on a BatchedIndustrialEnv for rollout_mlp_projected(n, self.max_iters, self.step)."""
        env.set_mlp_policy(self.weights)
        env.set_mlp_constraint(pad_safety_member(self.predictor), self.threshold, self.tolerance)

    # ---- device (torch) forms of the law ----
    def _forward_device(self, obs, actions):
        """(z [n, C], m1 [n, h], m2 [n, h]): the predictor's logits and the masks z > 0 of its two hidden layers."""
        import torch
        (W1, b1), (W2, b2), (W3, b3) = self.predictor_layers
        y1 = torch.addmm(b1, torch.cat([obs, actions], dim=1), W1)
        y2 = torch.addmm(b2, torch.relu(y1), W2)
        return torch.addmm(b3, torch.relu(y2), W3), y1 > 0, y2 > 0

    def _gradient_device(self, z, m1, m2):
        """dG/da [n, A], G = sum_c relu(f_c): W1[S:S+A, :] (m1 . (W2 (m2 . (W3 d)))), d_c = (z_c > 0)."""
        import torch
        (W1, _), (W2, _), (W3, _) = self.predictor_layers
        zero = torch.zeros((), dtype=z.dtype, device=z.device)
        d = torch.where(z > 0, torch.ones_like(z), torch.zeros_like(z))
        g2 = torch.where(m2, d @ W3.t(), zero)
        g1 = torch.where(m1, g2 @ W2.t(), zero)
        return g1 @ W1[self.state_dim:].t()

    def violation_probs_device(self, obs, actions):
        """sigmoid(f(obs, actions)) [n, C]."""
        import torch
        return torch.sigmoid(self._forward_device(obs, actions)[0])

    def get_safe_action_device(self, obs, preferred=None):
        """get_safe_action on device tensors, a batch of states at once: (actions [n, A], {"violations" [n, C]: sigmoid(f) of
        the returned action, "projected" [n] bool, "iterations" [n] int32: gradient steps taken, -1 where the action was kept})."""
        import torch
        a = (self.actor.predict_device(obs) if preferred is None else preferred).clone()
        z, m1, m2 = self._forward_device(obs, a)
        projected = ~(torch.sigmoid(z) < self.threshold).all(dim=1)
        active = projected.clone()
        iters = torch.where(projected, 0, -1).to(torch.int32)
        one = torch.ones((), dtype=a.dtype, device=a.device)
        for _ in range(self.max_iters):
            active = active & ~(z < self.tolerance).all(dim=1)          # (the raw logits, as the reference; false on NaN)
            if not bool(active.any()):
                break
            v = a - self.step * self._gradient_device(z, m1, m2)
            v = torch.where(v < -1, -one, torch.where(v > 1, one, v))   # (the select form: a NaN stays a NaN)
            a = torch.where(active[:, None], v, a)
            iters = iters + active.to(torch.int32)
            z2, n1, n2 = self._forward_device(obs, a)
            z, m1, m2 = torch.where(active[:, None], z2, z), torch.where(active[:, None], n1, m1), torch.where(active[:, None], n2, m2)
        return a, {"violations": torch.sigmoid(z), "projected": projected, "iterations": iters}

    def predict_device(self, obs):
        return self.get_safe_action_device(obs)[0]

    # ---- host forms (the reference's contract) ----
    def _host(self, x, width):
        import torch
        t = torch.as_tensor(np.asarray(x, dtype=f32), device=self.device)
        return t.reshape(-1, width), t.dim() == 1

    def violation_probs(self, observations, actions):
        """sigmoid(f) as a NumPy array, [C] for a single observation."""
        o, single = self._host(observations, self.state_dim)
        p = self.violation_probs_device(o, self._host(actions, self.action_dim)[0]).cpu().numpy()
        return p[0] if single else p

    def get_safe_action(self, observations, preferred=None):
        """ConstrainedIQLAgent.get_safe_action on host arrays, `preferred` defaulting to the actor's action: (action,
        {"violations", "projected", "iterations"}) -- the reference's dict plus the step count (arrays for a batch of
        observations, whose rows are decided one by one)."""
        o, single = self._host(observations, self.state_dim)
        pa = None if preferred is None else self._host(preferred, self.action_dim)[0]
        a, info = self.get_safe_action_device(o, pa)
        a, info = a.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}
        if single:
            return a[0], {"violations": info["violations"][0], "projected": bool(info["projected"][0]), "iterations": int(info["iterations"][0])}
        return a, info

    def predict(self, observations, deterministic: bool = True):
        return self.get_safe_action(observations)[0]


def ensemble_active_weights(weights, n_members: int, method: str):
    """The weights np.average receives in agents/ensemble.py:236-249 and their NumPy sum: the FIRST n_members entries of the
    agent's weight vector (whichever members were trained), divided by their sum for "mean", as they are for "weighted"."""
    aw = np.asarray(weights, dtype=np.float64)[:n_members]
    if aw.shape != (n_members,):
        raise ValueError(f"{n_members} active members need at least as many weights, got {np.shape(weights)}")
    if method == "mean":
        aw = aw / np.sum(aw)
    return aw, np.sum(aw)


def ensemble_action(preds, weights, method: str):
    """EnsembleAgent._predict_impl's combination of the members' float32 actions preds [K, ..., A], in the order the library
    documents (include/nig.h, nig_set_mlp_ensemble) -- bit for bit np.average / np.mean of the reference:
    "mean" / "weighted": float64 ((double)p_0 w_0 + (double)p_1 w_1 + ...) / np.sum(w); "voting": float32 (p_0 + p_1 + ...) / K."""
    preds = np.asarray(preds, dtype=f32)
    K = preds.shape[0]
    if method == "voting":
        acc = preds[0]
        for k in range(1, K):
            acc = acc + preds[k]
        return acc / f32(K)
    if method not in ("mean", "weighted"):
        raise ValueError(f"Unknown ensemble method: {method}")
    aw, wsum = ensemble_active_weights(weights, K, method)
    acc = preds[0].astype(np.float64) * aw[0]
    for k in range(1, K):
        acc = acc + preds[k].astype(np.float64) * aw[k]
    return acc / wsum


def ensemble_uncertainty(preds):
    """np.std over the members, mean over the action dimensions (ensemble.py:304-310), float32, in the library's documented
    order: per dimension about member 0, d_k = p_k - p_0, s1 = sum d_k, s2 = sum d_k^2 (k = 1 .. K-1 in order),
    v = max(s2 - s1^2 / K, 0), sd = sqrt(v / K); then ((sd_0 + sd_1) + ...) / A.  Exactly 0 for identical members and K = 1."""
    preds = np.asarray(preds, dtype=f32)
    K, A = preds.shape[0], preds.shape[-1]
    kf = f32(K)
    s1 = np.zeros(preds.shape[1:], dtype=f32)
    s2 = np.zeros(preds.shape[1:], dtype=f32)
    for k in range(1, K):
        d = preds[k] - preds[0]
        s1 = s1 + d
        s2 = s2 + d * d
    v = s2 - (s1 * s1) / kf
    v = np.where(v > 0, v, f32(0.0)).astype(f32)
    sd = np.sqrt(v / kf)
    usum = np.zeros(preds.shape[1:-1], dtype=f32)
    for j in range(A):
        usum = usum + sd[..., j]
    return usum / f32(A)


class EnsemblePolicy:
    """The reference's EnsembleAgent (agents/ensemble.py) over K MLPPolicy members, kept on the GPU: predict is the weighted
    average ("mean", "weighted": float64, as np.average returns it) or the plain mean ("voting": float32) of the members'
    actions; predict_with_uncertainty / get_high_uncertainty_mask / evaluate_diversity report how much the members disagree.
    The arithmetic is the one include/nig.h documents for nig_set_mlp_ensemble (ensemble_action, ensemble_uncertainty above).

    `members`: MLPPolicy objects or weight lists, in the agent's list order; `weights`: the agent's weight vector -- its FIRST
    len(members) entries are the active ones (ensemble.py:238), default 1 / K each.  When every member has the reference shape
    (`fusable`), evaluate_with_safety runs the ensemble fused into the env kernel (BatchedIndustrialEnv.rollout_mlp_ensemble)."""
    is_trained = True

    def __init__(self, members, weights=None, method: str = "mean", uncertainty_threshold: float = 0.2, device="cuda:0"):
        if method not in ("mean", "weighted", "voting"):
            raise ValueError(f"Unknown ensemble method: {method}")
        # (a member is an MLPPolicy, a weight list, or any object with MLPPolicy's predict / state_dim / action_dim surface)
        self.members = [m if hasattr(m, "predict") else MLPPolicy(m, device=device) for m in members]
        if not self.members:
            raise RuntimeError("No trained agents in ensemble")
        K = len(self.members)
        self.device = getattr(self.members[0], "device", device)
        self.state_dim, self.action_dim = self.members[0].state_dim, self.members[0].action_dim
        if any((m.state_dim, m.action_dim) != (self.state_dim, self.action_dim) for m in self.members):
            raise ValueError("ensemble members must share the state and action dimensions")
        self.weights = np.ones(K) / K if weights is None else np.asarray(weights, dtype=np.float64)
        if self.weights.ndim != 1 or self.weights.shape[0] < K:
            raise ValueError(f"{K} members need at least {K} weights, got shape {self.weights.shape}")
        self.ensemble_method = method
        self.uncertainty_threshold = uncertainty_threshold
        self.fusable = all(getattr(m, "fusable", False) for m in self.members) and K <= 8          # NIG_MAX_ENSEMBLE

    @classmethod
    def from_agent(cls, agent, device="cuda:0"):
        """From a reference EnsembleAgent: the trained members of agent.agents in list order (MLPPolicy.from_agent each; a
        LayerNorm member is refused), agent.weights, agent.ensemble_method, agent.uncertainty_threshold."""
        trained = [a for a in agent.agents if getattr(a, "is_trained", False)]
        if not trained:
            raise RuntimeError("No trained agents in ensemble")
        return cls([MLPPolicy.from_agent(a, device=device) for a in trained], weights=np.asarray(agent.weights, dtype=np.float64),
                   method=agent.ensemble_method, uncertainty_threshold=agent.uncertainty_threshold, device=device)

    def install(self, env):
        """Install the ensemble on a BatchedIndustrialEnv for rollout_mlp_ensemble()."""
        K = len(self.members)
        if self.ensemble_method == "voting":
            aw = wsum = None
        else:
            aw, wsum = ensemble_active_weights(self.weights, K, self.ensemble_method)
        env.set_mlp_ensemble([m.weights for m in self.members], aw, wsum, self.ensemble_method, self.uncertainty_threshold)

    # ---- device (torch) forms of the same law ----
    def member_actions_device(self, obs):
        import torch
        return torch.stack([m.predict_device(obs) for m in self.members])

    def _action_device(self, preds, method):
        import torch
        K = preds.shape[0]
        if method == "voting":
            acc = preds[0]
            for k in range(1, K):
                acc = acc + preds[k]
            return acc / torch.tensor(K, dtype=torch.float32, device=preds.device)
        aw, wsum = ensemble_active_weights(self.weights, K, method)
        acc = preds[0].double() * float(aw[0])
        for k in range(1, K):
            acc = acc + preds[k].double() * float(aw[k])
        return acc / float(wsum)

    @staticmethod
    def _uncertainty_device(preds):
        import torch
        K, A = preds.shape[0], preds.shape[-1]
        kf = torch.tensor(K, dtype=torch.float32, device=preds.device)
        s1 = torch.zeros_like(preds[0])
        s2 = torch.zeros_like(preds[0])
        for k in range(1, K):
            d = preds[k] - preds[0]
            s1 = s1 + d
            s2 = s2 + d * d
        v = s2 - (s1 * s1) / kf
        v = torch.where(v > 0, v, torch.zeros_like(v))
        sd = torch.sqrt(v / kf)
        usum = torch.zeros_like(sd[..., 0])
        for j in range(A):
            usum = usum + sd[..., j]
        return usum / torch.tensor(A, dtype=torch.float32, device=preds.device)

    def predict_device(self, obs):
        return self._action_device(self.member_actions_device(obs), self.ensemble_method)

    def predict_with_uncertainty_device(self, obs):
        """(actions, uncertainties) on device tensors; the action is the "mean" law whatever the method (ensemble.py:298-302)."""
        import torch
        preds = self.member_actions_device(obs)
        if preds.shape[0] < 2:
            return preds[0], torch.zeros(preds.shape[1], dtype=torch.float32, device=preds.device)
        return self._action_device(preds, "mean"), self._uncertainty_device(preds)

    # ---- host forms (agent.predict contract) ----
    def _member_actions(self, observations):
        return np.array([m.predict(observations) for m in self.members])

    def predict(self, observations, deterministic: bool = True):
        return ensemble_action(self._member_actions(observations), self.weights, self.ensemble_method)

    def predict_with_uncertainty(self, observations, return_individual: bool = False):
        preds = self._member_actions(observations)
        if preds.shape[0] < 2:                     # ensemble.py:288-292: the single member's own action, uncertainty 0
            action = preds[0]
            unc = np.zeros(action.shape[0]) if action.ndim > 1 else 0.0
            return (action, unc, [action]) if return_individual else (action, unc)
        action, unc = ensemble_action(preds, self.weights, "mean"), ensemble_uncertainty(preds)
        return (action, unc, preds) if return_individual else (action, unc)

    def get_high_uncertainty_mask(self, observations, threshold=None):
        _, unc = self.predict_with_uncertainty(observations)
        return unc > (threshold or self.uncertainty_threshold)

    def evaluate_diversity(self, observations):
        preds = self._member_actions(observations)
        K = preds.shape[0]
        if K < 2:
            return {"diversity_score": 0.0, "disagreement": 0.0}
        dist = [np.mean(np.abs(preds[i] - preds[j])) for i in range(K) for j in range(i + 1, K)]
        unc = ensemble_uncertainty(preds.reshape(K, -1, preds.shape[-1]))
        return {"diversity_score": float(np.mean(dist)), "disagreement": float(np.mean(unc)), "n_agents": K}


def _named_layers(tree, names, what):
    """[(kernel, bias), ...] of the modules `names` of a Flax parameter tree (any nested mapping), found under any chain of
    single-child mappings (the tree's "params")."""
    t = tree
    while hasattr(t, "items") and not all(n in t.keys() for n in names):
        subs = [v for v in t.values() if hasattr(v, "items")]
        if len(subs) != 1:
            raise ValueError(f"{what}: cannot find the layers {list(names)} of the parameter tree (keys {list(t.keys())})")
        t = subs[0]
    if not hasattr(t, "items"):
        raise ValueError(f"{what}: cannot find the layers {list(names)} of the parameter tree")
    return [(np.asarray(t[n]["kernel"], dtype=f32), np.asarray(t[n]["bias"], dtype=f32)) for n in names]


def _dense_layers(tree, what):
    """[(kernel, bias), ...] of Dense_0, Dense_1, ... of a Flax parameter tree (any nested mapping)."""
    def walk(t, path):
        for k, v in t.items():
            if str(k).startswith("LayerNorm"):
                raise ValueError(f"{what}: LayerNorm networks are not supported ({'/'.join(path + [str(k)])})")
            if hasattr(v, "items"):
                walk(v, path + [str(k)])
    walk(tree, [])
    t = tree
    while hasattr(t, "items") and not any(str(k).startswith("Dense_") for k in t.keys()):
        subs = [v for v in t.values() if hasattr(v, "items")]
        if len(subs) != 1:
            raise ValueError(f"{what}: cannot find the Dense layers of the parameter tree (keys {list(t.keys())})")
        t = subs[0]
    dense = sorted((k for k in t.keys() if str(k).startswith("Dense_")), key=lambda k: int(str(k)[6:]))
    return [(np.asarray(t[k]["kernel"], dtype=f32), np.asarray(t[k]["bias"], dtype=f32)) for k in dense]
