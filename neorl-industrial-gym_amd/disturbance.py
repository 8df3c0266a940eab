"""Sensor / actuator noise around an agent ("nig-disturb-v1", include/nig.h) and the robustness evaluation built on it.

  * Disturbance: the noise model -- per-dimension Gaussian sigmas on the observation the policy sees and on the action the
    plant receives, a clip of the noisy action, and whether the draws are fresh every step or held for an episode;
  * Disturbed(agent, disturbance): the agent under that model.  evaluate_with_safety runs it fused into the env kernel
    (BatchedIndustrialEnv.rollout_policy_disturbed / rollout_mlp_disturbed) when the inner agent is a DevicePolicy or a fusable
    unshielded MLPPolicy; everything else takes the host loop with the wrapper's own NumPy / torch draws;
  * evaluate_robustness: the reference's RobustnessBenchmark (benchmarks/industrial_benchmarks.py:455-573) on batched lanes.
"""
from typing import Any, Dict, Optional, Sequence

import numpy as np

from . import _lib

f32 = np.float32
_HOLDS = {"step": _lib.HOLD_STEP, "episode": _lib.HOLD_EPISODE}


def _sigma(x, what):
    a = np.asarray(x, dtype=f32)
    if a.ndim > 1:
        raise ValueError(f"{what} is a scalar or one value per dimension, got shape {a.shape}")
    if not np.all(np.isfinite(a)) or np.any(a < 0):
        raise ValueError(f"{what} must be finite and >= 0")
    return a


class Disturbance:
    """obs_noise / action_noise: standard deviations, a scalar (every dimension) or one value per dimension; clip = (lo, hi)
    of the noisy action, None = no clip; hold = "step" (fresh draws every step) or "episode" (one draw vector per episode,
    reused on each of its steps: what the reference's benchmark does).  Validated as nig_set_disturbance validates."""

    def __init__(self, obs_noise=0.0, action_noise=0.0, clip=None, hold: str = "step"):
        self.obs_noise, self.action_noise = _sigma(obs_noise, "obs_noise"), _sigma(action_noise, "action_noise")
        lo, hi = (-np.inf, np.inf) if clip is None else clip
        self.clip = (f32(lo), f32(hi))
        if not self.clip[0] <= self.clip[1]:
            raise ValueError(f"clip needs lo <= hi (no NaN), got {clip}")
        if hold not in _HOLDS:
            raise ValueError(f"hold is 'step' or 'episode', not {hold!r}")
        self.hold = hold

    @staticmethod
    def _spread(a, n, what):
        if a.ndim == 0:
            return np.full(n, a, dtype=f32)
        if a.shape != (n,):
            raise ValueError(f"{what} has {a.shape[0]} values, the env has {n} dimensions")
        return a

    def sigmas(self, state_dim: int, action_dim: int):
        """(sigma_obs [S], sigma_act [A]) float32, scalars broadcast."""
        return self._spread(self.obs_noise, state_dim, "obs_noise"), self._spread(self.action_noise, action_dim, "action_noise")

    def to_struct(self, state_dim: int, action_dim: int) -> _lib.DisturbanceStruct:
        if state_dim > 32 or action_dim > 10:
            raise ValueError("at most 32 state and 10 action dimensions (NIG_MAX_STATE_DIM / NIG_MAX_ACTION_DIM)")
        so, sa = self.sigmas(state_dim, action_dim)
        D = _lib.DisturbanceStruct()
        for k in range(state_dim):
            D.sigma_obs[k] = float(so[k])
        for j in range(action_dim):
            D.sigma_act[j] = float(sa[j])
        D.clip_lo, D.clip_hi, D.hold = float(self.clip[0]), float(self.clip[1]), _HOLDS[self.hold]
        return D

    def scaled(self, level: float) -> "Disturbance":
        """The same model with every sigma multiplied by `level`."""
        return Disturbance(self.obs_noise * f32(level), self.action_noise * f32(level), self.clip, self.hold)


class Disturbed:
    """`agent` under `disturbance`: predict(obs) = clip(agent.predict(obs + sigma_obs * zo) + sigma_act * za), float32, with
    the "nig-disturb-v1" switches (no observation draw when every sigma_obs is zero, likewise the action).  The host form draws
    from a NumPy generator, predict_device from a torch generator on the observations' device; the fused kernels draw from
    the library's counter-based generator, so the three agree in distribution, not draw for draw.
    hold="episode": the draw vectors are kept from the first call after begin_episode() to the next begin_episode()."""

    def __init__(self, agent, disturbance: Disturbance, seed: Optional[int] = None):
        self.agent, self.disturbance = agent, disturbance
        self._rng = np.random.default_rng(seed)
        self._seed = seed
        self._tgen = None
        self._held = None            # (zo, za) of the running episodes, NumPy or torch

    @property
    def is_trained(self):
        return getattr(self.agent, "is_trained", False)

    @property
    def state_dim(self):
        return self.agent.state_dim

    @property
    def action_dim(self):
        return self.agent.action_dim

    def begin_episode(self, n: Optional[int] = None):
        """A new episode starts in every lane (n lanes): held draw vectors are redrawn at the next predict."""
        self._held = None

    def _draws(self, shape_o, shape_a, normal):
        d = self.disturbance
        any_o, any_a = bool(np.any(d.obs_noise != 0)), bool(np.any(d.action_noise != 0))
        if d.hold == "episode" and self._held is not None and tuple(self._held[2]) == (tuple(shape_o), tuple(shape_a)):
            return self._held[0], self._held[1]
        zo = normal(shape_o) if any_o else None
        za = normal(shape_a) if any_a else None
        if d.hold == "episode":
            self._held = (zo, za, (tuple(shape_o), tuple(shape_a)))
        return zo, za

    def predict(self, observations, deterministic: bool = True):
        d = self.disturbance
        obs = np.asarray(observations, dtype=f32)
        a_shape = obs.shape[:-1] + (self.action_dim,)
        zo, za = self._draws(obs.shape, a_shape, lambda s: self._rng.standard_normal(s, dtype=f32))
        o = obs if zo is None else (obs + d.obs_noise * zo).astype(f32)
        u = np.asarray(self.agent.predict(o, deterministic=True), dtype=f32)
        if za is not None:
            u = (u + d.action_noise * za).astype(f32)
        return np.minimum(np.maximum(u, d.clip[0]), d.clip[1])

    def predict_device(self, obs):
        import torch
        d = self.disturbance
        if self._tgen is None or self._tgen.device != obs.device:
            self._tgen = torch.Generator(device=obs.device)
            self._tgen.manual_seed(int(self._rng.integers(2 ** 62)) if self._seed is None else int(self._seed))
        a_shape = tuple(obs.shape[:-1]) + (self.action_dim,)
        zo, za = self._draws(tuple(obs.shape), a_shape,
                             lambda s: torch.randn(s, dtype=torch.float32, device=obs.device, generator=self._tgen))
        o = obs if zo is None else obs + torch.as_tensor(d.obs_noise, device=obs.device) * zo
        if hasattr(self.agent, "predict_device"):
            u = self.agent.predict_device(o)
        else:
            u = torch.as_tensor(np.asarray(self.agent.predict(o.contiguous().cpu().numpy(), deterministic=True), dtype=f32),
                                device=obs.device)
        u = u.to(torch.float32)
        if za is not None:
            u = u + torch.as_tensor(d.action_noise, device=obs.device) * za
        return torch.clamp(u, min=float(d.clip[0]), max=float(d.clip[1]))


def robustness_scores(results: Dict[str, Dict[float, Dict[str, Any]]], noise_levels: Sequence[float],
                      disturbance_types: Sequence[str]):
    """The reference's score arithmetic (industrial_benchmarks.py:535-547) on robustness_results[type][level]["mean_return"]:
    per type the mean over the levels after the first of degraded_mean / baseline_mean (0.0 for a zero baseline), the baseline
    being the FIRST level of the FIRST type; overall = the mean over the types.  Returns (scores, overall)."""
    baseline = results[disturbance_types[0]][noise_levels[0]]["mean_return"]
    scores = {}
    for kind in disturbance_types:
        ratios = [results[kind][lv]["mean_return"] / baseline if baseline != 0 else 0.0 for lv in noise_levels[1:]]
        scores[kind] = float(np.mean(ratios)) if ratios else 0.0
    return scores, float(np.mean(list(scores.values()))) if scores else 0.0


def evaluate_robustness(agent, environment, n_episodes: int = 100, noise_levels=(0.0, 0.1, 0.2, 0.3),
                        disturbance_types=("observation_noise", "action_noise", "dynamics_noise"), hold: str = "episode",
                        batch: Optional[int] = None, seed: int = 0x5EED, device="cuda:0") -> Dict[str, Any]:
    """RobustnessBenchmark.evaluate_agent on batched lanes.  `environment`: an env id, or a BatchedIndustrialEnv whose
    construction arguments (id, batch, device, seed, max_episode_steps, dt) are reused and whose added safety constraints
    (add_safety_constraint) are installed on every cell's handle.  Every (type, level) cell plays
    n_episodes // len(noise_levels) episodes on a FRESH handle with the same seed -- tallies start at zero and the cells share
    their random numbers, as upstream's fixed episode keys do.  The level multiplies a unit sigma on every dimension;
    "dynamics_noise" runs undisturbed, as upstream.  safety_violations = the sum of the per-step violation counts
    (evaluate_with_safety's figure), violation_rate = the share of episodes with at least one violation (upstream reads a
    field that does not exist for both).  `path`: "fused-mlp", "fused-policy" or "host" -- how the disturbed cells ran."""
    from .batched import BatchedIndustrialEnv
    from .core import BoxConstraint
    from .utils import _disturbed_route, _evaluate_batched
    if not getattr(agent, "is_trained", False):
        raise RuntimeError("Agent must be trained before evaluation")
    for kind in disturbance_types:
        if kind not in ("observation_noise", "action_noise", "dynamics_noise"):
            raise ValueError(f"unknown disturbance type {kind!r}")
    noise_levels, disturbance_types = list(noise_levels), list(disturbance_types)
    kw: Dict[str, Any] = {}
    added = []                                     # the BoxConstraints added to `environment`: every cell's fresh handle takes them too
    if isinstance(environment, BatchedIndustrialEnv):
        added = [c for c in environment.safety_constraints if isinstance(c, BoxConstraint)]
        env_id, device, seed = environment.env_id, environment.device, environment.seed
        batch = batch or environment.batch
        kw = dict(max_episode_steps=environment.max_episode_steps, dt=environment.dt, env_index0=environment.env_index0)
    else:
        env_id = environment
    per_cell = int(n_episodes) // len(noise_levels)
    if per_cell < 1:
        raise ValueError("n_episodes // len(noise_levels) must be at least 1")
    batch = int(batch or min(per_cell, 65536))
    results: Dict[str, Dict[float, Dict[str, Any]]] = {}
    path = None
    for kind in disturbance_types:
        results[kind] = {}
        for level in noise_levels:
            cell_agent = agent
            if kind == "observation_noise":
                cell_agent = Disturbed(agent, Disturbance(obs_noise=level, hold=hold), seed=seed)
            elif kind == "action_noise":
                cell_agent = Disturbed(agent, Disturbance(action_noise=level, hold=hold), seed=seed)
            env = BatchedIndustrialEnv(env_id, batch, device=device, seed=seed, tally=True, autoreset=False, **kw)
            try:
                for c in added:
                    env.add_safety_constraint(c)
                if cell_agent is not agent and path is None:
                    path = _disturbed_route(cell_agent, env)[0]
                with_violation = [0]

                def count(e, k):                   # after a round: the finished lanes' counter words still hold their episode's count
                    with_violation[0] += int((e.violation_count[:k] > 0).sum().item())
                m = _evaluate_batched(cell_agent, env, per_cell, reduce_across_ranks=False, round_hook=count)
            finally:
                env.close()
            results[kind][level] = {"mean_return": float(m["return_mean"]), "std_return": float(m["return_std"]),
                                    "safety_violations": int(m["safety_violations"]),
                                    "violation_rate": with_violation[0] / per_cell}
    scores, overall = robustness_scores(results, noise_levels, disturbance_types)
    return {"robustness_results": results, "robustness_scores": scores, "overall_robustness": overall,
            "noise_levels": noise_levels, "disturbance_types": disturbance_types, "path": path or "host"}
