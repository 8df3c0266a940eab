"""make / make_batched / evaluate_with_safety -- mirror of neorl_industrial/utils.py."""
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import _lib
from .batched import BatchedIndustrialEnv
from .envs import (AdvancedChemicalReactorEnv, AdvancedPowerGridEnv, ChemicalReactorEnv, HVACControlEnv, PowerGridEnv,
                   RobotAssemblyEnv, SteelAnnealingEnv, SupplyChainEnv, WaterTreatmentEnv)
from .parallel import all_reduce_partial, metrics_from_partial

_REGISTRY = {
    "ChemicalReactor-v0": ChemicalReactorEnv,
    "PowerGrid-v0": PowerGridEnv,
    "RobotAssembly-v0": RobotAssemblyEnv,
    "AdvancedChemicalReactor-v0": AdvancedChemicalReactorEnv,     # utils.py:30-31: registered upstream but
    "AdvancedPowerGrid-v0": AdvancedPowerGridEnv,                 # not instantiable there (candidate rows)
    # README.md:28-32 lists these four; upstream ni.make() raises for them (no implementation).  Build-specified.
    "HVACControl-v0": HVACControlEnv,
    "WaterTreatment-v0": WaterTreatmentEnv,
    "SteelAnnealing-v0": SteelAnnealingEnv,
    "SupplyChain-v0": SupplyChainEnv,
}


def make(env_id: str, **kwargs) -> Any:
    """utils.py:12-39.  Unknown ids raise the reference's ValueError text.  The two 'Advanced*'
    ids are registered as upstream; there they raise TypeError on construction (abstract methods
    missing, SURVEY.md finding 2), here they are built from the source text (candidate rows)."""
    if env_id not in _REGISTRY:
        available = ", ".join(_REGISTRY.keys())
        raise ValueError(f"Unknown environment '{env_id}'. Available: {available}")
    return _REGISTRY[env_id](**kwargs)


def make_batched(env_id: str, batch: int, **kwargs) -> BatchedIndustrialEnv:
    """B independent instances of `env_id` on one GPU (no upstream equivalent: the reference
    has no vectorised env)."""
    return BatchedIndustrialEnv(env_id, batch, **kwargs)


def _predict(agent, obs_dev: torch.Tensor) -> torch.Tensor:
    """agent.predict contract (agents/base.py:106-141): float32 [n,S] -> float32 [n,A].
    An agent exposing `predict_device(obs_tensor)` is called without leaving the GPU."""
    if hasattr(agent, "predict_device"):
        return agent.predict_device(obs_dev)
    obs = obs_dev.contiguous().cpu().numpy()
    act = agent.predict(obs, deterministic=True)
    return torch.as_tensor(np.asarray(act, dtype=np.float32))


def _round_is_over(env, t: int, on_device: bool) -> bool:
    """All lanes finished?  Reading the answer synchronises the stream, so a device-resident
    policy is only asked every 16 steps (finished lanes are frozen; extra steps are no-ops)."""
    if on_device and (t % 16) != 0 and t <= env.max_episode_steps:
        return False
    return bool(env.done.all().item())


def evaluate_with_safety(agent: Any, env: Any, n_episodes: int = 100, record_video: bool = False,
                         render: bool = False, step_noise_fn=None, reset_noise_fn=None) -> Dict[str, Any]:
    """utils.py:42-154.  With a single env this is the reference's loop verbatim in behaviour;
    with a BatchedIndustrialEnv (created with tally=True, autoreset=False) the n_episodes
    episodes run in parallel lanes and the 13 aggregates come from the device tallies."""
    if not hasattr(agent, "is_trained") or not agent.is_trained:
        raise RuntimeError("Agent must be trained before evaluation")
    if isinstance(env, BatchedIndustrialEnv):
        return _evaluate_batched(agent, env, n_episodes, step_noise_fn, reset_noise_fn)

    runs = [_play_episode(agent, env, render) for _ in range(n_episodes)]
    return _summarise(runs, n_episodes)


def _play_episode(agent, env, render):
    """One episode of the reference's evaluation loop (utils.py:80-118): returns
    (return, length, sum of violation_count, sum of critical_violations, shutdown steps,
    per-step satisfaction rates).  `ret += reward` keeps the reward's own type, as upstream."""
    obs, _ = env.reset()
    if hasattr(agent, "begin_episode"):
        agent.begin_episode(1)
    ret, length, viol, crit, shut, rates = 0.0, 0, 0, 0, 0, []
    finished = False
    while not finished:
        obs, reward, terminated, truncated, info = env.step(agent.predict(obs[None], deterministic=True)[0])
        finished = terminated or truncated
        ret += reward
        length += 1
        sm = info.get("safety_metrics")
        if sm is not None:
            viol += sm.violation_count
            crit += sm.critical_violations
            rates.append(sm.satisfaction_rate)
        shut += 1 if info.get("critical_shutdown", False) else 0
        if render:
            try:
                env.render()
            except Exception:
                pass
    return ret, length, viol, crit, shut, rates


def _summarise(runs, n_episodes):
    """The 13 aggregates of utils.py:128-152 from per-episode tuples."""
    rets = [r[0] for r in runs]
    lens = [r[1] for r in runs]
    rates = [x for r in runs for x in r[5]]
    viol = sum(r[2] for r in runs)
    wins = sum(1 for x in rets if x > 0)
    return {
        "return_mean": np.mean(rets), "return_std": np.std(rets), "return_min": np.min(rets), "return_max": np.max(rets),
        "length_mean": np.mean(lens), "length_std": np.std(lens),
        "safety_violations": viol, "safety_violations_per_episode": viol / n_episodes,
        "critical_violations": sum(r[3] for r in runs), "emergency_shutdowns": sum(r[4] for r in runs),
        "constraint_satisfaction_rate": np.mean(rates) if rates else 1.0,
        "successful_episodes": wins, "success_rate": wins / n_episodes,
    }


def _disturbed_route(agent, env):
    """How a disturbance.Disturbed agent runs on `env`: ("fused-policy", DevicePolicy), ("fused-mlp", MLPPolicy) -- the inner
    agent goes into the env kernel with the disturbance beside it -- or ("host", None): shielded, ensemble and non-fusable
    agents keep the per-step loop with the wrapper's own draws.  A reference agent MLPPolicy.from_agent can read is upgraded."""
    from .policies import MLPPolicy
    inner = agent.agent
    if hasattr(inner, "to_struct"):
        return "fused-policy", inner
    if not hasattr(inner, "fusable") and hasattr(inner, "state") and not hasattr(inner, "agents"):
        try:
            inner = MLPPolicy.from_agent(inner, device=env.device)
        except Exception:
            return "host", None
    if (isinstance(inner, MLPPolicy) and inner.fusable and env.state_dim % 2 == 0 and env.action_dim <= 16
            and env.state_dim <= 32 and env.action_dim <= 10):
        return "fused-mlp", inner
    return "host", None


# The shape classes whose shielded form _install_agent sends to the fused shaped shield: those whose new kernel is below the host
# route in every round on both timed envs of profiles/shape_shield/ab.txt (written by profiles/bench_shape_shield.py) -- all four, by
# 5.9 x / 4.6 x (128x128) down to 1.49 x / 1.46 x (512x512) on ChemicalReactor / PowerGrid ("The shaped shield").
# A class that a later measurement does not admit is taken out here and keeps the host loop; its C entry point still runs.
SHAPE_SHIELD_ROUTED = ("128x128", "512x256", "512x512", "256x256x256")


def _install_agent(agent, env: BatchedIndustrialEnv, plain: bool = True):
    """Where `agent` runs on `env`, and its installation there -- the routing _evaluate_batched and episodes.evaluate_episodes
    share.  Returns (agent, rollout, disturbed): `rollout` is the env method that plays n closed-loop steps with the agent in the
    env kernel (rollout_policy, rollout_mlp, rollout_mlp_bf16, rollout_mlp_safe, rollout_mlp_search, rollout_mlp_gated, rollout_mlp_projected, rollout_mlp_ensemble or a _disturbed twin; policy, weights,
    shield, ensemble and disturbance are installed on the handle), or None -- the agent stays on the host and takes the
    per-step loop; `agent` may come back upgraded (a reference EnsembleAgent as an EnsemblePolicy); `disturbed` names the
    fused route of a disturbance.Disturbed ("fused-policy" / "fused-mlp": the caller removes the disturbance afterwards).
    plain = no recorded draws are injected (with them every agent takes the host loop).
    On an env with added safety constraints (add_safety_constraint) every route is the same and ends at the `_limited` method of
    its family (rollout_policy_limited, rollout_mlp_limited, rollout_mlp_safe_limited, ..., rollout_mlp_disturbed_limited), whose
    kernels check the constraints on the action the env receives; an MFMA family on an env without the MFMA actor takes the host
    loop there, whose env.step knows the constraints.  Only agents that take the host loop without added constraints take it with them."""
    limited = bool(getattr(env, "has_limits", False))
    mfma_env = env.state_dim % 2 == 0 and env.action_dim <= 16        # the env shapes with the MFMA actor (has_mlp_actor)
    device_policy = hasattr(agent, "to_struct") and plain
    if plain and all(hasattr(agent, k) for k in ("agents", "weights", "ensemble_method")) and not hasattr(agent, "install"):
        # the reference's EnsembleAgent: its K actors fused into the env kernel where members and env allow it (EnsemblePolicy);
        # otherwise the agent stays as it is and takes the host loop below
        from .policies import EnsemblePolicy
        try:
            upgraded = EnsemblePolicy.from_agent(agent, device=env.device)
            if upgraded.fusable and mfma_env:
                agent = upgraded
        except Exception:
            pass
    ensemble = plain and hasattr(agent, "install") and getattr(agent, "fusable", False) and mfma_env
    gated = ensemble and hasattr(agent, "max_uncertainty")        # SafetyEnsemblePolicy: its install() puts actor and members on the handle
    projecting = ensemble and hasattr(agent, "max_iters")         # ConstraintProjectionPolicy: install() puts actor and predictor on the handle
    # Bf16MLPPolicy (MLPPolicy.bf16()): ahead of the fused_mlp test, which its `fusable` would send to the float32 kernel.  The bf16
    # family has no _limited twin: with added constraints, as on an env without the MFMA actor, the agent takes the host loop
    # through its predict_device.
    bf16 = getattr(agent, "precision", None) == "bf16" and not hasattr(agent, "install")
    fused_bf16 = bf16 and getattr(agent, "fusable", False) and plain and mfma_env and not limited
    # LayerNormMLPPolicy ("nig-mlp-ln-v1"): ahead of the fused_mlp test as well.  Only the explicit policy goes to the device -- a raw
    # reference agent with LayerNorm keeps the host loop, as it always has -- and the family has no _limited twin: with added
    # constraints, as on an env without the MFMA actor, it takes the host loop through its predict_device.
    layer_norm = getattr(agent, "normalization", None) == "layer_norm" and not hasattr(agent, "install")
    fused_ln = layer_norm and getattr(agent, "fusable", False) and plain and mfma_env and not limited
    # LayerNormMLPPolicy.shielded() ("nig-mlp-ln-shield-v1"): the same conditions, actor and critic both installed
    ln_shielded = fused_ln and hasattr(agent, "base") and hasattr(agent, "threshold")
    fused_mlp = not bf16 and not layer_norm and not hasattr(agent, "install") and getattr(agent, "fusable", False) and plain and (mfma_env or not limited)
    # The other hidden shapes ("nig-mlp-shape-v1"): a plain MLPPolicy -- unshielded, undisturbed, float32 -- whose hidden widths ARE a
    # shaped class's (128x128, 512x256, 512x512, 256x256x256: with (256, 256) the five hidden_dims the reference's tuner builds) goes to
    # set_mlp_policy_dims + rollout_mlp, and so does a reference agent MLPPolicy.from_agent can read into such a policy.  A network that
    # only fits a class after zero-padding -- (64, 64), (200, 200), (400, 300) -- keeps the host loop here, as it always has
    # (tests/test_limits_families_host.py holds that); it runs fused where the caller installs it with env.set_mlp_policy_dims.
    # The family has no _limited twin: with added constraints the agent takes the host loop, as bf16 does.
    fused_shape = False
    if plain and mfma_env and not limited and not bf16 and not layer_norm:
        from .policies import MLPPolicy
        cand = agent
        if (not hasattr(agent, "fusable") and hasattr(agent, "state") and not any(hasattr(agent, k) for k in ("agents", "install", "to_struct", "disturbance"))):
            try:
                cand = MLPPolicy.from_agent(agent, device=env.device)
            except Exception:
                cand = agent
        if type(cand) is MLPPolicy and not cand.fusable and cand.shape_class_exact:
            agent, fused_shape = cand, True
    # The shaped shield ("nig-mlp-shape-shield-v1"): MLPPolicy.shielded() whose actor AND sigmoid critic have the widths of one shaped
    # class (`shape_shield_exact`: the reference builds the SafetyCritic with the actor's hidden_dims) goes to set_mlp_policy_dims +
    # set_mlp_safety_dims + rollout_mlp_safe, for the classes of SHAPE_SHIELD_ROUTED.  A critic of other widths than the actor's, a
    # pair that needs padding, a categorical critic and a raw reference agent keep the routes they had; the family has no _limited
    # twin: with added constraints the agent takes the host loop.
    shape_shielded = False
    if plain and mfma_env and not limited:
        from .policies import ShieldedMLPPolicy
        shape_shielded = (type(agent) is ShieldedMLPPolicy and bool(getattr(agent, "shape_shield_exact", False))
                          and agent.base.shape_class in SHAPE_SHIELD_ROUTED)
    shielded = fused_mlp and getattr(agent, "safety_weights", None) is not None and hasattr(agent, "threshold")
    searching = shielded and hasattr(agent, "n_candidates")       # MLPPolicy.searching(): get_safe_action instead of the halving
    disturbed = None           # a disturbance.Disturbed whose inner agent runs in the env kernel: "fused-policy" / "fused-mlp"
    if plain and hasattr(agent, "disturbance") and hasattr(agent, "agent"):
        route, inner = _disturbed_route(agent, env)
        if route != "host":
            disturbed = route
            (env.set_policy if route == "fused-policy" else lambda a: env.set_mlp_policy(a.weights))(inner)
            env.set_disturbance(agent.disturbance)
        device_policy = ensemble = gated = projecting = fused_mlp = fused_bf16 = fused_ln = ln_shielded = fused_shape = shape_shielded = shielded = searching = False
    if disturbed:
        device_policy = True
    elif device_policy:
        env.set_policy(agent)
    elif ensemble:
        agent.install(env)
        device_policy = True
    elif fused_bf16:
        env.set_mlp_policy_bf16(agent.weights)
        device_policy = True
    elif fused_ln:
        env.set_mlp_policy_ln(agent.base if ln_shielded else agent)
        if ln_shielded:
            env.set_mlp_safety_ln(agent.base, agent.threshold)
        device_policy = True
    elif fused_shape:
        env.set_mlp_policy_dims(agent.weights)
        device_policy = True
    elif shape_shielded:
        env.set_mlp_policy_dims(agent.weights)
        env.set_mlp_safety_dims(agent.safety_weights, agent.threshold)
        device_policy = True
    elif fused_mlp:
        env.set_mlp_policy(agent.weights)
        if shielded:        # MLPPolicy.shielded() / searching(): actor + safety critic + shield in the same kernel
            from .policies import pad_critic
            if getattr(agent, "safety_kind", "sigmoid") == "categorical":      # the distributional critic ("nig-categorical-v1"): the same
                env.set_mlp_safety_categorical(agent.safety_weights, agent.threshold, agent.below_mask)   # rollouts, p from its softmax
            else:
                env.set_mlp_safety(pad_critic(agent.safety_weights), agent.threshold)
        device_policy = True
    rollout = None
    if device_policy:
        name = ("rollout_policy_disturbed" if disturbed == "fused-policy" else "rollout_mlp_disturbed" if disturbed
                else "rollout_mlp_gated" if gated else "rollout_mlp_projected" if projecting else "rollout_mlp_ensemble" if ensemble
                else "rollout_mlp_bf16" if fused_bf16
                else "rollout_mlp_search" if searching else "rollout_mlp_safe" if shielded or ln_shielded or shape_shielded else "rollout_mlp" if fused_mlp or fused_shape or fused_ln
                else "rollout_policy")
        method = getattr(env, name + "_limited" if limited else name)
        rollout = ((lambda n, *a, **k: method(n, agent.max_iters, agent.step, *a, **k)) if projecting
                   else (lambda n, *a, **k: method(n, agent.n_candidates, *a, **k)) if searching else method)
    return agent, rollout, disturbed


def _evaluate_batched(agent, env: BatchedIndustrialEnv, n_episodes: int, step_noise_fn=None, reset_noise_fn=None,
                      group=None, reduce_across_ranks: bool = True, round_hook=None, episode_log=None, chunk: int = 250,
                      launches=None) -> Dict[str, Any]:
    """Episodes in parallel lanes.  Rounds of up to B episodes: reset the needed lanes, step
    until every one of them is done (finished lanes are frozen by the kernel), tallies
    accumulate on the device; one reduction (+ all-gather across ranks) at the end.

    step_noise_fn(round, t) / reset_noise_fn(round) may supply recorded draws (parity tests).
    round_hook(env, k): called after every round of k episodes (lanes [0, k) hold their finished episodes' counters).
    episode_log (episodes.EpisodeLog): every launch writes its reward / flag rows and the log collects them -- a fused round in
    pieces of `chunk` steps (a rollout cut into several launches equals one launch), the host loop step by step; `launches`
    (a one-element list) counts the env launches then.  Without a log nothing changes."""
    if not env.tally_enabled or env.autoreset:
        raise ValueError("batched evaluation needs make_batched(..., tally=True, autoreset=False)")
    B = env.batch
    remaining, rnd = int(n_episodes), 0
    plain = step_noise_fn is None and reset_noise_fn is None
    agent, rollout, disturbed = _install_agent(agent, env, plain)
    if episode_log is not None:
        P = max(1, int(chunk))
        rew = torch.empty(P, env.ld, dtype=torch.float32, device=env.device)
        fl = torch.empty(P, env.ld, dtype=torch.int32, device=env.device)
    while remaining > 0 and rollout is not None:
        # the agent runs ON the device: one fused launch plays every episode of the round to its end
        k = min(B, remaining)
        mask = torch.zeros(B, dtype=torch.uint8, device=env.device)
        mask[:k] = 1
        env.ctr.fill_(_lib.CTR_DONE)
        env.reset(mask=mask)
        # the Advanced envs truncate on the step AFTER the cap (advanced_chemical_reactor.py:351 and
        # advanced_power_grid.py:331 test episode_step before its increment): one step more for them
        extra = 1 if env.env_id.startswith("Advanced") else 0
        if episode_log is None:
            rollout(env.max_episode_steps + extra)
        else:
            for s0 in range(0, env.max_episode_steps + extra, P):
                n = min(P, env.max_episode_steps + extra - s0)
                rollout(n, rew, fl)
                episode_log.collect(n, rew, fl)
                if launches is not None:
                    launches[0] += 1
        if round_hook is not None:
            round_hook(env, k)
        remaining -= k
    if disturbed:
        env.set_disturbance(None)
    while remaining > 0:
        k = min(B, remaining)
        mask = torch.zeros(B, dtype=torch.uint8, device=env.device)
        mask[:k] = 1
        env.reset(mask=mask, init_noise=None if reset_noise_fn is None else reset_noise_fn(rnd))
        if hasattr(agent, "begin_episode"):
            agent.begin_episode(B)
        t = 0
        while True:
            act = _predict(agent, env.obs)
            env.step(act, step_noise=None if step_noise_fn is None else step_noise_fn(rnd, t), layout="aos")
            if episode_log is not None:
                episode_log.collect(1, env.reward, env.flags)
                if launches is not None:
                    launches[0] += 1
            t += 1
            if _round_is_over(env, t, hasattr(agent, "predict_device")) or t > _lib.MAX_EPISODE_STEPS:
                break
        if round_hook is not None:
            round_hook(env, k)
        remaining -= k
        rnd += 1
    partial = env.reduce_tally()
    total = all_reduce_partial(partial, group) if reduce_across_ranks else partial
    import torch.distributed as dist
    n_total = n_episodes
    if reduce_across_ranks and dist.is_available() and dist.is_initialized():
        n_total = int(round(float(total[_lib.T_EPISODES].item())))
    return metrics_from_partial(total, n_total)


def uniform_action_statistics(env_id: str, batch: int, episodes_per_lane: int, device="cuda:0", seed: int = 0xBEEF,
                              plan_steps: int = 250, outputs: str = "min", action_source: str = "ring") -> Dict[str, Any]:
    """Episode statistics of the reference's measurement loop (performance_benchmark.py:106-133: a uniform random action per
    step, reset on done) in FAST MODE -- fused rollout launches, in-kernel generator, auto-reset -- over the first
    `episodes_per_lane` episodes of every lane.  A fixed episode count per lane is an unbiased sample ("episodes finished
    inside a window of steps" favours short ones); every step gets a fresh action (slot k of a `plan_steps`-slot ring, refilled
    for every launch).  All reductions run on the device from the per-step flag words and rewards the kernel writes.
    Returns sums over the counted episodes: episodes, steps, viol (base.py:179-183 violation counts), crit, c0..c2 (steps on
    which built-in constraint k failed), term / trunc / shut (how the episodes ended), ret (sum of rewards), hist (episode
    lengths, index = length), launches.  outputs: "min" = reward + flag rows; "full" also writes the observation
    trajectory (the kernel instantiation bench.py's headline times).
    action_source: "ring" (the default) fills the ring with `plan_steps` fill_actions launches before every rollout launch;
    "generated" allocates no ring and runs no fill launches -- rollout_sampled draws every step's action in the kernel, from the
    same action stream (at the launch's own counters t instead of 7000 + t: the same distribution)."""
    if action_source not in ("ring", "generated"):
        raise ValueError(f"action_source is 'ring' or 'generated', not {action_source!r}")
    generated = action_source == "generated"
    L = _lib
    env = make_batched(env_id, batch, device=device, seed=seed, autoreset=True)
    dev, B, K, P = env.device, env.batch, int(episodes_per_lane), int(plan_steps)
    env.reset()
    ring = None if generated else torch.empty(P, env.action_dim, env.ld, dtype=torch.float32, device=dev)
    rew = torch.empty(P, env.ld, dtype=torch.float32, device=dev)
    fl = torch.empty(P, env.ld, dtype=torch.int32, device=dev)
    traj = torch.empty(P, B, env.state_dim, dtype=torch.float32, device=dev) if outputs == "full" else None
    epcount = torch.zeros(B, dtype=torch.int32, device=dev)
    acc = {k: torch.zeros((), dtype=torch.int64, device=dev)
           for k in ("steps", "viol", "crit", "c0", "c1", "c2", "episodes", "term", "trunc", "shut")}
    ret = torch.zeros((), dtype=torch.float64, device=dev)
    hist = torch.zeros(env.max_episode_steps + 1, dtype=torch.int64, device=dev)
    launches = t = 0
    while True:
        if generated:
            env.rollout_sampled(P, rew, fl, traj)
        else:
            for s in range(P):
                t += 1
                env.fill_actions(7000 + t, ring[s])
            env.rollout(P, ring, rew, fl, traj)
        f = fl[:, :B]
        done = (f & (L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0
        cum = done.cumsum(0, dtype=torch.int32)
        valid = (epcount.unsqueeze(0) + cum - done.to(torch.int32)) < K          # the step belongs to one of the lane's first K episodes
        acc["steps"] += valid.sum()
        acc["viol"] += ((((f >> L.FLAG_NVIOL_SHIFT) & 3) + ((f >> 13) & 1) * 4) * valid).sum()
        acc["crit"] += (((f >> L.FLAG_NCRIT_SHIFT) & 3) * valid).sum()
        for k in range(3):
            acc[f"c{k}"] += (((f >> (L.FLAG_VIOL_SHIFT + k)) & 1) * valid).sum()
        ret += (rew[:, :B].to(torch.float64) * valid).sum()
        dv = done & valid
        acc["episodes"] += dv.sum()
        acc["term"] += (dv & ((f & L.FLAG_TERMINATED) != 0)).sum()
        acc["trunc"] += (dv & ((f & L.FLAG_TRUNCATED) != 0)).sum()
        acc["shut"] += (dv & ((f & L.FLAG_SHUTDOWN) != 0)).sum()
        hist += torch.bincount(((f >> L.FLAG_STEP_SHIFT) & 0xFFFF)[dv].to(torch.int64), minlength=hist.numel())[:hist.numel()]
        epcount += cum[-1]
        launches += 1
        if int(epcount.min().item()) >= K:
            break
        if launches * P > K * env.max_episode_steps + P:
            raise RuntimeError("a lane did not finish its episodes within episodes_per_lane x max_episode_steps steps")
    out: Dict[str, Any] = {k: int(v.item()) for k, v in acc.items()}
    out.update(ret=float(ret.item()), hist=hist.cpu().numpy(), launches=launches, batch=B, episodes_per_lane=K)
    env.close()
    return out
