"""Per-episode records from the reward / flag rows of the rollouts, and evaluate_episodes on top of them.

The tally (NIG_F_TALLY) knows thirteen sums of the episodes it saw.  What the reference's evaluation layer does with single
episodes -- SafetyBenchmark / PerformanceBenchmark's median_return, violation_rate, metadata["individual_returns"] and
["episode_violations"] (benchmarks/industrial_benchmarks.py:95-341), the per-episode lists of
benchmarks/statistical_analysis.py -- needs one number per episode: an EpisodeLog (include/nig.h nig_episode_log_*,
nig_collect_episodes, nig_reduce_episodes; the law is csrc/nig_episodes.hpp episode_row) built from the per-step rows every
rollout entry point writes.  episodes_from_rows restates that law in NumPy: the host reference."""
import ctypes as C
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import _lib

_END_MASK = _lib.FLAG_TERMINATED | _lib.FLAG_TRUNCATED | (3 << _lib.FLAG_NCRIT_SHIFT) | _lib.FLAG_SHUTDOWN


def episodes_from_rows(reward, flags, ret_f32: bool, capacity: int, carry: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, np.ndarray]:
    """The state machine of csrc/nig_episodes.hpp (episode_row) on host arrays: reward float32 [T, B], flags uint32 [T, B],
    rows in step order.  Returns a dict of
        ret float64 [capacity, B], w uint32 [5, capacity, B]   the records (entries at or beyond a lane's count: as they were,
                                                                zero in a fresh log),
        count uint32 [B]                                        finished episodes per lane (keeps counting beyond capacity),
        carry_ret float64 [B], carry_w uint32 [4, B]            the running return / violations, w[2], w[3], w[4] so far.
    `carry`: the dict a previous call returned -- rows cut into several calls give the records of one call.  It is not changed.
    ret_f32: the env accumulates its return in float32 (nig_env_spec.reward_is_f32): (double)((float)ret + reward), the
    kernels' own sum bit for bit; otherwise float64 over the float32 rows."""
    L = _lib
    reward = np.asarray(reward, dtype=np.float32)
    flags = np.asarray(flags).astype(np.uint32, copy=False) if np.asarray(flags).dtype != np.int32 else np.asarray(flags).view(np.uint32)
    assert reward.ndim == 2 and reward.shape == flags.shape
    T, B = reward.shape
    K = int(capacity)
    if carry is None:
        out = {"ret": np.zeros((K, B), np.float64), "w": np.zeros((5, K, B), np.uint32), "count": np.zeros(B, np.uint32),
               "carry_ret": np.zeros(B, np.float64), "carry_w": np.zeros((4, B), np.uint32)}
    else:
        out = {k: np.array(v, copy=True) for k, v in carry.items()}
        assert out["ret"].shape == (K, B) and out["w"].shape == (5, K, B)
    ret, w, count, cret, cw = out["ret"], out["w"], out["count"], out["carry_ret"], out["carry_w"]
    lanes = np.arange(B)
    one = np.uint32(1)
    for t in range(T):
        f, r = flags[t], reward[t]
        live = (f & np.uint32(L.FLAG_INACTIVE)) == 0
        if ret_f32:
            new = (cret.astype(np.float32) + r).astype(np.float64)            # one float32 add, as add_reward
        else:
            new = cret + r.astype(np.float64)
        cret[live] = new[live]
        bit = lambda s: (f >> np.uint32(s)) & one                              # noqa: E731
        add = np.stack([bit(L.FLAG_NVIOL_SHIFT) + (bit(L.FLAG_NVIOL_SHIFT + 1) << one) + (bit(13) << np.uint32(2)),
                        bit(L.FLAG_VIOL_SHIFT) + (bit(L.FLAG_VIOL_SHIFT + 1) << np.uint32(16)),
                        bit(L.FLAG_VIOL_SHIFT + 2) + (bit(12) << np.uint32(16)),
                        bit(14) + (bit(15) << np.uint32(16))]).astype(np.uint32)
        cw[:, live] += add[:, live]
        done = live & ((f & np.uint32(L.FLAG_TERMINATED | L.FLAG_TRUNCATED)) != 0)
        wr = done & (count < K)
        if wr.any():
            k, i = count[wr].astype(np.int64), lanes[wr]
            ret[k, i] = cret[wr]
            w[0, k, i] = ((f[wr] >> np.uint32(L.FLAG_STEP_SHIFT)) & np.uint32(L.CTR_STEP_MASK)) | np.uint32(L.CTR_DONE) | (cw[0, wr] << np.uint32(L.CTR_VIOL_SHIFT))
            w[1, k, i] = f[wr] & np.uint32(_END_MASK)
            w[2, k, i], w[3, k, i], w[4, k, i] = cw[1, wr], cw[2, wr], cw[3, wr]
        count[done] += one
        cret[done] = 0.0
        cw[:, done] = 0
    return out


def counted(count, batch: int, capacity: int, n_episodes: int) -> np.ndarray:
    """Bool [capacity, batch]: record (k, i) takes part in a reduction over n_episodes iff k < min(count[i], capacity) and
    k * batch + i < n_episodes (include/nig.h nig_reduce_episodes)."""
    k = np.arange(capacity, dtype=np.int64)[:, None]
    i = np.arange(batch, dtype=np.int64)[None, :]
    have = np.minimum(np.asarray(count, dtype=np.int64), capacity)[None, :]
    return (k < have) & (k * batch + i < int(n_episodes))


class EpisodeLog:
    """`capacity` records per lane of a BatchedIndustrialEnv, in device memory this object owns (benv.episode_log(capacity)).
    Views (torch, on the env's device; [K, B] = [capacity, batch], entry (k, i) = episode k of lane i, meaningful for
    k < min(count[i], capacity)):
        count [B] int32 (finished episodes, keeps counting beyond capacity), returns [K, B] float64, length, violations,
        critical [K, B] int32, terminated / truncated / shutdown [K, B] bool, constraint_steps [4, K, B], shielded_steps,
        uncertain_steps [K, B] int32."""

    def __init__(self, env, capacity: int, ld: Optional[int] = None, memory: Optional[torch.Tensor] = None):
        self.env, self.capacity = env, int(capacity)
        lay = _lib.episode_log_query(env.batch, self.capacity, int(ld or 0))
        self.layout, self.ld = lay, int(lay.ld)
        if memory is None:
            memory = torch.empty(int(lay.bytes), dtype=torch.uint8, device=env.device)
        assert memory.dtype == torch.uint8 and memory.is_contiguous() and memory.numel() >= int(lay.bytes) and memory.data_ptr() % 8 == 0
        self.memory = memory[:int(lay.bytes)]
        K, B, pitch = self.capacity, env.batch, self.ld

        def view(off, rows, dtype, size):
            return self.memory[off:off + rows * pitch * size].view(dtype).view(rows, pitch)[:, :B]

        self._ret = view(lay.off_ret, K, torch.float64, 8)
        self._w = [view(lay.off_w[j], K, torch.int32, 4) for j in range(5)]
        self.count = view(lay.off_count, 1, torch.int32, 4)[0]
        self.carry_ret = view(lay.off_carry_ret, 1, torch.float64, 8)[0]
        self.carry_w = view(lay.off_carry_w, 4, torch.int32, 4)
        self.clear()

    def _call(self, fn, *args):
        with torch.cuda.device(self.env._dev_index):
            _lib.check(fn(self.env._h, *args, self.env._stream()))

    def _ptr(self):
        return C.c_void_p(self.memory.data_ptr())

    def clear(self):
        """No episode finished, nothing running (nig_episode_log_init); the record rows are left as they are."""
        self._call(self.env._L.nig_episode_log_init, self._ptr(), self.capacity, self.ld)

    def collect(self, n_steps: int, reward_rows: torch.Tensor, flag_rows: torch.Tensor):
        """nig_collect_episodes: reward float32 / flags int32, [>= n_steps, >= B] with one row stride, or [B] with n_steps 1."""
        from .batched import _rows
        rp, rs = _rows(reward_rows, torch.float32, n_steps if reward_rows.dim() == 2 else None)
        fp, fs = _rows(flag_rows, torch.int32, n_steps if flag_rows.dim() == 2 else None)
        assert rs == fs, "reward and flag rows share their row stride"
        assert reward_rows.shape[-1] >= self.env.batch and flag_rows.shape[-1] >= self.env.batch
        self._call(self.env._L.nig_collect_episodes, int(n_steps), rp, fp, rs, self._ptr(), self.capacity, self.ld)

    def reduce(self, n_episodes: int) -> torch.Tensor:
        """nig_reduce_episodes: float64 [T_ROWS + 1] on the device -- the tally rows of the records that count (record (k, i)
        counts iff k * batch + i < n_episodes), then the number of counted episodes with at least one violation."""
        out = torch.empty(_lib.T_ROWS + 1, dtype=torch.float64, device=self.env.device)
        self._call(self.env._L.nig_reduce_episodes, self._ptr(), self.capacity, self.ld, int(n_episodes), C.c_void_p(out.data_ptr()))
        return out

    returns = property(lambda self: self._ret)
    length = property(lambda self: self._w[0] & _lib.CTR_STEP_MASK)
    violations = property(lambda self: (self._w[0] >> _lib.CTR_VIOL_SHIFT) & 0xFFFF)
    critical = property(lambda self: (self._w[1] >> _lib.FLAG_NCRIT_SHIFT) & 3)
    terminated = property(lambda self: (self._w[1] & _lib.FLAG_TERMINATED) != 0)
    truncated = property(lambda self: (self._w[1] & _lib.FLAG_TRUNCATED) != 0)
    shutdown = property(lambda self: (self._w[1] & _lib.FLAG_SHUTDOWN) != 0)
    shielded_steps = property(lambda self: self._w[4] & 0xFFFF)
    uncertain_steps = property(lambda self: (self._w[4] >> 16) & 0xFFFF)

    @property
    def words(self) -> torch.Tensor:
        """The five record words as stored, int32 [5, K, B] (a copy)."""
        return torch.stack(self._w)

    @property
    def constraint_steps(self) -> torch.Tensor:
        return torch.stack([self._w[2] & 0xFFFF, (self._w[2] >> 16) & 0xFFFF, self._w[3] & 0xFFFF, (self._w[3] >> 16) & 0xFFFF])

    def episodes(self, n_episodes: int) -> Dict[str, torch.Tensor]:
        """The counted records as 1-D device tensors in episode order (k * batch + i): returns, lengths, violations, critical,
        terminated, truncated, shutdown.  Needs every counted record to exist (count[i] > k, k < capacity)."""
        n, B = int(n_episodes), self.env.batch
        rows = -(-n // B)
        assert rows <= self.capacity, "n_episodes beyond capacity * batch"

        def flat(x):
            return x[:rows].reshape(-1)[:n]
        return {"returns": flat(self.returns), "lengths": flat(self.length), "violations": flat(self.violations),
                "critical": flat(self.critical), "terminated": flat(self.terminated), "truncated": flat(self.truncated),
                "shutdown": flat(self.shutdown)}


def _confidence_interval(returns: np.ndarray, sem: float, level: float):
    try:                                       # the reference imports scipy inside the function as well
        from scipy import stats
    except Exception:
        return None
    if returns.size < 2:
        return None
    lo, hi = stats.t.interval(level, returns.size - 1, loc=float(np.mean(returns)), scale=sem)
    return float(lo), float(hi)


def evaluate_episodes(agent: Any, env_or_id, n_episodes: int = 100, episodes_per_lane: Optional[int] = None, chunk: int = 250,
                      batch: Optional[int] = None, seed: int = 0x5EED, device="cuda:0", confidence_level: float = 0.95) -> Dict[str, Any]:
    """evaluate_with_safety with one record per episode: what SafetyBenchmark / PerformanceBenchmark.evaluate_agent
    (benchmarks/industrial_benchmarks.py:95-341) report.  Two ways to play the episodes, chosen by the handle:

    * autoreset=False, tally=True (what evaluate_with_safety needs): the same rounds -- one episode per lane per round, fused
      launches where the agent runs in the kernel (in pieces of `chunk` steps), the host loop otherwise -- with the rows of
      every launch collected into an EpisodeLog.  Episode k * batch + i is lane i's episode of round k.
    * autoreset=True: QUOTA mode -- every lane plays `episodes_per_lane` (default ceil(n_episodes / batch)) episodes back to
      back, `chunk` steps per launch, until the slowest lane has its quota; a finished lane never waits for the round's longest
      episode.  A fixed episode count per lane is an unbiased sample; the first n_episodes in the order
      k * batch + i are counted.  Needs an agent that runs in the kernel (DevicePolicy, MLPPolicy, EnsemblePolicy, a fusable
      Disturbed): ValueError otherwise.
    `env_or_id`: a BatchedIndustrialEnv, or an env id -- then a handle of min(n_episodes, 65536) lanes (or `batch`) is made here,
    auto-reset if the agent can run in the kernel.

    Returns evaluate_with_safety's thirteen aggregates (parallel.metrics_from_partial on the reduced records), plus
    return_median, return_sem (scipy.stats.sem: ddof = 1), violation_rate, sample_efficiency = return_mean / length_mean
    (industrial_benchmarks.py:198), confidence_interval (scipy.stats.t.interval at confidence_level; None where scipy is not
    installed -- the reference imports it lazily too), the per-episode DEVICE tensors returns / lengths / violations / critical /
    terminated / truncated / shutdown, n_episodes, mode ("rounds" / "quota") and launches.

    Upstream's SafetyBenchmark reads SafetyMetrics.total_violations, a field that does not exist (core/types.py:67-78), so it
    cannot run; safety_violations (the sum of the per-step violation counts) and violation_rate (the share of episodes with
    at least one violation) follow evaluate_robustness's definitions."""
    from .batched import BatchedIndustrialEnv
    from .parallel import metrics_from_partial
    from .utils import _evaluate_batched, _install_agent
    if not getattr(agent, "is_trained", False):
        raise RuntimeError("Agent must be trained before evaluation")
    n = int(n_episodes)
    if n < 1:
        raise ValueError("n_episodes must be at least 1")
    own = None
    if isinstance(env_or_id, BatchedIndustrialEnv):
        env = env_or_id
        env._refuse_limits("evaluate_episodes (episode records are decoded from the main flag word alone)")
    else:
        b = int(batch or min(n, 65536))
        env = own = BatchedIndustrialEnv(env_or_id, b, device=device, seed=seed, autoreset=True)
    try:
        rollout = None
        if env.autoreset:
            agent_in, rollout, disturbed = _install_agent(agent, env)
            if rollout is None and own is not None:          # a host-only agent: the rounds of evaluate_with_safety
                own.close()
                env = own = BatchedIndustrialEnv(env_or_id, env.batch, device=device, seed=seed, autoreset=False, tally=True)
            elif rollout is None:
                raise ValueError("an auto-reset handle needs an agent that runs in the kernel (DevicePolicy, MLPPolicy, EnsemblePolicy); "
                                 "use make_batched(..., tally=True, autoreset=False) for a host agent")
        B = env.batch
        if env.autoreset:
            quota = int(episodes_per_lane) if episodes_per_lane else -(-n // B)
            if n > quota * B:
                raise ValueError("n_episodes > episodes_per_lane * batch")
            log = env.episode_log(quota)
            P = max(1, int(chunk))
            rew = torch.empty(P, env.ld, dtype=torch.float32, device=env.device)
            fl = torch.empty(P, env.ld, dtype=torch.int32, device=env.device)
            env.reset()
            launches = 0
            try:
                while True:
                    rollout(P, rew, fl)
                    log.collect(P, rew, fl)
                    launches += 1
                    if int(log.count.min().item()) >= quota:
                        break
                    if launches * P > quota * (env.max_episode_steps + (1 if env.env_id.startswith("Advanced") else 0)) + P:
                        raise RuntimeError("a lane did not finish its episodes within episodes_per_lane x max_episode_steps steps")
            finally:
                if disturbed:
                    env.set_disturbance(None)
            mode = "quota"
        else:
            log = env.episode_log(-(-n // B))
            launches = [0]
            _evaluate_batched(agent, env, n, reduce_across_ranks=False, episode_log=log, chunk=chunk, launches=launches)
            mode, launches = "rounds", launches[0]
        partial = log.reduce(n).cpu().numpy()
        if int(round(partial[_lib.T_EPISODES])) != n:
            raise RuntimeError(f"{int(round(partial[_lib.T_EPISODES]))} of {n} episodes were recorded")
        out: Dict[str, Any] = metrics_from_partial(partial[:_lib.T_ROWS], n)
        eps = {k: v.clone() for k, v in log.episodes(n).items()}
        r = eps["returns"].cpu().numpy()
        sem = float(np.std(r, ddof=1) / np.sqrt(r.size)) if r.size > 1 else float("nan")
        out.update(return_median=float(np.median(r)), return_sem=sem, violation_rate=float(partial[_lib.T_ROWS]) / n,
                   sample_efficiency=out["return_mean"] / out["length_mean"],
                   confidence_interval=_confidence_interval(r, sem, confidence_level), n_episodes=n, mode=mode, launches=launches)
        out.update(eps)
        return out
    finally:
        if own is not None:
            own.close()
