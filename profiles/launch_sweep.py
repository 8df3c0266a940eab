"""One fixed, seeded sweep through nig_rollout / nig_rollout_sampled / nig_rollout_noise / nig_rollout_policy, n_steps = 3:
every kernel-form threshold from both sides (knobs set small by ni.tune), four output modes, even and odd starting counters,
auto-reset on / off, a held lane, rows and row-major action rings.  Run under rocprofv3 --kernel-trace (profiles/launch_ab.sh); the
library comes from NIG_LIB_PATH (or the tree's libnig.so).  Which kernels it launches, in which order, with which grids, is what
profiles/launch_trace.py writes down: two libraries with the same host launch rule give the same list."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import neorl_industrial_gym_amd as ni
from neorl_industrial_gym_amd.batched import ENV_IDS

T = 3
BATCHES = [100, 300, 1024, 1280, 1572, 1792, 2048, 2304]
NOISE_ENVS = ("ChemicalReactor-v0", "PowerGrid-v0", "RobotAssembly-v0")
dev = "cuda:0"
calls = 0


def outputs(env, mode):
    B, S, ld = env.batch, env.state_dim, env.ld
    if mode == 0:
        return None, None, None
    rew = torch.zeros(T, ld, dtype=torch.float32, device=dev)
    fl = torch.zeros(T, ld, dtype=torch.int32, device=dev)
    obs = None
    if mode == 2:
        obs = torch.zeros(T, S, ld, dtype=torch.float32, device=dev)
    elif mode == 3:
        obs = torch.zeros(T, B, S, dtype=torch.float32, device=dev)
    return rew, fl, obs


def make(name, B, kind):
    env = ni.make_batched(name, B, device=dev, seed=1234, autoreset=(kind != "noreset"), max_episode_steps=5)
    if kind == "held":                             # lane 0 is never reset: the handle keeps its may-hold-done bit
        mask = torch.ones(B, dtype=torch.uint8, device=dev)
        mask[0] = 0
        env.reset(mask=mask)
    else:
        env.reset()
    return env


def sweep(envs, batches, kinds):
    global calls
    g = torch.Generator(device="cpu").manual_seed(99)
    for name in envs:
        for B in batches:
            for kind in kinds:
                env = make(name, B, kind)
                A, S, ld = env.action_dim, env.state_dim, env.ld
                rows = torch.empty(T, A, ld, dtype=torch.float32, device=dev)
                for s in range(T):
                    env.fill_actions(700 + s, rows[s])
                aos = rows[:, :, :B].permute(0, 2, 1).contiguous()
                modes = (0, 1, 2, 3) if kind == "plain" else (1, 3)
                for mode in modes:
                    rew, fl, obs = outputs(env, mode)
                    for start in (10, 11):
                        for ring in (rows, aos):
                            env.counter = start
                            env.rollout(T, ring, rew, fl, obs)
                            calls += 1
                        env.counter = start
                        env.rollout_sampled(T, rew, fl, obs)
                        calls += 1
                    torch.cuda.synchronize()
                if name in NOISE_ENVS:
                    K, KR = int(env.spec.k_step), int(env.spec.k_reset)
                    nz = (0.1 * torch.randn(T, K, ld, generator=g, dtype=torch.float64)).to(dev) if K else None
                    rz = (0.1 * torch.randn(T, KR, ld, generator=g, dtype=torch.float64)).to(dev) if KR else None
                    rew, fl, obs = outputs(env, 3)
                    for start in (10, 11):
                        env.counter = start
                        env.rollout_noise(T, rows, nz, rz, rew, fl, obs)
                        calls += 1
                    torch.cuda.synchronize()
                for pol in (ni.constant_agent(S, A), ni.pid_agent(S, A)):
                    env.set_policy(pol)
                    for mode in (1, 3):
                        rew, fl, obs = outputs(env, mode)
                        env.counter = 10
                        env.rollout_policy(T, rew, fl, obs)
                        calls += 1
                    torch.cuda.synchronize()
                env.close()


def main():
    print("libnig:", ni._lib.lib().nig_version().decode(), flush=True)
    ni.tune(split_blocks=4, wide_min_blocks=3)
    sweep(list(ENV_IDS), BATCHES, ("plain", "noreset", "held"))
    ni.tune(split_blocks=0, wide_min_blocks=2 ** 30)           # both knobs off
    sweep(NOISE_ENVS, [1024, 1572], ("plain",))
    ni.tune(split_blocks=1, wide_min_blocks=0)                 # one block per round; wide from the first 512 lanes
    sweep(NOISE_ENVS, [256, 512, 768], ("plain",))
    torch.cuda.synchronize()
    print("calls", calls, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
