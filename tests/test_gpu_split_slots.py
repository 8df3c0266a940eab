"""-m gpu: the three-wave rollout kernels with the ring slot as a compile-time constant (csrc/nig_split_body.inc: the
integrator's step loop is unrolled by lcm(2, K), the recorder's by K, the producer's by lcm(look-ahead, K); K = 6 ring slots
for ChemicalReactor, 3 for RobotAssembly; the steps behind the last whole iteration run at their static positions under
`if (i < n)`).  What can go wrong is a step that reads or writes another slot than its partners, or a tail position that is
skipped or run twice -- so every launch length around the unrolled lengths (1, K - 1, K, K + 1, ... 3 K + 1) runs in the
three-wave form and in the one-wave rollout_kernel on the same handle state, at one and two blocks, and everything a rollout
leaves behind must be bit-identical."""
import types

import numpy as np
import pytest
import torch

from conftest import ENV_NAME, load_golden

pytestmark = pytest.mark.gpu

KERNEL = {"cr": "ChemicalReactor", "ra": "RobotAssembly"}
MODES = ("none", "last", "rows", "soa", "aos")
LENGTHS = (1, 5, 6, 7, 11, 12, 13, 17, 18, 19)


@pytest.fixture(scope="module")
def ni():
    import neorl_industrial_gym_amd as ni
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield ni
    ni.tune(split_blocks=-1, wide_min_blocks=-1)


def _kernel(ni, key, B, outputs="full"):
    import bench
    return bench.rollout_kernel_name(types.SimpleNamespace(key=key, B=B, outputs=outputs, ni=ni))


def _run(ni, split, key, B, chunks, outputs, sampled, max_steps, first_counter=0, seed=11):
    """Roll `chunks` (step counts of consecutive launches) through one handle, ring-fed (slot s of the ring holds
    fill_actions(70 + s)) or with the actions sampled in the kernel; returns every observable as CPU tensors."""
    ni.tune(split_blocks=256 if split else 0)
    if not sampled:
        want = ("split_rollout_kernel<%s,3,4>" if split else "rollout_kernel<%s,3>") % KERNEL[key]
        assert _kernel(ni, key, B) == want
    env = ni.make_batched(ENV_NAME[key], B, seed=seed, autoreset=True, tally=True, max_episode_steps=max_steps)
    ring = None
    if not sampled:
        ring = torch.empty(7, env.action_dim, env.ld, dtype=torch.float32, device=env.device)
        for s in range(7):
            env.fill_actions(70 + s, ring[s])
    env.reset()
    env.counter = first_counter
    got = []
    for T in chunks:
        rew = fl = obs = None
        if outputs != "none":
            rows = () if outputs == "last" else (T,)
            rew = torch.full(rows + (env.ld,), float("nan"), dtype=torch.float32, device=env.device)
            fl = torch.zeros(rows + (env.ld,), dtype=torch.int32, device=env.device)
        if outputs == "aos":
            obs = torch.full((T, B, env.state_dim), float("nan"), dtype=torch.float32, device=env.device)
        elif outputs == "soa":
            obs = torch.full((T, env.state_dim, env.ld), float("nan"), dtype=torch.float32, device=env.device)
        if sampled:
            env.rollout_sampled(T, rew, fl, obs)
        else:
            env.rollout(T, ring, rew, fl, obs)
        torch.cuda.synchronize()
        got += [t.cpu() if (t is obs and outputs == "aos") else t[..., :B].cpu() for t in (rew, fl, obs) if t is not None]
    got += [env.state_soa.cpu(), env.ctr.cpu(), env.life_viol.cpu(), env.ep_return.cpu(), env.tally.cpu()]
    assert env.counter == first_counter + sum(chunks)
    env.close()
    return got


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i)
        assert torch.equal(_bits(x), _bits(y)), f"{what}: observable {i} differs"


@pytest.mark.parametrize("n_steps", LENGTHS)
@pytest.mark.parametrize("sampled", [False, True], ids=["ring", "sampled"])
@pytest.mark.parametrize("key", ["cr", "ra"])
def test_every_tail_length_equals_the_one_wave_form(ni, key, sampled, n_steps):
    """Two chained launches of n_steps (the second starts from the carried state, counters and returns), every output mode,
    one and two 256-lane blocks, from an even and an odd launch counter (ChemicalReactor's three-wave form starts on an odd
    one: from an even counter the host peels one step, so the kernel runs n_steps and n_steps - 1 steps in turn); 5-step
    episodes, so resets fall into the unrolled iterations and into the tails."""
    for outputs in MODES:
        for B in (256, 512):
            for first_counter in ((0, 1) if key == "cr" else (0,)):      # (no pairing of launch counters for RobotAssembly)
                kw = dict(key=key, B=B, chunks=[n_steps, n_steps], outputs=outputs, sampled=sampled, max_steps=5, first_counter=first_counter)
                _same(_run(ni, True, **kw), _run(ni, False, **kw), f"{key} B={B} {outputs} n={n_steps} from {first_counter}")


@pytest.mark.parametrize("sampled", [False, True], ids=["ring", "sampled"])
@pytest.mark.parametrize("B", [256, 512])
@pytest.mark.parametrize("key", ["cr", "ra"])
def test_resets_on_every_slot_position(ni, oracle, key, B, sampled):
    """7-step episodes over 43 steps: 7 is coprime to the unrolled lengths (6 and 12), so the truncations -- and the in-kernel
    resets behind them -- land on every slot position of every role.  Against the one-wave form; ChemicalReactor's sampled
    launch (the action of launch counter t is the generator's, as in the oracle) also against the CPU oracle bit for bit."""
    kw = dict(key=key, B=B, chunks=[43], outputs="aos", sampled=sampled, max_steps=7, seed=0x5EED)
    a = _run(ni, True, **kw)
    _same(a, _run(ni, False, **kw), f"{key} B={B}")
    L = ni._lib
    assert int(a[-1][L.T_EPISODES].sum().item()) >= 6 * B             # every lane: six truncations at the least
    if key == "cr" and sampled:
        st, sc, total, _ = oracle.rollout("cr", B, 43, seed=0x5EED, max_steps=7, flavor=oracle.MATH_POLY)
        state = a[-5][:, :B].numpy().T                                 # state_soa [S, ld] -> [B, S]
        assert np.array_equal(np.ascontiguousarray(state).view(np.uint32), st.view(np.uint32))
        assert np.array_equal(a[-4][:B].numpy() & L.CTR_STEP_MASK, sc)
        fl = a[1].numpy()
        assert int(((fl >> L.FLAG_NVIOL_SHIFT) & 3).sum()) == total.violations
        assert int(((fl >> L.FLAG_NCRIT_SHIFT) & 3).sum()) == total.critical
        assert int(a[-1][L.T_EPISODES].sum().item()) == total.episodes


def test_recorded_draws_equal_the_parity_step_kernel(ni):
    """nig_rollout_noise in the three-wave form (the NOISE instantiation of the same body: the producer loads the recorded
    step draws, a finishing lane restarts from the recorded initial-state draws) on the committed ChemicalReactor rows at 256
    lanes, two chained launches, against step_kernel's parity mode fed the same row sets step by step: bit-identical state,
    rewards and flags.  200 steps: the three shortest recorded episodes (172, 177, 190 steps) end inside the run."""
    from test_gpu_noise_rollout import _chain
    key, B, T = "cr", 256, 200
    d = load_golden(key, "g3")
    act, nz, rz, idx, first = _chain(d, B, T)
    done = (d["terminated"][idx] | d["truncated"][idx]) != 0
    assert done.any()
    outs = []
    for fused in (True, False):
        ni.tune(split_blocks=256 if fused else 0, wide_min_blocks=-1)
        env = ni.make_batched(ENV_NAME[key], B, autoreset=True)
        pad = lambda x: torch.from_numpy(np.concatenate([x, np.zeros(x.shape[:-1] + (env.ld - B,), x.dtype)], -1)).cuda()
        env.reset(init_noise=d["ep_init_noise"][first].T)
        rew = torch.zeros(T, env.ld, dtype=torch.float32, device="cuda")
        fl = torch.zeros(T, env.ld, dtype=torch.int32, device="cuda")
        obs = torch.zeros(T, B, 12, dtype=torch.float32, device="cuda")
        if fused:
            assert _kernel(ni, key, B) == "split_rollout_kernel<ChemicalReactor,3,4>"
            ring, nzt, rzt = pad(act), pad(nz), pad(rz)
            for t0, t1 in ((0, 67), (67, T)):
                env.rollout_noise(t1 - t0, ring[t0:t1], nzt[t0:t1], rzt[t0:t1], rew[t0:t1], fl[t0:t1], obs[t0:t1])
        else:
            for t in range(T):
                o, r, te, tr, info = env.step(act[t].T.copy(), step_noise=nz[t], reset_noise=rz[t], layout="aos")
                rew[t, :B] = r; fl[t, :B] = info.flags
        torch.cuda.synchronize()
        outs.append((env.get_state().cpu().numpy(), rew.cpu().numpy()[:, :B], fl.cpu().numpy()[:, :B]))
        env.close()
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    assert np.array_equal(outs[0][2], outs[1][2])
