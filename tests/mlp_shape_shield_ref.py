"""The host restatement of "nig-mlp-shape-shield-v1" (csrc/nig_mlp_shape_shield.hpp) for test_mlp_shape_shield_host.py and
test_gpu_mlp_shape_shield.py: a wrapper of tests/mlp_shape_ref.py (the restatement of "nig-mlp-shape-v1", general in S, A and the
widths) and the oracle's det_tanhf / det_sigmoidf.  No arithmetic of its own: the critic is the restated network with IN = S + A,
OUT = 1 on [obs, raw action] (the zero pad of an odd S + A is a skipped term there).  A plain helper module (no fixtures, no
collection hooks)."""
import numpy as np

import mlp_shape_ref as ref

f32 = np.float32


def random_critic(S, A, dims, seed, state_scale=None, head=1.0):
    """ref.random_actor(S + A, 1, dims, seed) as a critic.  state_scale [S]: the first layer's state rows scaled by 20 * state_scale
    (test_gpu_mlp_shape._actor's scaling) and its action rows by 20, so that no single state column decides every unit's sign and
    the action reaches the layer; head: a factor on the head's weights, against a saturated sigmoid."""
    ws = ref.random_actor(S + A, 1, dims, seed)
    C1 = ws[0][0].copy()
    if state_scale is not None:
        C1[:S] = C1[:S] * f32(20.0) * np.asarray(state_scale, dtype=f32)[:, None]
        C1[S:] = C1[S:] * f32(20.0)
    ws[0] = (C1.astype(f32), ws[0][1])
    ws[-1] = ((ws[-1][0] * f32(head)).astype(f32), ws[-1][1])
    return ws


def critic_pre(critic, obs, raw):
    """the critic's head pre-activation [n] (float32) on [obs, raw], in the law's order"""
    x = np.concatenate([np.asarray(obs, dtype=f32), np.asarray(raw, dtype=f32)], axis=1)
    return ref.pre(critic, np.ascontiguousarray(x))[:, 0]


def prob(oracle, critic, obs, raw):
    """p [n]: the oracle's det_sigmoidf of critic_pre()"""
    return oracle.detmath_unary("sigmoidf", critic_pre(critic, obs, raw))


def step(oracle, pol, obs, threshold):
    """The law on observations [n, S] for a policy with .weights and .safety_weights: (raw action, p, shield, the action the env
    receives)"""
    raw = ref.act(oracle, pol.weights, obs)
    p = prob(oracle, pol.safety_weights, obs, raw)
    shield = ~(p < f32(threshold))
    return raw, p, shield, np.where(shield[:, None], raw * f32(0.5), raw).astype(f32)


def pre64(critic, obs, raw):
    """the critic's head pre-activation [n] in NumPy float64 on [obs, raw]"""
    return ref.pre64(critic, np.concatenate([np.asarray(obs, dtype=np.float64), np.asarray(raw, dtype=np.float64)], axis=1))[:, 0]


U = 2.0 ** -24                                     # float32 unit roundoff


def pre_bound(critic, x):
    """The forward-error bound of the law's float32 evaluation of the critic's pre-activation against exact arithmetic, per sample
    (profiles/shapes/fidelity.txt's derivation): a chain of n fused multiply-adds into one accumulator satisfies |fl - exact| <=
    gamma_n sum |w_k| |x_k|, gamma_n = n u / (1 - n u), u = 2^-24.  Layer 1 is a chain of even(S + A) + 1 terms (the zero pad and
    the bias), a later hidden unit one of K + 1; ReLU is 1-Lipschitz; an input error e_k enters the next layer as sum |w_k| e_k; the
    head is two chains of at most K / 2 + 1 terms and one add: gamma_{K/2+2}."""
    g = lambda n: n * U / (1 - n * U)
    z = np.asarray(x, dtype=np.float64)
    e = np.zeros_like(z)
    for i, (W, b) in enumerate(critic):
        W, b = np.asarray(W, dtype=np.float64).reshape(z.shape[-1], -1), np.asarray(b, dtype=np.float64).reshape(-1)
        K = W.shape[0]
        terms = (K + (K & 1) + 1 if i == 0 else K + 1) if i + 1 < len(critic) else K // 2 + 2
        mag = (np.abs(z) + e) @ np.abs(W) + np.abs(b)
        e = e @ np.abs(W) + g(terms) * mag
        z = z @ W + b
        if i + 1 < len(critic):
            z = np.maximum(z, 0)
    return e[:, 0]


def p_bound(critic, x):
    """|p - p64| <= pre_bound / 4 + 3 ulp + 2^-50: the sigmoid's slope is at most 1/4, det_sigmoidf is within 3 ulp of the sigmoid on
    normal results (tests/detmath_check.c) and p <= 1 puts an ulp at 2^-23 at most; p64 itself carries a float64 rounding"""
    return pre_bound(critic, x) / 4 + 3.0 * 2.0 ** -23 + 2.0 ** -50
