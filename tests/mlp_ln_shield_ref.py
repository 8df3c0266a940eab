"""The host restatement of "nig-mlp-ln-shield-v1" (csrc/nig_mlp_ln_shield.hpp) for test_mlp_ln_shield_host.py and
test_gpu_mlp_ln_shield.py: a wrapper of tests/mlp_ln_ref.py (the restatement of "nig-mlp-ln-v1", general in IN / OUT) and the oracle's
det_tanhf / det_sigmoidf.  No arithmetic of its own: the critic is the restated network with IN = S + A, OUT = 1 on [obs, raw action],
zero-row-padded to an even IN.  A plain helper module (no fixtures, no collection hooks)."""
import numpy as np

import mlp_ln_ref as ref

f32 = np.float32


def padded(cweights, x):
    """(weights, x) with one zero row behind C1 and one zero column behind x where S + A is odd: the layer-1 width of mlp_layer1"""
    (C1, c1), l2, l3 = cweights
    C1, x = np.asarray(C1, dtype=f32), np.asarray(x, dtype=f32)
    if C1.shape[0] % 2:
        C1 = np.concatenate([C1, np.zeros((1, C1.shape[1]), f32)], axis=0)
        x = np.concatenate([x, np.zeros((x.shape[0], 1), f32)], axis=1)
    return [(C1, c1), l2, l3], np.ascontiguousarray(x)


def critic_pre(cweights, cnorms, obs, raw, eps=ref.EPS):
    """the critic's head pre-activation [n] (float32) on [obs, raw], in the law's order"""
    w, x = padded(cweights, np.concatenate([np.asarray(obs, dtype=f32), np.asarray(raw, dtype=f32)], axis=1))
    return ref.pre(w, cnorms, x, eps)[:, 0]


def prob(oracle, cweights, cnorms, obs, raw, eps=ref.EPS):
    """p [n]: the oracle's det_sigmoidf of critic_pre()"""
    return oracle.detmath_unary("sigmoidf", critic_pre(cweights, cnorms, obs, raw, eps))


def step(oracle, pol, obs, threshold):
    """The law on observations [n, S] for a LayerNormMLPPolicy with a critic: (raw action, p, shield, the action the env receives)"""
    raw = ref.act(oracle, pol.weights, pol.norms, obs, pol.eps)
    p = prob(oracle, pol.safety_weights, pol.safety_norms, obs, raw, pol.safety_eps)
    shield = ~(p < f32(threshold))
    return raw, p, shield, np.where(shield[:, None], raw * f32(0.5), raw).astype(f32)


def model64(cweights, cnorms, obs, raw, eps=ref.EPS):
    """ref.model64 of the critic on [obs, raw] in float64 (no padding: a zero row changes nothing there)"""
    return ref.model64(cweights, cnorms, np.concatenate([np.asarray(obs, dtype=np.float64), np.asarray(raw, dtype=np.float64)], axis=1), eps)


def random_ln_critic(S, A, seed, state_scale=None, head=1.0):
    """ref.random_ln_actor(S + A, 1, seed) as a critic: (weights, norms).  state_scale [S]: the first layer's state rows scaled by
    20 * state_scale (test_gpu_mlp_ln._policy's scaling) and its action rows by 20, so that no single state column decides every
    unit's sign and the action reaches the layer; head: a factor on the head's weights, against a saturated sigmoid."""
    ws, norms = ref.random_ln_actor(S + A, 1, seed)
    C1 = ws[0][0].copy()
    if state_scale is not None:
        C1[:S] = C1[:S] * f32(20.0) * np.asarray(state_scale, dtype=f32)[:, None]
        C1[S:] = C1[S:] * f32(20.0)
    return [(C1.astype(f32), ws[0][1]), ws[1], ((ws[2][0] * f32(head)).astype(f32), ws[2][1])], norms
