"""The distillation loss of rfn_kd_logits_fwd / _bwd (include/rfn.h) restated in float64 NumPy: what the GPU tests compare the
kernels with, and what tests/test_distill_cpu.py checks against torch's float64 autograd.

Rows are (b, t).  x = the student's logits row, z = the teacher's row (logits or log-probs: every term is invariant to a per-row
shift of z), q = the one-hot or label-smoothed target of rfn_xe_logits_*, m = mask[b, t], it = 1 / temperature as a float32,
alpha in [0, 1]:

    p_t(v)  = softmax(z * it)(v)            p_s(v) = softmax(x * it)(v)
    KL(b,t) = sum_{v : p_t(v) > 0} p_t(v) * (log p_t(v) - log p_s(v))
    xe      = sum_{b,t} m * ( -q . log_softmax(x) ) / B
    kd      = sum_{b,t} m * KL(b,t) / (it*it) / B
    loss    = (1 - alpha) * xe + alpha * kd
    d loss / d x[v] = m * g / B * ( (1 - alpha) * (softmax(x)[v] - q[v]) + alpha / it * (p_s(v) - p_t(v)) )

A -inf teacher entry contributes 0; a row with m == 0 has loss terms and a gradient of exactly 0 whatever its teacher row holds
(NaN included); an out-of-range target is class 0, as in rfn_xe_logits_*."""
import numpy as np


def f32(v):
    """`v` rounded to float32, as a Python float: the inv_temp the C ABI receives."""
    return float(np.float32(v))


def _lse(a):
    """log sum exp over the last axis; -inf entries count as exp(-inf) = 0."""
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.max(a, axis=-1, keepdims=True)
        return (m + np.log(np.sum(np.exp(a - m), axis=-1, keepdims=True)))[..., 0]


def _targets(target, V1, eps):
    """q (B, T, V1): eps / V1 everywhere, 1 - eps more on the (clamped) target."""
    tg = np.asarray(target).astype(np.int64).copy()
    tg[(tg < 0) | (tg >= V1)] = 0
    q = np.full(tg.shape + (V1,), eps / V1, dtype=np.float64)
    np.put_along_axis(q, tg[..., None], 1.0 - eps + eps / V1, axis=-1)
    return q


def xe_reference(x, target, mask, eps, g=1.0):
    """The language term alone (rfn_xe_logits_*): -> dict(loss, rows (B, T), lse (B, T), grad (B, T, V1))."""
    x = np.asarray(x, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    B, T, V1 = x.shape
    q = _targets(target, V1, eps)
    lse = _lse(x)
    lp = x - lse[..., None]
    rows = m * -(q * lp).sum(-1)
    grad = (m * g / B)[..., None] * (np.exp(lp) - q)
    return dict(loss=rows.sum() / B, rows=rows, lse=lse, grad=grad)


def kd_reference(x, z, target, mask, eps, alpha, it, g=1.0):
    """x, z (B, T, V1); target, mask (B, T); `it` is taken as given (pass f32(1 / temperature) to share the kernels' value).
    -> dict(loss, xe, kd, grad (B, T, V1), stats (3, B, T) = lse(x), lse(x * it), lse(z * it))."""
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    B, T, V1 = x.shape
    live = m != 0
    base = xe_reference(x, target, mask, eps, g)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        xs, zs = x * it, z * it
        lse_s, lse_t = _lse(xs), _lse(zs)
        lps, lpt = xs - lse_s[..., None], zs - lse_t[..., None]
        ps, pt = np.exp(lps), np.exp(lpt)
        kl = np.where(pt > 0, pt * (lpt - lps), 0.0).sum(-1)
        kd_rows = np.where(live, m * kl / (it * it), 0.0)
        gk = (m * g / B)[..., None] * (alpha / it) * (ps - pt)
    grad = np.where(live[..., None], (1.0 - alpha) * base['grad'] + gk, 0.0)
    xe, kd = base['loss'], kd_rows.sum() / B
    return dict(loss=(1.0 - alpha) * xe + alpha * kd, xe=xe, kd=kd, grad=grad, stats=np.stack([base['lse'], lse_s, lse_t]))
