"""NumPy fp64 restatement of the multi-sample self-critical reward (include/rfn.h "multi-sample self-critical"; not a test
module).  Rows are image-major: row r = k * n + j is draw j of image k.  Every sum, product and quotient is one fp64 operation,
in the order the header states, written as a Python loop so that nothing is vectorised into another order."""
import numpy as np


def loo_diff(s, n, baseline='loo'):
    """s (B,) float64 -> s - base with base[k*n+j] = (((0.0 + s[k*n+i0]) + s[k*n+i1]) + ...) / (n - 1), i != j ascending;
    baseline 'none': s itself."""
    s = np.asarray(s, dtype=np.float64)
    B = s.shape[0]
    assert n >= 1 and B % n == 0 and baseline in ('loo', 'none')
    if baseline == 'none':
        return s.copy()
    assert n >= 2
    out = np.empty(B, dtype=np.float64)
    for r in range(B):
        k0 = r - r % n
        acc = np.float64(0.0)
        for i in range(n):
            if k0 + i != r:
                acc = acc + s[k0 + i]
        out[r] = s[r] - acc / np.float64(n - 1)
    return out


def group_reward(cider, bleu, n, T, cider_weight=1.0, bleu4_weight=0.0, baseline='loo'):
    """cider: None or (B,) scores; bleu: None or (B, 4) scores (column 3 is BLEU-4) -> (B, T) float64
    ((diff_bleu4 * bleu4_weight) + (diff_cider * cider_weight)) + 0.0; a missing scorer is the reference's 0 * weight."""
    assert cider is not None or bleu is not None
    B = len(cider) if cider is not None else len(bleu)
    db = loo_diff(np.asarray(bleu, dtype=np.float64)[:, 3], n, baseline) if bleu is not None else np.zeros(B)
    dc = loo_diff(cider, n, baseline) if cider is not None else np.zeros(B)
    out = np.empty((B, T), dtype=np.float64)
    for r in range(B):
        tb = db[r] * np.float64(bleu4_weight)
        tc = dc[r] * np.float64(cider_weight)
        out[r, :] = (tb + tc) + 0.0
    return out
