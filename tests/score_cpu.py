"""fp64 restatement of caption scoring (include/rfn.h "caption scoring") from a logits array: the live rule, the given token's
log-prob, its rank, the step's entropy and the per-caption sums.  numpy only -- nothing from the package."""
import numpy as np


def clamp_ids(target, V1):
    """An id outside [0, V1) reads as 0."""
    t = np.asarray(target, dtype=np.int64)
    return np.where((t < 0) | (t >= V1), 0, t)


def live_mask(target, V1, include_end):
    """(B, T) bool: position (b, t) is live iff every earlier id of the row is non-zero and (include_end or its own id is)."""
    ids = clamp_ids(target, V1)
    B, T = ids.shape
    live = np.zeros((B, T), dtype=bool)
    for b in range(B):
        for t in range(T):
            if ids[b, t] == 0:
                live[b, t] = bool(include_end)
                break
            live[b, t] = True
    return live


def score_logits(logits, target, include_end):
    """logits (T, B, V1), time-major, any float dtype (compared and summed as fp64 of the values given); target (B, >= T) ->
    tok_lp (B, T) f64 (0 where dead), rank (B, T) int64 (-1 where dead), ent (B, T) f64 (0 where dead)."""
    x = np.asarray(logits)
    T, B, V1 = x.shape
    ids = clamp_ids(np.asarray(target)[:, :T], V1)
    live = live_mask(ids, V1, include_end)
    lp = np.zeros((B, T))
    rank = np.full((B, T), -1, dtype=np.int64)
    ent = np.zeros((B, T))
    v = np.arange(V1)
    with np.errstate(all='ignore'):
        for t in range(T):
            for b in range(B):
                if not live[b, t]:
                    continue
                row = x[t, b].astype(np.float64)
                tg = int(ids[b, t])
                m = row.max()                                    # NaN if the row holds one
                lse = m + np.log(np.exp(row - m).sum())
                lp[b, t] = row[tg] - lse
                rank[b, t] = int(((row > row[tg]) | ((row == row[tg]) & (v < tg))).sum())
                logp = row - lse
                p = np.exp(logp)
                terms = np.where(p == 0.0, 0.0, -(p * logp))     # an entry of probability 0 counts 0, not 0 * inf
                ent[b, t] = terms.sum()
    return lp, rank, ent


def score_captions(tok_lp, target, V1, include_end):
    """tok_lp (B, T) float32 -> cap_lp (B,) f64 = ((0.0 + lp[0]) + lp[1]) + ... over the live positions ascending, one fp64 add
    each; cap_len (B,) the number of live positions."""
    lp = np.asarray(tok_lp, dtype=np.float32)
    B, T = lp.shape
    live = live_mask(np.asarray(target)[:, :T], V1, include_end)
    cap = np.zeros(B, dtype=np.float64)
    n = np.zeros(B, dtype=np.int32)
    with np.errstate(all='ignore'):
        for b in range(B):
            s = np.float64(0.0)
            for t in range(T):
                if live[b, t]:
                    s = s + np.float64(lp[b, t])
                    n[b] += 1
            cap[b] = s
    return cap, n
