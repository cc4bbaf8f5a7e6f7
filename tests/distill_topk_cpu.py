"""The compact-teacher distillation of rfn_kd_topk_fwd / _bwd (include/rfn.h) restated in float64 NumPy.  A teacher row is K
(id, value) pairs; its meaning is the dense row z with z[id_k] = val_k and -inf everywhere else, so the restatement builds that
row and calls distill_cpu.kd_reference.  An entry whose id is outside [0, V1) or whose value is -inf is padding.  Also here:
the top-k selection in the order rfn_log_softmax_topk lists it (value descending, token ascending), and the rule by which a
loader turns a caption into labels and masks (what decode.labels_from_seq computes on the device)."""
import numpy as np

import distill_cpu as D


def live_entries(ids, val, V1):
    ids, val = np.asarray(ids), np.asarray(val)
    return (ids >= 0) & (ids < V1) & ~np.isneginf(val)        # a NaN value on a live id is live (and the caller's error)


def dense_rows(ids, val, V1):
    """ids, val (B, T, K) -> z (B, T, V1) float64: val at the live ids, -inf elsewhere.  Live ids of a row are distinct."""
    ids, val = np.asarray(ids).astype(np.int64), np.asarray(val, dtype=np.float64)
    B, T, K = ids.shape
    z = np.full((B, T, V1), -np.inf)
    live = live_entries(ids, val, V1)
    for b in range(B):
        for t in range(T):
            row = ids[b, t][live[b, t]]
            assert len(set(row.tolist())) == len(row), 'duplicate live ids in row (%d, %d)' % (b, t)
            z[b, t, row] = val[b, t][live[b, t]]
    return z


def kd_topk_reference(x, ids, val, target, mask, eps, alpha, it, g=1.0):
    """As distill_cpu.kd_reference, the teacher given as (ids, val) (B, T, K).  The teacher entries of rows with mask == 0 are
    never looked at (they may hold NaN and any ids): such rows get a harmless row before the dense restatement runs.
    stats[2] of such a row is 0."""
    x = np.asarray(x, dtype=np.float64)
    V1 = x.shape[2]
    m = np.asarray(mask, dtype=np.float64)
    ids, val = np.array(ids, dtype=np.int64), np.array(val, dtype=np.float64)
    ids[m == 0], val[m == 0] = 0, -np.inf
    ids[m == 0, 0], val[m == 0, 0] = 0, 0.0
    ref = D.kd_reference(x, dense_rows(ids, val, V1), target, mask, eps, alpha, it, g)
    ref['stats'][2][m == 0] = 0.0
    return ref


def topk_rows(x, k):
    """x (..., V1) -> (ids (..., k) int64, logp (..., k) float64): the k best entries of log_softmax(x), ordered by (value
    descending, token ascending) on the values of x themselves -- x - lse is monotone in x, which is how the kernel's float32
    log-probs keep the order and the ties of the logits."""
    x = np.asarray(x)
    order = np.lexsort((np.broadcast_to(np.arange(x.shape[-1]), x.shape), -x.astype(np.float64)), axis=-1)[..., :k]
    x64 = x.astype(np.float64)
    lp = x64 - D._lse(x64)[..., None]
    return order.astype(np.int64), np.take_along_axis(lp, order, axis=-1)


def labels_masks(seq, seq_length=None):
    """The loader's rule, one caption at a time: seq (B, S') ids -> labels (B, S + 2) int64 with the caption's words before its
    first 0 in columns 1 .. n, masks (B, S + 2) float32 with ones over the first n + 2 columns (BOS, the words, END)."""
    seq = np.asarray(seq)
    B, Sp = seq.shape
    S = Sp if seq_length is None else seq_length
    labels, masks = np.zeros((B, S + 2), dtype=np.int64), np.zeros((B, S + 2), dtype=np.float32)
    for i in range(B):
        n = 0
        while n < Sp and seq[i, n] != 0:
            n += 1
        labels[i, 1:n + 1] = seq[i, :n]
        masks[i, :n + 2] = 1.0
    return labels, masks
