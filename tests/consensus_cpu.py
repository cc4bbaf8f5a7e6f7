"""CPU restatement of consensus (minimum-Bayes-risk) reranking under CIDEr-D (include/rfn.h, "consensus reranking").

Plain numpy / Python floats on top of ciderd_cpu's `_vector` and `_pair`: the pairwise utility U, the weighted leave-one-out
consensus score, the pick and the bad-input rules.  The checker of tests/test_consensus_gpu.py and, against the committed
goldens (tools/make_consensus_golden.py), the proof that the statement is right (tests/test_consensus_cpu.py).

  - a caption is the ids of its row up to and including the first 0 (end_token=False: strictly before it);
  - U[k][i][j] = CIDEr-D of candidate i of image k against the single reference candidate j: ((((0 + s0) + s1) + s2) + s3) / 4 * 10
    with s_n the per-order term of ciderd_cpu._pair;
  - corpus df (df=None): a document is an image; df(g) = the sum of n_cand[k] over the images whose valid candidates hold g,
    ref_docs = the sum of all n_cand[k] -- what ciderd_cpu.score_rows computes for the compacted candidates as res and gts;
  - c[k][i] = (sum_{j != i} w_j U[k][i][j]) / (sum_{j != i} w_j) over the valid j, ascending; 0 when the weight sum is 0;
  - best[k] = the lowest i whose c[k][i] is the maximum;
  - an id outside [0, vocab] in a valid candidate, a negative or NaN weight on one, n_cand[k] outside [1, n] or (end_token=False)
    an empty valid candidate: the image's c and U are NaN and its best is -1.  Entries at or beyond n_cand[k] are NaN.
"""
import numpy as np

import ciderd_cpu as CPU


def caption(ids, end_token=True):
    words = CPU.caption(ids)
    if not end_token and words and words[-1] == 0:
        words = words[:-1]
    return words


def _counts(cands, n_cand, end_token, vocab):
    """Per image: None when a valid candidate is bad (or n_cand is out of range), else the n-gram counts of its valid candidates;
    and the count's range check per image."""
    B, n, _ = cands.shape
    out, in_range = [], []
    for k in range(B):
        nc = int(n_cand[k])
        in_range.append(1 <= nc <= n)
        if not in_range[-1]:
            out.append(None)
            continue
        caps = [caption(cands[k, j], end_token) for j in range(nc)]
        if any(min(w, default=0) < 0 or max(w, default=0) > vocab or len(w) == 0 for w in caps):
            out.append(None)
            continue
        out.append([CPU.ngram_counts(w) for w in caps])
    return out, in_range


def utilities(cands, n_cand=None, df=None, ref_docs=None, sigma=6.0, end_token=True, vocab=32767):
    """cands (B, n, T) ids -> U (B, n, n) float64 (NaN for a bad image and at or beyond n_cand)."""
    cands = np.asarray(cands)
    B, n, _ = cands.shape
    n_cand = np.full(B, n) if n_cand is None else np.asarray(n_cand)
    counts, in_range = _counts(cands, n_cand, end_token, vocab)
    if df is None:
        df = {}
        for k in range(B):
            if counts[k] is None:
                continue
            for g in set().union(*counts[k]):
                df[g] = df.get(g, 0.0) + float(n_cand[k])
        ref_docs = sum(int(n_cand[k]) for k in range(B) if in_range[k])
    ref_len = np.log(float(ref_docs)) if ref_docs > 0 else -np.inf
    U = np.full((B, n, n), np.nan)
    for k in range(B):
        if counts[k] is None:
            continue
        vecs = [CPU._vector(c, df, ref_len) for c in counts[k]]
        for i, (vh, nh, lh) in enumerate(vecs):
            for j, (vr, nr, lr) in enumerate(vecs):
                s = CPU._pair(vh, nh, lh, vr, nr, lr, sigma)
                U[k, i, j] = ((((0.0 + s[0]) + s[1]) + s[2]) + s[3]) / 4.0 * 10.0
    return U


def consensus(cands, n_cand=None, weights=None, df=None, ref_docs=None, sigma=6.0, end_token=True, vocab=32767):
    """-> (best (B,) int64, c (B, n) float64, U (B, n, n) float64)."""
    cands = np.asarray(cands)
    B, n, _ = cands.shape
    n_cand = np.full(B, n) if n_cand is None else np.asarray(n_cand)
    U = utilities(cands, n_cand, df, ref_docs, sigma, end_token, vocab)
    c = np.full((B, n), np.nan)
    best = np.full(B, -1, dtype=np.int64)
    for k in range(B):
        nc = int(n_cand[k])
        if not 1 <= nc <= n or np.isnan(U[k, 0, 0]):
            continue
        w = np.ones(nc) if weights is None else np.asarray(weights, dtype=np.float64)[k, :nc]
        if not np.all(w >= 0.0):          # negative or NaN
            U[k] = np.nan
            continue
        for i in range(nc):
            num, den = 0.0, 0.0
            for j in range(nc):
                if j != i:
                    num = num + float(w[j]) * float(U[k, i, j])
                    den = den + float(w[j])
            c[k, i] = 0.0 if den == 0.0 else num / den
        best[k] = int(np.argmax(c[k, :nc]))   # the first maximum
    return best, c, U


def compact(cands, n_cand):
    """The valid candidates as score rows -> (res (sum n_cand, T), row_img)."""
    cands = np.asarray(cands)
    rows = [cands[k, j] for k in range(cands.shape[0]) for j in range(int(n_cand[k]))]
    img = [k for k in range(cands.shape[0]) for _ in range(int(n_cand[k]))]
    return np.array(rows, dtype=np.int64), np.array(img, dtype=np.int32)


def min_relative_gap(c, cands, n_cand):
    """Per image the gap between the best score and the best score of a candidate whose caption differs from the best's, relative
    to max(1, |best score|) (inf when every candidate is the same caption)."""
    out = []
    for k in range(c.shape[0]):
        nc = int(n_cand[k])
        b = int(np.argmax(c[k, :nc]))
        cap = CPU.caption(cands[k, b])
        others = [c[k, i] for i in range(nc) if CPU.caption(cands[k, i]) != cap]
        out.append((c[k, b] - max(others)) / max(1.0, abs(c[k, b])) if others else np.inf)
    return np.array(out)
