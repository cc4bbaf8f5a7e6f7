"""CPU restatement of the caption-set diversity metrics (include/rfn.h, "caption-set diversity"): Div-m, mBLEU, Self-CIDEr and the
best-of-n / mean-of-n reduction, in NumPy fp64 on top of consensus_cpu (the pairwise utility U and the bad-input rules), bleud_cpu
(components and formula) and evalcap_cpu (the oracle's LanguageEval numbers).  The checker of tests/test_diversity_gpu.py and,
against the committed goldens (tools/make_diversity_golden.py), the proof that the statement is right (tests/test_diversity_cpu.py).

  - a caption is the ids of its row up to and including the first 0 (end_token=False: strictly before it), as everywhere;
  - an image is bad when n_cand[k] lies outside [1, n], a valid candidate holds an id outside [0, vocab] or (end_token=False) a valid
    candidate is empty: its float outputs are NaN, its integer outputs 0;
  - distinct[k][m-1] = the number of distinct m-grams over the image's valid candidates, words[k] = the sum of their word counts,
    div = distinct / (1e-6 + words);
  - mbleu[k][i] = BLEU-D (bleud_cpu) of candidate i against the image's other valid candidates; NaN behind n_cand and for
    n_cand = 1; mbleu_corpus[i] = the formula over the sums of slot i's components across the images whose row is not NaN (NaN when
    there is none); the reported mBleu_m = the mean of mbleu_corpus[:, m-1] over the slots that are not NaN;
  - K = (U + U^T) / 2 / 10 over the valid candidates; eig = its eigenvalues ascending; eigenvalues below 1e-12 * lambda_max count
    as 0; self_cider = -log(max sqrt(lambda) / sum sqrt(lambda)) / log(n_cand), NaN for n_cand = 1 or lambda_max <= 0;
  - group_stats: per image the maximum, its lowest index and the mean (ascending sum, one division) of the valid scores; one NaN
    among them gives NaN, -1, NaN.
"""
import math

import numpy as np

import bleud_cpu as BCPU
import ciderd_cpu as CPU
import consensus_cpu as CC

EIG_CUT = 1e-12


def captions_of(cands, n_cand, end_token, vocab):
    """Per image: None when it is bad, else the word lists of its valid candidates."""
    cands = np.asarray(cands)
    B, n, _ = cands.shape
    out = []
    for k in range(B):
        nc = int(n_cand[k])
        if not 1 <= nc <= n:
            out.append(None)
            continue
        caps = [CC.caption(cands[k, j], end_token) for j in range(nc)]
        bad = any(min(w, default=0) < 0 or max(w, default=0) > vocab or len(w) == 0 for w in caps)
        out.append(None if bad else caps)
    return out


def div(caps):
    """One image's word lists -> (distinct[4], words, div[4])."""
    grams = set()
    for w in caps:
        grams.update(CPU.ngram_counts(w))
    distinct = [sum(1 for g in grams if len(g) == m) for m in range(1, 5)]
    words = sum(len(w) for w in caps)
    return distinct, words, [d / (1e-6 + words) for d in distinct]


def self_cider_of(eig, nc):
    """The formula from ascending eigenvalues (what the GPU's own `eig` is run through as well)."""
    eig = [float(x) for x in eig[:nc]]
    if nc < 2 or not eig[-1] > 0.0:
        return float('nan')
    cut = EIG_CUT * eig[-1]
    s = [math.sqrt(x) for x in eig if not x < cut]
    total = 0.0
    for x in s:
        total = total + x
    return -math.log(s[-1] / total) / math.log(float(nc))


def kernel_matrix(U, nc):
    u = np.asarray(U)[:nc, :nc]
    return (u + u.T) / 2 / 10


def corpus_rows(comps, valid):
    """comps (B, n, 10), valid (B, n) bool -> (n, 4): the formula over the column sums of every slot's valid rows."""
    B, n, _ = comps.shape
    out = np.full((n, 4), np.nan)
    for i in range(n):
        rows = comps[valid[:, i], i].astype(np.int64)
        if len(rows):
            tot = [int(x) for x in rows.sum(0)]
            out[i] = BCPU.formula(tot[0], tot[1], tot[2:6], tot[6:10])
    return out


def diversity(cands, n_cand=None, df=None, ref_docs=None, sigma=6.0, end_token=False, vocab=32767):
    """cands (B, n, T) ids -> dict of distinct (B, 4) int32, words (B,) int32, div (B, 4), mbleu (B, n, 4), mbleu_comps (B, n, 10)
    int32, mbleu_corpus (n, 4), U (B, n, n), K (list of per-image matrices or None), eig (B, n), self_cider (B,), in float64."""
    cands = np.asarray(cands)
    B, n, _ = cands.shape
    n_cand = np.full(B, n, dtype=np.int32) if n_cand is None else np.asarray(n_cand)
    caps = captions_of(cands, n_cand, end_token, vocab)
    out = dict(distinct=np.zeros((B, 4), dtype=np.int32), words=np.zeros(B, dtype=np.int32), div=np.full((B, 4), np.nan),
               mbleu=np.full((B, n, 4), np.nan), mbleu_comps=np.zeros((B, n, BCPU.COMPS), dtype=np.int32),
               eig=np.full((B, n), np.nan), self_cider=np.full(B, np.nan), K=[None] * B)
    out['U'] = CC.utilities(cands, n_cand, df, ref_docs, sigma, end_token, vocab)
    valid = np.zeros((B, n), dtype=bool)
    for k in range(B):
        if caps[k] is None:
            continue
        nc = len(caps[k])
        out['distinct'][k], out['words'][k], out['div'][k] = div(caps[k])
        if nc > 1:
            for i in range(nc):
                testlen, reflen, guess, correct = BCPU.components(caps[k][i], caps[k][:i] + caps[k][i + 1:])
                out['mbleu_comps'][k, i] = [testlen, reflen] + guess + correct
                out['mbleu'][k, i] = BCPU.formula(testlen, reflen, guess, correct)
                valid[k, i] = True
        K = kernel_matrix(out['U'][k], nc)
        out['K'][k] = K
        out['eig'][k, :nc] = np.linalg.eigvalsh(K)
        out['self_cider'][k] = self_cider_of(out['eig'][k], nc)
    out['mbleu_corpus'] = corpus_rows(out['mbleu_comps'], valid)
    return out


def report(d):
    """The corpus numbers of one `diversity` result: the means over the images that are not NaN, and mBleu over the slots."""
    out = {}
    with np.errstate(invalid='ignore'):
        for m in range(4):
            out['Div_%d' % (m + 1)] = float(np.nanmean(d['div'][:, m]))
            out['mBleu_%d' % (m + 1)] = float(np.nanmean(d['mbleu_corpus'][:, m]))
        out['Self_CIDEr'] = float(np.nanmean(d['self_cider']))
    return out


def ambiguous_threshold(eig, nc):
    """True when an eigenvalue lies inside [1e-13, 1e-11] * lambda_max, where the cut is decided by the solver's rounding."""
    e = np.asarray(eig[:nc], dtype=np.float64)
    top = e[-1]
    return bool(top > 0 and np.any((e >= 1e-13 * top) & (e <= 1e-11 * top)))


def group_stats(scores, n, n_cand=None, stride=1):
    """scores: flat, entry (k * n + j) * stride -> (best (B,), arg (B,) int64, mean (B,))."""
    col = np.asarray(scores, dtype=np.float64).reshape(-1)[::stride]
    B = len(col) // n
    col = col[:B * n].reshape(B, n)
    n_cand = np.full(B, n) if n_cand is None else np.asarray(n_cand)
    best, arg, mean = np.full(B, np.nan), np.full(B, -1, dtype=np.int64), np.full(B, np.nan)
    for k in range(B):
        nc = int(n_cand[k])
        if not 1 <= nc <= n or np.isnan(col[k, :nc]).any():
            continue
        arg[k] = int(np.argmax(col[k, :nc]))
        best[k] = col[k, arg[k]]
        total = 0.0
        for j in range(nc):
            total = total + float(col[k, j])
        mean[k] = total / float(nc)
    return best, arg, mean
