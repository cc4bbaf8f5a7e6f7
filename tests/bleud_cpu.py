"""CPU restatement of BLEU-D (n = 4, closest reference length) over token-id captions, as the self-critical reward uses it.

A plain-Python statement of the semantics recurrent_fusion_network_amd.rewards.BleuD reproduces on the GPU, written out
from the metric's definition: the fuzz checker of tests/test_bleud_gpu.py and, against the committed goldens, the proof
that the statement is right (tests/test_bleud_cpu.py).

  - a caption is the ids of its row up to and including the first 0 (all ids when there is none); testlen is its word count;
  - guess[n] = max(0, testlen - n + 1); correct[n] = sum over the caption's distinct n-grams of min(its count, the largest
    count of that n-gram in any one reference of the image);
  - reflen is the reference length closest to testlen, the shorter one on a tie;
  - p = 1; for k in 0..3: p *= (correct[k] + 1e-15) / (guess[k] + 1e-9); bleu[k] = p ** (1 / (k + 1)); when
    (testlen + 1e-15) / (reflen + 1e-9) < 1 every bleu[k] is multiplied by exp(1 - 1 / ratio);
  - the corpus-level four: the same formula over the sums of the rows' components.
"""
import math

import numpy as np

from ciderd_cpu import caption, ngram_counts

COMPS = 10   # testlen, reflen, guess[4], correct[4]


def components(hyp, refs):
    """hyp: the words of one caption, refs: the word lists of its image's references -> (testlen, reflen, guess, correct)."""
    testlen = len(hyp)
    most = {}
    for ref in refs:
        for g, c in ngram_counts(ref).items():
            most[g] = max(most.get(g, 0), c)
    correct = [0] * 4
    for g, c in ngram_counts(hyp).items():
        correct[len(g) - 1] += min(c, most.get(g, 0))
    guess = [max(0, testlen - n + 1) for n in range(1, 5)]
    reflen = min((abs(len(ref) - testlen), len(ref)) for ref in refs)[1]
    return testlen, reflen, guess, correct


def formula(testlen, reflen, guess, correct):
    out = []
    p = 1.0
    for k in range(4):
        p *= (float(correct[k]) + 1e-15) / (float(guess[k]) + 1e-9)
        out.append(p ** (1.0 / (k + 1)))
    ratio = (testlen + 1e-15) / (reflen + 1e-9)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


def score_rows(res, row_img, gts, n_refs):
    """res (N, T) ids, row_img (N,), gts (n_img, R, Tg), n_refs (n_img,) -> bleu (N, 4) float64, comps (N, 10) int32,
    corpus (4,) float64."""
    res, gts = np.asarray(res), np.asarray(gts)
    refs = [[caption(gts[i, j]) for j in range(int(n_refs[i]))] for i in range(gts.shape[0])]
    bleu = np.zeros((len(row_img), 4))
    comps = np.zeros((len(row_img), COMPS), dtype=np.int32)
    for r, i in enumerate(row_img):
        testlen, reflen, guess, correct = components(caption(res[r]), refs[int(i)])
        comps[r] = [testlen, reflen] + guess + correct
        bleu[r] = formula(testlen, reflen, guess, correct)
    return bleu, comps, corpus_of(comps)


def corpus_of(comps):
    tot = [int(x) for x in np.asarray(comps, dtype=np.int64).sum(0)]
    return np.array(formula(tot[0], tot[1], tot[2:6], tot[6:10]))


def mix(bleu, cider, B, T, bleu4_weight, cider_weight, use_baseline=True):
    """compute_reward's bleu4 * w_b + cider * w_c + spice * 0 over the B sampled rows followed by the B greedy rows (a
    missing term is the array of zeros the reference uses) -> (B, T) float64."""
    b4 = np.zeros(2 * B) if bleu is None else np.asarray(bleu)[:, 3]
    c = np.zeros(2 * B) if cider is None else np.asarray(cider)
    if use_baseline:
        b4, c = b4[:B] - b4[B:], c[:B] - c[B:]
    else:
        b4, c = b4[:B], c[:B]
    s = b4 * bleu4_weight + c * cider_weight + np.zeros(B) * 0
    return np.repeat(s[:, None], T, 1)
