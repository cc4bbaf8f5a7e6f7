"""CPU restatement of the validation metrics over token-id captions: corpus BLEU-1..4, ROUGE-L and CIDEr as
eval_utils.language_eval gets them from pycocoevalcap's Bleu(4), Rouge() and Cider(), one hypothesis per image.

A plain-Python statement of the semantics recurrent_fusion_network_amd.evalcap.LanguageEval and rewards.RougeL reproduce on the
GPU, written out from the metrics' definitions: the fuzz checker of tests/test_evalcap_gpu.py and, against the committed goldens,
the proof that the statement is right (tests/test_evalcap_cpu.py).

  - a validation caption is the ids of its row strictly BEFORE the first 0 (all ids when there is none), as
    eval_utils.decode_sequence writes it: no end token, and it may be empty.  (`end_token=True` gives the reward's convention,
    the ids up to and including the first 0, for ROUGE-L in both.)
  - BLEU: bleud_cpu's components and formula on those captions (closest reference length); the corpus four come from the sums
    of the components.  An empty caption has testlen 0 and guess 0: a score of 0 through the brevity penalty.
  - CIDEr: ciderd_cpu's arithmetic (this checkout's cider_scorer clips and has the Gaussian length penalty) with one document per
    image: df[g] = the number of images whose references hold g, ref_len = log(number of images).
  - ROUGE-L: lcs = the longest common subsequence of the caption and one reference; p = max over references of lcs / len(caption),
    q = max of lcs / len(reference); score = (1 + beta^2) p q / (q + beta^2 p) when both are non-zero, else 0; beta = 1.2.  An empty
    caption scores 0.
"""
import numpy as np

import bleud_cpu as BCPU
import ciderd_cpu as CPU

BETA = 1.2


def caption(ids, end_token=False):
    """The words of one id row: before the first 0, or (end_token) up to and including it."""
    out = []
    for x in ids:
        if int(x) == 0:
            if end_token:
                out.append(0)
            break
        out.append(int(x))
    return out


def lcs_length(a, b):
    """Length of the longest common subsequence of two word lists (the textbook table, one row at a time)."""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for k, y in enumerate(b):
            cur.append(prev[k] + 1 if x == y else max(prev[k + 1], cur[k]))
        prev = cur
    return prev[len(b)]


def rouge_l(hyp, refs, beta=BETA):
    """-> score, [lcs per reference]."""
    lcs = [lcs_length(hyp, ref) for ref in refs]
    if not hyp:
        return 0.0, lcs
    p = max(x / float(len(hyp)) for x in lcs)
    q = max(x / float(len(ref)) for x, ref in zip(lcs, refs))
    if p != 0 and q != 0:
        return ((1 + beta ** 2) * p * q) / float(q + beta ** 2 * p), lcs
    return 0.0, lcs


def _captions(res, gts, n_refs, end_token):
    res, gts = np.asarray(res), np.asarray(gts)
    hyps = [caption(row, end_token) for row in res]
    refs = [[caption(gts[i, j], end_token) for j in range(int(n_refs[i]))] for i in range(gts.shape[0])]
    return hyps, refs


def rouge_rows(res, row_img, gts, n_refs, end_token=False, beta=BETA):
    """res (N, T) ids, row_img (N,), gts (n_img, R, Tg), n_refs (n_img,) -> scores (N,) float64, lcs (N, R) int32 (0 behind an
    image's references)."""
    hyps, refs = _captions(res, gts, n_refs, end_token)
    scores = np.zeros(len(hyps))
    lcs = np.zeros((len(hyps), np.asarray(gts).shape[1]), dtype=np.int32)
    for r, i in enumerate(row_img):
        scores[r], row = rouge_l(hyps[r], refs[int(i)], beta)
        lcs[r, :len(row)] = row
    return scores, lcs


def bleu_rows(res, row_img, gts, n_refs, end_token=False):
    """-> bleu (N, 4) float64, comps (N, 10) int32, corpus (4,) float64."""
    hyps, refs = _captions(res, gts, n_refs, end_token)
    bleu = np.zeros((len(hyps), 4))
    comps = np.zeros((len(hyps), BCPU.COMPS), dtype=np.int32)
    for r, i in enumerate(row_img):
        testlen, reflen, guess, correct = BCPU.components(hyps[r], refs[int(i)])
        comps[r] = [testlen, reflen] + guess + correct
        bleu[r] = BCPU.formula(testlen, reflen, guess, correct)
    return bleu, comps, BCPU.corpus_of(comps)


def cider_rows(res, row_img, gts, n_refs, end_token=False, sigma=6.0, no_document=()):
    """Corpus-df CIDEr, one document per score row -> (N,) float64.  no_document: images whose rows add no document to the
    frequencies (an image with an unusable reference is left out of them; ref_len still counts every row)."""
    hyps, refs = _captions(res, gts, n_refs, end_token)
    df = CPU.corpus_df([i for i in row_img if int(i) not in no_document], refs)
    ref_len = np.log(float(len(row_img)))
    out = np.zeros(len(hyps))
    for r, i in enumerate(row_img):
        vh, nh, lh = CPU._vector(CPU.ngram_counts(hyps[r]), df, ref_len)
        acc = np.zeros(4)
        for ref in refs[int(i)]:
            vr, nr, lr = CPU._vector(CPU.ngram_counts(ref), df, ref_len)
            acc += CPU._pair(vh, nh, lh, vr, nr, lr, sigma)
        out[r] = np.mean(acc) / len(refs[int(i)]) * 10.0
    return out


def language_eval(seq, gts, n_refs):
    """One hypothesis row per image (seq (n_img, S), gts (n_img, R, Tg), n_refs) in the validation convention -> dict with the six
    corpus numbers and the per-image arrays (bleu, comps, rouge, lcs, cider)."""
    row_img = np.arange(len(seq), dtype=np.int32)
    bleu, comps, corpus = bleu_rows(seq, row_img, gts, n_refs)
    rouge, lcs = rouge_rows(seq, row_img, gts, n_refs)
    cider = cider_rows(seq, row_img, gts, n_refs)
    out = {'Bleu_%d' % (k + 1): float(corpus[k]) for k in range(4)}
    out.update(ROUGE_L=float(np.mean(rouge)), CIDEr=float(np.mean(cider)))
    return out, dict(bleu=bleu, comps=comps, rouge=rouge, lcs=lcs, cider=cider)
