"""CPU restatement of CIDEr-D (n = 4) over token-id captions, as the self-critical reward uses it.

A plain-numpy statement of the semantics recurrent_fusion_network_amd.rewards reproduces on the GPU, written out
from the metric's definition: the fuzz checker of tests/test_ciderd_gpu.py and, against the committed goldens, the
proof that the statement is right (tests/test_ciderd_cpu.py).

  - a caption is the ids of its row up to and including the first 0 (all ids when there is none);
  - n-grams n = 1..4 with their counts; an n-gram's weight is count * (ref_len - log(max(1, df)));
  - a caption's "length" is its number of bigrams;
  - per n: sum over the hypothesis n-grams of min(w_h, w_r) * w_r (w_r = 0 when the reference lacks it), divided by
    |h| |r| when both norms are non-zero, times exp(-(len_h - len_r)^2 / (2 sigma^2));
  - score = 10 * mean over n of the sum over references, divided by the image's number of references.
"""
import math

import numpy as np

LOG_COCO = {'coco-all': 123287, 'coco-train': 113287, 'coco-val': 5000}


def caption(ids):
    """The words of one id row: up to and including the first 0."""
    out = []
    for x in ids:
        out.append(int(x))
        if int(x) == 0:
            break
    return out


def ngram_counts(words):
    c = {}
    for n in range(1, 5):
        for p in range(len(words) - n + 1):
            g = tuple(words[p:p + n])
            c[g] = c.get(g, 0) + 1
    return c


def corpus_df(row_img, refs_of_image):
    """df[g] = number of score rows whose image's references contain g."""
    df = {}
    for i in row_img:
        seen = set()
        for ref in refs_of_image[int(i)]:
            seen.update(ngram_counts(ref))
        for g in seen:
            df[g] = df.get(g, 0.0) + 1.0
    return df


def _vector(counts, df, ref_len):
    vec = [dict() for _ in range(4)]
    norm = [0.0] * 4
    length = 0
    for g, tf in counts.items():
        n = len(g) - 1
        w = float(tf) * (ref_len - np.log(max(1.0, df.get(g, 0.0))))
        vec[n][g] = w
        norm[n] += w * w
        if n == 1:
            length += tf
    return vec, [math.sqrt(x) for x in norm], length


def _pair(vh, nh, lh, vr, nr, lr, sigma):
    out = np.zeros(4)
    pen = math.exp(-float(lh - lr) ** 2 / (2.0 * sigma * sigma))
    for n in range(4):
        s = 0.0
        for g, w in vh[n].items():
            wr = vr[n].get(g, 0.0)
            s += min(w, wr) * wr
        if nh[n] != 0 and nr[n] != 0:
            s /= nh[n] * nr[n]
        out[n] = s * pen
    return out


def score_rows(res, row_img, gts, n_refs, df=None, ref_docs=None, sigma=6.0):
    """res (N, T) ids, row_img (N,), gts (n_img, R, Tg), n_refs (n_img,); df None = corpus mode, else a dict of
    id-tuples -> df with ref_docs documents.  -> (N,) float64."""
    res, gts = np.asarray(res), np.asarray(gts)
    refs = [[caption(gts[i, j]) for j in range(int(n_refs[i]))] for i in range(gts.shape[0])]
    if df is None:
        df = corpus_df(row_img, refs)
        ref_docs = len(row_img)
    ref_len = np.log(float(ref_docs))
    ref_vecs = {}
    out = np.zeros(len(row_img))
    for r, i in enumerate(row_img):
        i = int(i)
        if i not in ref_vecs:
            ref_vecs[i] = [_vector(ngram_counts(ref), df, ref_len) for ref in refs[i]]
        vh, nh, lh = _vector(ngram_counts(caption(res[r])), df, ref_len)
        acc = np.zeros(4)
        for vr, nr, lr in ref_vecs[i]:
            acc += _pair(vh, nh, lh, vr, nr, lr, sigma)
        out[r] = np.mean(acc) / len(refs[i]) * 10.0
    return out


def scst_rows(B, seq_per_img):
    """row_img of compute_reward's 2B score rows: the sampled rows, then the greedy rows."""
    return np.array([(r % B) // seq_per_img for r in range(2 * B)], dtype=np.int32)


def reward(scores, B, T, weight=1.0, use_baseline=True):
    s = scores[:B] - scores[B:] if use_baseline else scores[:B]
    return np.repeat(((0.0 + s * weight) + 0.0)[:, None], T, 1)


def pad_gts(gts_list):
    """list of (n_i, T) id arrays -> (n_img, max n_i, T) int64 padded with 0, n_refs (int32)."""
    n = np.array([len(g) for g in gts_list], dtype=np.int32)
    T = max(np.asarray(g).shape[1] for g in gts_list)
    out = np.zeros((len(gts_list), int(n.max()), T), dtype=np.int64)
    for i, g in enumerate(gts_list):
        g = np.asarray(g)
        out[i, :g.shape[0], :g.shape[1]] = g
    return out, n


def df_from_arrays(ids, counts):
    """(n, 4) int ids padded with -1, (n,) counts -> dict of id tuples."""
    return {tuple(int(x) for x in row if x >= 0): float(c) for row, c in zip(ids, counts)}
