"""Inputs that the validation-metric tests, tools/make_evalcap_golden.py and tools/bench_reward.py share: a validation split of
one hypothesis per image whose captions resemble their references (so that 3- and 4-grams match and the LCS is long), the
hand-written edge tiers, and fuzzed cases in the validation convention."""
import types

import numpy as np


def val_split(seed, n_img, refs_lo=5, refs_hi=5, T=16, vocab=9487):
    """-> seq (n_img, T), gts (n_img, refs_hi, T), n_refs (n_img,) int32, vocab.  Every image draws its words from a pool of 18
    (12 of them from 40 words common to the split); a reference is 4 .. T-1 pool words and a 0, or (one in ten) T words without
    one; the hypothesis is one of the image's references with words substituted (p = 0.15), then truncated, or one word repeated,
    or pool words appended; one in eight is random pool words instead.  Ids behind a row's 0 are noise that is never read."""
    rng = np.random.default_rng(seed)
    common = rng.integers(1, vocab + 1, 40)
    n_refs = rng.integers(refs_lo, refs_hi + 1, n_img).astype(np.int32)
    gts = np.zeros((n_img, refs_hi, T), dtype=np.int64)
    seq = np.zeros((n_img, T), dtype=np.int64)

    def put(row, body):
        body = body[:T]
        row[:len(body)] = body
        if len(body) < T:
            row[len(body)] = 0
            row[len(body) + 1:] = rng.integers(1, vocab + 1, T - len(body) - 1)
    for i in range(n_img):
        pool = np.concatenate([rng.choice(common, 12), rng.integers(1, vocab + 1, 6)])
        bodies = []
        for j in range(int(n_refs[i])):
            L = T if rng.random() < 0.1 else int(rng.integers(4, T))
            bodies.append([int(x) for x in rng.choice(pool, L)])
            put(gts[i, j], bodies[-1])
        if rng.random() < 0.125:
            body = [int(x) for x in rng.choice(pool, int(rng.integers(1, T)))]
        else:
            body = [int(rng.choice(pool)) if rng.random() < 0.15 else w for w in bodies[int(rng.integers(0, len(bodies)))]]
            u = rng.random()
            if u < 0.25:
                body = body[:int(rng.integers(1, len(body)))]
            elif u < 0.4:
                p = int(rng.integers(0, len(body)))
                body = body[:p] + [body[p]] * int(rng.integers(2, 5)) + body[p:]
            elif u < 0.5:
                body = body + [int(x) for x in rng.choice(pool, int(rng.integers(1, 4)))]
        put(seq[i], body)
    return seq, gts, n_refs, vocab


def edge_tier():
    """-> res (7, 8), gts (7, 7, 8), n_refs, vocab: one hypothesis per image."""
    T = 8
    z = [0] * T
    refs = [
        [[4, 5, 6, 0] + z[:4]],
        [[4, 5, 6, 7, 8, 9, 10, 11], [4, 5, 0, 9, 9, 9, 9, 9], [3, 3, 3, 3, 0, 0, 0, 0], [7, 0, 7, 7, 7, 7, 7, 7],
         [1, 2, 3, 4, 5, 6, 7, 0], [5, 6, 7, 8, 9, 10, 11, 12], [11, 10, 9, 8, 7, 6, 5, 4]],
        [[2, 2, 2, 2, 2, 2, 2, 2], [2, 2, 0] + z[:5], [6, 2, 2, 0] + z[:4]],
        [[3, 1, 0] + z[:5], [1, 0] + z[:6]],
        [[13, 14, 15, 16, 0] + z[:3], [13, 14, 15, 16, 17, 18, 19, 20], [14, 15, 0] + z[:5], [16, 13, 0] + z[:5],
         [20, 19, 18, 17, 16, 15, 14, 13]],
        [[9, 8, 7, 0] + z[:4], [9, 8, 7, 9, 8, 7, 0, 0], [9, 0] + z[:6], [8, 7, 9, 8, 7, 9, 8, 7]],
        [[13, 14, 15, 0] + z[:4], [4, 5, 0] + z[:5]],
    ]
    res = [[0] + [5] * (T - 1),               # an empty hypothesis (the ids behind the 0 are not read)
           [4, 5, 6, 7, 8, 9, 10, 11],         # full width, no 0, equal to a reference
           [2, 2, 2, 2, 2, 2, 0, 3],           # one word repeated
           [1, 0] + z[:6],                     # a single token, equal to a reference
           [13, 14, 15, 16, 0] + z[:3],        # equal to a reference
           [7, 8, 9, 7, 8, 9, 0, 1],           # a common subsequence that is no common substring
           [21, 22, 23, 0] + z[:4]]            # nothing in common
    n_refs = np.array([len(r) for r in refs], dtype=np.int32)
    gts = np.zeros((len(refs), int(n_refs.max()), T), dtype=np.int64)
    for i, rs in enumerate(refs):
        gts[i, :len(rs)] = np.array(rs)
    return np.array(res, dtype=np.int64), gts, n_refs, 23


def edge1_tier():
    """n_img = 1 (CIDEr's ref_len = log(1) = 0: every weight, and the score, is 0)."""
    gts = np.array([[[5, 6, 7, 8, 0, 0], [6, 7, 9, 0, 0, 0], [8, 7, 6, 5, 4, 3]]], dtype=np.int64)
    return np.array([[5, 6, 9, 8, 7, 0]], dtype=np.int64), gts, np.array([3], dtype=np.int32), 9


def fuzz_case(seed):
    """reward_cases.fuzz_case's shapes with references that are never empty in either caption convention (id 0 only behind the
    first word)."""
    from reward_cases import fuzz_case as base
    f = base(4000, seed)
    rng = np.random.default_rng(5000 + seed)
    for i in range(f.n_img):
        for j in range(int(f.n_refs[i])):
            if f.gts[i, j, 0] == 0:
                f.gts[i, j, 0] = int(rng.integers(1, f.vocab + 1))
    return types.SimpleNamespace(**vars(f))
