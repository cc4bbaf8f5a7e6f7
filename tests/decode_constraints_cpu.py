"""NumPy / plain-Python restatement of the decoding constraints (include/rfn.h, "decoding constraints"): what
rfn_decode_blocklist lists, what the masked log-prob row looks like, and how length_penalty orders done beams.

history: the tokens a row has emitted so far (BOS excluded); step t >= 1 picks the t-th token, so len(history) == t - 1.
"""
import numpy as np


def blocked_ids(history, t, n=0, banned=(), bad_endings=()):
    """The row's block list at step t, in the order the kernel writes it: banned ids (ascending), the continuations of
    earlier occurrences of the history's last n - 1 tokens (history order, duplicates kept), then 0 after a bad ending.
    A finished row (last token 0) is left alone."""
    h = [int(x) for x in history]
    assert len(h) == t - 1
    if h and h[-1] == 0:
        return []
    out = sorted(int(b) for b in banned)
    if n >= 2 and t >= n:
        g = h[len(h) - (n - 1):]
        for j in range(len(h)):
            if j + n - 1 < len(h) and h[j:j + n - 1] == g and h[j + n - 1] != 0:
                out.append(h[j + n - 1])
    if h and h[-1] in set(int(b) for b in bad_endings):
        out.append(0)
    return out


def mask_rows(logp, histories, t, n=0, banned=(), bad_endings=()):
    """logp (rows, V1) with every row's blocked entries set to -inf (a copy); nothing is renormalised."""
    out = np.array(logp, copy=True)
    for r, h in enumerate(histories):
        ids = blocked_ids(h, t, n, banned, bad_endings)
        if ids:
            out[r, ids] = -np.inf
    return out


def caption_len(seq, S):
    """Tokens up to and including the first 0, or S without one."""
    s = [int(x) for x in seq][:S]
    return s.index(0) + 1 if 0 in s else S


def rank_done(ps, lens, alpha):
    """Order of the done beams: by p / len^alpha descending, ties in construction order (stable).  p is the fp32 sum,
    the quotient one fp64 division."""
    score = [float(np.float64(np.float32(p)) / np.float64(float(n) ** float(alpha))) if alpha else float(np.float32(p))
             for p, n in zip(ps, lens)]
    return sorted(range(len(score)), key=lambda i: -score[i])


def has_repeated_ngram(seq, n):
    """True if the caption (tokens before its first 0) holds the same n-gram twice."""
    s = [int(x) for x in seq]
    if 0 in s:
        s = s[:s.index(0)]
    grams = [tuple(s[i:i + n]) for i in range(len(s) - n + 1)]
    return len(grams) != len(set(grams))
