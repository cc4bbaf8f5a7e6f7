"""NumPy fp64 restatement of stochastic beam search as include/rfn.h defines it ("stochastic beam search"; Kool, van Hoof, Welling,
ICML 2019, "Stochastic beams and where to find them").  Written from that text, not from the device code.  The step reads FULL
log-prob rows: that the rows' W best keys suffice is a claim of the definition which the device tests check against this.

    root       row 0 of an image starts live with phi = 0 and G = the draw e of (r = k * W, v = 0, t = 0); the other rows are dead
    noise      n = Philox4x32-10(key = seed, counter = (r * V1 + v, offset0 + t)) word 0 >> 8;  u = (n + 0.5) / 2^24;  e = -ln(-ln u)
    candidate  key = double(x_v) + e;  gamma = phi_j + key;  Z_j = max gamma;  phi' = phi_j + double(x_v)
               d = G_j - gamma + log1mexp(gamma - Z_j);  G' = G_j - max(0, d) - log1p(exp(-|d|));  the argmax child: G' = G_j
    finished   a live row whose last token is 0 is carried as the single candidate "itself"
    selection  the min(W, candidates) largest G', ties by source row, then token; the rest of the rows are dead
    weights    kappa = G of the last live row; weight = exp(phi) / -expm1(-exp(phi - kappa)) before it, 0 for it and the dead rows
"""
import numpy as np

import philox_cpu as P

INF = float('inf')
_M32 = np.uint64(0xFFFFFFFF)


def gumbels(seed, offset, rows, V1):
    """e[i, v] for the global rows `rows` (any integer array) and tokens v < V1 at counter offset `offset` -> (len(rows), V1) f64."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1)
    idx = rows[:, None] * np.uint64(V1) + np.arange(V1, dtype=np.uint64)[None, :]
    ctr = np.stack([idx & _M32, idx >> np.uint64(32), np.full_like(idx, offset & 0xFFFFFFFF), np.full_like(idx, offset >> 32)], -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    n = (P.philox4x32_10(ctr, key)[..., 0] >> np.uint32(8)).astype(np.float64)
    u = (n + 0.5) / 2.0 ** 24
    return -np.log(-np.log(u))


def root_gumbel(seed, offset0, k, W, V1):
    """The G of image k's root: the draw of (row k * W, token 0) at step 0."""
    return float(gumbels(seed, offset0, [k * W], V1)[0, 0])


def candidates_of(x):
    """Tokens of a log-prob row that may be chosen: every entry that is neither -inf nor NaN."""
    x = np.asarray(x)
    return ~(np.isnan(x) | (x == -INF))


def row_list(x, e, W):
    """The W best candidates of one row by key = double(x) + e (descending, token ascending) -> (keys (W,) f64, x values (W,) f32,
    tokens (W,) int32, gap): short lists are filled with (-inf, -inf, 0); gap = the smallest difference between neighbouring keys
    of the list down to the first rejected one (inf when there is no neighbour)."""
    x = np.asarray(x, dtype=np.float32)
    v = np.nonzero(candidates_of(x))[0]
    keys = x[v].astype(np.float64) + e[v]
    o = np.lexsort((v, -keys))
    v, keys = v[o], keys[o]
    m = min(W, v.size)
    tk, tv, ti = np.full(W, -INF), np.full(W, -INF, dtype=np.float32), np.zeros(W, dtype=np.int32)
    tk[:m], tv[:m], ti[:m] = keys[:m], x[v[:m]], v[:m]
    head = keys[:W + 1]
    gap = float(np.min(head[:-1] - head[1:])) if head.size > 1 else INF
    return tk, tv, ti, gap


def log1mexp(a):
    """ln(1 - exp(a)) for a <= 0; -inf at 0."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide='ignore'):
        return np.where(a > -np.log(2.0), np.log(-np.expm1(a)), np.log1p(-np.exp(a)))


def child_g(G, gamma, Z):
    d = G - gamma + log1mexp(gamma - Z)
    return G - np.maximum(0.0, d) - np.log1p(np.exp(-np.abs(d)))


class Beams:
    """The state of one image."""

    def __init__(self, W, S, g_root=0.0):
        """g_root: the root's G -- root_gumbel() for a search whose weights are to mean anything; any constant draws the same
        captions."""
        self.W, self.S = W, S
        self.seq, self.lp = np.zeros((W, S), dtype=np.int64), np.zeros((W, S), dtype=np.float32)
        self.phi, self.G = np.full(W, -INF), np.full(W, -INF)
        self.live, self.fin = np.zeros(W, dtype=bool), np.zeros(W, dtype=bool)
        self.live[0], self.phi[0], self.G[0] = True, 0.0, g_root
        self.order, self.next_ids = np.arange(W), np.zeros(W, dtype=np.int64)
        self.events = set()           # 'fin_survives', 'fin_displaced', 'dead': what a test asserts it has seen
        self.parents = None           # per new row of the last step: (parent's G, is the parent's argmax child)


def step(b, x, e, t):
    """Step t (1-based) of one image.  x (W, V1) fp32 log-prob rows (blocked tokens -inf), e (W, V1) f64 noise of this step."""
    W = b.W
    cG, cphi, crow, ctok, clp, cpar, carg = [], [], [], [], [], [], []
    for j in range(W):
        if not b.live[j]:
            continue
        if b.fin[j]:
            cG.append([b.G[j]]), cphi.append([b.phi[j]]), crow.append([j]), ctok.append([0]), clp.append(np.zeros(1, np.float32))
            cpar.append([b.G[j]]), carg.append([True])
            continue
        xj = np.asarray(x[j], dtype=np.float32)
        v = np.nonzero(candidates_of(xj))[0]
        if v.size == 0:
            continue
        xd = xj[v].astype(np.float64)
        key = xd + e[j][v]
        gamma = b.phi[j] + key
        first = np.lexsort((v, -key))[0]                     # the argmax child
        g = child_g(b.G[j], gamma, gamma[first])
        g[first] = b.G[j]
        arg = np.zeros(v.size, dtype=bool)
        arg[first] = True
        cG.append(g), cphi.append(b.phi[j] + xd), crow.append(np.full(v.size, j)), ctok.append(v), clp.append(xj[v])
        cpar.append(np.full(v.size, b.G[j])), carg.append(arg)
    seq, lp = np.zeros_like(b.seq), np.zeros_like(b.lp)
    phi, G = np.full(W, -INF), np.full(W, -INF)
    live, fin = np.zeros(W, dtype=bool), np.zeros(W, dtype=bool)
    order, nxt = np.arange(W), np.zeros(W, dtype=np.int64)
    b.parents = []
    if cG:
        cG, cphi, crow, ctok, clp, cpar, carg = (np.concatenate(a) for a in (cG, cphi, crow, ctok, clp, cpar, carg))
        o = np.lexsort((ctok, crow, -cG))[:W]
        for i, c in enumerate(o):
            q = crow[c]
            seq[i, :t - 1], lp[i, :t - 1] = b.seq[q, :t - 1], b.lp[q, :t - 1]
            seq[i, t - 1], lp[i, t - 1] = ctok[c], clp[c]
            phi[i], G[i], live[i], fin[i] = cphi[c], cG[c], True, ctok[c] == 0
            order[i], nxt[i] = q, ctok[c]
            b.parents.append((cpar[c], bool(carg[c])))
        kept = set(int(crow[c]) for c in o if b.fin[crow[c]])
        for j in range(W):
            if b.live[j] and b.fin[j]:
                b.events.add('fin_survives' if j in kept else 'fin_displaced')
    if not live.all():
        b.events.add('dead')
    b.seq, b.lp, b.phi, b.G, b.live, b.fin, b.order, b.next_ids = seq, lp, phi, G, live, fin, order, nxt


def weights(b):
    """-> (weight (W,) f64, n_live) after the last step."""
    n = int(b.live.sum())
    w = np.zeros(b.W)
    if n >= 2:
        kappa = b.G[n - 1]
        with np.errstate(all='ignore'):
            w[:n - 1] = np.exp(b.phi[:n - 1]) / -np.expm1(-np.exp(b.phi[:n - 1] - kappa))
    return w, n


def search(x_of, W, S, seed, offset0, k, V1):
    """A whole search of image k: x_of(t, beams) -> (W, V1) fp32 log-prob rows of step t.  -> Beams."""
    b = Beams(W, S, root_gumbel(seed, offset0, k, W, V1))
    for t in range(1, S + 1):
        step(b, x_of(t, b), gumbels(seed, offset0 + t, k * W + np.arange(W), V1), t)
    return b


# ---- a small Markov model over 4 tokens (0 = END): every test that needs a distribution it can enumerate uses this one ----------
MARKOV_V1 = 4


def markov_rows():
    """(first (4,), trans (4, 4)) fp32 LOG-prob rows: first[v] for the first token, trans[u, v] after token u != 0.  The values are
    fp32 first, and the probabilities the tests enumerate are exp of those fp32 values, renormalised by nothing: the rows are built
    so that they sum to 1 within fp32 rounding."""
    p0 = np.array([0.10, 0.45, 0.30, 0.15])
    pt = np.array([[0.25, 0.25, 0.25, 0.25], [0.20, 0.10, 0.50, 0.20], [0.35, 0.30, 0.05, 0.30], [0.15, 0.40, 0.25, 0.20]])
    return np.log(p0).astype(np.float32), np.log(pt).astype(np.float32)


def markov_x(first, trans, t, b):
    """The log-prob rows of step t for the beams b: a row depends on its last token only."""
    if t == 1:
        return np.tile(first, (b.W, 1))
    return trans[b.seq[:, t - 2]]


def markov_captions(first, trans, S):
    """Every caption of at most S tokens (END-terminated, or S tokens long) with its probability, in fp64 from the fp32 rows,
    normalised to sum to 1 -> (list of tuples padded with zeros to S, probabilities)."""
    caps, probs = [], []

    def rec(prefix, lp):
        if len(prefix) == S or (prefix and prefix[-1] == 0):
            caps.append(tuple(prefix) + (0,) * (S - len(prefix)))
            probs.append(np.exp(lp))
            return
        row = first if not prefix else trans[prefix[-1]]
        for v in range(MARKOV_V1):
            rec(prefix + [v], lp + float(row[v]))
    rec([], 0.0)
    probs = np.array(probs)
    return caps, probs / probs.sum()
