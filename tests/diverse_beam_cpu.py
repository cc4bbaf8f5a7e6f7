"""NumPy restatement of diverse beam search (include/rfn.h "diverse beam search"): one step of one image on FULL log-prob rows,
and a whole-search driver around a step callback.  np.float32 arithmetic exactly as the header states it: p = fp32(sum + local),
key = p, or fp32(sum + fp32(local - fp32(lambda * count))) for a token that earlier groups chose at this step -- three separate
roundings.  Nothing here knows about top-W lists: `ncols` only exists so that a test can feed each row's W best entries and
compare (the sufficiency claim)."""
import numpy as np

F = np.float32


class Beams:
    """The state of one image's search: what rfn_beam_step_div keeps per image."""

    def __init__(self, W, S):
        self.W, self.S = W, S
        self.seq = np.zeros((S, W), dtype=np.int64)
        self.lp = np.zeros((S, W), dtype=np.float32)
        self.sum = np.zeros(W, dtype=np.float32)
        self.done = []                               # dicts seq, logps, p, group -- in construction order
        self.active = True
        self.order = np.arange(W)
        self.next_ids = np.zeros(W, dtype=np.int64)
        self.inert_groups = []                       # per step: the groups that had no candidate while another had one


def sorted_rows(logp, ncols=None):
    """Every row sorted descending by value, then ascending by token id -> (values, ids), cut to the first ncols columns."""
    logp = np.asarray(logp, dtype=np.float32)
    ix = np.argsort(-logp, axis=1, kind='stable')
    ys = np.take_along_axis(logp, ix, axis=1)
    if ncols is not None:
        ys, ix = ys[:, :ncols], ix[:, :ncols]
    return ys, ix


def step(b, logp, t, G=1, lam=0.5, ncols=None, max_done=None):
    """Step t (1 .. S) of one image.  logp: (W, V1) rows; ncols: None = full rows, else only each row's first ncols sorted
    columns give candidates.  Updates `b` in place; b.order / b.next_ids are the step's outputs."""
    W, S = b.W, b.S
    Wg = W // G
    assert W % G == 0 and G >= 1 and 1 <= t <= S
    max_done = W * S if max_done is None else max_done
    b.order, b.next_ids = np.arange(W), np.zeros(W, dtype=np.int64)
    if not b.active:
        return
    ys, ix = sorted_rows(logp, ncols)
    cols = ys.shape[1]
    prev_seq, prev_lp, prev_sum = b.seq.copy(), b.lp.copy(), b.sum.copy()
    lam = F(lam)
    chosen = []                                      # tokens != 0 newly selected by the earlier groups at this step
    had = []
    for g in range(G):
        b0 = g * Wg
        live = [b0] if t == 1 else [q for q in range(b0, b0 + Wg) if prev_seq[t - 2, q] != 0]
        cands = []
        for c in range(cols):
            for q in live:
                local, v = F(ys[q, c]), int(ix[q, c])
                p = F(prev_sum[q] + local)
                count = chosen.count(v) if v != 0 else 0
                key = p if count == 0 else F(prev_sum[q] + F(local - F(lam * F(count))))
                cands.append((key, p, local, v, q))
        had.append(len(cands) > 0)
        if not cands:
            continue                                 # the group's rows stay inert
        rank = sorted(range(len(cands)), key=lambda i: -float(cands[i][0]))   # stable; fp32 -> fp64 is exact
        nnew = min(Wg, len(cands))
        for vix in range(Wg):
            beam = b0 + vix
            if vix >= nnew:                          # keeps its previous state and tokens
                b.next_ids[beam] = b.seq[t - 1, beam]
                continue
            _, p, local, v, q = cands[rank[vix]]
            b.seq[:t - 1, beam], b.lp[:t - 1, beam] = prev_seq[:t - 1, q], prev_lp[:t - 1, q]
            b.seq[t - 1, beam], b.lp[t - 1, beam], b.sum[beam] = v, local, p
            b.order[beam], b.next_ids[beam] = q, v
            if (v == 0 or t == S) and len(b.done) < max_done:
                b.done.append(dict(seq=b.seq[:, beam].copy(), logps=b.lp[:, beam].copy(), p=F(p), group=g))
            if v != 0:
                chosen.append(v)
    if not any(had):
        b.active = False
    elif not all(had):
        b.inert_groups.append((t, [g for g in range(G) if not had[g]]))


def synthetic_rows(seed, NB, W, S, V1, end_bias=2.0):
    """Log-prob rows of a synthetic search that do not depend on its state: a list over decoder steps 0 .. S-1 of (NB, W, V1)
    float32.  Step 0 (read at t = 1): the W rows of an image are equal, as a model's are after BOS, with the tokens 1 .. V1-1 in
    a random order 0.25 apart in logits and END last -- every group's first choice collides with the earlier groups', and the
    runner-up is closer than the smallest lambda the tests use (0.5).  Later steps: an image-wide component plus a row's own,
    every third row quantised to halves (exact ties within a row, equal tokens across groups), and a bias on token 0 so that
    beams end early."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(S):
        if s == 0:
            x = np.empty((NB, W, V1))
            for k in range(NB):
                row = np.empty(V1)
                row[rng.permutation(np.arange(1, V1))] = -0.25 * np.arange(V1 - 1)
                row[0] = -0.25 * (V1 - 1)
                x[k] = row
        else:
            x = 2.0 * rng.standard_normal((NB, 1, V1)) + 2.0 * rng.standard_normal((NB, W, V1))
            flat = x.reshape(NB * W, V1)
            flat[::3] = np.round(flat[::3] * 2.0) / 2.0
            x = flat.reshape(NB, W, V1)
            x[..., 0] += end_bias
        m = x.max(-1, keepdims=True)
        out.append((x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32))
    return out


def search(step_fn, W, S, G=1, lam=0.5, ncols=None):
    """The whole search of one image around step_fn(t, order, next_ids) -> (W, V1) log-prob rows of decoder step t (t = 0 feeds
    BOS: order is the identity, next_ids zeros; t >= 1: row r continues the state of row order[r] and is fed next_ids[r])."""
    b = Beams(W, S)
    logp = step_fn(0, np.arange(W), np.zeros(W, dtype=np.int64))
    for t in range(1, S + 1):
        step(b, logp, t, G, lam, ncols)
        if t == S or not b.active:
            break
        logp = step_fn(t, b.order.copy(), b.next_ids.copy())
    return b
