"""NumPy restatement of lexically constrained beam search (include/rfn.h "lexically constrained beam search"): one step of one
image on FULL log-prob rows, a whole-search driver, the ranking of the done beams, the host's parse of the required sets, and
the synthetic rows the tests feed.  np.float32 arithmetic exactly as the header states it: p = fp32(sum + local).  Nothing here
knows about top-W lists: every row gives all its V1 entries as candidates, and any Wb is allowed."""
import numpy as np

F = np.float32
NEG = -np.inf


def popcount(x):
    return bin(int(x)).count('1')


def parse_sets(sets, C):
    """One image's required sets (a list of lists of ids; -1 entries are padding) -> (want ids, want bits, init_state): the unique
    ids in order of first appearance, bit i of an id's mask set when it is in set i, and the bits of the empty or missing sets."""
    want, bits, init = [], [], 0
    for i in range(C):
        ids = [int(v) for v in (sets[i] if i < len(sets) else []) if int(v) >= 0]
        if not ids:
            init |= 1 << i
        for v in ids:
            if v not in want:
                want.append(v)
                bits.append(0)
            bits[want.index(v)] |= 1 << i
    return want, bits, init


class LexBeams:
    """The state of one image's search: what rfn_beam_step_lex keeps per image."""

    def __init__(self, Wb, C, S, init_state=0):
        self.Wb, self.C, self.S = Wb, C, S
        self.G = 1 << C
        self.W = W = self.G * Wb
        self.seq = np.zeros((S, W), dtype=np.int64)
        self.lp = np.zeros((S, W), dtype=np.float32)
        self.sum = np.zeros(W, dtype=np.float32)
        self.state_n = np.zeros(self.G, dtype=np.int64)
        self.state_n[init_state] = 1
        self.done = []                               # dicts seq, logps, p, state -- in construction order
        self.active = True
        self.order = np.arange(W)
        self.next_ids = np.zeros(W, dtype=np.int64)
        self.moves_outside = 0                       # selected move candidates whose token is not among the row's W best
        self.occupancy = []                          # state_n after every step

    def occupied(self):
        return [s * self.Wb + i for s in range(self.G) for i in range(int(self.state_n[s]))]


def step(b, logp, t, want, want_bits, max_done=None):
    """Step t (1 .. S) of one image.  logp: (W, V1) rows (an unoccupied row's content is never read); want / want_bits: the
    image's unique required ids and their set masks (-1 ids are padding).  Updates `b` in place."""
    W, S, G, Wb = b.W, b.S, b.G, b.Wb
    assert 1 <= t <= S
    max_done = W * S if max_done is None else max_done
    b.order, b.next_ids = np.arange(W), np.zeros(W, dtype=np.int64)
    if not b.active:
        b.occupancy.append(b.state_n.copy())
        return
    logp = np.asarray(logp, dtype=np.float32)
    V1 = logp.shape[1]
    ix = np.argsort(-logp, axis=1, kind='stable')    # value descending, token ascending
    ys = np.take_along_axis(logp, ix, axis=1)
    prev_seq, prev_lp, prev_sum, prev_n = b.seq.copy(), b.lp.copy(), b.sum.copy(), b.state_n.copy()
    bits_of = {int(v): int(m) for v, m in zip(want, want_bits) if int(v) >= 0}
    any_cand = False
    for s in range(G):
        cands = []                                   # (p, local, token, source row, is a move)
        for sp in range(s + 1):
            if sp & ~s:
                continue
            live = [q for q in range(sp * Wb, sp * Wb + int(prev_n[sp])) if t == 1 or prev_seq[t - 2, q] != 0]
            if sp == s:                              # stay: (column outer, row inner)
                for c in range(V1):
                    for q in live:
                        v, local = int(ix[q, c]), F(ys[q, c])
                        if (sp | bits_of.get(v, 0)) == sp and local != NEG:
                            cands.append((F(prev_sum[q] + local), local, v, q, False))
            else:                                    # move: (want index outer, row inner)
                for v, m in zip(want, want_bits):
                    v, m = int(v), int(m)
                    if v < 0 or not (m & ~sp) or (sp | m) != s:
                        continue
                    for q in live:
                        local = F(logp[q, v])
                        if local != NEG:
                            cands.append((F(prev_sum[q] + local), local, v, q, True))
        any_cand |= len(cands) > 0
        rank = sorted(range(len(cands)), key=lambda i: -float(cands[i][0]))   # stable; fp32 -> fp64 is exact
        nnew = min(Wb, len(cands))
        b.state_n[s] = nnew
        for vix in range(nnew):
            beam = s * Wb + vix
            p, local, v, q, move = cands[rank[vix]]
            b.seq[:t - 1, beam], b.lp[:t - 1, beam] = prev_seq[:t - 1, q], prev_lp[:t - 1, q]
            b.seq[t - 1, beam], b.lp[t - 1, beam], b.sum[beam] = v, local, p
            b.order[beam], b.next_ids[beam] = q, v
            if move and v not in ix[q, :min(W, V1)]:
                b.moves_outside += 1
            if (v == 0 or t == S) and len(b.done) < max_done:
                b.done.append(dict(seq=b.seq[:, beam].copy(), logps=b.lp[:, beam].copy(), p=F(p), state=s))
    if not any_cand:
        b.active = False
    b.occupancy.append(b.state_n.copy())


def caption_len(seq, S):
    s = [int(x) for x in seq][:S]
    return s.index(0) + 1 if 0 in s else S


def rank_done(done, S, alpha=0.0):
    """Order of the done beams: satisfied sets descending, then p (or p / len^alpha, one fp64 division) descending, ties in
    construction order."""
    def score(d):
        p = float(np.float32(d['p']))
        return float(np.float64(p) / np.float64(float(caption_len(d['seq'], S)) ** float(alpha))) if alpha else p
    return sorted(range(len(done)), key=lambda i: (-popcount(done[i]['state']), -score(done[i])))


def search(step_fn, Wb, C, S, want, want_bits, init_state):
    """The whole search of one image around step_fn(t, b) -> (W, V1) log-prob rows of decoder step t, b the LexBeams after step t
    (t = 0: before any step; row r then continues b.order[r] and is fed b.next_ids[r], and holds the prefix b.seq[:t, r])."""
    b = LexBeams(Wb, C, S, init_state)
    logp = step_fn(0, b)
    for t in range(1, S + 1):
        step(b, logp, t, want, want_bits)
        if t == S or not b.active:
            break
        logp = step_fn(t, b)
    return b


def case_sets(NB, C, NW, V1, seed):
    """The required sets of the NB images of a synthetic case: image 0 has C sets over NW ids; image 1 (NB = 3) has one set fewer
    (ragged: its last set is missing); image 2 has C sets with one id shared by sets 0 and 1 when C >= 2.  Ids are drawn from
    [1, V1).  -> per image (want padded with -1 to NW, bits, init_state)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(NB):
        n = min(NW, V1 - 1)
        ids = [int(v) for v in rng.permutation(np.arange(1, V1))[:n]]
        c = C - 1 if k == 1 else C
        sets = [[] for _ in range(C)]
        for j, v in enumerate(ids):
            if c:
                sets[j % c].append(v)
        if k == 2 and C >= 2 and sets[0]:
            sets[1].append(sets[0][0])
        want, bits, init = parse_sets(sets, C)
        assert len(want) <= NW
        pad = NW - len(want)
        out.append((want + [-1] * pad, bits + [0] * pad, init))
    return out


def synthetic_rows(seed, NB, W, S, V1, sets, blocked=(), end_bias=1.0, rare=6.0):
    """Log-prob rows of a synthetic search that do not depend on its state: a list over decoder steps 0 .. S-1 of (NB, W, V1)
    float32.  Step 0: the W rows of an image are equal, as a model's are after BOS.  Later steps: an image-wide component plus a
    row's own, every third row quantised to halves (exact ties), a bias on token 0 so that beams end early.  Required ids (sets[k]
    = (want, bits, init)) are made rare -- `rare` logits lower -- at two steps of every three, step 0 among them, so that their
    log-probs fall outside a row's W best and only the want values can bring them into the search; at the third they compete as
    they are.  blocked[k]: ids of image k that read -inf at every step (a banned required word)."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(S):
        if s == 0:
            x = np.repeat(2.0 * rng.standard_normal((NB, 1, V1)), W, axis=1)
        else:
            x = 2.0 * rng.standard_normal((NB, 1, V1)) + 2.0 * rng.standard_normal((NB, W, V1))
            flat = x.reshape(NB * W, V1)
            flat[::3] = np.round(flat[::3] * 2.0) / 2.0
            x = flat.reshape(NB, W, V1)
            x[..., 0] += end_bias
        if s % 3 != 2:
            for k in range(NB):
                ids = [v for v in sets[k][0] if v >= 0]
                x[k][:, ids] -= rare
        m = x.max(-1, keepdims=True)
        lp = (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32)
        for k in range(NB):
            if k < len(blocked) and len(blocked[k]):
                lp[k][:, list(blocked[k])] = NEG
        out.append(lp)
    return out


# The cases of the GPU step test (tests/test_lexical_beam_gpu.py) and of the non-vacuity checks on the restatement alone.
SHAPES = [(1, 1), (2, 1), (16, 1), (3, 2), (8, 2), (1, 3), (4, 3)]


def step_cases(Wb, C):
    """-> (NB, S, V1, NW, sets, rows) for every case of one (Wb, C) shape.  V1 in {W, 37} plus one V1 < W; NW in {1, min(16, W -
    Wb)}; in the S == 4 cases image 0's first set is blocked (-inf at every step), so that image cannot reach the accepting state."""
    W = Wb << C
    v1s = [W, 37] + ([W - 1] if W > 2 else [])
    for NB in (1, 3):
        for S in (1, 4, 17):
            for V1 in v1s:
                if V1 < 2:
                    continue
                for NW in sorted({1, min(16, W - Wb)}):
                    seed = 100000 * Wb + 10000 * C + 1000 * NB + 10 * S + V1 + 7 * NW
                    sets = case_sets(NB, C, NW, V1, seed)
                    blocked = [[v for v, m in zip(sets[0][0], sets[0][1]) if v >= 0 and m & 1]] if S == 4 else []
                    yield NB, S, V1, NW, sets, synthetic_rows(seed, NB, W, S, V1, sets, blocked)


def run_case(Wb, C, NB, S, sets, rows):
    """The restatement over one case -> the NB LexBeams at the end."""
    ref = [LexBeams(Wb, C, S, sets[k][2]) for k in range(NB)]
    for t in range(1, S + 1):
        for k in range(NB):
            step(ref[k], rows[t - 1][k], t, sets[k][0], sets[k][1])
    return ref
