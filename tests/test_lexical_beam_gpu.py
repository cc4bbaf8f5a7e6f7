"""GPU: lexically constrained beam search (include/rfn.h "lexically constrained beam search"):
rfn_log_softmax_topk_want against rfn_log_softmax_topk_masked and rfn_log_softmax_fwd, rfn_beam_step_lex against the NumPy
restatement (tests/lexical_beam_cpu.py, which reads FULL rows) over whole synthetic searches, and sample_beam's device loop
against a search stepped from the host whose bookkeeping is the restatement.

Everything is exact: ids equal, floats bit-equal.  The kernels select and copy; the only arithmetic is the stated fp32 add
p = beam_sum + local, so there is no tolerance to derive."""
import numpy as np
import pytest
import torch

import decode_constraints_cpu as D
import diverse_beam_cpu as Dv
import lexical_beam_cpu as Lx
import test_decode_constraints_gpu as T

pytestmark = pytest.mark.gpu
bits, same = T.bits, T.same
INF = float('inf')


def nat():
    import recurrent_fusion_network_amd._native as N
    return N


def i32(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


# =================================================================================================================
# rfn_log_softmax_topk_want
# =================================================================================================================
# 10240 is the largest row lsm_vec_ok keeps in registers, 10244 the first multiple of 4 beyond it; (1000, 1001) is V1 = 1000
# with a row stride that breaks the 16-byte alignment (the scalar form on a row the register form would take)
WANT_ROWS = [(5, 5), (37, 37), (1000, 1000), (1001, 1001), (1000, 1001), (10240, 10240), (10244, 10244)]


@pytest.mark.parametrize('V1,ldl', WANT_ROWS)
def test_topk_want(dev, V1, ldl):
    N = nat()
    st = N.stream_ptr()
    g = torch.Generator().manual_seed(V1 + ldl)
    rng = np.random.default_rng(V1 + ldl)
    for W in (4, 8, 16, 32):
        if W > V1:
            continue
        rows = 2 * W
        buf = torch.zeros(rows, ldl)
        buf[:, :V1] = torch.randn(rows, V1, generator=g) * 3.0
        buf[::3, :V1] = torch.round(buf[::3, :V1] * 2.0) / 2.0
        xd = buf.to(dev)
        lp = torch.empty(rows, V1, device=dev)
        N.check(N.lib.rfn_log_softmax_fwd(xd.data_ptr(), ldl, rows, V1, rows, V1, 0, lp.data_ptr(), st))
        lp_h = lp.cpu()
        arg = lp_h.argmax(1)
        for with_blk in (False, True):
            blk = torch.full((rows, 8), -1, dtype=torch.int32)
            blk_n = torch.zeros(rows, dtype=torch.int32)
            if with_blk:
                for r in range(rows):
                    ids = [int(arg[r])] if r % 2 else rng.integers(0, V1, size=5).tolist()   # odd rows: the arg-max is blocked
                    blk[r, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
                    blk_n[r] = len(ids)
            bd, nd = blk.to(dev), blk_n.to(dev)
            bp, ld_b, np_ = (bd.data_ptr(), 8, nd.data_ptr()) if with_blk else (None, 0, None)
            tv0 = torch.empty(rows, W, device=dev)
            ti0 = torch.empty(rows, W, dtype=torch.int32, device=dev)
            N.check(N.lib.rfn_log_softmax_topk_masked(xd.data_ptr(), ldl, rows, V1, W, bp, ld_b, np_, tv0.data_ptr(), ti0.data_ptr(), st))
            masked = lp_h.clone()
            for r in range(rows):
                masked[r, blk[r, :int(blk_n[r])].long()] = -INF
            for NW in (1, 16):
                for row_div in (1, W):
                    n_img = rows // row_div
                    ld_want = NW + 2
                    want = torch.full((n_img, ld_want), 3, dtype=torch.int32)      # the stride's padding is never read
                    for k in range(n_img):
                        r0 = k * row_div
                        # -1, a blocked id (of the image's first row), the arg-max id, id V1 - 1, then random ids
                        ids = [-1, int(blk[r0, 0]) if with_blk else 0, int(arg[r0]), V1 - 1] + rng.integers(0, V1, size=16).tolist()
                        ids = ids[:NW] if NW > 1 else [ids[(k + (row_div > 1)) % 4]]
                        want[k, :NW] = torch.tensor(ids, dtype=torch.int32)
                    wd = want.to(dev)
                    tv = torch.full((rows, W), 7.0, device=dev)
                    ti = torch.full((rows, W), -7, dtype=torch.int32, device=dev)
                    wv = torch.full((rows + 1, NW), 7.0, device=dev)
                    N.check(N.lib.rfn_log_softmax_topk_want(xd.data_ptr(), ldl, rows, V1, W, row_div, wd.data_ptr(), ld_want, NW, bp, ld_b,
                                                            np_, tv.data_ptr(), ti.data_ptr(), wv.data_ptr(), st))
                    where = (V1, ldl, W, with_blk, NW, row_div)
                    assert torch.equal(ti.cpu(), ti0.cpu()) and torch.equal(bits(tv), bits(tv0)), where
                    expect = torch.full((rows + 1, NW), 7.0)
                    for r in range(rows):
                        for j in range(NW):
                            v = int(want[r // row_div, j])
                            expect[r, j] = masked[r, v] if v >= 0 else -INF
                    assert torch.equal(bits(wv), bits(expect)), where
            # want == NULL: the masked kernel
            tv = torch.full((rows, W), 7.0, device=dev)
            ti = torch.full((rows, W), -7, dtype=torch.int32, device=dev)
            N.check(N.lib.rfn_log_softmax_topk_want(xd.data_ptr(), ldl, rows, V1, W, 1, None, 0, 0, bp, ld_b, np_, tv.data_ptr(),
                                                    ti.data_ptr(), None, st))
            assert torch.equal(ti.cpu(), ti0.cpu()) and torch.equal(bits(tv), bits(tv0)), (V1, ldl, W, with_blk)


# =================================================================================================================
# rfn_beam_step_lex
# =================================================================================================================
class DevLex:
    """The arrays rfn_beam_step_lex updates, for NB images of W = Wb * 2^C rows."""

    def __init__(self, NB, Wb, C_, S, dev, init):
        self.NB, self.C, self.G, self.W, self.S = NB, C_, 1 << C_, Wb << C_, S
        W, self.max_done = self.W, self.W * S
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        self.bs, self.bl, self.bsum = z(S, NB, W, dt=torch.long), z(S, NB, W), z(NB, W)
        self.order, self.ids = z(NB * W, dt=torch.int32), z(NB * W, dt=torch.long)
        self.done_seq, self.done_lp = z(NB, self.max_done, S, dt=torch.long), z(NB, self.max_done, S)
        self.done_p, self.done_n = z(NB, self.max_done), z(NB, dt=torch.int32)
        self.done_state = torch.full((NB, self.max_done), -1, dtype=torch.int32, device=dev)
        self.state_n = torch.full((NB, self.G), -9, dtype=torch.int32, device=dev)       # step 1 must not read it
        self.init = torch.tensor(init, dtype=torch.int32, device=dev)
        self.active = torch.ones(NB, dtype=torch.int32, device=dev)

    def step(self, N, topv, topi, wantv, want, wbits, NW, V1, t, C_=None):
        p = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
        return N.lib.rfn_beam_step_lex(p(topv), p(topi), p(wantv), p(want), p(wbits), NW, self.C if C_ is None else C_, V1, self.W, self.S,
                                       t, self.NB, self.max_done, self.bs.data_ptr(), self.bl.data_ptr(), self.bsum.data_ptr(),
                                       self.order.data_ptr(), self.ids.data_ptr(), self.done_seq.data_ptr(), self.done_lp.data_ptr(),
                                       self.done_p.data_ptr(), self.done_n.data_ptr(), self.state_n.data_ptr(),
                                       self.done_state.data_ptr(), self.init.data_ptr(), self.active.data_ptr(), N.stream_ptr())

    def state(self):
        return [bits(x) if x.is_floating_point() else x.cpu() for x in (self.bs, self.bl, self.bsum, self.order, self.ids, self.active)]

    def done(self, k):
        """Image k's done beams in construction order: (ids, log-prob bits, p bits, state)."""
        n = int(self.done_n[k])
        seq, lp, p, s = self.done_seq[k, :n].cpu(), bits(self.done_lp[k, :n]), bits(self.done_p[k, :n]), self.done_state[k, :n].cpu()
        return [(seq[i].tolist(), lp[i].tolist(), int(p[i]), int(s[i])) for i in range(n)]


def want_done(b):
    return [([int(x) for x in d['seq']], i32(d['logps']).tolist(), int(i32([d['p']])[0]), d['state']) for d in b.done]


def top_lists(rows, W, dev):
    """(NB, W, V1) log-prob rows -> the (NB * W, W) top lists (value descending, token ascending; -inf entries last, lowest ids
    first, as rfn_log_softmax_topk_masked fills a short row); with V1 < W the columns past V1 hold a poison."""
    NB, _, V1 = rows.shape
    ys, ix = Dv.sorted_rows(rows.reshape(NB * W, V1), min(W, V1))
    tv, ti = np.full((NB * W, W), np.nan, dtype=np.float32), np.full((NB * W, W), -7, dtype=np.int32)
    tv[:, :ys.shape[1]], ti[:, :ix.shape[1]] = ys, ix
    return torch.from_numpy(tv).to(dev), torch.from_numpy(ti).to(dev)


def want_values(rows, sets, NW, dev):
    """(NB, W, V1) rows -> wantv (NB * W, NW): the log-prob of every want id, -inf for the -1 padding."""
    NB, W, _ = rows.shape
    out = np.full((NB, W, NW), -np.inf, dtype=np.float32)
    for k in range(NB):
        for j, v in enumerate(sets[k][0]):
            if v >= 0:
                out[k, :, j] = rows[k, :, v]
    return torch.from_numpy(out.reshape(NB * W, NW)).to(dev)


@pytest.mark.parametrize('Wb,C_', Lx.SHAPES)
def test_step_kernel_matches_the_restatement(dev, Wb, C_):
    """Whole synthetic searches, the state carried from step to step on the device and in the restatement: after every step the
    beam arrays, order, next_ids, active and state_n, at the end the done beams with their states.  (W = 2 has no V1 < W case: a
    vocabulary of one token holds no id a set could name.)"""
    N = nat()
    W, G = Wb << C_, 1 << C_
    for NB, S, V1, NW, sets, rows in Lx.step_cases(Wb, C_):
        want = torch.tensor([s[0] for s in sets], dtype=torch.int32, device=dev)
        wbits = torch.tensor([s[1] for s in sets], dtype=torch.int32, device=dev)
        d = DevLex(NB, Wb, C_, S, dev, [s[2] for s in sets])
        ref = [Lx.LexBeams(Wb, C_, S, sets[k][2]) for k in range(NB)]
        for t in range(1, S + 1):
            tv, ti = top_lists(rows[t - 1], W, dev)
            N.check(d.step(N, tv, ti, want_values(rows[t - 1], sets, NW, dev), want, wbits, NW, V1, t), 'rfn_beam_step_lex')
            for k in range(NB):
                Lx.step(ref[k], rows[t - 1][k], t, sets[k][0], sets[k][1])
            got = d.state()
            where = (NB, S, V1, NW, t)
            assert d.state_n.cpu().tolist() == [b.state_n.tolist() for b in ref], where
            assert got[0].permute(1, 0, 2).tolist() == [b.seq.tolist() for b in ref], where
            assert got[1].permute(1, 0, 2).tolist() == [i32(b.lp).tolist() for b in ref], where
            assert got[2].tolist() == [i32(b.sum).tolist() for b in ref], where
            assert got[3].view(NB, W).tolist() == [(k * W + b.order).tolist() for k, b in enumerate(ref)], where
            assert got[4].view(NB, W).tolist() == [b.next_ids.tolist() for b in ref], where
            assert got[5].tolist() == [int(b.active) for b in ref], where
        for k in range(NB):
            assert d.done(k) == want_done(ref[k]), (NB, S, V1, NW, k)
        assert (d.done_state.cpu()[torch.arange(d.max_done)[None, :] >= d.done_n.cpu()[:, None]] == -1).all()


@pytest.mark.parametrize('W', [1, 5, 32])
def test_no_sets_forwards_to_the_plain_kernel(dev, W):
    """C == 0 through rfn_beam_step_lex: rfn_beam_step_topk bit for bit; the lexical arguments may be NULL."""
    import test_diverse_beam_gpu as Tg
    N = nat()
    NB, S, V1 = 3, 6, 37
    rows = Dv.synthetic_rows(91 + W, NB, W, S, V1)
    a, b = Tg.DevBeams(NB, W, S, dev), Tg.DevBeams(NB, W, S, dev)
    for t in range(1, S + 1):
        tv, ti = Tg.top_lists(rows[t - 1], W, dev)
        N.check(N.lib.rfn_beam_step_lex(tv.data_ptr(), ti.data_ptr(), None, None, None, 0, 0, V1, W, S, t, NB, a.max_done, a.bs.data_ptr(),
                                        a.bl.data_ptr(), a.bsum.data_ptr(), a.order.data_ptr(), a.ids.data_ptr(), a.done_seq.data_ptr(),
                                        a.done_lp.data_ptr(), a.done_p.data_ptr(), a.done_n.data_ptr(), None, None, None,
                                        a.active.data_ptr(), N.stream_ptr()))
        b.step_topk(N, tv, ti, V1, t)
        for x, y in zip(a.state(), b.state()):
            assert torch.equal(x, y), (W, t)
    for k in range(NB):
        assert [m[:3] for m in a.done(k)] == [m[:3] for m in b.done(k)]


def test_nan_want_values_stay_in_bounds(dev):
    """NaN keys (a NaN logit reaches the want values; the top lists never hold one) are not ordered: the step selects no defined
    set, but every row still continues a row of its own image with a token of the vocabulary, and the counts stay in range."""
    N = nat()
    Wb, C_, NB, S, V1, NW = 3, 2, 2, 4, 37, 6
    W = Wb << C_
    sets = Lx.case_sets(NB, C_, NW, V1, 11)
    rows = Lx.synthetic_rows(11, NB, W, S, V1, sets)
    want = torch.tensor([s[0] for s in sets], dtype=torch.int32, device=dev)
    wbits = torch.tensor([s[1] for s in sets], dtype=torch.int32, device=dev)
    d = DevLex(NB, Wb, C_, S, dev, [s[2] for s in sets])
    for t in range(1, S + 1):
        tv, ti = top_lists(rows[t - 1], W, dev)
        wv = want_values(rows[t - 1], sets, NW, dev)
        wv[::2] = float('nan')
        N.check(d.step(N, tv, ti, wv, want, wbits, NW, V1, t), 'rfn_beam_step_lex')
        order, ids, n = d.order.cpu().view(NB, W), d.ids.cpu(), d.state_n.cpu()
        lo = torch.arange(NB)[:, None] * W
        assert ((order >= lo) & (order < lo + W)).all() and ((ids >= 0) & (ids < V1)).all(), t
        assert ((n >= 0) & (n <= Wb)).all() and int(d.done_n.max()) <= d.max_done, t


def test_refused_shapes_launch_nothing(dev):
    N = nat()
    S, V1 = 4, 37
    for Wb, C_, NW, call_C, call_W, call_S in ((4, 2, 2, 4, None, None), (4, 2, 2, -1, None, None), (3, 1, 1, 2, None, None),
                                               (4, 1, -1, None, None, None), (16, 1, 17, None, None, None), (4, 1, 5, None, None, None),
                                               (4, 2, 13, None, None, None), (4, 1, 1, None, 34, None), (4, 1, 1, None, None, 65)):
        sets = Lx.case_sets(1, C_, max(NW, 1), V1, 5)
        rows = Lx.synthetic_rows(5, 1, Wb << C_, 1, V1, sets)
        d = DevLex(1, Wb, C_, S, dev, [sets[0][2]])
        tv, ti = top_lists(rows[0], d.W, dev)
        wv = torch.zeros(d.W, 32, device=dev)
        want = torch.ones(1, 32, dtype=torch.int32, device=dev)
        if call_W is not None:
            d.W = call_W
        if call_S is not None:
            d.S = call_S
        assert d.step(N, tv, ti, wv, want, want, NW, V1, 1, call_C) == -1, (Wb, C_, NW, call_C, call_W, call_S)
        torch.cuda.synchronize()
        assert int(d.done_n[0]) == 0 and int(d.bs.abs().sum()) == 0 and int(d.order.abs().sum()) == 0      # nothing ran
        assert (d.state_n == -9).all() and int(d.active[0]) == 1


# =================================================================================================================
# whole path
# =================================================================================================================
def met_by(seq, sets):
    s = set(int(x) for x in seq)
    return sum(1 for ids in sets if ids and s & set(ids))


@torch.no_grad()
def host_lexical_beam(model, fc, att, Wb, req, cons, alpha=0.0):
    """sample_beam stepped from the host: every step's full log-prob rows come back, get the constraints' mask, and the full-row
    restatement does the bookkeeping.  -> (seq (B, S), seq_lp (B, S), done beams as (ids, log-prob bits, p bytes, state) in the
    call's ranking, lexical_met)."""
    N = nat()
    B, S, V1 = fc[0].size(0), model.seq_length, model.vocab_size + 1
    dev = fc[0].device
    C_ = max(len(img) for img in req)
    W = Wb << C_
    parsed = [Lx.parse_sets(img, C_) for img in req]
    steppers = T._members([model], fc, att, repeat=W)
    rows = B * W
    ref = [Lx.LexBeams(Wb, C_, S, parsed[k][2]) for k in range(B)]
    ids = torch.zeros(rows, dtype=torch.long, device=dev)
    logit_sum, logit_m, logp = (torch.empty(rows, V1, device=dev) for _ in range(3))
    for t in range(S + 1):
        if t >= 1:
            for k in range(B):
                Lx.step(ref[k], masked[k * W:(k + 1) * W], t, parsed[k][0], parsed[k][1])
            if t == S:
                break
            order = torch.from_numpy(np.concatenate([k * W + b.order for k, b in enumerate(ref)])).to(torch.int32).to(dev)
            ids = torch.from_numpy(np.concatenate([b.next_ids for b in ref])).to(dev)
            for sp in steppers:
                sp.reorder(order)
        T._averaged_logp(N, steppers, ids, logit_sum, logit_m, logp)
        hist = np.concatenate([b.seq[:t].T for b in ref])                       # row k * W + w continues beam (k, w)
        masked = D.mask_rows(logp.cpu().numpy(), hist, t + 1, **cons)
    seq, seq_lp = torch.zeros(B, S, dtype=torch.long), torch.zeros(B, S)
    done_beams, met = [], []
    for k, b in enumerate(ref):
        ranked = [b.done[i] for i in Lx.rank_done(b.done, S, alpha)]
        seq[k], seq_lp[k] = torch.from_numpy(ranked[0]['seq']), torch.from_numpy(ranked[0]['logps'])
        done_beams.append([(d['seq'].tolist(), i32(d['logps']).tolist(), np.float32(d['p']).tobytes(), d['state']) for d in ranked])
        met.append(Lx.popcount(ranked[0]['state'] & ~parsed[k][2]))
    return seq, seq_lp, done_beams, met


def with_states(done_beams):
    return [[t + (d['state'],) for t, d in zip(img_t, img)] for img_t, img in zip(T.beams_of(done_beams), done_beams)]


def requirements(model, fc, att, C_, per_set, seed):
    """Per image C sets of `per_set` ids the unconstrained best beam does not hold (so that the constraint has to bite); image 1
    has one set fewer (ragged), and with C >= 2 image 0's sets 0 and 1 share an id."""
    V1 = model.vocab_size + 1
    base = model.sample_beam(fc, att, {'beam_size': 2})[0].cpu()
    rng = np.random.default_rng(seed)
    req = []
    for k in range(base.size(0)):
        free = [v for v in rng.permutation(np.arange(1, V1)).tolist() if v not in set(base[k].tolist())]
        sets = [free[i * per_set:(i + 1) * per_set] for i in range(C_)]
        if k == 1:
            sets = sets[:C_ - 1]
        if k == 0 and C_ >= 2:
            sets[1] = sets[1][:-1] + [sets[0][0]] if per_set > 1 else [sets[0][0]]
        req.append(sets)
    return base, req


RUNS = [(3, 1, 2, {}), (2, 2, 2, {}), (1, 3, 1, {}), (2, 2, 2, {'block_ngram': 3, 'banned_ids': 'B'}), (2, 2, 2, {'length_penalty': 0.7}),
        (3, 1, 2, {'length_penalty': 1.0})]


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_device_loop_equals_the_host_stepped_search(dev, name):
    """sample_beam(..., {'beam_size': Wb, 'require': req}) against the host-stepped search on full rows: alone, with block_ngram =
    3 plus a banned id, and with a length penalty; lexical_met and every done beam's 'state' agree with the ids."""
    model, fc, att = T.setup(name, dev)
    B = fc[0].size(0)
    bitten = 0
    with torch.no_grad():
        _, banned, _ = T.bite_ids(model, fc, att)
        for Wb, C_, per_set, extra in RUNS:
            extra = {k: (banned if v == 'B' else v) for k, v in extra.items()}
            base, req = requirements(model, fc, att, C_, per_set, 3 * Wb + C_)
            want = host_lexical_beam(model, fc, att, Wb, req, T.cons_of(extra), extra.get('length_penalty', 0.0))
            tag = (name, Wb, C_, extra)
            for form in (req, None):
                if form is None:                                                 # the same sets as a padded tensor
                    form = torch.full((B, C_, per_set + 1), -1, dtype=torch.long)
                    for k, img in enumerate(req):
                        for i, ids in enumerate(img):
                            form[k, i, :len(ids)] = torch.tensor(ids)
                out = model.sample_beam(fc, att, dict(extra, beam_size=Wb, require=form))
                assert same(out[0], want[0]) and same(out[1], want[1]), tag
                assert with_states(model.done_beams) == want[2], tag
                assert model.lexical_met.dtype == torch.int32 and model.lexical_met.tolist() == want[3], tag
            kept = model.sample_beam(fc, att, dict(extra, beam_size=Wb, require=req, keep_candidates=True))
            assert same(kept[0], want[0]) and model.candidates['seq'].size(1) == Wb, tag          # the first Wb beams of the ranking
            for k in range(B):
                n = int(model.candidates['n_cand'][k])
                assert n == min(Wb, len(want[2][k])) and model.candidates['seq'][k, :n].tolist() == [d[0] for d in want[2][k][:n]], tag
            for k in range(B):
                full = [ids for ids in req[k]] + [[]] * (C_ - len(req[k]))
                assert int(model.lexical_met[k]) == met_by(out[0][k].tolist(), full), tag
                for d in model.done_beams[k]:
                    holds = sum(1 << i for i, ids in enumerate(full) if not ids or set(ids) & set(d['seq'].tolist()))
                    assert d['state'] == holds, (tag, k)
                bitten += int(model.lexical_met[k]) > 0 and out[0][k].tolist() != base[k].tolist()
    assert bitten > 0, 'no caption that the required words changed'


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_all_empty_equals_today(dev, name):
    """require with every set empty: the tensors and done_beams of the call without the key, bit for bit; no 'state', no
    lexical_met."""
    model, fc, att = T.setup(name, dev)
    B = fc[0].size(0)
    with torch.no_grad():
        for W in (1, 3):
            a = model.sample_beam(fc, att, {'beam_size': W})
            want = T.beams_of(model.done_beams)
            for off in ([[] for _ in range(B)], [[[], []] for _ in range(B)], torch.full((B, 2, 3), -1, dtype=torch.long), None):
                b = model.sample_beam(fc, att, {'beam_size': W, 'require': off})
                assert same(a[0], b[0]) and same(a[1], b[1]) and T.beams_of(model.done_beams) == want
                assert all('state' not in d for img in model.done_beams for d in img) and model.lexical_met is None


def test_refusals(dev):
    from recurrent_fusion_network_amd import rewards as RW
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    model, fc, att = T.setup('mid', dev)
    B = fc[0].size(0)
    req = [[[1], [2]] for _ in range(B)]
    scorer = RW.CiderD.__new__(RW.CiderD)                                        # the combination is refused before it is used
    with torch.no_grad():
        for bad in ({'group_size': 2}, {'consensus': scorer}):
            with pytest.raises(ValueError):
                model.sample_beam(fc, att, dict(bad, beam_size=2, require=req))
        with pytest.raises(ValueError):
            EnsembleDecoder([model]).sample_beam(fc, att, {'beam_size': 2, 'require': req})
        for bad_req, Wb in (([[[1], [2], [3], [4]]] * B, 1), ([[[0]]] * B, 2), ([[[1, 2, 3]]] * B, 2), ([[[1], [2]]] * B, 9)):
            with pytest.raises(ValueError):
                model.sample_beam(fc, att, {'beam_size': Wb, 'require': bad_req})
