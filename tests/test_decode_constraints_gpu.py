"""GPU: decoding constraints (include/rfn.h "decoding constraints"): the three kernels through the C ABI
against the NumPy restatement (tests/decode_constraints_cpu.py), and the constrained device loops against a loop that is
stepped from the host with the restatement's mask applied between the steps.

Everything here is exact: ids equal, log-probs bit-equal.  The masks only ever write -inf, and the unblocked entries are the
bits rfn_log_softmax_fwd / rfn_log_softmax_topk produce, so there is no tolerance to derive."""
import copy

import numpy as np
import pytest
import torch

import decode_constraints_cpu as D
from conftest import load_case

pytestmark = pytest.mark.gpu
INF = float('inf')


def nat():
    import recurrent_fusion_network_amd._native as N
    return N


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# =================================================================================================================
# kernels
# =================================================================================================================
def _id_lists(rng, k_banned, k_bad, V1):
    banned = sorted(rng.choice(np.arange(1, V1), size=k_banned, replace=False).tolist()) if k_banned else []
    bad = rng.choice(np.arange(3, V1), size=k_bad, replace=False).tolist() if k_bad else []
    if bad:
        bad[0] = 2                                          # a letter of the histories' alphabet: the rule fires often
    return banned, sorted(set(bad))


@pytest.mark.parametrize('n', [2, 3, 4])
@pytest.mark.parametrize('layout', ['matrix', 'beam'])
def test_decode_blocklist_matches_the_restatement(dev, layout, n):
    """Histories over the letters {1, 2, 3} so that n-grams repeat; one row in seven has finished.  A history of t - 1 tokens
    has t - n earlier n-gram positions, each matching with probability 3^-(n-1): where S - n >= 2 * 3^(n-1) well over half
    the rows must list an n-gram continuation at t = S, which is asserted on the restatement so the test cannot pass
    vacuously."""
    N = nat()
    V1 = 100
    rng = np.random.default_rng(100 * n + (layout == 'beam'))
    counts = [(0, 0), (1, 1), (64, 64), (64, 0), (0, 64)]
    case = 0
    for S in (4, 17, 64):
        for t in sorted({1, max(1, n - 1), min(n, S), S}):
            for rows in ((1, 3, 64, 130) if t == S else (130,)):
                kb, ke = counts[case % len(counts)]
                case += 1
                banned, bad = _id_lists(rng, kb, ke, V1)
                hist = rng.integers(1, 4, size=(rows, S))
                hist[::7, max(0, t - 2):] = 0                                   # finished rows (when t >= 2)
                order = rng.permutation(rows) if layout == 'beam' and case % 2 else None
                src = hist if order is None else hist[order]
                want = [D.blocked_ids(src[r, :t - 1], t, n, banned, bad) for r in range(rows)]
                if t == S and S - n >= 2 * 3 ** (n - 1) and rows >= 64:
                    grams = [len(D.blocked_ids(src[r, :t - 1], t, n)) > 0 for r in range(rows)]
                    assert sum(grams) * 2 >= rows, (S, n, rows, sum(grams))
                if layout == 'matrix':
                    h = torch.zeros(rows, S + 3, dtype=torch.long)
                    h[:, :S] = torch.from_numpy(hist)
                    h[:, t - 1:] = 77                                           # columns the step has not written yet
                    hd, s_row, s_tok = h.to(dev), S + 3, 1
                else:
                    h = torch.from_numpy(hist.T.copy())                        # (S, rows): the beam arrays (S, NB, W)
                    h[t - 1:] = 77
                    hd, s_row, s_tok = h.to(dev), 1, rows
                od = torch.from_numpy(order).to(torch.int32).to(dev) if order is not None else None
                bd = torch.tensor(banned or [0], dtype=torch.int32, device=dev)
                ed = torch.tensor(bad or [0], dtype=torch.int32, device=dev)
                blk = torch.full((rows + 1, 64 + S), -5, dtype=torch.int32, device=dev)
                blk_n = torch.full((rows + 1,), -5, dtype=torch.int32, device=dev)
                N.check(N.lib.rfn_decode_blocklist(hd.data_ptr(), s_row, s_tok, N.ptr(od), rows, S, t, n, bd.data_ptr(), len(banned),
                                                   ed.data_ptr(), len(bad), V1, blk.data_ptr(), blk_n.data_ptr(), N.stream_ptr()))
                got, got_n = blk.cpu().numpy(), blk_n.cpu().numpy()
                assert (got[rows] == -5).all() and got_n[rows] == -5           # nothing past the last row
                for r in range(rows):
                    k = int(got_n[r])
                    assert k == len(want[r]), (S, t, rows, r, k, want[r])
                    assert set(got[r, :k].tolist()) == set(want[r]), (S, t, rows, r, got[r, :k], want[r])
                    assert (got[r, k:] == -1).all()


def _block_kind(kind, lp_row, W, V1, rng):
    top = torch.topk(lp_row, min(W, V1)).indices.tolist()
    if kind == 0:
        return []
    if kind == 1:                                                                       # duplicates
        return rng.integers(0, V1, size=min(2 * V1, 40)).tolist() + top[:1] * 3
    if kind == 2:                                                                       # the whole unmasked top-W
        return top
    if kind == 3:                                                                       # fewer than W left unblocked
        keep = set(top[:max(0, min(W, V1) - 2)])
        return [v for v in range(V1) if v not in keep]
    return list(range(1, V1))                                                           # everything except token 0


@pytest.mark.parametrize('V1', [5, 64, 65, 1000, 9488])
def test_log_softmax_topk_masked(dev, V1):
    """Expected list: the device's own log-prob bits (rfn_log_softmax_fwd) with the blocked entries at -inf, sorted descending
    and stably -- fp32 rounding is monotone, so this is the fp64 log-softmax order with fp32 ties broken by token, the order
    rfn_log_softmax_topk documents.  Rows r % 3 == 0 hold quantised logits (many exact ties)."""
    N = nat()
    st = N.stream_ptr()
    rng = np.random.default_rng(V1)
    g = torch.Generator().manual_seed(V1)
    ld = max(V1 + 3, 48)                                    # the duplicated list holds up to 43 entries
    for rows in (1, 7, 160):
        x = torch.randn(rows, V1, generator=g) * 3.0
        x[::3] = torch.round(x[::3] * 2.0) / 2.0
        xd = x.to(dev)
        lp = torch.empty(rows, V1, device=dev)
        N.check(N.lib.rfn_log_softmax_fwd(xd.data_ptr(), V1, rows, V1, rows, V1, 0, lp.data_ptr(), st))
        lp_h = lp.cpu()
        for W in (1, 2, 5, 16, 32):
            if W > V1:
                continue
            tv0 = torch.empty(rows, W, device=dev)
            ti0 = torch.empty(rows, W, dtype=torch.int32, device=dev)
            N.check(N.lib.rfn_log_softmax_topk(xd.data_ptr(), V1, rows, V1, W, tv0.data_ptr(), ti0.data_ptr(), st))
            tv = torch.full((rows, W), 7.0, device=dev)
            ti = torch.full((rows, W), -7, dtype=torch.int32, device=dev)
            N.check(N.lib.rfn_log_softmax_topk_masked(xd.data_ptr(), V1, rows, V1, W, None, 0, None, tv.data_ptr(), ti.data_ptr(), st))
            assert torch.equal(ti.cpu(), ti0.cpu()) and torch.equal(bits(tv), bits(tv0))          # blk == NULL: the old kernel
            for shift in (range(5) if rows == 1 else (0,)):
                blk = torch.full((rows, ld), -1, dtype=torch.int32)
                blk_n = torch.zeros(rows, dtype=torch.int32)
                masked = lp_h.clone()
                for r in range(rows):
                    ids = _block_kind((r + shift) % 5, lp_h[r], W, V1, rng)
                    blk[r, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
                    blk_n[r] = len(ids)
                    if ids:
                        masked[r, ids] = -INF
                bd, nd = blk.to(dev), blk_n.to(dev)
                N.check(N.lib.rfn_log_softmax_topk_masked(xd.data_ptr(), V1, rows, V1, W, bd.data_ptr(), ld, nd.data_ptr(),
                                                          tv.data_ptr(), ti.data_ptr(), st))
                want_i = torch.sort(masked, dim=1, descending=True, stable=True).indices[:, :W]
                got_i = ti.cpu().long()
                assert torch.equal(got_i, want_i), (V1, rows, W, shift)
                assert torch.equal(bits(tv), bits(masked.gather(1, want_i))), (V1, rows, W, shift)


def test_logp_mask_rows_touches_only_the_listed_entries(dev):
    N = nat()
    rng = np.random.default_rng(5)
    for rows, V1 in ((1, 5), (130, 333), (7, 9488)):
        ld = V1 + 5
        buf = torch.randn(rows, ld)
        blk = torch.full((rows, 72), -1, dtype=torch.int32)
        blk_n = torch.zeros(rows, dtype=torch.int32)
        want = buf.clone()
        for r in range(rows):
            k = int(rng.integers(0, 73)) if r % 4 else 0
            ids = rng.integers(0, V1, size=k)                                   # duplicates included
            blk[r, :k] = torch.from_numpy(ids).to(torch.int32)
            blk[r, k:] = int(rng.integers(0, V1))                               # entries past blk_n[r] are not read
            blk_n[r] = k
            want[r, ids] = -INF
        d, bd, nd = buf.to(dev), blk.to(dev), blk_n.to(dev)
        N.check(N.lib.rfn_logp_mask_rows(d.data_ptr(), ld, rows, V1, bd.data_ptr(), 72, nd.data_ptr(), N.stream_ptr()))
        assert torch.equal(bits(d), bits(want))                                 # the padding columns V1 .. ld-1 included


# =================================================================================================================
# whole path
# =================================================================================================================
# (tier, seed, embed scale, logit scale, END bias): random weights of the tier's shapes.  The seeded weights give a nearly flat
# distribution that never ends a caption; scaling the embedding and the logit layer makes the fed token matter, and the END
# bias sits in the middle of the window (0.33 wide for tiny0, 2.2 for mid, in logits) in which the CPU oracle's greedy captions
# repeat a bigram AND some of them end after a few tokens.
MODELS = {'tiny0': ('tiny0', 104, 30.0, 100.0, 2.2537), 'mid': ('mid', 100, 100.0, 100.0, 11.2852)}
_cache = {}


def setup(name, dev, seq_length=None, low_id=None, seed_shift=0):
    from oracle import rfn_oracle as O
    import recurrent_fusion_network_amd as R
    key = (name, seq_length, low_id, seed_shift)
    if key not in _cache:
        tier, seed, es, ls, beta = MODELS[name]
        cfg, spec, _, batch, _ = load_case(tier)
        cfg = copy.copy(cfg)
        if seq_length is not None:
            cfg.seq_length = seq_length
        P = dict(O.seeded_params(cfg, seed + seed_shift))
        P['embed.weight'] = P['embed.weight'] * es
        P['logit.weight'] = P['logit.weight'] * ls
        b = P['logit.bias'].clone()
        b[0] += beta
        if low_id is not None:
            b[low_id] = -1e4                                                    # a token no decoder ever picks
        P['logit.bias'] = b
        model = R.RecurrentFusionModel(cfg)
        model.load_state_dict(P)
        model = model.to(dev).eval()
        fc, att = [f.to(dev) for f in batch[0]], [a.to(dev) for a in batch[1]]
        _cache[key] = (model, fc, att)
    return _cache[key]


def pad_seq(seq, S):
    out = torch.zeros(seq.size(0), S, dtype=torch.long)
    out[:, :seq.size(1)] = seq.cpu()
    return out


def same(a, b):
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape:
        return False
    return torch.equal(bits(a), bits(b)) if a.is_floating_point() else torch.equal(a, b)


def beams_of(done_beams):
    return [[(d['seq'].tolist(), bits(d['logps']).tolist(), np.float32(d['p']).tobytes()) for d in img] for img in done_beams]


def _members(models, fc, att, repeat=1):
    from recurrent_fusion_network_amd.decode import _Stepper
    out = []
    for m in models:
        comb, h, c, _ = m._prefix(fc, att, False, 0)
        if repeat > 1:
            comb = comb.repeat_interleave(repeat, dim=1).contiguous()
            h, c = h.repeat_interleave(repeat, dim=0).contiguous(), c.repeat_interleave(repeat, dim=0).contiguous()
        out.append(_Stepper(m, comb, h.clone(), c.clone()))
    return out


def _averaged_logp(N, steppers, ids, logit_sum, logit_m, out):
    """The ensemble's step (ensemble.py): members' logits summed, divided by their number, log-softmax."""
    rows, V1 = logit_sum.shape
    st = N.stream_ptr()
    for j, sp in enumerate(steppers):
        sp.step(ids, out=logit_sum if j == 0 else logit_m, want='logits')
        if j:
            N.check(N.lib.rfn_axpby_2d(1.0, logit_m.data_ptr(), V1, 1.0, logit_sum.data_ptr(), V1, rows, V1, st))
    N.check(N.lib.rfn_div_2d(logit_sum.data_ptr(), V1, rows, V1, float(len(steppers)), st))
    N.check(N.lib.rfn_log_softmax_fwd(logit_sum.data_ptr(), V1, rows, V1, rows, V1, 0, out.data_ptr(), st))


@torch.no_grad()
def host_sample(models, fc, att, cons, u=None, inv_temp=1.0):
    """sample() stepped from the host: every step's log-probs come back, get the restatement's mask, and the pick is made
    here (first maximum; a row of -inf picks 0) or, for the multinomial form, by rfn_multinomial_pick on the masked rows."""
    N = nat()
    m0 = models[0]
    B, S, V1 = fc[0].size(0), m0.seq_length, m0.vocab_size + 1
    dev = fc[0].device
    steppers = _members(models, fc, att)
    logit_sum, logit_m, logp = (torch.empty(B, V1, device=dev) for _ in range(3))
    it = torch.zeros(B, dtype=torch.long, device=dev)
    seq, slp = np.zeros((B, S), dtype=np.int64), np.zeros((B, S), dtype=np.float32)
    unf = np.ones(B, dtype=bool)
    t_stop = S + 1
    for t in range(S + 1):
        if t >= 1:
            masked = D.mask_rows(logp.cpu().numpy(), [seq[b, :t - 1] for b in range(B)], t, **cons)
            if u is None:
                pick = masked.argmax(1)
            else:
                md = torch.from_numpy(masked).to(dev)
                ud = u[t - 1].contiguous()
                N.check(N.lib.rfn_multinomial_pick(md.data_ptr(), V1, B, V1, inv_temp, ud.data_ptr(), None, 1.0, it.data_ptr(), 1,
                                                   N.stream_ptr()))
                pick = it.cpu().numpy()
            unf = unf & (pick > 0)
            seq[:, t - 1] = np.where(unf, pick, 0)
            slp[:, t - 1] = masked[np.arange(B), pick]
            if not unf.any() and t_stop == S + 1:
                t_stop = t
            it = torch.from_numpy(pick).to(dev)
        _averaged_logp(N, steppers, it, logit_sum, logit_m, logp)
    return torch.from_numpy(seq[:, :t_stop - 1]), torch.from_numpy(slp[:, :t_stop - 1])


@torch.no_grad()
def host_beam(models, fc, att, W, cons, alpha=0.0):
    """sample_beam stepped from the host with rfn_beam_step in its full-row form on the masked log-prob rows."""
    from recurrent_fusion_network_amd.decode import BeamBuffers, _sorted_done_beams
    N = nat()
    m0 = models[0]
    B, S, V1 = fc[0].size(0), m0.seq_length, m0.vocab_size + 1
    dev = fc[0].device
    st = N.stream_ptr()
    steppers = _members(models, fc, att, repeat=W)
    b = BeamBuffers(B, W, S, dev)
    rows, max_done, bs, bl, bsum, order, ids = b.rows, b.max_done, b.bs, b.bl, b.bsum, b.order, b.ids
    done_seq, done_lp, done_p, done_n, active = b.done_seq, b.done_lp, b.done_p, b.done_n, b.active
    logit_sum, logit_m, logp = (torch.empty(rows, V1, device=dev) for _ in range(3))
    for t in range(S + 1):
        if t >= 1:
            N.check(N.lib.rfn_beam_step(logp.data_ptr(), V1, V1, W, S, t, B, max_done, bs.data_ptr(), bl.data_ptr(), bsum.data_ptr(),
                                        order.data_ptr(), ids.data_ptr(), done_seq.data_ptr(), done_lp.data_ptr(), done_p.data_ptr(),
                                        done_n.data_ptr(), active.data_ptr(), st))
            if t == S:
                break
            for sp in steppers:
                sp.reorder(order)
        _averaged_logp(N, steppers, ids, logit_sum, logit_m, logp)
        hist = bs.cpu().numpy()[:t].reshape(t, rows).T                          # row k * W + w continues beam (k, w)
        logp.copy_(torch.from_numpy(D.mask_rows(logp.cpu().numpy(), hist, t + 1, **cons)).to(dev))
    return _sorted_done_beams(b, alpha)


def cons_of(opt):
    return dict(n=opt.get('block_ngram', 0), banned=opt.get('banned_ids', ()), bad_endings=opt.get('bad_endings', ()))


def bite_ids(model, fc, att):
    """(banned, bad_endings) for a model, read off its unconstrained greedy captions: the last word of a caption that ends,
    and the most frequent word."""
    S = model.seq_length
    seq = pad_seq(model.sample(fc, att, {})[0], S)
    bad = sorted({int(r[r.tolist().index(0) - 1]) for r in seq if 0 in r.tolist() and r.tolist().index(0) >= 1})
    words = seq[seq > 0]
    banned = [int(torch.mode(words).values)]
    return seq, banned, bad


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_constraints_bite(dev, name):
    """First the premise: the unconstrained greedy captions repeat a bigram and some end on a word of bad_endings.  Then no
    constrained caption (greedy or best beam) repeats an n-gram, holds a banned id, or has a bad ending right before END."""
    model, fc, att = setup(name, dev)
    S = model.seq_length
    with torch.no_grad():
        seq0, banned, bad = bite_ids(model, fc, att)
        assert any(D.has_repeated_ngram(r, 2) for r in seq0), seq0
        assert bad, seq0
        for n in (2, 3):
            opt = {'block_ngram': n, 'banned_ids': banned, 'bad_endings': bad}
            outs = [pad_seq(model.sample(fc, att, opt)[0], S), model.sample_beam(fc, att, dict(opt, beam_size=3))[0].cpu()]
            assert not torch.equal(outs[0], seq0)
            for seq in outs:
                for r in seq.tolist():
                    assert not D.has_repeated_ngram(r, n), (n, r)
                    assert not set(banned) & set(r), (banned, r)
                    if 0 in r and r.index(0) >= 1:
                        assert r[r.index(0) - 1] not in bad, (bad, r)


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_off_equals_today(dev, name):
    """Every constraint at its default, and constraints that cannot trigger (block_ngram = 4 on seq_length 3; a banned id whose
    logit bias is -1e4), give the tensors of the unconstrained call bit for bit -- through the constrained kernels."""
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    LOW = 7
    for S3, off in ((None, {'block_ngram': 0, 'banned_ids': [], 'bad_endings': [], 'length_penalty': 0.0}),
                    (None, {'banned_ids': [LOW]}), (3, {'block_ngram': 4})):
        model, fc, att = setup(name, dev, seq_length=S3, low_id=LOW)
        B, S = fc[0].size(0), model.seq_length
        ens = EnsembleDecoder([model])

        def same3(a, b):      # seq, seqLogprobs, and the full log-probs but for the banned column (-inf once masked)
            la, lb = a[2].clone(), b[2].clone()
            la[..., LOW], lb[..., LOW] = 0.0, 0.0
            return same(a[0], b[0]) and same(a[1], b[1]) and same(la, lb)

        with torch.no_grad():
            a, b = model.sample(fc, att, {}), model.sample(fc, att, dict(off))
            assert same3(a, b)
            model._ss_uniforms = torch.rand(2, S + 1, B, generator=torch.Generator().manual_seed(3)).to(dev)
            try:
                a, b = model.sample(fc, att, {'sample_max': 0}), model.sample(fc, att, dict(off, sample_max=0))
            finally:
                model._ss_uniforms = None
            assert same3(a, b)
            for W in (1, 3, 5):
                a = model.sample_beam(fc, att, {'beam_size': W})
                want = beams_of(model.done_beams)
                b = model.sample_beam(fc, att, dict(off, beam_size=W))
                assert same(a[0], b[0]) and same(a[1], b[1]) and beams_of(model.done_beams) == want
            a, b = ens.sample(fc, att), ens.sample(fc, att, dict(off))
            assert same3(a, b)
            a = ens.sample_beam(fc, att, {'beam_size': 3})
            want = beams_of(ens.done_beams)
            b = ens.sample_beam(fc, att, dict(off, beam_size=3))
            assert same(a[0], b[0]) and same(a[1], b[1]) and beams_of(ens.done_beams) == want


CASES = [dict(block_ngram=2), dict(block_ngram=3), dict(block_ngram=2, banned_ids='B', bad_endings='E'),
         dict(block_ngram=3, banned_ids='B', bad_endings='E')]


def _fill(case, banned, bad):
    return {k: (banned if v == 'B' else bad if v == 'E' else v) for k, v in case.items()}


@pytest.mark.parametrize('members', [1, 2])
@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_device_loops_equal_the_host_stepped_loop(dev, name, members):
    """members = 1: RecurrentFusionModel.sample / sample_beam AND the one-member EnsembleDecoder against the host-stepped loop;
    members = 2: the two-member ensemble's decoders against it."""
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    model, fc, att = setup(name, dev)
    models = [model] + [setup(name, dev, seed_shift=1)[0]] * (members - 1)
    ens = EnsembleDecoder(models)
    B, S = fc[0].size(0), model.seq_length
    with torch.no_grad():
        _, banned, bad = bite_ids(model, fc, att)
        for case in CASES:
            opt = _fill(case, banned, bad)
            want_seq, want_lp = host_sample(models, fc, att, cons_of(opt))
            got = [ens.sample(fc, att, opt)] + ([model.sample(fc, att, opt)] if members == 1 else [])
            for g in got:
                assert same(g[0], want_seq) and same(g[1], want_lp), (case, g[0], want_seq)
            for W in (2, 3, 5):
                want = host_beam(models, fc, att, W, cons_of(opt))
                bopt = dict(opt, beam_size=W)
                outs = [(ens.sample_beam(fc, att, bopt), ens)] + ([(model.sample_beam(fc, att, bopt), model)] if members == 1 else [])
                for out, owner in outs:
                    assert same(out[0], want[0]) and same(out[1], want[1]), (case, W)
                    assert beams_of(owner.done_beams) == beams_of(want[4]), (case, W)
        if members == 1:                                     # multinomial with fixed uniforms
            r = torch.rand(2, S + 1, B, generator=torch.Generator().manual_seed(11)).to(dev)
            for case in CASES[1:3]:
                opt = _fill(case, banned, bad)
                want_seq, want_lp = host_sample(models, fc, att, cons_of(opt), u=r[0, 1:], inv_temp=1.0 / 0.7)
                model._ss_uniforms = r
                try:
                    g = model.sample(fc, att, dict(opt, sample_max=0, temperature=0.7))
                finally:
                    model._ss_uniforms = None
                assert same(g[0], want_seq) and same(g[1], want_lp), (case, g[0], want_seq)


def test_length_penalty_reorders_the_done_beams(dev):
    model, fc, att = setup('mid', dev)
    S = model.seq_length
    changed = 0
    with torch.no_grad():
        base_out = model.sample_beam(fc, att, {'beam_size': 5})
        base = beams_of(model.done_beams)
        base_p = [list(p) for p in base_out[3]]
        for alpha in (0.5, 1.0):
            out = model.sample_beam(fc, att, {'beam_size': 5, 'length_penalty': alpha})
            got = beams_of(model.done_beams)
            for k, img in enumerate(base):
                ps = [float(np.frombuffer(d[2], dtype=np.float32)[0]) for d in img]
                rank = D.rank_done(ps, [D.caption_len(d[0], S) for d in img], alpha)
                assert got[k] == [img[i] for i in rank], (alpha, k)
                assert out[0][k].tolist() == img[rank[0]][0] and bits(out[1][k]).tolist() == img[rank[0]][1]
                assert list(out[3][k]) == [base_p[k][i] for i in rank]                     # top_prob: still the raw sums
                changed += rank[0] != 0
    assert changed > 0, 'no image whose best beam changes under the length penalty'


def test_refusals(dev):
    model, fc, att = setup('mid', dev)
    V1 = model.vocab_size + 1
    force = torch.ones(fc[0].size(0), model.seq_length, dtype=torch.long)
    beam = lambda f, a, o: model.sample_beam(f, a, dict(o, beam_size=2))  # noqa: E731
    with torch.no_grad():
        for bad in ({'banned_ids': list(range(1, 66))}, {'bad_endings': list(range(1, 66))}, {'banned_ids': [0]},
                    {'banned_ids': [V1]}, {'block_ngram': 1}, {'block_ngram': 5}):
            for call in (model.sample, beam):
                with pytest.raises(ValueError):
                    call(fc, att, bad)
        for cons in ({'block_ngram': 2}, {'banned_ids': [3]}, {'bad_endings': [3]}):
            with pytest.raises(ValueError):
                model.sample(fc, att, dict(cons, sample_max=0, force_ids=force))
        with pytest.raises(ValueError):
            beam(fc, att, {'length_penalty': 1.0, 'force_ids': force})
    N = nat()
    buf = torch.zeros(256, dtype=torch.int64, device=dev)
    args = lambda n, nb, ne: (buf.data_ptr(), 8, 1, None, 1, 4, 1, n, buf.data_ptr(), nb, buf.data_ptr(), ne, V1, buf.data_ptr(),  # noqa: E731
                              buf.data_ptr(), N.stream_ptr())
    assert N.lib.rfn_decode_blocklist(*args(2, 65, 0)) == -1 and N.lib.rfn_decode_blocklist(*args(2, 0, 65)) == -1
    assert N.lib.rfn_decode_blocklist(*args(1, 0, 0)) == -1 and N.lib.rfn_decode_blocklist(*args(5, 0, 0)) == -1
