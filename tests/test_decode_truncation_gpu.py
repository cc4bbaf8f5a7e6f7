"""GPU: truncated sampling (include/rfn.h "truncated sampling"): rfn_logp_truncate_rows through the C ABI against
the NumPy fp64 restatement (tests/decode_truncation_cpu.py, which also derives the `near` margin and caps the share of near
rows), its repeatability, the distribution of the draws that follow it, and rfn_decoder_loop_ex2 / RecurrentFusionModel.sample
with top_k / top_p / sample_n against a loop stepped from the host.

Apart from the near rule of the restatement everything is exact: the kernel only ever writes -inf, kept entries keep their
bits, and the loops are compared bit for bit."""
import numpy as np
import pytest
import torch

import decode_truncation_cpu as T
from test_decode_constraints_gpu import pad_seq, same, setup

pytestmark = pytest.mark.gpu
INF = float('inf')
SENTINEL = 7.0


def nat():
    import recurrent_fusion_network_amd._native as N
    return N


def ibits(a):
    return np.ascontiguousarray(a).view(np.int32)


def is_off(V1, k, p):
    return not 0 < k < V1 and p >= 1.0


def truncate(dev, x, ld, k, p, it):
    """x (rows, V1) numpy -> (the rows after the kernel, with their padding columns; kept_n with one guard entry)."""
    N = nat()
    rows, V1 = x.shape
    buf = torch.full((rows, ld), SENTINEL)
    buf[:, :V1] = torch.from_numpy(x)
    d = buf.to(dev)
    kept = torch.full((rows + 1,), -9, dtype=torch.int32, device=dev)
    N.check(N.lib.rfn_logp_truncate_rows(d.data_ptr(), ld, rows, V1, k, p, it, kept.data_ptr(), N.stream_ptr()))
    return d.cpu().numpy(), kept.cpu().numpy()


def check_against_restatement(P, out, kept, k, p, it, what):
    """out: the kernel's rows (padding included).  -> the number of near rows."""
    x, rows, V1 = P.X, P.rows, P.V1
    assert (out[:, V1:] == SENTINEL).all(), what                                   # the padding survives
    assert kept[rows] == -9, what                                                  # nothing past the last row
    got = out[:, :V1]
    if is_off(V1, k, p):                                                            # nothing is launched
        assert np.array_equal(ibits(got), ibits(x)) and (kept[:rows] == -9).all(), what
        return 0
    unt = ~P.touched
    assert np.array_equal(ibits(got[unt]), ibits(x[unt])), what                     # all -inf / NaN rows: bit for bit
    nan_row = np.isnan(x).any(1)
    assert (kept[:rows][nan_row] == -1).all() and (kept[:rows][unt & ~nan_row] == 0).all(), what
    got_mask = got > -INF
    assert np.array_equal(ibits(got)[got_mask], ibits(x)[got_mask]), what           # kept entries keep their bits
    assert (got_mask[P.touched].sum(1) == kept[:rows][P.touched]).all(), what       # kept_n
    got_mask[unt] = True
    ok, near = T.agrees(P, got_mask, k, p, it)
    assert ok.all(), (what, np.flatnonzero(~ok), near[~ok])
    assert near.sum() <= T.NEAR_CAP * rows, (what, near.sum())
    return int(near.sum())


# =================================================================================================================
# the kernel
# =================================================================================================================
@pytest.mark.parametrize('V1', T.V1S)
def test_truncate_rows_matches_the_restatement(dev, V1):
    """Every shape x every (top_k, top_p, inv_temperature) of the restatement's table, contiguous and with a padded row
    stride.  The rows carry 0, 1 or about half of their entries at -inf beforehand (so top_k = 50 exceeds the finite count of
    the short rows), every third row is rounded to multiples of 0.5 (ties across the cut), and the 130-row cases hold an
    all -inf row and a NaN row."""
    for rows in T.ROWS:
        P = T.Prepared(T.case(V1, rows))
        for k, p, it in T.params(V1):
            for ld in (V1, V1 + 3):
                out, kept = truncate(dev, P.X, ld, k, p, it)
                check_against_restatement(P, out, kept, k, p, it, (V1, rows, k, p, it, ld))
            if p == 1e-6 and k == 0:                                                # exactly the first maximum
                got = out[:, :V1] > -INF
                t = P.touched
                assert (got[t].sum(1) == 1).all() and (got[t].argmax(1) == P.order[t, 0]).all()


def test_flat_row_is_cut_by_count(dev):
    x, p = T.flat_case()
    P = T.Prepared(x)
    for it in T.INV_TEMPS:
        out, kept = truncate(dev, x, 1003, 0, p, it)
        assert check_against_restatement(P, out, kept, 0, p, it, ('flat', it)) == 0
        assert (kept[:3] == 334).all() and (out[:, :334] > -INF).all() and (out[:, 334:1000] == -INF).all()


def test_tie_group_straddling_the_cut_keeps_its_lowest_ids(dev):
    """Ten entries at -1 (scattered), 300 at -2, the rest far below.  top_k = 17: the ten and the SEVEN lowest ids of the -2
    group.  top_p = 0.2 at temperature 1: total 10 + 300 / e = 120.36, target 24.07, the ten give 10, so ceil(14.07 * e) = 39
    of the -2 group -- its 39 lowest ids.  Both: top_k = 100 first (ten + 90), total 43.11, p = 0.5 -> 21.55 -> 32 of them."""
    V1 = 700
    rng = np.random.default_rng(17)
    perm = rng.permutation(V1)
    ones, twos = np.sort(perm[:10]), np.sort(perm[10:310])
    x = np.full((2, V1), -40.0, dtype=np.float32)
    x[:, ones], x[:, twos] = -1.0, -2.0
    x[1, twos[3]] = -INF                                       # a blocked id inside the group: the next one moves up
    P = T.Prepared(x)
    for k, p, n_twos in ((17, 1.0, 7), (0, 0.2, 39), (100, 0.5, 32)):
        out, kept = truncate(dev, x, V1, k, p, 1.0)
        assert check_against_restatement(P, out, kept, k, p, 1.0, ('ties', k, p)) == 0
        for r in range(2):
            group = twos if r == 0 else np.delete(twos, 3)
            want = np.sort(np.concatenate([ones, group[:n_twos]]))
            assert np.array_equal(np.flatnonzero(out[r] > -INF), want), (k, p, r)
            assert kept[r] == 10 + n_twos


@pytest.mark.parametrize('V1', [9488, 15361])
def test_kept_set_is_repeatable(dev, V1):
    """The same 130 rows in reversed row order, at another (odd) row stride and alone (rows = 1) give the same bits: the kept
    set is a function of the row.  9488: keys staged in LDS; 15361: rows re-read."""
    x = T.case(V1, 130)
    for k, p, it in ((50, 0.9, 1.0), (0, 0.5, 2.5), (V1 - 1, 1.0, 1.0), (0, 0.9, 0.4)):
        base, kept = truncate(dev, x, V1, k, p, it)
        rev, kept_r = truncate(dev, x[::-1].copy(), V1, k, p, it)
        assert np.array_equal(ibits(rev[::-1]), ibits(base)) and np.array_equal(kept_r[:130][::-1], kept[:130])
        wide, kept_w = truncate(dev, x, V1 + 5, k, p, it)
        assert np.array_equal(ibits(wide[:, :V1]), ibits(base)) and np.array_equal(kept_w, kept)
        again, _ = truncate(dev, x, V1, k, p, it)
        assert np.array_equal(ibits(again), ibits(base))
        for r in (0, 1, 7, 11, 64, 129):
            one, kept_1 = truncate(dev, x[r:r + 1], V1, k, p, it)
            assert np.array_equal(ibits(one[0]), ibits(base[r])) and kept_1[0] == kept[r], (k, p, it, r)


def test_draws_follow_the_renormalised_kept_distribution(dev):
    """No statistics: one 5-word row copied to 4096 rows, row i drawn with u = (i + 0.5) / 4096.  The inverse-CDF draw then
    gives token v exactly the rows whose u falls into its stretch of the renormalised CDF: 4096 * p_v of them, give or take
    the two ends of the stretch -- within 2 -- and none for a cut token."""
    N = nat()
    n = 4096
    prob = np.array([0.15, 0.4, 0.05, 0.3, 0.1])
    x = np.tile(np.log(prob).astype(np.float32), (n, 1))
    u = ((torch.arange(n, dtype=torch.float64) + 0.5) / n).float().to(dev)
    for k, p, it, kept_ids in ((3, 1.0, 1.0, [1, 3, 0]), (0, 0.6, 1.0, [1, 3]), (0, 0.8, 1.0, [1, 3, 0]), (4, 0.85, 2.0, [1, 3]),
                               (1, 1.0, 1.0, [1]), (0, 1e-6, 1.0, [1])):
        d = torch.from_numpy(x).to(dev)
        ids = torch.full((n,), -1, dtype=torch.long, device=dev)
        N.check(N.lib.rfn_logp_truncate_rows(d.data_ptr(), 5, n, 5, k, p, it, None, N.stream_ptr()))
        N.check(N.lib.rfn_multinomial_pick(d.data_ptr(), 5, n, 5, it, u.data_ptr(), None, 1.0, ids.data_ptr(), 1, N.stream_ptr()))
        counts = np.bincount(ids.cpu().numpy(), minlength=5)
        w = np.zeros(5)
        w[kept_ids] = prob[kept_ids] ** it
        want = n * w / w.sum()
        assert counts.sum() == n and (counts[w == 0] == 0).all(), (k, p, it, counts)
        assert (np.abs(counts - want) <= 2).all(), (k, p, it, counts, want)


# =================================================================================================================
# the loop and sample()
# =================================================================================================================
TEMPERATURE = 1.5


def sample_with(model, fc, att, opt, r):
    model._ss_uniforms = r
    try:
        return model.sample(fc, att, opt)
    finally:
        model._ss_uniforms = None


def uniforms(S, rows, dev, seed):
    return torch.rand(2, S + 1, rows, generator=torch.Generator().manual_seed(seed)).to(dev)


@torch.no_grad()
def host_loop(model, fc, att, opt, r, inv_temp):
    """The device loop's calls issued from the host: _Stepper.step, then per step blocklist and mask (constraints), truncate,
    multinomial pick, record -- on buffers of the same layout."""
    from recurrent_fusion_network_amd.decode import GreedyBuffers, _Constraints, _Stepper
    N = nat()
    st = N.stream_ptr()
    comb, h, c, _ = model._prefix(fc, att, False, 0)
    B, S, V1 = h.size(0), model.seq_length, model.vocab_size + 1
    stepper = _Stepper(model, comb, h.clone(), c.clone())
    b = GreedyBuffers(B, S, V1, h.device, bos=True)
    cons = _Constraints.parse(opt, V1, S)
    if cons is not None:
        cons.bind(B, h.device)
    u = r[0, 1:].contiguous()
    for t in range(S + 1):
        if t >= 1:
            prev = b.logp_all[:, t - 1]
            if cons is not None:
                cons.blocklist(b.seq, b.seq.stride(0), 1, t)
                cons.mask(prev)
            N.check(N.lib.rfn_logp_truncate_rows(prev.data_ptr(), prev.stride(0), B, V1, opt.get('top_k', 0), opt.get('top_p', 1.0),
                                                 inv_temp, None, st))
            N.check(N.lib.rfn_multinomial_pick(prev.data_ptr(), prev.stride(0), B, V1, inv_temp, u[t - 1].data_ptr(), None, 1.0,
                                               b.it.data_ptr(), 1, st))
            N.check(N.lib.rfn_pick_record(prev.data_ptr(), prev.stride(0), B, V1, t, b.it.data_ptr(), b.it.data_ptr(),
                                          b.seq[:, t - 1].data_ptr(), b.seq.stride(0), b.seq_lp[:, t - 1].data_ptr(),
                                          b.seq_lp.stride(0), b.unf[t - 1].data_ptr() if t > 1 else None, b.unf[t].data_ptr(), st))
        stepper.step(b.it, out=b.logp_all[:, t])
    return b.read_back()


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_device_loop_equals_the_host_stepped_loop(dev, name):
    model, fc, att = setup(name, dev)
    B, S = fc[0].size(0), model.seq_length
    r = uniforms(S, B, dev, 21)
    cut = 0
    for trunc in ({'top_k': 5}, {'top_p': 0.8}, {'top_k': 8, 'top_p': 0.9}):
        for extra in ({}, {'block_ngram': 2}):
            opt = dict(trunc, **extra)
            want = host_loop(model, fc, att, opt, r, 1.0 / TEMPERATURE)
            with torch.no_grad():
                got = sample_with(model, fc, att, dict(opt, sample_max=0, temperature=TEMPERATURE), r)
            for g, w in zip(got[:3], want):
                assert same(g, w), (name, opt)
            cut += int((got[2][:, :-1] == -INF).sum())
    assert cut > 0                                                     # the truncation did cut something


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_truncated_log_probs_are_the_models_own(dev, name):
    """Replaying the sampled ids (force_ids) gives the untruncated log-probs of the same steps.  For every step a row takes
    while unfinished: the finite set of the returned log-probs is the restatement's mask of the untruncated row (near rule and
    cap), finite entries carry the untruncated bits, the sampled token is inside, and seq_lp is ITS untruncated log-prob."""
    model, fc, att = setup(name, dev)
    B, S = fc[0].size(0), model.seq_length
    k, p = 8, 0.9
    with torch.no_grad():
        seq, seq_lp, logp, _ = sample_with(model, fc, att, {'sample_max': 0, 'temperature': TEMPERATURE, 'top_k': k, 'top_p': p},
                                           uniforms(S, B, dev, 22))
        rseq, _, full, _ = model.sample(fc, att, {'sample_max': 0, 'force_ids': pad_seq(seq, S).to(dev)})
    assert same(rseq, seq)
    seq, seq_lp, logp, full = seq.cpu(), seq_lp.cpu(), logp.cpu(), full.cpu()
    n_seq = seq.size(1)
    alive = torch.ones(B, n_seq, dtype=torch.bool)                      # unfinished BEFORE token t
    alive[:, 1:] = torch.cumprod((seq[:, :-1] > 0).long(), 1).bool()
    bb, tt = torch.nonzero(alive, as_tuple=True)
    assert len(bb) >= B
    full_rows, cut_rows, tok = full[bb, tt].numpy(), logp[bb, tt].numpy(), seq[bb, tt].numpy()
    got_mask = cut_rows > -INF
    assert np.array_equal(ibits(cut_rows)[got_mask], ibits(full_rows)[got_mask])
    P = T.Prepared(full_rows)
    ok, near = T.agrees(P, got_mask, k, p, 1.0 / TEMPERATURE)
    assert ok.all() and near.sum() <= T.NEAR_CAP * len(bb), (np.flatnonzero(~ok), near.sum())
    assert (got_mask.sum(1) <= k).all() and (got_mask.sum(1) < k).any()          # both knobs cut somewhere
    rows = np.arange(len(bb))
    assert got_mask[rows, tok].all()
    assert np.array_equal(ibits(seq_lp[bb, tt].numpy()), ibits(full_rows[rows, tok]))


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_one_kept_token_is_greedy_and_all_off_is_todays_call(dev, name):
    model, fc, att = setup(name, dev)
    B, S = fc[0].size(0), model.seq_length
    with torch.no_grad():
        greedy = model.sample(fc, att, {})
        for one in ({'top_k': 1}, {'top_p': 1e-6}):
            got = sample_with(model, fc, att, dict(one, sample_max=0, temperature=TEMPERATURE), uniforms(S, B, dev, 23))
            assert same(got[0], greedy[0]) and same(got[1], greedy[1]), (name, one)
            assert ((got[2][:, :got[0].size(1)] > -INF).sum(2) == 1).all()
        # sample_max = 1 takes top_k / top_p and ignores them
        assert all(same(a, b) for a, b in zip(model.sample(fc, att, {'top_k': 3, 'top_p': 0.5})[:3], greedy[:3]))
        torch.manual_seed(5)
        a = model.sample(fc, att, {'sample_max': 0, 'temperature': TEMPERATURE})
        torch.manual_seed(5)
        b = model.sample(fc, att, {'sample_max': 0, 'temperature': TEMPERATURE, 'top_k': 0, 'top_p': 1.0, 'sample_n': 1})
        assert all(same(x, y) for x, y in zip(a[:3], b[:3]))
        assert not (b[2] == -INF).any()


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_sample_n_equals_repeated_features(dev, name):
    """n = 3 draws per image, stages I and II run once, against the same call on features repeated three times: the same
    (2, S + 1, 3B) uniforms give the same bits, image-major.  reason_pred stays per image."""
    model, fc, att = setup(name, dev)
    B, S, n = fc[0].size(0), model.seq_length, 3
    r = uniforms(S, B * n, dev, 24)
    opt = {'sample_max': 0, 'temperature': TEMPERATURE, 'top_k': 20, 'top_p': 0.95}
    with torch.no_grad():
        got = sample_with(model, fc, att, dict(opt, sample_n=n), r)
        want = sample_with(model, [f.repeat_interleave(n, dim=0) for f in fc], [a.repeat_interleave(n, dim=0) for a in att], opt, r)
        only_n = sample_with(model, fc, att, {'sample_max': 0, 'temperature': TEMPERATURE, 'sample_n': n}, r)
    assert got[0].size(0) == B * n and got[1].size(0) == B * n and got[2].size(0) == B * n
    for g, w in zip(got[:3], want[:3]):
        assert same(g, w), name
    assert all(t.size(0) == B for t in got[3]) and all(same(g, w[::n]) for g, w in zip(got[3], want[3]))
    seq = pad_seq(got[0], S).view(B, n, S)
    assert any(len({tuple(row.tolist()) for row in img}) == n for img in seq), seq      # an image whose draws all differ
    assert only_n[0].size(0) == B * n and not (only_n[2] == -INF).any()                 # sample_n alone: nothing is cut


def test_refusals(dev):
    from recurrent_fusion_network_amd.decode import GreedyBuffers, _Sampling, _Stepper, run_greedy_loop
    N = nat()
    model, fc, att = setup('mid', dev)
    B, S, V1 = fc[0].size(0), model.seq_length, model.vocab_size + 1
    force = torch.ones(B, S, dtype=torch.long)
    for on in ({'top_k': 5}, {'top_p': 0.9}, {'sample_n': 2}):
        with torch.enable_grad():
            with pytest.raises(N.RfnError):
                model.sample(fc, att, dict(on, sample_max=0))
        with torch.no_grad():
            with pytest.raises(ValueError):
                model.sample(fc, att, dict(on, sample_max=0, force_ids=force))
            with pytest.raises(ValueError):
                model.sample(fc, att, dict(on, sample_max=0, beam_size=3))
    with torch.no_grad():
        with pytest.raises(ValueError):
            model.sample(fc, att, {'sample_max': 1, 'sample_n': 2})
        for bad in ({'top_k': -1}, {'top_p': 0.0}, {'top_p': 1.5}, {'sample_n': 0}):
            with pytest.raises(ValueError):
                model.sample(fc, att, dict(bad, sample_max=0))
        with pytest.raises(N.RfnError):                                 # the uniforms of B rows, not of 2 B
            sample_with(model, fc, att, {'sample_max': 0, 'sample_n': 2}, uniforms(S, B, dev, 1))
        # the C entry point: rows_per_image must divide B; n > 1 needs the hoisted decoder cell
        comb, h, c, _ = model._prefix(fc, att, False, 0)
        stepper = _Stepper(model, comb, h.clone(), c.clone())
        bufs = GreedyBuffers(B, S, V1, dev)
        u = uniforms(S, B, dev, 2)[0, 1:].contiguous()
        with pytest.raises(N.RfnError):
            run_greedy_loop(stepper, bufs, 1, 1.0, u, None, _Sampling.parse({'sample_n': B + 1}))
        flags = model.path_flags
        model.path_flags = flags | N.PATH_OPT_DEC_UNHOISTED
        try:
            with pytest.raises(N.RfnError):
                model.sample(fc, att, {'sample_max': 0, 'sample_n': 2})
            out = model.sample(fc, att, {'sample_max': 0, 'top_k': 5})  # one row per image: the three-launch cell is fine
            assert out[0].size(0) == B
        finally:
            model.path_flags = flags
