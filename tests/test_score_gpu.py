"""Caption scoring on the GPU (include/rfn.h "caption scoring"): rfn_score_logits / rfn_score_captions through the C ABI against
the fp64 restatement (tests/score_cpu.py) and against rfn_log_softmax_fwd's bits; RecurrentFusionModel.score against the
teacher-forced pass, the reference oracle, the XE criterion and the decoders' own seqLogprobs; EnsembleDecoder.score; and
decode.rescore on kept beam candidates."""
import functools

import numpy as np
import pytest
import torch

import score_cpu as SC
from conftest import load_case
from test_model_gpu import build, to_dev

pytestmark = pytest.mark.gpu


def native():
    import recurrent_fusion_network_amd._native as N
    return N


# =================================================================================================================================
# 1. the kernels against the restatement
# =================================================================================================================================
def run_score_logits(x, ldl, B, T, V1, target, include_end, t0=0, ld_out=None, want=('rank', 'ent'), outs=None):
    """x: device float tensor whose data_ptr() is row 0 of the T * B time-major rows (stride ldl) of steps t0 .. t0 + T - 1."""
    N = native()
    ld_out = ld_out or (t0 + T)
    dev = x.device
    if outs is None:
        outs = (torch.full((B, ld_out), 7.0, device=dev), torch.full((B, ld_out), 7, dtype=torch.int32, device=dev),
                torch.full((B, ld_out), 7.0, device=dev))
    lp, rank, ent = outs
    N.check(N.lib.rfn_score_logits(x.data_ptr(), ldl, B, T, t0, V1, target.data_ptr(), target.stride(0), int(include_end),
                                   lp.data_ptr(), rank.data_ptr() if 'rank' in want else None,
                                   ent.data_ptr() if 'ent' in want else None, ld_out, N.stream_ptr()), 'rfn_score_logits')
    return lp, rank, ent


def log_softmax_rows(x, ldl, rows, V1):
    """rfn_log_softmax_fwd of the same rows -> (rows, V1)."""
    N = native()
    out = torch.empty(rows, V1, device=x.device)
    N.check(N.lib.rfn_log_softmax_fwd(x.data_ptr(), ldl, rows, V1, rows, V1, 0, out.data_ptr(), N.stream_ptr()), 'rfn_log_softmax_fwd')
    return out


def make_logits(gen, rows, V1, ldl, dev, misalign=False, quant=False):
    """rows x V1 seeded randn * 3 logits at row stride ldl -> (device buffer view starting at row 0, host (rows, V1) float32)."""
    host = torch.randn(rows, V1, generator=gen) * 3
    if quant:
        host = (host * 4).round() / 4
    buf = torch.full((rows * ldl + 1,), 123.0)                     # the padding behind a row is never read as data
    view = buf[1:] if misalign else buf[:-1]
    view.view(rows, ldl)[:, :V1] = host
    d = buf.to(dev)
    return (d[1:] if misalign else d[:-1]), host


def make_target(gen, B, T, V1):
    """Row 0 never ends; the last row (B > 1, T > 1) holds a 0 at column 1 with words behind it; the rest end at random."""
    t = torch.randint(1, max(V1, 2), (B, T + 1), generator=gen).clamp(max=V1 - 1)
    for b in range(1, B):
        cut = int(torch.randint(0, T + 1, (1,), generator=gen))
        if cut < T:
            t[b, cut] = 0
    if B > 1 and T > 1:
        t[B - 1, 1] = 0
        t[B - 1, 0] = max(V1 - 1, 0)
    return t


def check_against_restatement(x_dev, host, ldl, B, T, V1, target, include_end, quant=False):
    tgt_dev = target.to(x_dev.device)
    lp, rank, ent = run_score_logits(x_dev, ldl, B, T, V1, tgt_dev, include_end)
    full = log_softmax_rows(x_dev, ldl, T * B, V1).view(T, B, V1)
    want_lp, want_rank, want_ent = SC.score_logits(host.view(T, B, V1).numpy(), target.numpy(), include_end)
    live = SC.live_mask(target.numpy()[:, :T], V1, include_end)
    ids = torch.from_numpy(SC.clamp_ids(target.numpy()[:, :T], V1)).to(x_dev.device)
    gathered = full.permute(1, 0, 2).gather(2, ids.unsqueeze(2)).squeeze(2)               # (B, T): rfn_log_softmax_fwd's entries
    live_d = torch.from_numpy(live).to(x_dev.device)
    assert torch.equal(lp, torch.where(live_d, gathered, torch.zeros_like(gathered))), 'tok_lp is not the log-softmax entry'
    assert np.array_equal(rank.cpu().numpy(), want_rank), 'rank'
    got_ent, got_lp = ent.cpu().double().numpy(), lp.cpu().double().numpy()
    assert np.all(got_ent[~live] == 0.0)
    err = np.abs(got_ent - want_ent)
    print('score_logits B=%d T=%d V1=%d ldl=%d end=%d quant=%d: entropy err %.3g, lp err %.3g'
          % (B, T, V1, ldl, include_end, quant, err.max(), np.abs(got_lp - want_lp).max()))
    assert np.all(err <= 1e-5 * np.maximum(1.0, np.abs(want_ent)))
    assert np.all(np.abs(got_lp - want_lp) <= 1e-5 * np.maximum(1.0, np.abs(want_lp)))
    return lp, rank, ent


# (B, T, V1, ldl, misaligned base): scalar; vector, mostly padding lanes; one f32x4 per thread; one lane into the second; the
# headline vocabulary; the register limit; past it (scalar); a stride that is no multiple of 4 (scalar); padded vector rows; the
# base one float off alignment (scalar); the smallest call
SHAPES = [(3, 4, 50, 50, False), (2, 3, 52, 52, False), (2, 2, 1024, 1024, False), (2, 2, 1028, 1028, False),
          (2, 3, 9488, 9488, False), (1, 2, 10240, 10240, False), (1, 2, 10244, 10244, False), (2, 2, 1024, 1025, False),
          (2, 2, 1024, 1028, False), (2, 2, 1024, 1024, True), (1, 1, 1, 1, False)]


@pytest.mark.parametrize('B,T,V1,ldl,misalign', SHAPES)
def test_score_logits_against_the_restatement(dev, B, T, V1, ldl, misalign):
    gen = torch.Generator(device='cpu').manual_seed(1000 + V1 + ldl + int(misalign))
    target = make_target(gen, B, T, V1)
    for quant in (False, True):                       # multiples of 0.25: ties decide the rank
        x_dev, host = make_logits(gen, T * B, V1, ldl, dev, misalign, quant)
        if quant and V1 > 8:
            ids = SC.clamp_ids(target.numpy()[:, :T], V1)
            r = host.view(T, B, V1)
            assert any(int((r[t, b] == r[t, b, ids[b, t]]).sum()) > 1 for t in range(T) for b in range(B)), 'no tie to decide'
        for include_end in (1, 0):
            check_against_restatement(x_dev, host, ldl, B, T, V1, target, include_end, quant)


@pytest.mark.parametrize('V1', [50, 52])
def test_score_logits_target_cases(dev, V1):
    """First 0 at column 0; no 0; a 0 followed by words; an id < 0; an id >= V1; and a plain row -- on the scalar and the vector
    path, END included and not, the optional outputs present and absent."""
    B, T = 6, 4
    gen = torch.Generator(device='cpu').manual_seed(77 + V1)
    target = torch.randint(1, V1, (B, T + 2), generator=gen)
    target[0, 0] = 0
    target[2, 1] = 0
    target[3, 1] = -5
    target[4, 2] = V1 + 3
    target[5, 3] = 0
    x_dev, host = make_logits(gen, T * B, V1, V1, dev)
    for include_end in (1, 0):
        lp, rank, ent = check_against_restatement(x_dev, host, V1, B, T, V1, target, include_end)
        live = SC.live_mask(target.numpy()[:, :T], V1, include_end)
        assert live[1].all() and not live[0, 1:].any() and live[0, 0] == bool(include_end)
        assert live[2].tolist() == [True, bool(include_end), False, False] == live[3].tolist()
        assert live[4].tolist() == [True, True, bool(include_end), False]
        assert np.array_equal(rank.cpu().numpy() == -1, ~live) and np.all(lp.cpu().numpy()[~live] == 0.0)
        # without the optional outputs: the same tok_lp, and the NULL outputs are not written
        lp2, rank2, ent2 = run_score_logits(x_dev, V1, B, T, V1, target.to(dev), include_end, want=())
        assert torch.equal(lp2, lp) and bool((rank2 == 7).all()) and bool((ent2 == 7.0).all())
        # a wider output matrix: the columns behind t0 + T stay as they were
        lp3, rank3, _ = run_score_logits(x_dev, V1, B, T, V1, target.to(dev), include_end, ld_out=T + 3)
        assert torch.equal(lp3[:, :T], lp) and torch.equal(rank3[:, :T], rank) and bool((lp3[:, T:] == 7.0).all())


@pytest.mark.parametrize('B,T,V1', [(3, 4, 50), (2, 3, 9488)])
def test_one_step_at_a_time_is_the_whole_call(dev, B, T, V1):
    gen = torch.Generator(device='cpu').manual_seed(5 + V1)
    target = make_target(gen, B, T, V1)
    target[:, :3] = target[:, :3].clamp(min=1)                    # step 2 is live in every row
    x_dev, _ = make_logits(gen, T * B, V1, V1, dev)
    tgt = target.to(dev)
    lp, rank, ent = run_score_logits(x_dev, V1, B, T, V1, tgt, 1)
    outs = (torch.zeros_like(lp), torch.zeros_like(rank), torch.zeros_like(ent))
    lp1, rank1, ent1 = run_score_logits(x_dev[2 * B * V1:], V1, B, 1, V1, tgt, 1, t0=2, ld_out=T, outs=outs)
    assert torch.equal(lp1[:, 2], lp[:, 2]) and torch.equal(rank1[:, 2], rank[:, 2]) and torch.equal(ent1[:, 2], ent[:, 2])
    assert bool((lp[:, 2] != 0).all())
    for col in (0, 1, 3)[:T - 1]:
        assert bool((lp1[:, col] == 0).all()) and bool((rank1[:, col] == 0).all())       # only column t0 is written


@pytest.mark.parametrize('V1', [50, 1024])
def test_minus_inf_entries_and_a_nan_row(dev, V1):
    B, T = 3, 2
    gen = torch.Generator(device='cpu').manual_seed(9 + V1)
    target = torch.randint(1, V1, (B, T + 1), generator=gen)
    host = torch.randn(T * B, V1, generator=gen) * 3
    host[0, 5:20] = float('-inf')
    host[1, 3] = float('-inf')
    target[0, 0], target[1, 0] = 7, 3                             # rows 0 and 1 of step 0 score a -inf target
    x = host.to(dev)
    lp, rank, ent = run_score_logits(x, V1, B, T, V1, target.to(dev), 1)
    want_lp, want_rank, want_ent = SC.score_logits(host.view(T, B, V1).numpy(), target.numpy(), 1)
    assert lp[0, 0] == float('-inf') == lp[1, 0] and bool(torch.isfinite(ent).all())
    assert np.array_equal(rank.cpu().numpy(), want_rank)
    assert rank[0, 0] == V1 - 15 + 2                              # every finite entry, and the -inf entries 5 and 6 before 7
    assert np.all(np.abs(ent.cpu().double().numpy() - want_ent) <= 1e-5 * np.maximum(1.0, np.abs(want_ent)))
    # one NaN row: it is NaN, the others keep their bits
    bad = host.clone()
    bad[B + 1, 11] = float('nan')                                 # step 1, caption 1
    lp_n, rank_n, ent_n = run_score_logits(bad.to(dev), V1, B, T, V1, target.to(dev), 1)
    assert bool(torch.isnan(lp_n[1, 1])) and bool(torch.isnan(ent_n[1, 1]))
    tg = int(target[1, 1])
    assert int(rank_n[1, 1]) == int(((bad[B + 1] > bad[B + 1, tg]) | ((bad[B + 1] == bad[B + 1, tg]) & (torch.arange(V1) < tg))).sum())
    keep = torch.ones(B, T, dtype=torch.bool, device=dev)
    keep[1, 1] = False
    assert torch.equal(lp_n[keep], lp[keep]) and torch.equal(rank_n[keep], rank[keep]) and torch.equal(ent_n[keep], ent[keep])


@pytest.mark.parametrize('B,T', [(1, 1), (5, 7), (300, 17)])
def test_score_captions_is_the_host_loop(dev, B, T):
    N = native()
    V1 = 40
    gen = torch.Generator(device='cpu').manual_seed(B * 31 + T)
    target = torch.randint(-2, V1 + 2, (B, T + 2), generator=gen)           # zeros, and ids out of range that read as 0
    target[0] = 3
    tok = (torch.randn(B, T + 1, generator=gen) * 5).exp().neg()            # magnitudes from 1e-7 to 1e7: the order matters
    for include_end in (1, 0):
        cap = torch.full((B,), 7.0, dtype=torch.float64, device=dev)
        n = torch.full((B,), 7, dtype=torch.int32, device=dev)
        tok_d, tgt_d = tok.to(dev), target.to(dev)
        N.check(N.lib.rfn_score_captions(tok_d.data_ptr(), tok_d.stride(0), tgt_d.data_ptr(), tgt_d.stride(0), B, T, V1, include_end,
                                         cap.data_ptr(), n.data_ptr(), N.stream_ptr()), 'rfn_score_captions')
        want_cap, want_n = SC.score_captions(tok.numpy()[:, :T], target.numpy(), V1, include_end)
        assert np.array_equal(cap.cpu().numpy(), want_cap) and np.array_equal(n.cpu().numpy(), want_n)
        assert want_n[0] == T
        N.check(N.lib.rfn_score_captions(tok_d.data_ptr(), tok_d.stride(0), tgt_d.data_ptr(), tgt_d.stride(0), B, T, V1, include_end,
                                         cap.data_ptr(), None, N.stream_ptr()), 'rfn_score_captions')      # the length is optional
        assert np.array_equal(cap.cpu().numpy(), want_cap)


# =================================================================================================================================
# 2. - 6. the model
# =================================================================================================================================
@functools.lru_cache(maxsize=None)
def tier(name):
    """(cfg, P, model, device batch, host batch) of a golden tier, built once and shared (nothing below changes them)."""
    cfg, spec, P, batch, gold = load_case(name)
    dev = torch.device('cuda:0')
    return cfg, P, build(cfg, P, dev), to_dev(batch, dev), batch


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize('name', ['tiny0', 'mid', 'c2'])
def test_score_against_the_teacher_forced_pass(dev, name):
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    cfg, P, model, (fc, att, labels, masks, top), host = tier(name)
    if name == 'c2':
        assert bool((labels[:, 1:1 + cfg.seq_length] > 0).all())              # captions of exactly seq_length words
    with torch.no_grad():
        log_prob, reason = model(fc, att, labels)
    out = model.score(fc, att, labels[:, 1:], {'outputs': ('rank', 'entropy')})
    rows, S = labels.size(0), log_prob.size(1)
    steps = cfg.seq_length + 1
    tok = out['token_logprobs']
    assert tuple(tok.shape) == (rows, steps) and tok.dtype == torch.float32
    assert out['logprob'].dtype == torch.float64 and out['length'].dtype == torch.int32 and out['score'].dtype == torch.float64
    assert out['rank'].dtype == torch.int32 and out['entropy'].dtype == torch.float32
    target = labels[:, 1:1 + S]
    live = torch.from_numpy(SC.live_mask(labels[:, 1:].cpu().numpy(), cfg.vocab_size + 1, True)).to(dev)
    assert bool(live[:, S:].logical_not().all())
    gathered = log_prob.gather(2, target.unsqueeze(2)).squeeze(2)
    assert torch.equal(tok[:, :S], torch.where(live[:, :S], gathered, torch.zeros_like(gathered)))
    assert bool((tok[:, S:] == 0).all())
    # the reference's log-probs
    o_lp, _ = O.forward(cfg, P, *host[:3])
    o_g = o_lp.gather(2, host[2][:, 1:1 + S].unsqueeze(2)).squeeze(2)
    err = float(((tok[:, :S].cpu() - o_g) * live[:, :S].cpu()).abs().max())
    print('%s: token log-probs against the oracle: %.3g' % (name, err))
    assert err < 1e-3
    # the XE criterion's language term
    crit = R.ReviewNetEnsembleCriterion(cfg)
    loss = float(crit(log_prob, labels[:, 1:], masks[:, 1:], reason, top, 0.0))
    got = float(-out['logprob'].sum() / rows)
    print('%s: -logprob.sum() / rows = %.9g, criterion %.9g' % (name, got, loss))
    assert abs(got - loss) <= 2e-6 * max(1.0, abs(loss))
    # the sums, the lengths and the optional outputs agree with the per-token output
    cap, n = SC.score_captions(tok.cpu().numpy(), labels[:, 1:].cpu().numpy(), cfg.vocab_size + 1, True)
    assert np.array_equal(out['logprob'].cpu().numpy(), cap) and np.array_equal(out['length'].cpu().numpy(), n)
    assert torch.equal(out['score'], out['logprob'])                          # alpha = 0 divides by 1
    assert torch.equal(out['rank'] >= 0, live) and bool((out['entropy'][~live] == 0).all()) and bool((out['entropy'][live] > 0).all())
    lp_rank = (log_prob > gathered.unsqueeze(2)).sum(2)                       # ties aside, the rank counts the larger entries
    assert bool((out['rank'][:, :S][live[:, :S]] >= lp_rank[live[:, :S]]).all())
    ent = -(log_prob.double().exp() * log_prob.double()).sum(2)
    assert float(((out['entropy'][:, :S].double() - ent) * live[:, :S]).abs().max()) <= 1e-5 * max(1.0, float(ent.max()))
    # the words alone, and the module's mode does not matter
    words = model.score(fc, att, labels[:, 1:], {'include_end': False})
    assert sorted(words) == ['length', 'logprob', 'score', 'token_logprobs']
    wl = torch.from_numpy(SC.live_mask(labels[:, 1:].cpu().numpy(), cfg.vocab_size + 1, False)).to(dev)
    assert torch.equal(words['token_logprobs'], torch.where(wl, tok, torch.zeros_like(tok)))
    assert torch.equal(words['length'], out['length'] - 1)
    model.train()
    try:
        again = model.score(fc, att, labels[:, 1:])
    finally:
        model.eval()
    assert torch.equal(again['token_logprobs'], tok) and not again['logprob'].requires_grad


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_n_captions_per_image_and_chunking(dev, name):
    cfg, P, model, (fc, att, labels, masks, top), _ = tier(name)
    B, n, T = labels.size(0), 3, cfg.seq_length
    gen = torch.Generator(device='cpu').manual_seed(4)
    seq = torch.randint(1, cfg.vocab_size + 1, (B, n, T), generator=gen)
    for k in range(B):
        for j in range(n):
            seq[k, j, int(torch.randint(0, T + 1, (1,), generator=gen)):] = 0
    seq = seq.to(dev)
    opt = {'outputs': ('rank', 'entropy'), 'length_penalty': 0.5}
    one = model.score(fc, att, seq, opt)
    rep = model.score([f.repeat_interleave(n, 0) for f in fc], [a.repeat_interleave(n, 0) for a in att], seq.view(B * n, T), opt)
    flat = model.score(fc, att, seq.view(B * n, T), dict(opt, n=n))
    assert sorted(one) == ['entropy', 'length', 'logprob', 'rank', 'score', 'token_logprobs']
    for k in one:
        assert bits_equal(one[k], rep[k]) and bits_equal(one[k], flat[k]), k
    assert tuple(one['token_logprobs'].shape) == (B * n, T + 1)
    for max_rows in (n, 2 * n + 1, 1):                                         # one image per call; a remainder; below n
        part = model.score(fc, att, seq, dict(opt, max_rows=max_rows))
        for k in one:
            assert bits_equal(one[k], part[k]), (k, max_rows)
    want = one['logprob'].cpu().numpy() / np.array([1.0] + [float(k) ** 0.5 for k in range(1, T + 2)])[one['length'].cpu().numpy()]
    assert np.array_equal(one['score'].cpu().numpy(), want)


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_score_returns_the_decoders_own_logprobs(dev, name):
    cfg, P, model, (fc, att, labels, masks, top), _ = tier(name)
    S = cfg.seq_length

    def check(seq, seq_lp, feats, opt):
        out = model.score(*feats, seq, dict(opt, include_end=False))
        tok, w = out['token_logprobs'], seq.size(1)
        assert torch.equal(tok[:, :w], torch.where(seq > 0, seq_lp, torch.zeros_like(seq_lp)))
        assert bool((tok[:, w:] == 0).all())
        return out

    with torch.no_grad():
        seq, seq_lp, _, _ = model.sample(fc, att, {'sample_max': 1})
        check(seq, seq_lp, (fc, att), {})
        torch.manual_seed(11)
        seq, seq_lp, _, _ = model.sample_group(fc, att, 3)
        assert seq.size(0) == 3 * labels.size(0) and bool((seq > 0).any())       # draws hold words, whatever the argmax is
        check(seq, seq_lp, (fc, att), {'n': 3})
        seq, seq_lp, _, top_prob, _ = model.sample_beam(fc, att, {'beam_size': 3})
    out = check(seq, seq_lp, (fc, att), {})
    # the fp64 sum of a done beam against its fp32 running sum p: p covers the beam's END when it has one
    with_end = model.score(fc, att, seq)
    ended = (seq == 0).any(1)
    logprob = torch.where(ended, with_end['logprob'], out['logprob'])
    tok = torch.where(ended[:, None], with_end['token_logprobs'], out['token_logprobs'])
    p = torch.tensor([tp[0] for tp in top_prob], dtype=torch.float64, device=dev)
    bound = S * 2.0 ** -24 * tok.double().abs().sum(1)
    print('%s: |logprob - p| %s, bound %s' % (name, (logprob - p).abs().tolist(), bound.tolist()))
    assert bool(((logprob - p).abs() <= bound).all())


def test_ensemble_score(dev):
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    from oracle import rfn_oracle as O
    cfg, P, model, (fc, att, labels, masks, top), _ = tier('mid')
    opt = {'outputs': ('rank', 'entropy'), 'length_penalty': 0.3}
    one = EnsembleDecoder([model]).score(fc, att, labels[:, 1:], opt)
    ref = model.score(fc, att, labels[:, 1:], opt)
    assert sorted(one) == sorted(ref)
    for k in ref:
        assert bits_equal(one[k], ref[k]), k
    other = build(cfg, O.seeded_params(cfg, 12345), dev)
    two = EnsembleDecoder([model, other])
    got = two.score(fc, att, labels[:, 1:])
    with torch.no_grad():
        lps = [m(fc, att, labels)[0].double() for m in (model, other)]
    S = lps[0].size(1)
    mean = torch.log_softmax((lps[0] + lps[1]) / 2, 2)             # shift-invariant: the log-softmax of the mean logits
    live = torch.from_numpy(SC.live_mask(labels[:, 1:].cpu().numpy(), cfg.vocab_size + 1, True)).to(dev)
    want = mean.gather(2, labels[:, 1:1 + S].unsqueeze(2)).squeeze(2) * live[:, :S]
    err = float((got['token_logprobs'][:, :S].double() - want).abs().max())
    print('two-member ensemble against the mean-logits rule: %.3g' % err)
    assert err <= 1e-5 and bool((got['token_logprobs'][:, S:] == 0).all())
    assert float((got['token_logprobs'] - ref['token_logprobs']).abs().max()) > 1e-3           # the second member matters
    # n = 2 captions per image against repeated features
    B, T = labels.size(0), cfg.seq_length
    seq = torch.stack([labels[:, 1:1 + T], labels.flip(0)[:, 1:1 + T]], 1).contiguous()
    pair = two.score(fc, att, seq, opt)
    rep = two.score([f.repeat_interleave(2, 0) for f in fc], [a.repeat_interleave(2, 0) for a in att], seq.view(2 * B, T), opt)
    for k in rep:
        assert bits_equal(pair[k], rep[k]), k
    assert torch.equal(pair['token_logprobs'][0::2], two.score(fc, att, labels[:, 1:1 + T], opt)['token_logprobs'])


def test_rescore_kept_beam_candidates(dev):
    from recurrent_fusion_network_amd import decode
    cfg, P, model, (fc, att, labels, masks, top), _ = tier('mid')
    with torch.no_grad():
        model.sample_beam(fc, att, {'beam_size': 4, 'keep_candidates': True})
    cands, n_cand = model.candidates['seq'], model.candidates['n_cand']
    B, m, S = cands.shape
    assert m == 4 and bool((n_cand >= 1).all())
    n_cand = n_cand.clone()
    n_cand[0], n_cand[1] = 0, 2                                    # an image without candidates, and one with two
    fc_r, att_r = [f.repeat_interleave(m, 0) for f in fc], [a.repeat_interleave(m, 0) for a in att]
    for alpha in (0.0, 0.7):
        opt = {'length_penalty': alpha} if alpha else {}
        best, scores = decode.rescore(model, fc, att, cands, n_cand, opt)
        assert best.dtype == torch.int64 and tuple(best.shape) == (B,) and scores.dtype == torch.float64 and tuple(scores.shape) == (B, m)
        each = model.score(fc_r, att_r, cands.view(B * m, S), opt)                  # every candidate on its own row
        valid = (torch.arange(m, device=dev)[None, :] < n_cand[:, None])
        assert torch.equal(scores[valid], each['score'].view(B, m)[valid])
        assert bool((scores[~valid] == float('-inf')).all()) and int((~valid).sum()) == int((m - n_cand).sum()) >= 6
        # the pick: a host re-sort of (logprob, length), first maximum
        lp, ln, nc = each['logprob'].view(B, m).cpu().tolist(), each['length'].view(B, m).cpu().tolist(), n_cand.cpu().tolist()
        want = []
        for k in range(B):
            sc = [lp[k][j] / (float(ln[k][j]) ** alpha if ln[k][j] else 1.0) for j in range(nc[k])]
            want.append(sc.index(max(sc)) if sc else -1)
        assert best.cpu().tolist() == want and want[0] == -1 and want[1] in (0, 1)
    all_best, all_scores = decode.rescore(model, fc, att, cands)                     # n_cand = None: every candidate counts
    assert bool(torch.isfinite(all_scores).all()) and bool((all_best >= 0).all())
    assert torch.equal(all_scores, model.score(fc, att, cands)['score'].view(B, m))
