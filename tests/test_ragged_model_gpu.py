"""Ragged attention maps through the model (`att_lens`, INTEGRATION.md "Ragged attention maps"): a tiny eval-mode configuration
(the tiny* goldens' options) with M = 2 encoders, maps (7, 8) and (12, 12), B = 3, lengths [[7, 1, 4], [12, 5, 9]].

1. Row b against image b ALONE, each map truncated to its length, through oracle/rfn_oracle.py: forward log-probs (LOGP_TOL of
   tests/test_model_gpu.py), the loss, every parameter gradient (that file's 1e-5 + 1e-3 * max|g|; the batch criterion divides by
   B, so the batch gradient is the mean of the three single-image ones), greedy ids (skipped from the first step whose top-2
   margin is under 1e-4: that file's `safe` rule).
2. Zeros against large finite noise in the padded rows: log-probs, loss and gradients torch.equal.
3. att_lens of full lengths is the call without it, bit for bit: forward, forward_loss + backward, sample, sample_beam, score.
4. sample_beam, sample_group, sample_distinct, score, get_thought_vectors and EnsembleDecoder.sample_beam with att_lens on one
   padded image agree with the same call on that image's truncated maps (a model built for those map sizes, same weights).
5. A path_flags form that was not taught lengths is refused by name."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LOGP_TOL = 1e-3                      # tests/test_model_gpu.py
LENS = [[7, 1, 4], [12, 5, 9]]
MAPS = [(7, 8), (12, 12)]
B = 3
DEV = 'cuda:0'


def cfg_for(att_nums):
    from oracle import rfn_oracle as O
    info = [dict(att_num=n, att_feat_size=D, fc_feat_size=D) for n, (_, D) in zip(att_nums, MAPS)]
    return O.make_cfg(info, vocab_size=50, rnn_size=16, input_encoding_size=16, att_hid_size=16, num_review_steps_0=3,
                      num_review_steps=3, top_words_count=20, seq_length=5)


def build(cfg, P):
    import recurrent_fusion_network_amd as R
    m = R.RecurrentFusionModel(cfg)
    m.load_state_dict(P)
    return m.to(DEV).eval()


def dv(ts):
    return [t.to(DEV) for t in ts]


def padded(att, std, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = [a.clone() for a in att]
    for i, a in enumerate(out):
        for b in range(B):
            pad = a[b, LENS[i][b]:]
            a[b, LENS[i][b]:] = torch.randn(pad.shape, generator=g) * std if std else torch.zeros_like(pad)
    return out


@pytest.fixture(scope='module')
def world():
    """The model, one batch, and the oracle's answer for every image alone on its truncated maps (computed once, read-only)."""
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    cfg = cfg_for([L for L, _ in MAPS])
    P = O.seeded_params(cfg, 11)
    fc, att, labels, masks, top = O.synthetic_batch(cfg, B, seed=21)
    att = padded(att, 1e3)
    single = []
    for b in range(B):
        fc_b = [f[b:b + 1] for f in fc]
        att_b = [a[b:b + 1, :LENS[i][b]] for i, a in enumerate(att)]
        loss, grads = O.train_step_loss_and_grads(cfg, P, fc_b, att_b, labels[b:b + 1], masks[b:b + 1], top[b:b + 1], 1.0)
        with torch.no_grad():
            lp, _ = O.forward(cfg, P, fc_b, att_b, labels[b:b + 1])
            seq, _, lp_all, _ = O.sample_greedy(cfg, P, fc_b, att_b)
        single.append(dict(loss=loss, grads=grads, lp=lp, seq=seq, lp_all=lp_all, fc=fc_b, att=att_b))
    return dict(cfg=cfg, P=P, model=build(cfg, P), crit=R.ReviewNetEnsembleCriterion(cfg), fc=fc, att=att, labels=labels,
                masks=masks, top=top, single=single)


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def loss_and_grads(w, att, att_lens, fused=True):
    m = w['model']
    m.zero_grad(set_to_none=True)
    lab, msk, top = w['labels'].to(DEV), w['masks'].to(DEV), w['top'].to(DEV)
    if fused:
        loss, _ = m.forward_loss(dv(w['fc']), dv(att), lab, msk, top, w['crit'], 1.0, att_lens=att_lens)
    else:
        lp, heads = m(dv(w['fc']), dv(att), lab, att_lens=att_lens)
        loss = w['crit'](lp, lab[:, 1:], msk[:, 1:], heads, top, 1.0)
    loss.backward()
    return loss.detach(), grads_of(m)


# ---- 1. against each image alone -------------------------------------------------------------------------------------------
def test_rows_match_each_image_alone(world):
    w = world
    m = w['model']
    with torch.no_grad():
        lp, _ = m(dv(w['fc']), dv(w['att']), w['labels'].to(DEV), att_lens=LENS)
        seq, _, _, _ = m.sample(dv(w['fc']), dv(w['att']), {'sample_max': 1}, att_lens=LENS)
    lp, seq = lp.cpu(), seq.cpu()
    for b, s in enumerate(w['single']):
        err = float((lp[b:b + 1] - s['lp']).abs().max())
        print('image %d: log_prob err %.3g' % (b, err))
        assert err < LOGP_TOL, (b, err)
        top2 = s['lp_all'].topk(2, dim=2).values[0]
        for t in range(s['seq'].size(1)):
            if float(top2[t, 0] - top2[t, 1]) <= 1e-4:
                break
            assert int(seq[b, t]) == int(s['seq'][0, t]) if t < seq.size(1) else int(s['seq'][0, t]) == 0, (b, t)
    want_loss = sum(float(s['loss']) for s in w['single']) / B
    for fused in (True, False):
        loss, grads = loss_and_grads(w, w['att'], LENS, fused)
        print('fused %d: loss %.7f, mean of the single-image losses %.7f' % (fused, float(loss), want_loss))
        assert abs(float(loss) - want_loss) < 1e-3 * max(1.0, abs(want_loss))
        assert set(grads) == set(w['single'][0]['grads'])
        for k, g in grads.items():
            ref = sum(s['grads'][k] for s in w['single']) / B
            err = float((g.cpu() - ref).abs().max())
            assert err < 1e-5 + 1e-3 * float(ref.abs().max()), (k, err, float(ref.abs().max()))


def test_device_lengths_and_one_vector_for_all(world):
    w = world
    m = w['model']
    lab = w['labels'].to(DEV)
    with torch.no_grad():
        want, _ = m(dv(w['fc']), dv(w['att']), lab, att_lens=LENS)
        got, _ = m(dv(w['fc']), dv(w['att']), lab, att_lens=[torch.tensor(v, device=DEV) for v in LENS])
        assert torch.equal(want, got)
        # beyond the map on the device: clamped by the kernels, no read-back
        got, _ = m(dv(w['fc']), dv(w['att']), lab, att_lens=[torch.tensor([99, 1, 4], device=DEV), torch.tensor([12, 5, 9], device=DEV)])
        assert torch.equal(want, got)
        one, _ = m(dv(w['fc']), dv(w['att']), lab, att_lens=[7, 1, 4])
        per, _ = m(dv(w['fc']), dv(w['att']), lab, att_lens=[[7, 1, 4], [7, 1, 4]])
        assert torch.equal(one, per) and not torch.equal(one, want)


# ---- 2. the padding is never read ----------------------------------------------------------------------------------------------
def test_padding_invariance(world):
    w = world
    m = w['model']
    zeros, noise = padded(w['att'], 0.0), padded(w['att'], 1e3, seed=6)
    with torch.no_grad():
        a, _ = m(dv(w['fc']), dv(zeros), w['labels'].to(DEV), att_lens=LENS)
        b, _ = m(dv(w['fc']), dv(noise), w['labels'].to(DEV), att_lens=LENS)
    assert torch.equal(a, b)
    la, ga = loss_and_grads(w, zeros, LENS)
    lb, gb = loss_and_grads(w, noise, LENS)
    assert torch.equal(la, lb) and set(ga) == set(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # ... and it IS read without the lengths (the test would otherwise prove nothing)
    with torch.no_grad():
        c, _ = m(dv(w['fc']), dv(noise), w['labels'].to(DEV))
    assert not torch.equal(a, c)


# ---- 3. full lengths ------------------------------------------------------------------------------------------------------------
def test_full_lengths_are_the_plain_calls(world):
    w = world
    m = w['model']
    full = [[L] * B for L, _ in MAPS]
    fc, att, lab = dv(w['fc']), dv(w['att']), w['labels'].to(DEV)
    with torch.no_grad():
        for lens in (full, [None, None], [None, full[1]]):
            a, ra = m(fc, att, lab)
            b, rb = m(fc, att, lab, att_lens=lens)
            assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(ra, rb))
        for x, y in zip(m.sample(fc, att, {'sample_max': 1})[:2], m.sample(fc, att, {'sample_max': 1}, att_lens=full)[:2]):
            assert torch.equal(x, y)
        for x, y in zip(m.sample_beam(fc, att, {'beam_size': 3})[:2], m.sample_beam(fc, att, {'beam_size': 3}, att_lens=full)[:2]):
            assert torch.equal(x, y)
        cap = lab[:, 1:]
        sa, sb = m.score(fc, att, cap), m.score(fc, att, cap, att_lens=full)
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    for fused in (True, False):
        la, ga = loss_and_grads(w, w['att'], None, fused)
        lb, gb = loss_and_grads(w, w['att'], full, fused)
        assert torch.equal(la, lb) and set(ga) == set(gb)
        for k in ga:
            assert torch.equal(ga[k], gb[k]), k


# ---- 4. every decode mode on one image --------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def one_image(world):
    """Image 1 (lengths 1 and 5): its padded maps with att_lens on the model, its truncated maps on a model built for them."""
    w, b = world, 1
    lens = [[LENS[0][b]], [LENS[1][b]]]
    cfg_small = cfg_for([lens[0][0], lens[1][0]])
    small = build(cfg_small, w['P'])
    P2 = {k: v * 0.9 for k, v in w['P'].items()}       # a second ensemble member: other weights, the same on both sides
    return dict(big=w['model'], small=small, big2=build(w['cfg'], P2), small2=build(cfg_small, P2), lens=lens, fc=dv([f[b:b + 1] for f in w['fc']]),
                att=dv([a[b:b + 1] for a in w['att']]), att_t=dv(w['single'][b]['att']), cap=w['labels'][b:b + 1, 1:].to(DEV))


def close(a, b):
    assert a.shape == b.shape
    fin = torch.isfinite(a.double())
    assert torch.equal(fin, torch.isfinite(b.double()))
    return float((a.double()[fin] - b.double()[fin]).abs().max()) < LOGP_TOL if bool(fin.any()) else True


def test_beam_on_one_image(one_image):
    o = one_image
    with torch.no_grad():
        a = o['big'].sample_beam(o['fc'], o['att'], {'beam_size': 3}, att_lens=o['lens'])
        b = o['small'].sample_beam(o['fc'], o['att_t'], {'beam_size': 3})
    assert torch.equal(a[0], b[0]) and close(a[1], b[1])
    with torch.no_grad():      # sample() forwards the keyword to the beam search
        c = o['big'].sample(o['fc'], o['att'], {'beam_size': 3}, att_lens=o['lens'])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_sample_group_on_one_image(one_image):
    o = one_image
    with torch.no_grad():
        torch.manual_seed(3)
        a = o['big'].sample_group(o['fc'], o['att'], 2, att_lens=o['lens'])
        torch.manual_seed(3)
        b = o['small'].sample_group(o['fc'], o['att_t'], 2)
    assert a[0].size(0) == 2 and torch.equal(a[0], b[0]) and close(a[1], b[1])


def test_sample_distinct_on_one_image(one_image):
    o = one_image
    with torch.no_grad():
        a = o['big'].sample_distinct(o['fc'], o['att'], 2, {'seed': 17}, att_lens=o['lens'])
        la = o['big'].stochastic_beams['logprob'].clone()
        b = o['small'].sample_distinct(o['fc'], o['att_t'], 2, {'seed': 17})
        lb = o['small'].stochastic_beams['logprob'].clone()
    assert torch.equal(a[0], b[0]) and close(a[1], b[1]) and close(la, lb)


def test_score_and_thoughts_on_one_image(one_image):
    from recurrent_fusion_network_amd.decode import rescore
    o = one_image
    a = o['big'].score(o['fc'], o['att'], o['cap'], att_lens=o['lens'])
    b = o['small'].score(o['fc'], o['att_t'], o['cap'])
    assert close(a['token_logprobs'], b['token_logprobs']) and close(a['logprob'], b['logprob'])
    assert torch.equal(a['length'], b['length'])
    cands = torch.stack([o['cap'][:, :5], o['cap'][:, :5].flip(1)], 1)
    ra = rescore(o['big'], o['fc'], o['att'], cands, att_lens=o['lens'])
    rb = rescore(o['small'], o['fc'], o['att_t'], cands)
    assert torch.equal(ra[0], rb[0]) and close(ra[1], rb[1])
    ta = o['big'].get_thought_vectors(o['fc'], o['att'], att_lens=o['lens'])
    tb = o['small'].get_thought_vectors(o['fc'], o['att_t'])
    assert float((ta[0] - tb[0]).abs().max()) < 1e-5
    # ... and from a given state (rfn_prefix_fwd_from_state_ex)
    tc = o['big'].get_thought_vectors(o['fc'], o['att'], o['big'].get_init_state(o['fc']), att_lens=o['lens'])
    assert float((ta[0] - tc[0]).abs().max()) < 1e-5
    td = o['big'].get_thought_vectors(o['fc'], o['att'], o['big'].get_init_state(o['fc']))
    assert float((tc[0] - td[0]).abs().max()) > 1e-5      # the padding (noise) would have been attended to


def test_ensemble_beam_on_one_image(one_image):
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    o = one_image
    big2, small2 = o['big2'], o['small2']
    with torch.no_grad():
        a = EnsembleDecoder([o['big'], big2]).sample_beam(o['fc'], o['att'], {'beam_size': 3}, att_lens=o['lens'])
        b = EnsembleDecoder([o['small'], small2]).sample_beam(o['fc'], o['att_t'], {'beam_size': 3})
    assert torch.equal(a[0], b[0]) and close(a[1], b[1])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_untaught_forms_are_refused_by_name(world):
    import recurrent_fusion_network_amd._native as N
    w = world
    m = build(w['cfg'], w['P'])
    fc, att, lab = dv(w['fc']), dv(w['att']), w['labels'].to(DEV)
    for bit, name in ((N.PATH_OPT_PERSIST_S2_FWD, 'RFN_PATH_OPT_PERSIST_S2_FWD'), (N.PATH_OPT_PERSIST_S2_BWD, 'RFN_PATH_OPT_PERSIST_S2_BWD')):
        m.path_flags = bit
        with pytest.raises(N.RfnError, match=name):
            m(fc, att, lab, att_lens=LENS)
        with pytest.raises(N.RfnError, match=name):
            m.sample_beam(fc, att, {'beam_size': 2}, att_lens=LENS)
    # the library refuses on its own as well (RFN_ERR_UNSUPPORTED = -2, nothing launched): the Python check is a courtesy
    import ctypes as C
    m.path_flags = N.PATH_OPT_PERSIST_S2_FWD
    d = m._dims_for(False)
    lens = N.att_lens_arg(LENS, m.att_num, B, DEV)
    table = m._param_table(m._params_of(m._prefix_slots), m._prefix_slots)
    ws_bytes = N.lib.rfn_prefix_ws_bytes(C.byref(d), B, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((d.T2 * B * d.R + 2 * B * d.R + 3 * B * d.K,), float('nan'), device=DEV)
    o1, o2, o3 = d.T2 * B * d.R, d.T2 * B * d.R + B * d.R, d.T2 * B * d.R + 2 * B * d.R
    rc = N.lib.rfn_prefix_fwd_ex(C.byref(d), B, table, N.ptr_array(fc), N.ptr_array(att), out.data_ptr(), out[o1:].data_ptr(),
                                 out[o2:].data_ptr(), out[o3:].data_ptr(), ws.data_ptr(), ws_bytes, 0, 0, N.ptr_array(lens),
                                 N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -2 and bool(torch.isnan(out).all())
