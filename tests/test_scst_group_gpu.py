"""GPU: multi-sample self-critical training (include/rfn.h "multi-sample self-critical"): n draws per image through ONE decoder
node that reads an image's thought-vector products at row / n, and the leave-one-out reward.

  1. rfn_scst_reward_group bit for bit against the NumPy restatement (tests/scst_group_cpu.py), and scst_group_reward end to end
     on a reference-scored CIDEr-D tier;
  2. the kernel pieces at their launchers' code-path edges: rfn_dec_attn_bwd_ex bit for bit against rfn_dec_attn_bwd on
     physically repeated proj / U; rfn_dec_du_ex and rfn_rowgroup_sum against fp64 within the worst case of any summation order;
  3. rfn_decoder_fwd_ex / rfn_decoder_bwd_ex against the plain entry points on repeated thought vectors;
  4. sample_group's forward against sample() on features repeated n times, same uniforms, bit for bit;
  5. every gradient element of a sample_group step against the fp64 oracle on repeated features, and far from the oracle on the
     un-repeated input (which is what a dropped fan-in computes);
  6. refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import scst_group_cpu as G
from conftest import load_case, load_drop_case
from rl_grad_check import compare_grads, grad_bar
from test_ciderd_cpu import golden
from test_rl_grads_gpu import ENTROPY_REG, _against_oracle, _criterion_backward, _oracle, _row_reward, _to
from test_model_gpu import build

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def same_bits(a, b):
    """two float arrays: NaN where the other is NaN, the same bits elsewhere (a -0 is not a +0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(u), b[~nan].view(u))


# =================================================================================================================
# 1. the reward kernel
# =================================================================================================================
def _group_call(N, dev, cider, bleu, wc, wb, n, T, baseline):
    B = len(cider) if cider is not None else len(bleu)
    cd = None if cider is None else torch.from_numpy(cider).to(dev)
    bd = None if bleu is None else torch.from_numpy(bleu).to(dev)
    o32 = torch.full((B, T), float('nan'), device=dev)
    o64 = torch.full((B, T), float('nan'), dtype=torch.float64, device=dev)
    N.check(N.lib.rfn_scst_reward_group(N.ptr(cd), C.c_double(wc), N.ptr(bd), C.c_double(wb), B, n, T, baseline, o32.data_ptr(),
                                        o64.data_ptr(), N.stream_ptr()), 'rfn_scst_reward_group')
    return o32, o64


@pytest.mark.parametrize('T', [1, 17])
@pytest.mark.parametrize('imgs', [1, 7])
@pytest.mark.parametrize('n', [2, 3, 5])
def test_group_reward_is_the_restatement_bit_for_bit(dev, n, imgs, T):
    N = native()
    rng = np.random.default_rng(100 * n + 10 * imgs + T)
    B = n * imgs
    cider, bleu = rng.random(B) * 4.0, rng.random((B, 4))
    nan_c = cider.copy()
    nan_c[B // 2] = np.nan
    variants = [('cider', cider, None, 0.7, 0.0, 'loo'), ('bleu', None, bleu, 0.0, 1.3, 'loo'), ('mixed', cider, bleu, 0.5, 2.0, 'loo'),
                ('nan', nan_c, bleu, 1.0, 0.25, 'loo'), ('none', cider, bleu, 0.5, 2.0, 'none')]
    for name, c, b, wc, wb, how in variants:
        o32, o64 = _group_call(N, dev, c, b, wc, wb, n, T, 1 if how == 'loo' else 0)
        want = G.group_reward(c, b, n, T, wc, wb, how)
        assert same_bits(o64.cpu().numpy(), want), name
        assert same_bits(o32.cpu().numpy(), want.astype(np.float32)), name
        if name == 'nan':
            k = (B // 2) // n
            assert np.isnan(want[k * n:(k + 1) * n]).all() and np.isfinite(np.delete(want, np.s_[k * n:(k + 1) * n], 0)).all()
    # either output alone
    cd = torch.from_numpy(cider).to(dev)
    only64 = torch.empty(B, T, dtype=torch.float64, device=dev)
    N.check(N.lib.rfn_scst_reward_group(cd.data_ptr(), C.c_double(0.7), None, C.c_double(0.0), B, n, T, 1, None, only64.data_ptr(),
                                        N.stream_ptr()))
    assert same_bits(only64.cpu().numpy(), G.group_reward(cider, None, n, T, 0.7))


def test_scst_group_reward_end_to_end_on_a_reference_scored_tier(dev):
    """The tier's 2B score rows (B sampled rows then B greedy rows of images with 5 captions each) regrouped image-major: 10 draws
    per image, the same rows scored against the same corpus, so the reference's recorded scores are the scores of this call."""
    from recurrent_fusion_network_amd import rewards as RW
    g = golden('spi5')
    B, spi = int(g['B']), int(g['seq_per_img'])
    n = 2 * spi
    perm = np.array([half * B + k * spi + j for k in range(B // spi) for half in (0, 1) for j in range(spi)])
    res = torch.from_numpy(g['res'][perm]).to(dev)
    gts, n_refs = torch.from_numpy(g['gts']).to(dev), torch.from_numpy(g['n_refs']).to(dev)
    T = res.shape[1]
    for how, w in (('loo', 1.0), ('none', 0.5)):
        out64 = torch.empty(2 * B, T, dtype=torch.float64, device=dev)
        r32 = RW.scst_group_reward(RW.CiderD(), res, gts, n_refs, n, cider_weight=w, baseline=how, out64=out64)
        want = G.group_reward(g['scores'][perm], None, n, T, w, baseline=how)
        np.testing.assert_allclose(out64.cpu().numpy(), want, rtol=1e-10, atol=1e-12)
        assert r32.dtype == torch.float32 and torch.equal(r32, out64.float())
    assert float(np.abs(want).max()) > 0


def test_scst_group_reward_is_repeatable_and_replays_in_a_graph(dev):
    """No allocation besides the results and no synchronisation after the first call at a shape: the call can be captured."""
    from recurrent_fusion_network_amd import rewards as RW
    g = golden('spi5')
    B, spi = int(g['B']), int(g['seq_per_img'])
    gen = torch.from_numpy(g['res'][:B]).to(dev)                        # image-major already: 5 captions per image
    gts, n_refs = torch.from_numpy(g['gts']).to(dev), torch.from_numpy(g['n_refs']).to(dev)
    sc = RW.CiderD()
    first = RW.scst_group_reward(sc, gen, gts, n_refs, spi).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        RW.scst_group_reward(sc, gen, gts, n_refs, spi)                 # workspace and row map exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = RW.scst_group_reward(sc, gen, gts, n_refs, spi)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first) and float(first.abs().max()) > 0
    gen.copy_(gen.flip(0).clone())                                       # new captions through the same graph
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert torch.equal(replayed, RW.scst_group_reward(sc, gen, gts, n_refs, spi)) and not torch.equal(replayed, first)


def test_get_self_critical_reward_group_drop_in(dev):
    import types
    import ciderd_cpu as CPU
    from recurrent_fusion_network_amd import rewards as RW
    rng = np.random.default_rng(5)
    data = {'gts': [rng.integers(1, 30, (int(k), 9)) for k in (4, 2, 5)]}
    for a in data['gts']:
        a[:, -2:] = 0
    n, T = 3, 7
    gen = torch.from_numpy(rng.integers(0, 30, (3 * n, T))).to(dev)
    opt = types.SimpleNamespace(bleu4_weight=0.5, spice_weight=0, cider_weight=2.0, use_baseline=1)
    gts, n_refs = CPU.pad_gts(data['gts'])
    row_img = torch.arange(3 * n, dtype=torch.int32) // n
    sc, bl = RW.CiderD(), RW.BleuD()
    s = sc.score_ids(gen, row_img, torch.from_numpy(gts), torch.from_numpy(n_refs)).cpu().numpy()
    b = bl.score_ids(gen, row_img, torch.from_numpy(gts), torch.from_numpy(n_refs)).cpu().numpy()
    got = RW.get_self_critical_reward_group(data, gen, n, opt, scorer=sc, bleu_scorer=bl)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64
    assert same_bits(got, G.group_reward(s, b, n, T, 2.0, 0.5))
    opt.use_baseline, opt.bleu4_weight = 0, 0
    dev_r = RW.get_self_critical_reward_group(data, gen, n, opt, device=True, scorer=sc, bleu_scorer=bl)
    assert dev_r.is_cuda and dev_r.dtype == torch.float32
    assert same_bits(dev_r.cpu().numpy(), G.group_reward(s, None, n, T, 2.0, baseline='none').astype(np.float32))


# =================================================================================================================
# 2. kernel pieces
# =================================================================================================================
ATTN_SHAPES = {'fast': dict(A=512, L=8, GD=2048), 'general_L9': dict(A=512, L=9, GD=2048), 'scalar': dict(A=6, L=5, GD=10)}


def _attn_bwd(N, dev, proj, U, hp, w, al, dg, row_div, acc, ex):
    """one call on packed operands -> (dproj, dhproj, dw_part); proj (Bp, L, A), U (Bp, L, GD) with Bp = B / row_div"""
    B, A = hp.shape
    L, GD = proj.shape[1], U.shape[2]
    dproj = rnd(B, L, A, seed=9).to(dev) if acc else torch.full((B, L, A), float('nan'), device=dev)
    dhp, dwp = torch.full((B, A), float('nan'), device=dev), torch.full((B, A), float('nan'), device=dev)
    head = (proj.data_ptr(), L * A, A, hp.data_ptr(), w.data_ptr(), al.data_ptr(), U.data_ptr(), L * GD, GD, dg.data_ptr(), GD, B)
    tail = (L, A, GD, dproj.data_ptr(), L * A, A, acc, dhp.data_ptr(), dwp.data_ptr(), N.stream_ptr())
    if ex:
        N.check(N.lib.rfn_dec_attn_bwd_ex(*head, row_div, *tail), 'rfn_dec_attn_bwd_ex')
    else:
        assert row_div == 1
        N.check(N.lib.rfn_dec_attn_bwd(*head, *tail), 'rfn_dec_attn_bwd')
    return dproj, dhp, dwp


@pytest.mark.parametrize('row_div', [1, 2, 3])
@pytest.mark.parametrize('shape', sorted(ATTN_SHAPES))
def test_attention_backward_reads_the_image_row_and_writes_per_row(dev, shape, row_div):
    """Every row has the arithmetic of the plain call on proj / U repeated row_div times: the same bits on the same kernel."""
    N = native()
    s = ATTN_SHAPES[shape]
    A, L, GD, B = s['A'], s['L'], s['GD'], 6
    Bc = B // row_div
    proj, U = rnd(Bc, L, A, seed=1).to(dev), rnd(Bc, L, GD, seed=2, scale=0.3).to(dev)
    hp, w, dg = rnd(B, A, seed=3).to(dev), rnd(A, seed=4).to(dev), rnd(B, GD, seed=5, scale=0.1).to(dev)
    al = torch.softmax(rnd(B, L, seed=6), 1).to(dev)
    proj_rep, U_rep = proj.repeat_interleave(row_div, 0).contiguous(), U.repeat_interleave(row_div, 0).contiguous()
    for acc in (0, 1):
        got = _attn_bwd(N, dev, proj, U, hp, w, al, dg, row_div, acc, True)
        want = _attn_bwd(N, dev, proj_rep, U_rep, hp, w, al, dg, 1, acc, False)
        for name, a, b in zip(('dproj', 'dhproj', 'dw_part'), got, want):
            assert bool(torch.isfinite(b).all()), name
            assert torch.equal(a, b), (name, acc, float((a - b).abs().max()))
    if row_div > 1:      # the rows of one image do differ: nothing was folded onto one row
        assert not torch.equal(got[0][0], got[0][1])


@pytest.mark.parametrize('GD', [1028, 35], ids=['vector', 'scalar'])
@pytest.mark.parametrize('imgs', [3, 10])
@pytest.mark.parametrize('row_div', [1, 2, 3, 5])
def test_du_sums_an_images_rows_and_steps(dev, row_div, imgs, GD):
    N = native()
    S, L, B = 5, 9, imgs * row_div
    al = torch.softmax(rnd(S, B, L, seed=11), 2).to(dev)
    dg = rnd(S, B, GD, seed=12).to(dev)
    dU = torch.full((imgs, L, GD), float('nan'), device=dev)
    N.check(N.lib.rfn_dec_du_ex(al.data_ptr(), dg.data_ptr(), S, B, L, GD, row_div, dU.data_ptr(), L * GD, GD, N.stream_ptr()))
    terms = al.double().view(S, imgs, row_div, L, 1) * dg.double().view(S, imgs, row_div, 1, GD)
    want, mag = terms.sum((0, 2)), terms.abs().sum((0, 2))
    bound = (S * row_div + 1) * U24 * mag
    err = (dU.double() - want).abs()
    print('du row_div %d imgs %d GD %d: worst err / bound %.3g' % (row_div, imgs, GD, float((err / bound).max())))
    assert bool((err <= bound).all())
    if row_div == 1:
        old = torch.full_like(dU, float('nan'))
        N.check(N.lib.rfn_dec_du(al.data_ptr(), dg.data_ptr(), S, B, L, GD, old.data_ptr(), L * GD, GD, N.stream_ptr()))
        assert torch.equal(dU, old)


@pytest.mark.parametrize('cols', [260, 35], ids=['vector', 'scalar'])
@pytest.mark.parametrize('imgs', [3, 10])
@pytest.mark.parametrize('n', [1, 2, 3, 5])
def test_rowgroup_sum_is_the_fan_in_of_the_per_row_slabs(dev, n, imgs, cols):
    N = native()
    T2 = 3
    x = rnd(T2, imgs * n, cols, seed=21).to(dev)                       # (T2, B, A): row t * B + k * n + j
    y = torch.full((T2, imgs, cols), float('nan'), device=dev)
    N.check(N.lib.rfn_rowgroup_sum(x.data_ptr(), cols, n, y.data_ptr(), cols, T2 * imgs, cols, N.stream_ptr()))
    xv = x.double().view(T2, imgs, n, cols)
    want, mag = xv.sum(2), xv.abs().sum(2)
    err = (y.double() - want).abs()
    assert bool((err <= (n + 1) * U24 * mag).all())
    if n == 1:
        assert torch.equal(y, x)
    # the stated order, bit for bit: ((0 + x0) + x1) + ...
    acc = torch.zeros(T2, imgs, cols, device=dev)
    for j in range(n):
        acc = acc + x.view(T2, imgs, n, cols)[:, :, j]
    assert torch.equal(y, acc)


# =================================================================================================================
# 3. the path, ABI level
# =================================================================================================================
class _Path:
    """The decoder entry points on a tier's model: thought vectors from its own stages I / II, random tokens and upstream gradients."""

    def __init__(self, dev, name='mid'):
        self.N = native()
        cfg, spec, P, batch, gold = load_case(name)
        self.model = build(cfg, P, dev)
        fc, att = _to(batch[0], dev), _to(batch[1], dev)
        with torch.no_grad():
            self.comb, self.h, self.c, _ = self.model._prefix(fc, att, False, 0)
        self.cfg, self.dev, self.Bc, self.S = cfg, dev, fc[0].size(0), 6
        self.d = self.model._dims_for(False)
        self.params = self.model._params_lookup(self.model._decoder_slots)
        self.table = self.model._param_table(self.params, self.model._decoder_slots)

    def run(self, n, ex, comb, ids, dlp):
        """forward (train = 1) + backward -> (log_prob, d_comb, d_h0, d_c0, {name: grad})"""
        N, d, m, dev = self.N, self.d, self.model, self.dev
        B, S = ids.shape
        h0, c0 = self.h.repeat_interleave(B // self.Bc, 0).contiguous(), self.c.repeat_interleave(B // self.Bc, 0).contiguous()
        size = N.lib.rfn_decoder_ws_bytes_ex(C.byref(d), B, S, 1, n) if ex else N.lib.rfn_decoder_ws_bytes(C.byref(d), B, S, 1)
        assert size > 0
        ws = torch.empty(size, dtype=torch.uint8, device=dev)
        lp = torch.full((B, S, d.V1), float('nan'), device=dev)
        st = N.stream_ptr()
        head = (C.byref(d), B, S, self.table, comb.data_ptr(), h0.data_ptr(), c0.data_ptr(), ids.data_ptr(), ids.stride(0))
        if ex:
            N.check(N.lib.rfn_decoder_fwd_ex(*head, lp.data_ptr(), ws.data_ptr(), size, 1, 0, n, st), 'rfn_decoder_fwd_ex')
        else:
            N.check(N.lib.rfn_decoder_fwd(*head, lp.data_ptr(), ws.data_ptr(), size, 1, 0, st), 'rfn_decoder_fwd')
        flats, by_slot, gtable = m._grad_buffers(['decoder'], dev)
        flats['decoder'].fill_(float('nan'))
        d_comb = torch.full_like(comb, float('nan'))
        d_h0, d_c0 = torch.full_like(h0, float('nan')), torch.full_like(c0, float('nan'))
        tail = (lp.data_ptr(), dlp.data_ptr(), d_comb.data_ptr(), d_h0.data_ptr(), d_c0.data_ptr(), gtable, ws.data_ptr(), size, 0)
        if ex:
            N.check(N.lib.rfn_decoder_bwd_ex(*head, *tail, n, st), 'rfn_decoder_bwd_ex')
        else:
            N.check(N.lib.rfn_decoder_bwd(*head, *tail, st), 'rfn_decoder_bwd')
        grads = {m._slot_names[s]: v.clone() for s, v in by_slot.items()}
        return lp, d_comb, d_h0, d_c0, grads


@pytest.fixture(scope='module')
def path(dev):
    return _Path(dev)


def _tokens(B, S, V, seed):
    ids = torch.randint(1, V + 1, (B, S), generator=torch.Generator().manual_seed(seed))
    ids[:, 0] = 0
    return ids


def test_decoder_with_three_rows_per_image_against_repeated_thought_vectors(dev, path):
    n, p = 3, path
    B = p.Bc * n
    ids = _tokens(B, p.S, p.cfg.vocab_size, 3).to(dev)
    dlp = rnd(B, p.S, p.d.V1, seed=4, scale=0.05).to(dev)
    got = p.run(n, True, p.comb, ids, dlp)
    rep = p.comb.repeat_interleave(n, 1).contiguous()
    want = p.run(1, False, rep, ids, dlp)
    assert bool(torch.isfinite(want[0]).all()) and torch.equal(got[0], want[0])                 # log-probs: bit for bit
    T2, R = rep.size(0), rep.size(2)
    folded = want[1].double().view(T2, p.Bc, n, R).sum(2)
    compare_grads({'d_comb': got[1], 'd_h0': got[2], 'd_c0': got[3]}, {'d_comb': folded, 'd_h0': want[2], 'd_c0': want[3]}, grad_bar)
    rep_ = compare_grads(got[4], want[4], grad_bar)
    print('decoder n = 3: worst gradient err / bar %.4f at %s' % (rep_['ratio'], rep_['name']))
    assert set(got[4]) == {k for k in p.model._slot_names if k.startswith(('embed.', 'logit.', 'decoder.'))}
    # not vacuous: one row's share of d_comb is far from the sum over the image's rows
    assert compare_grads({'d_comb': want[1].view(T2, p.Bc, n, R)[:, :, 0]}, {'d_comb': folded}, grad_bar, check=False)['ratio'] > 10


def test_decoder_with_one_row_per_image_is_the_plain_entry_points_bit_for_bit(dev, path):
    p = path
    ids = _tokens(p.Bc, p.S, p.cfg.vocab_size, 5).to(dev)
    dlp = rnd(p.Bc, p.S, p.d.V1, seed=6, scale=0.05).to(dev)
    got, want = p.run(1, True, p.comb, ids, dlp), p.run(1, False, p.comb, ids, dlp)
    for a, b in zip(got[:4], want[:4]):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    assert set(got[4]) == set(want[4]) and all(torch.equal(got[4][k], want[4][k]) for k in want[4])


# =================================================================================================================
# 4. sample_group, forward
# =================================================================================================================
def _rep(ts, n):
    return [t.repeat_interleave(n, 0).contiguous() for t in ts]


@pytest.mark.parametrize('name', ['tiny0', 'mid'])
def test_sample_group_equals_sample_on_repeated_features(dev, name):
    cfg, spec, P, batch, gold = load_case(name)
    model = build(cfg, P, dev)
    fc, att = _to(batch[0], dev), _to(batch[1], dev)
    Bc, S, n = fc[0].size(0), cfg.seq_length, 3
    u = torch.rand(2, S + 1, Bc * n, generator=torch.Generator().manual_seed(77)).to(dev)
    model._ss_uniforms, model._trace_ss = u, True
    try:
        with torch.no_grad():
            seq, lp, lp_all, reason = model.sample_group(fc, att, n)
            fed = model._sample_ids.clone()                                          # (B * n, steps): BOS, then the unmasked draws
            seq_r, lp_r, lp_all_r, reason_r = model.sample(_rep(fc, n), _rep(att, n), {'sample_max': 0})
        g_seq, g_lp, g_all, _ = model.sample_group(fc, att, n)                      # under grad: the same numbers
    finally:
        model._ss_uniforms = None
    assert tuple(seq.shape)[0] == Bc * n and torch.equal(seq, seq_r) and torch.equal(lp, lp_r) and torch.equal(lp_all, lp_all_r)
    assert g_all.requires_grad and torch.equal(g_seq, seq) and torch.equal(g_lp.detach(), lp) and torch.equal(g_all.detach(), lp_all)
    assert len(reason) == len(reason_r) == len(cfg.feat_array_info) + 1
    for a, b in zip(reason, reason_r):
        assert tuple(a.shape) == (Bc, cfg.top_words_count) and torch.equal(a, b[::n])
    assert any(not torch.equal(seq[k * n], seq[k * n + 1]) for k in range(Bc))       # an image whose draws differ
    # n = 1 is sample(sample_max = 0)
    model._ss_uniforms = u[:, :, :Bc].contiguous()
    try:
        with torch.no_grad():
            one, plain = model.sample_group(fc, att, 1), model.sample(fc, att, {'sample_max': 0})
    finally:
        model._ss_uniforms = None
    assert all(torch.equal(a, b) for a, b in zip(one[:3], plain[:3])) and all(torch.equal(a, b) for a, b in zip(one[3], plain[3]))
    # force_ids: the batched teacher-forced replay of the tokens the pass fed (rfn_decoder_fwd_ex) is the sampled pass, bit for bit
    draws = torch.cat([fed[:, 1:], fed.new_zeros(Bc * n, S + 1 - fed.size(1))], 1)
    assert bool((torch.cumprod((draws > 0).long(), 1)[:, fed.size(1) - 1:] == 0).all())
    with torch.no_grad():
        forced = model.sample_group(fc, att, n, {'force_ids': draws})
    assert torch.equal(forced[0], seq) and torch.equal(forced[1], lp) and torch.equal(forced[2], lp_all)


# =================================================================================================================
# 5. every gradient element against the fp64 oracle
# =================================================================================================================
def _group_masks(cfg, Bc, n, S, seed, dev):
    """The keep masks of a sample_group step as an oracle `drop` object for B = Bc * n rows: stages I / II draw one mask per image
    (they run once per image), repeated onto the image's rows; the decoder draws one per row."""
    from oracle import rfn_oracle as O
    from test_dropout_parity_gpu import OFF_DECODER, OFF_STAGE2
    N = native()
    M, R = len(cfg.feat_array_info), cfg.rnn_size

    def site(offset, p, rows):
        keep = torch.empty(rows, R, device=dev)
        N.check(N.lib.rfn_dropout_mask(seed, offset, rows * R, p, keep.data_ptr(), N.stream_ptr()), 'rfn_dropout_mask')
        return keep.cpu()

    fusion = [[site(t * M + i, cfg.drop_prob_fusion, Bc).repeat_interleave(n, 0) for i in range(M)]
              for t in range(cfg.num_review_steps_0)]
    review = [site(OFF_STAGE2 + t, cfg.drop_prob_reason, Bc).repeat_interleave(n, 0) for t in range(cfg.num_review_steps)]
    decoder = [site(OFF_DECODER + s, cfg.drop_prob_lm, Bc * n) for s in range(S)]
    return O.make_drop(cfg, fusion, review, decoder)


def _group_step(case, cfg, P, fc, att, top, n, train, dev, torch_seed=31):
    from recurrent_fusion_network_amd.fusion_model import _fresh_seed
    model = build(cfg, P, dev, train=train)
    Bc, S = fc[0].size(0), cfg.seq_length
    B = Bc * n
    u = torch.rand(2, S + 1, B, generator=torch.Generator().manual_seed(torch_seed + 1000)).to(dev)
    reward_row = _row_reward(B, torch_seed + 7)
    torch.manual_seed(torch_seed)
    seed = _fresh_seed() if train else 0
    torch.manual_seed(torch_seed)
    model._trace_ss, model._ss_uniforms = True, u
    try:
        seq, seq_lp, lp_all, reason = model.sample_group(_to(fc, dev), _to(att, dev), n)
    finally:
        model._ss_uniforms = None
    fed = model._sample_ids
    assert lp_all.requires_grad and tuple(fed.shape) == (B, lp_all.size(1)) and bool((fed[:, 0] == 0).all())
    assert all(tuple(r.shape) == (Bc, cfg.top_words_count) for r in reason)
    loss, grads = _criterion_backward(model, cfg, seq, seq_lp, lp_all, reason, reward_row, top, ENTROPY_REG)
    got = (loss, grads, seq, seq_lp.detach(), lp_all.detach())
    dropping = train and max(cfg.drop_prob_fusion, cfg.drop_prob_reason, cfg.drop_prob_lm) > 0
    drop = _group_masks(cfg, Bc, n, fed.size(1), seed, dev) if dropping else None
    want, secs = _oracle(cfg, P, _rep(fc, n), _rep(att, n), fed, reward_row, top.repeat_interleave(n, 0), drop=drop)
    _against_oracle(case, got, want, secs)
    return got, fed, reward_row


@pytest.mark.parametrize('n', [2, 3])
@pytest.mark.parametrize('name', ['tiny0', 'tinymax', 'odd', 'mid'])
def test_sample_group_every_gradient_element_against_the_fp64_oracle(dev, name, n):
    """The oracle runs the reference's self-critical step on features and top words repeated n times and the tokens the pass
    fed.  The policy term is divided by the B * n rows; the reason term is a mean over the images, which is the mean over the
    repeated rows.  Not vacuous: on the un-repeated input (draw 0 of every image), which is what a pass that dropped the
    fan-in of the image's rows computes, the oracle is more than ten bars away."""
    cfg, spec, P, batch, gold = load_case(name)
    fc, att, labels, masks, top = batch
    got, fed, reward_row = _group_step('group/%s/n%d' % (name, n), cfg, P, fc, att, top, n, False, dev)
    lone, _ = _oracle(cfg, P, fc, att, fed[::n].contiguous(), reward_row[::n].contiguous(), top)
    far = compare_grads(got[1], lone[1], grad_bar, check=False)
    print('group/%s/n%d: against the one-draw oracle err / bar %.1f at %s' % (name, n, far['ratio'], far['name']))
    assert far['ratio'] > 10.0


def test_sample_group_in_training_mode_with_the_products_own_masks(dev):
    cfg, spec, P, batch, gold, _ = load_drop_case('mid')
    fc, att, labels, masks, top = batch
    _group_step('group/mid_drop/n3', cfg, P, fc, att, top, 3, True, dev)


@pytest.mark.parametrize('retain', [False, True], ids=['recompute', 'retain_activations'])
def test_a_second_backward_over_the_group_graph_repeats_the_first(dev, retain):
    """loss.backward(retain_graph=True) twice (the PPO loop's pattern) with unchanged weights: the decoder node recomputes its
    pass with n rows per image (or restores its snapshot) and both backward passes give the same gradients, bit for bit."""
    cfg, spec, P, batch, gold = load_case('mid')
    model = build(cfg, P, dev)
    model.retain_activations = retain
    fc, att = _to(batch[0], dev), _to(batch[1], dev)
    seq, lp, lp_all, reason = model.sample_group(fc, att, 2)
    w = rnd(*lp_all.shape, seed=8).to(dev)
    loss = (lp_all * w).sum() + sum((r * r).sum() for r in reason)
    grads = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        loss.backward(retain_graph=True)
        grads.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    assert all(bool(torch.isfinite(g).all()) for g in grads[0].values()) and float(grads[0]['decoder.z2h.weight'].abs().max()) > 0
    differ = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    assert not differ, differ[:8]


# =================================================================================================================
# 6. refusals
# =================================================================================================================
def test_refusals(dev):
    N = native()
    cfg, spec, P, batch, gold = load_case('tiny0')
    model = build(cfg, P, dev)
    fc, att = _to(batch[0], dev), _to(batch[1], dev)
    Bc, S = fc[0].size(0), cfg.seq_length
    with pytest.raises(ValueError):
        model.sample_group(fc, att, 0)
    for opt in ({'block_ngram': 2}, {'top_k': 5}, {'top_p': 0.9}, {'beam_size': 2}, {'sample_max': 1}, {'banned_ids': [3]}):
        with pytest.raises(ValueError):
            model.sample_group(fc, att, 2, opt)
    with pytest.raises(ValueError):
        model.sample_group(fc, att, 2, {'force_ids': torch.ones(Bc, S, dtype=torch.long, device=dev)})     # B rows, not B * n
    model.path_flags = N.PATH_OPT_DEC_UNHOISTED
    with pytest.raises(N.RfnError):
        model.sample_group(fc, att, 2)
    with torch.no_grad():
        assert model.sample_group(fc, att, 1)[0].size(0) == Bc                    # one row per image: the un-hoisted cell serves
    model.path_flags = 0
    with pytest.raises(N.RfnError):
        model.sample(fc, att, {'sample_max': 0, 'sample_n': 2})                    # the differentiated pass of sample() still refuses
