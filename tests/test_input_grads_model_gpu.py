"""Gradients of fc_feats / att_feats through the model (INTEGRATION.md "Input gradients"): the eval-mode tiny options of
tests/test_ragged_model_gpu.py (R = E = 16, T1 = T2 = 3, vocabulary 50, seq 5, B = 3) in two feature configurations --
'vec': maps (7, 8), (12, 12), A = 16; 'scalar': maps (5, 6), (9, 10), fc_feat_size = D + 1, A = 10 (the kernel and the GEMM on
their scalar forms).  Reference: oracle.rfn_oracle forward + xe_criterion in float64 with the features as leaves.

Bar: per tensor 1e-3 * max|g_oracle| (max|g_oracle| > 0 asserted) -- the relative part of the project's gradient bar WITHOUT its
1e-5 floor: feature gradients here are 2e-4 .. 9e-4, and with the floor a gradient that lacks the projection term passes for one
encoder.  test_the_bar_separates_the_two_terms recomputes, in the oracle, what each term of
    d x = sum_t dP1[t] . W_att2att[t]  (A)  +  sum_t alpha[t] * dz[t]  (B)
contributes (one use of the map in stage-I attention detached) and asserts that either alone misses by >= 10 bars."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
B = 3
CONFIGS = {'vec': dict(maps=[(7, 8), (12, 12)], A=16, fc_extra=0),
           'scalar': dict(maps=[(5, 6), (9, 10)], A=10, fc_extra=1)}
LENS = [[7, 1, 4], [12, 5, 9]]          # 'vec' only


def cfg_for(name, att_nums=None, **extra):
    from oracle import rfn_oracle as O
    c = CONFIGS[name]
    nums = att_nums or [L for L, _ in c['maps']]
    info = [dict(att_num=n, att_feat_size=D, fc_feat_size=D + c['fc_extra']) for n, (_, D) in zip(nums, c['maps'])]
    return O.make_cfg(info, vocab_size=50, rnn_size=16, input_encoding_size=16, att_hid_size=c['A'], num_review_steps_0=3,
                      num_review_steps=3, top_words_count=20, seq_length=5, **extra)


def build(cfg, P, train=False):
    import recurrent_fusion_network_amd as R
    m = R.RecurrentFusionModel(cfg)
    m.load_state_dict(P)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def leaves(ts, need=True):
    return [t.detach().to(DEV).requires_grad_(need) for t in ts]


def oracle_feature_grads(cfg, P, fc, att, labels, masks, top, per_caption=False):
    """float64, features as leaves -> (d fc list, d att list) of the criterion's loss, or of sum_b s_b with s_b = sum_t mask *
    log p(seq_t) (per_caption: row b of the result is d s_b, captions do not mix)."""
    from oracle import rfn_oracle as O
    P64 = {k: v.double() for k, v in P.items()}
    f = [t.double().requires_grad_(True) for t in fc]
    a = [t.double().requires_grad_(True) for t in att]
    lp, heads = O.forward(cfg, P64, f, a, labels)
    if per_caption:
        S = lp.size(1)
        s = (lp.gather(2, labels[:, 1:S + 1].unsqueeze(2)).squeeze(2) * masks[:, 1:S + 1].double()).sum()
        g = torch.autograd.grad(s, a)
        return None, list(g)
    loss = O.xe_criterion(cfg, lp, labels[:, 1:], masks[:, 1:].double(), heads, top, 1.0)
    g = torch.autograd.grad(loss, f + a)
    return list(g[:len(f)]), list(g[len(f):])


@pytest.fixture(scope='module', params=sorted(CONFIGS))
def world(request):
    """Model, batch and the oracle's feature gradients of one configuration (computed once, read-only)."""
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    name = request.param
    cfg = cfg_for(name)
    P = O.seeded_params(cfg, 11)
    fc, att, labels, masks, top = O.synthetic_batch(cfg, B, seed=21)
    dfc, datt = oracle_feature_grads(cfg, P, fc, att, labels, masks, top)
    return dict(name=name, cfg=cfg, P=P, model=build(cfg, P), crit=R.ReviewNetEnsembleCriterion(cfg), fc=fc, att=att,
                labels=labels, masks=masks, top=top, dfc=dfc, datt=datt)


def bar_of(ref):
    m = float(ref.abs().max())
    assert m > 0
    return 1e-3 * m


def assert_close(got, ref, what):
    assert got is not None, '%s: no gradient' % what
    assert got.shape == ref.shape
    err = float((got.double().cpu() - ref).abs().max())
    print('%s: max|g| %.3g  err %.3g  = %.3g bars' % (what, float(ref.abs().max()), err, err / bar_of(ref)))
    assert err <= bar_of(ref), (what, err, bar_of(ref))


def step(w, fc, att, fused, model=None, att_lens=None):
    m = model or w['model']
    m.zero_grad(set_to_none=True)
    lab, msk, top = w['labels'].to(DEV), w['masks'].to(DEV), w['top'].to(DEV)
    if fused:
        loss, _ = m.forward_loss(fc, att, lab, msk, top, w['crit'], 1.0, att_lens=att_lens)
    else:
        lp, heads = m(fc, att, lab, att_lens=att_lens)
        loss = w['crit'](lp, lab[:, 1:], msk[:, 1:], heads, top, 1.0)
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


# ---- the bar cannot hide a dropped term --------------------------------------------------------------------------------------
def test_the_bar_separates_the_two_terms(world):
    from oracle import rfn_oracle as O
    w = world
    plain = O.attention

    def split(keep):
        def attention(pre_h, att_seq, P, prefix):
            if not prefix.startswith('review_steps_individual.'):      # stage II and the decoder attend over thought vectors
                return plain(pre_h, att_seq, P, prefix)
            x_proj = att_seq if keep == 'A' else att_seq.detach()      # the use behind term (A): att_2_att_h(x)
            x_ctx = att_seq if keep == 'B' else att_seq.detach()       # the use behind term (B): z = sum_l alpha x
            _, alpha, scores = plain(pre_h, x_proj, P, prefix)
            z = torch.bmm(x_ctx.transpose(1, 2), alpha.unsqueeze(2)).squeeze(2)
            return z, alpha, scores
        return attention

    parts = {}
    try:
        for keep in ('A', 'B'):
            O.attention = split(keep)
            parts[keep] = oracle_feature_grads(w['cfg'], w['P'], w['fc'], w['att'], w['labels'], w['masks'], w['top'])[1]
    finally:
        O.attention = plain
    for i, full in enumerate(w['datt']):
        bar = bar_of(full)
        assert float((parts['A'][i] + parts['B'][i] - full).abs().max()) < 1e-12      # the two uses are the whole gradient
        for keep in ('A', 'B'):
            miss = float((parts[keep][i] - full).abs().max()) / bar
            print('%s enc %d: term %s alone misses by %.1f bars' % (w['name'], i, keep, miss))
            assert miss >= 10, (w['name'], i, keep, miss)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [False, True], ids=['forward_criterion', 'forward_loss'])
def test_feature_gradients_match_the_oracle(world, fused):
    w = world
    fc, att = leaves(w['fc']), leaves(w['att'])
    step(w, fc, att, fused)
    for i in range(len(fc)):
        assert_close(fc[i].grad, w['dfc'][i], '%s fc_feats[%d]' % (w['name'], i))
        assert_close(att[i].grad, w['datt'][i], '%s att_feats[%d]' % (w['name'], i))


# ---- 2. nothing else moves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [False, True], ids=['forward_criterion', 'forward_loss'])
def test_loss_and_parameter_gradients_are_bit_identical(world, fused):
    w = world
    la, ga = step(w, leaves(w['fc'], False), leaves(w['att'], False), fused)
    lb, gb = step(w, leaves(w['fc']), leaves(w['att']), fused)
    assert torch.equal(la, lb) and set(ga) == set(gb) and len(ga) > 0
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    # training mode, dropout 0.3 in all three places: the same seed draws the same masks with and without the bit
    cfg = cfg_for(w['name'], drop_prob_lm=0.3, drop_prob_reason=0.3, drop_prob_fusion=0.3)
    m = build(cfg, w['P'], train=True)
    torch.manual_seed(5)
    la, ga = step(w, leaves(w['fc'], False), leaves(w['att'], False), fused, model=m)
    torch.manual_seed(5)
    lb, gb = step(w, leaves(w['fc']), leaves(w['att']), fused, model=m)
    torch.manual_seed(6)
    lc, _ = step(w, leaves(w['fc'], False), leaves(w['att'], False), fused, model=m)
    assert torch.equal(la, lb) and not torch.equal(la, lc) and set(ga) == set(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


# ---- 3. one tensor only ------------------------------------------------------------------------------------------------------------
def test_only_one_map_requires_grad(world):
    w = world
    fc, att = leaves(w['fc'], False), leaves(w['att'], False)
    att[1].requires_grad_(True)
    step(w, fc, att, True)
    assert all(t.grad is None for t in fc) and att[0].grad is None
    every_fc, every_att = leaves(w['fc']), leaves(w['att'])
    step(w, every_fc, every_att, True)
    assert torch.equal(att[1].grad, every_att[1].grad)
    assert_close(att[1].grad, w['datt'][1], '%s att_feats[1] alone' % w['name'])


# ---- 4. ragged maps ----------------------------------------------------------------------------------------------------------------
def test_ragged_maps_against_each_image_alone():
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    cfg = cfg_for('vec')
    P = O.seeded_params(cfg, 11)
    fc, att, labels, masks, top = O.synthetic_batch(cfg, B, seed=21)
    g = torch.Generator().manual_seed(5)
    for i, a in enumerate(att):          # large finite noise in the padded rows
        for b in range(B):
            a[b, LENS[i][b]:] = torch.randn(a[b, LENS[i][b]:].shape, generator=g) * 1e3
    w = dict(model=build(cfg, P), crit=R.ReviewNetEnsembleCriterion(cfg), labels=labels, masks=masks, top=top)
    for fused in (False, True):
        f, a = leaves(fc), leaves(att)
        step(w, f, a, fused, att_lens=LENS)
        for b in range(B):
            # image b alone on its truncated maps; the batch criterion divides by B
            fc_b = [t[b:b + 1] for t in fc]
            att_b = [t[b:b + 1, :LENS[i][b]] for i, t in enumerate(att)]
            dfc, datt = oracle_feature_grads(cfg_for('vec', [LENS[0][b], LENS[1][b]]), P, fc_b, att_b, labels[b:b + 1],
                                             masks[b:b + 1], top[b:b + 1])
            for i in range(2):
                n = LENS[i][b]
                assert_close(a[i].grad[b:b + 1, :n], datt[i] / B, 'ragged image %d att_feats[%d]' % (b, i))
                assert_close(f[i].grad[b:b + 1], dfc[i] / B, 'ragged image %d fc_feats[%d]' % (b, i))
                pad = a[i].grad[b, n:]
                assert bool((pad == 0).all()), (b, i)


# ---- 5. the sampled pass ---------------------------------------------------------------------------------------------------------
def test_sample_group_feature_gradients(world):
    w = world
    m = w['model']
    reward = torch.tensor([0.7, -0.3, 0.2, 1.1, -0.9, 0.4], device=DEV)
    runs = []
    for _ in range(2):
        fc, att = leaves(w['fc']), leaves(w['att'])
        m.zero_grad(set_to_none=True)
        torch.manual_seed(3)
        seq, slp, _, _ = m.sample_group(fc, att, 2)
        assert seq.size(0) == 2 * B
        (-(slp * reward[:, None]).sum() / (2 * B)).backward()
        runs.append([t.grad.clone() for t in fc + att])
    for x, y in zip(*runs):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0
        assert torch.equal(x, y)


# ---- 6. saliency -------------------------------------------------------------------------------------------------------------------
def test_saliency(world):
    w = world
    m = w['model']
    fc, att = [t.to(DEV) for t in w['fc']], [t.to(DEV) for t in w['att']]
    lab, msk = w['labels'].to(DEV), w['masks'].to(DEV)
    _, want = oracle_feature_grads(w['cfg'], w['P'], w['fc'], w['att'], w['labels'], w['masks'], w['top'], per_caption=True)
    # parameter gradients as a trainer would hold them: some set, some None
    step(w, leaves(w['fc'], False), leaves(w['att'], False), True)
    named = dict(m.named_parameters())
    named['logit.bias'].grad = None
    snap = {k: (None if p.grad is None else (p.grad, p.grad.clone())) for k, p in named.items()}
    raw = m.saliency(fc, att, lab, msk, mode='raw')
    gxi = m.saliency(fc, att, lab, msk)
    nrm = m.saliency(fc, att, lab, msk, mode='grad_norm')
    for k, p in named.items():
        if snap[k] is None:
            assert p.grad is None, k
        else:
            assert p.grad is snap[k][0] and torch.equal(p.grad, snap[k][1]), k
    for i in range(len(att)):
        assert_close(raw[i], want[i], '%s saliency raw[%d]' % (w['name'], i))
        assert gxi[i].shape == nrm[i].shape == att[i].shape[:2]
        assert torch.allclose(gxi[i], (raw[i] * att[i]).sum(2), rtol=1e-5, atol=1e-9)
        assert torch.allclose(nrm[i], raw[i].norm(dim=2), rtol=1e-5, atol=1e-12)
        assert not raw[i].requires_grad and att[i].grad is None
    # masks=None: every target up to and including the first END -- the synthetic captions are full length, masks all one
    for x, y in zip(m.saliency(fc, att, lab, mode='raw'), raw):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match='mode'):
        m.saliency(fc, att, lab, msk, mode='integrated')


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_reason(world):
    import recurrent_fusion_network_amd._native as N
    from recurrent_fusion_network_amd.graphed import GraphedTrainStep
    w = world
    m = build(w['cfg'], w['P'])
    m.gemm_flags = N.GEMM_OPT_BF16X3 | N.GEMM_OPT_BF16X3_ANY_SIZE
    lab = w['labels'].to(DEV)
    with pytest.raises(N.RfnError, match='RFN_GEMM_OPT_BF16X3'):
        m(leaves(w['fc'], False), leaves(w['att']), lab)
    with torch.no_grad():                     # no gradient wanted: the flag is fine
        m(leaves(w['fc'], False), leaves(w['att']), lab)
    m.gemm_flags = 0
    fc, att = leaves(w['fc'], False), leaves(w['att'])
    with pytest.raises(N.RfnError, match=r'att_feats\[0\] requires grad'):
        GraphedTrainStep(m, w['crit'], None, fc, att, lab, w['masks'].to(DEV), w['top'].to(DEV))
    step_obj = GraphedTrainStep.__new__(GraphedTrainStep)      # an unbuilt step: the refusal comes before anything else
    with pytest.raises(N.RfnError, match=r'fc_feats\[0\] requires grad'):
        step_obj(fc_feats=leaves(w['fc']), att_feats=None)
