"""The reward of a distinct-sample set and the step it makes trainable.

  1. rfn_scst_reward_distinct bit for bit against the NumPy restatement (tests/rl_logits_cpu.py distinct_reward) on constructed
     (weight, score) sets: every row live, one live row, a dead image, a NaN score on a weighted and on a zero-weight row, no
     baseline, the n < 3 refusal;
  2. end to end: sample_distinct(n = 4) with a fixed seed, scst_distinct_reward, rl_loss(n = 4), backward -- finite gradients, equal
     to the two-call form (sample_group(force_ids) + ReviewNetRewardCriterion) on the same rows at the project's gradient bar, and
     rows with a zero reward contribute exactly nothing whatever their tokens are."""
import ctypes as C

import numpy as np
import pytest
import torch

import rl_logits_cpu as RL
from conftest import load_case
from rl_grad_check import compare_grads, grad_bar
from test_model_gpu import LOGP_TOL, build, maxerr

pytestmark = pytest.mark.gpu


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def same_bits(a, b):
    """two float arrays: NaN where the other is NaN, the same bits elsewhere (a -0 is not a +0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(u), b[~nan].view(u))


def _call(N, dev, cider, bleu, weight, wc, wb, n, T, baseline, want32=True, want64=True):
    B = len(weight)
    cd = None if cider is None else torch.from_numpy(cider).to(dev)
    bd = None if bleu is None else torch.from_numpy(bleu).to(dev)
    wd = torch.from_numpy(weight).to(dev)
    o32 = torch.full((B, T), float('nan'), device=dev) if want32 else None
    o64 = torch.full((B, T), float('nan'), dtype=torch.float64, device=dev) if want64 else None
    rc = N.lib.rfn_scst_reward_distinct(N.ptr(cd), C.c_double(wc), N.ptr(bd), C.c_double(wb), wd.data_ptr(), B, n, T, baseline,
                                        N.ptr(o32) or None, N.ptr(o64) or None, N.stream_ptr())
    return rc, o32, o64


@pytest.mark.parametrize('T', [1, 17])
@pytest.mark.parametrize('n', [3, 4, 5])
def test_distinct_reward_is_the_restatement_bit_for_bit(dev, n, T):
    N = native()
    rng = np.random.default_rng(10 * n + T)
    imgs = 6
    B = n * imgs
    cider, bleu = rng.random(B) * 4.0, rng.random((B, 4))
    w = rng.random(B) * np.exp(rng.standard_normal(B) * 3.0)          # importance weights span orders of magnitude
    w[n - 1::n] = 0.0                                                 # the threshold row of every image
    all_live = rng.random(B) + 0.1
    one_live = w.copy()
    one_live[n:2 * n] = 0.0
    one_live[n] = 0.37                                                # image 1: one weighted row
    dead = w.copy()
    dead[2 * n:3 * n] = 0.0                                           # image 2: no weighted row
    dead[3 * n + 1] = -1.0                                            # a negative and a NaN weight are no weight
    dead[4 * n] = np.nan
    nan_live, nan_zero = cider.copy(), cider.copy()
    nan_live[0] = np.nan                                              # weighted row of image 0
    nan_zero[n - 1] = np.nan                                          # its threshold row
    variants = [('all live', cider, bleu, all_live, 0.5, 2.0, 'weighted'), ('cider', cider, None, w, 0.7, 0.0, 'weighted'),
                ('bleu', None, bleu, w, 0.0, 1.3, 'weighted'), ('one live', cider, bleu, one_live, 0.5, 2.0, 'weighted'),
                ('dead image', cider, None, dead, 1.0, 0.0, 'weighted'), ('nan weighted', nan_live, bleu, w, 1.0, 0.25, 'weighted'),
                ('nan zero-weight', nan_zero, None, w, 1.0, 0.0, 'weighted'), ('none', cider, bleu, w, 0.5, 2.0, 'none'),
                ('none nan', nan_live, None, w, 1.0, 0.0, 'none')]
    for name, c, b, wt, wc, wb, how in variants:
        rc, o32, o64 = _call(N, dev, c, b, wt, wc, wb, n, T, 1 if how == 'weighted' else 0)
        assert rc == 0, name
        want = RL.distinct_reward(c, b, wt, n, T, wc, wb, how)
        assert same_bits(o64.cpu().numpy(), want), name
        assert same_bits(o32.cpu().numpy(), want.astype(np.float32)), name
        zero_w = ~(wt > 0)
        assert (want[zero_w] == 0).all() and not np.signbit(want[zero_w]).any(), name
        if name == 'one live':
            assert not want[n:2 * n].any() and want[:n].any()
        if name == 'dead image':
            assert not want[2 * n:3 * n].any() and np.isfinite(want).all() and not want[3 * n + 1].any() and not want[4 * n].any()
        if name == 'nan weighted':
            assert np.isnan(want[:n - 1]).all() and np.isfinite(want[n - 1:]).all()
        if name == 'nan zero-weight':
            assert np.isfinite(want).all()
        if name == 'none nan':
            assert np.isnan(want[0]).all() and np.isfinite(want[1:]).all()
    # either output alone
    rc, _, only64 = _call(N, dev, cider, None, w, 0.7, 0.0, n, T, 1, want32=False)
    assert rc == 0 and same_bits(only64.cpu().numpy(), RL.distinct_reward(cider, None, w, n, T, 0.7))
    rc, only32, _ = _call(N, dev, cider, None, w, 0.7, 0.0, n, T, 1, want64=False)
    assert rc == 0 and same_bits(only32.cpu().numpy(), RL.distinct_reward(cider, None, w, n, T, 0.7).astype(np.float32))


def test_two_rows_per_image_need_no_baseline(dev):
    N = native()
    w = np.array([0.5, 0.0, 0.25, 0.0])
    s = np.array([1.0, 2.0, 3.0, 4.0])
    assert _call(N, dev, s, None, w, 1.0, 0.0, 2, 3, 1)[0] == -1                      # RFN_ERR_SHAPE: the weighted baseline needs n >= 3
    rc, o32, o64 = _call(N, dev, s, None, w, 1.0, 0.0, 2, 3, 0)
    assert rc == 0 and same_bits(o64.cpu().numpy(), RL.distinct_reward(s, None, w, 2, 3, baseline='none'))
    from recurrent_fusion_network_amd import rewards as RW
    gen = torch.zeros(4, 3, dtype=torch.int64, device=dev)
    gts, n_refs = torch.ones(2, 1, 3, dtype=torch.int64, device=dev), torch.ones(2, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match='n >= 3'):
        RW.scst_distinct_reward(RW.CiderD(), gen, torch.from_numpy(w).to(dev), gts, n_refs, 2)
    assert tuple(RW.scst_distinct_reward(RW.CiderD(), gen, torch.from_numpy(w).to(dev), gts, n_refs, 2, baseline='none').shape) == (4, 3)


def _grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize('name', ['tiny0', 'odd'])
def test_distinct_set_trains_end_to_end(dev, name):
    import types
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd import rewards as RW
    cfg, spec, P, batch, gold = load_case(name)
    fc, att, labels, masks, top = batch
    fc, att, top = [t.to(dev) for t in fc], [t.to(dev) for t in att], top.to(dev)
    model = build(cfg, P, dev)
    B, n, S = fc[0].size(0), 4, cfg.seq_length
    with torch.no_grad():
        refs = model.sample_distinct(fc, att, n, {'seed': 99})[0].view(B, n, S).clone()      # another draw serves as references
        seq, seq_lp, _ = model.sample_distinct(fc, att, n, {'seed': 7})
    sb = model.stochastic_beams
    n_refs = torch.full((B,), n, dtype=torch.int32, device=dev)
    out64 = torch.empty(B * n, S, dtype=torch.float64, device=dev)
    sc = RW.CiderD()
    reward = RW.scst_distinct_reward(sc, seq, sb['weight'], refs, n_refs, n, out64=out64)
    # the wrapper is the kernel on the scorer's scores, and the reference-style entry point is the wrapper
    row_img = torch.arange(B * n, dtype=torch.int32, device=dev) // n
    scores = sc.score_ids(seq, row_img, refs, n_refs).cpu().numpy()
    want = RL.distinct_reward(scores, None, sb['weight'].cpu().numpy(), n, S)
    assert same_bits(out64.cpu().numpy(), want) and torch.equal(reward, out64.float())
    opt = types.SimpleNamespace(bleu4_weight=0, spice_weight=0, cider_weight=1.0, use_baseline=1)
    data = {'gts': [r.cpu().numpy() for r in refs]}
    assert same_bits(RW.get_self_critical_reward_distinct(data, seq, sb, opt, scorer=RW.CiderD()), want)
    w = sb['weight'].view(-1)
    zero = ~(w > 0)
    assert bool(zero.any()) and bool((reward[zero] == 0).all()) and float(reward.abs().max()) > 0
    # the two-call form trims at the reference's early exit: both forms get the trimmed rows
    cfg.use_ppo = 0
    seq2, lp2, lp_all, reason = model.sample_group(fc, att, n, {'force_ids': seq})
    T = seq2.size(1)
    assert torch.equal(seq2, seq[:, :T])
    rw = reward[:, :T].contiguous()
    loss2 = R.ReviewNetRewardCriterion(cfg)(lp2, seq2, rw, lp_all, 0.0, reason, top, 1.0, None, cfg)
    model.zero_grad(set_to_none=True)
    loss2.backward()
    want_g = _grads_of(model)

    def fused(tokens):
        loss, _ = model.rl_loss(fc, att, tokens, rw, top, n=n)
        model.zero_grad(set_to_none=True)
        loss.backward()
        return loss.detach().clone(), _grads_of(model)

    loss, got = fused(seq2.contiguous())
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    assert abs(float(loss) - float(loss2.detach())) < 1e-4 * max(1.0, abs(float(loss2.detach())))
    assert maxerr(model.last_rl['logprobs'], lp2.detach().cpu()) < LOGP_TOL
    words = seq2 > 0                                                                        # the search's own log-probs of the words
    assert maxerr(model.last_rl['logprobs'][words], seq_lp[:, :T][words].cpu()) < LOGP_TOL
    rep = compare_grads(got, want_g, grad_bar, check=False)
    print('distinct/%s: worst err/bar %.4f at %s' % (name, rep['ratio'], rep['name']))
    assert not rep['failures'], rep['failures'][:10]
    assert float(got['logit.weight'].abs().max()) > 0
    # zero-reward rows contribute exactly nothing: other tokens in those rows (their words reversed), the same bits everywhere
    moved = seq2.clone()
    changed = 0
    for r in torch.nonzero(zero).view(-1).tolist():
        L = int((moved[r] > 0).sum())
        if L > 1 and not torch.equal(moved[r, :L], moved[r, :L].flip(0)):
            moved[r, :L] = moved[r, :L].flip(0)
            changed += 1
    assert changed > 0
    loss_m, got_m = fused(moved)
    assert torch.equal(loss_m, loss)
    assert all(torch.equal(got_m[k], got[k]) for k in got), [k for k in got if not torch.equal(got_m[k], got[k])][:5]
