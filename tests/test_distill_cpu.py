"""CPU: the distillation restatement (tests/distill_cpu.py) against torch's float64 autograd and against its own definition's
properties; the rfn_kd_logits_* ABI is declared, exported and refuses bad calls before any launch; forward_loss(teacher=)
refuses what it cannot honour before any native call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_cpu as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITS = (1.0, 0.5, 2.0, D.f32(1.0 / 3.0))


def rows(seed, B=3, T=4, V1=37):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, T, V1)) * 3
    z = g.standard_normal((B, T, V1)) * 3
    tgt = g.integers(-2, V1 + 2, (B, T))                    # some out of range
    mask = g.choice([0.0, 1.0, 0.5], (B, T), p=[0.3, 0.5, 0.2])
    mask[0, 0], mask[1, 1] = 0.0, 1.0
    return x, z, tgt, mask


def torch_form(x, z, tgt, mask, eps, alpha, it):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    zt, m = torch.tensor(z, dtype=torch.float64), torch.tensor(mask, dtype=torch.float64)
    B, T, V1 = x.shape
    tg = torch.tensor(tgt).clone()
    tg[(tg < 0) | (tg >= V1)] = 0
    lp = torch.log_softmax(xt, 2)
    q = torch.full_like(lp, eps / V1)
    q.scatter_(2, tg.unsqueeze(2), 1 - eps + eps / V1)
    xe = (m * -(q * lp).sum(2)).sum() / B
    kl = F.kl_div(torch.log_softmax(xt * it, 2), torch.softmax(zt * it, 2), reduction='none').sum(2)
    kd = (m * kl).sum() / (it * it) / B
    loss = (1 - alpha) * xe + alpha * kd
    loss.backward()
    return float(loss.detach()), float(xe.detach()), float(kd.detach()), xt.grad.numpy()


@pytest.mark.parametrize('it', ITS)
@pytest.mark.parametrize('alpha', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_restatement_matches_torch_float64_autograd(it, alpha, eps):
    x, z, tgt, mask = rows(1)
    got = D.kd_reference(x, z, tgt, mask, eps, alpha, it)
    loss, xe, kd, grad = torch_form(x, z, tgt, mask, eps, alpha, it)
    assert abs(got['loss'] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert abs(got['xe'] - xe) <= 1e-12 * max(1.0, abs(xe)) and abs(got['kd'] - kd) <= 1e-12 * max(1.0, abs(kd))
    assert np.abs(got['grad'] - grad).max() <= 1e-12
    lse = torch.logsumexp(torch.tensor(x), 2).numpy(), torch.logsumexp(torch.tensor(x * it), 2).numpy(), \
        torch.logsumexp(torch.tensor(z * it), 2).numpy()
    assert np.abs(got['stats'] - np.stack(lse)).max() <= 1e-12
    assert got['kd'] > 0


def test_a_per_row_shift_of_the_teacher_changes_nothing():
    x, z, tgt, mask = rows(2)
    shift = np.random.default_rng(3).standard_normal(z.shape[:2] + (1,)) * 7
    for it in ITS:
        a, b = D.kd_reference(x, z, tgt, mask, 0.1, 0.3, it), D.kd_reference(x, z + shift, tgt, mask, 0.1, 0.3, it)
        assert abs(a['loss'] - b['loss']) <= 1e-12 * abs(a['loss']) and abs(a['kd'] - b['kd']) <= 1e-12 * abs(a['kd'])
        assert np.abs(a['grad'] - b['grad']).max() <= 1e-13
        # log-probs are such a shift: the teacher may be handed over either way
        c = D.kd_reference(x, z - D._lse(z)[..., None], tgt, mask, 0.1, 0.3, it)
        assert abs(a['loss'] - c['loss']) <= 1e-12 * abs(a['loss']) and np.abs(a['grad'] - c['grad']).max() <= 1e-13


def test_minus_infinity_in_the_teacher_contributes_zero():
    x, z, tgt, mask = rows(4)
    hole = np.random.default_rng(5).random(z.shape) < 0.3
    hole[..., 0] = False                                     # every row keeps a finite entry
    z[hole] = -np.inf
    for it in ITS:
        got = D.kd_reference(x, z, tgt, mask, 0.1, 0.3, it)
        assert np.isfinite(got['loss']) and np.isfinite(got['kd']) and np.isfinite(got['grad']).all() and np.isfinite(got['stats']).all()
        # the same as a teacher that is merely very unlikely there
        z2 = np.where(hole, -1e4, z)
        ref = D.kd_reference(x, z2, tgt, mask, 0.1, 0.3, it)
        assert abs(got['loss'] - ref['loss']) <= 1e-12 * abs(ref['loss']) and np.abs(got['grad'] - ref['grad']).max() <= 1e-13


def test_nan_teacher_rows_under_a_zero_mask_stay_out():
    x, z, tgt, mask = rows(6)
    clean = D.kd_reference(x, z, tgt, mask, 0.1, 0.3, 0.5)
    z2 = z.copy()
    z2[mask == 0] = np.nan
    got = D.kd_reference(x, z2, tgt, mask, 0.1, 0.3, 0.5)
    assert (mask == 0).sum() >= 2
    assert got['loss'] == clean['loss'] and got['kd'] == clean['kd'] and np.array_equal(got['grad'], clean['grad'])
    assert (got['grad'][mask == 0] == 0).all() and np.isfinite(got['grad']).all()


def test_alpha_zero_is_the_xe_restatement():
    x, z, tgt, mask = rows(7)
    for eps in (0.0, 0.1):
        a, b = D.kd_reference(x, z, tgt, mask, eps, 0.0, 0.5), D.xe_reference(x, tgt, mask, eps)
        assert a['loss'] == b['loss'] == a['xe'] and np.array_equal(a['grad'], b['grad'])


def test_a_teacher_equal_to_the_student_has_no_kd_term():
    x, _, tgt, mask = rows(8)
    for it in ITS:
        for alpha in (0.3, 1.0):
            a, b = D.kd_reference(x, x, tgt, mask, 0.1, alpha, it), D.xe_reference(x, tgt, mask, 0.1)
            assert abs(a['kd']) <= 1e-14 and abs(a['loss'] - (1 - alpha) * b['loss']) <= 1e-13
            assert np.abs(a['grad'] - (1 - alpha) * b['grad']).max() <= 1e-15


# ---- the ABI: declared, exported, and refusing bad calls before any launch -------------------------------------------------
def native():
    import recurrent_fusion_network_amd._native as N
    return N


def test_both_symbols_are_declared_and_exported():
    N = native()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rfn.h')).read(), flags=re.S)
    for name in ('rfn_kd_logits_fwd', 'rfn_kd_logits_bwd'):
        assert re.search(r'\bint %s\s*\(' % name, src), name
        assert name in N.EXPORTS and hasattr(N.lib, name)
    assert N.lib.rfn_abi_version() == 9                      # additive: the ABI version stays


def fwd_call(N, ldl=51, B=3, T=4, V1=51, eps=0.1, z_sb=4 * 51, z_st=51, alpha=0.3, it=0.5, logits=256, target=256, mask=256,
             teacher=256, row_stats=256, scratch=256, loss_out=256, terms_out=256):
    return N.lib.rfn_kd_logits_fwd(logits, ldl, B, T, V1, target, 8, mask, 8, eps, teacher, z_sb, z_st, alpha, it, row_stats,
                                   scratch, loss_out, 0, terms_out, None)


def bwd_call(N, ldl=51, B=3, T=4, V1=51, eps=0.1, z_sb=4 * 51, z_st=51, alpha=0.3, it=0.5, logits=256, target=256, mask=256,
             teacher=256, row_stats=256):
    return N.lib.rfn_kd_logits_bwd(logits, ldl, B, T, V1, target, 8, mask, 8, eps, teacher, z_sb, z_st, alpha, it, row_stats,
                                   1.0, None, None)


@pytest.mark.parametrize('call', [fwd_call, bwd_call])
def test_kd_logits_reject_bad_calls_without_launching(call):
    """Every pointer is the same dummy address: a refused call returns before it reads through any of them and before anything
    is launched."""
    N = native()
    SHAPE, ARG = -1, -5
    for bad in (dict(B=0), dict(T=0), dict(V1=0), dict(ldl=50), dict(eps=-0.1), dict(eps=1.0),           # rfn_xe_logits_*'s
                dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float('nan')),
                dict(it=0.0), dict(it=-1.0), dict(it=float('inf')), dict(it=float('nan')),
                dict(z_sb=50), dict(z_sb=-50), dict(z_st=50), dict(z_st=0), dict(z_st=-50)):
        assert call(N, **bad) == SHAPE, bad
    names = ['logits', 'target', 'mask', 'teacher', 'row_stats'] + (['scratch', 'loss_out'] if call is fwd_call else [])
    for name in names:
        assert call(N, **{name: None}) == ARG, name
    assert call(N, alpha=2.0, teacher=None) == SHAPE         # the shape checks come first, as in rfn_xe_logits_*


# ---- the host: refusals before any native call ------------------------------------------------------------------------------
def test_forward_loss_refuses_a_bad_teacher_without_a_gpu():
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    info = [dict(att_num=5, att_feat_size=24, fc_feat_size=24), dict(att_num=7, att_feat_size=40, fc_feat_size=32)]
    cfg = O.make_cfg(info, vocab_size=50, rnn_size=16, input_encoding_size=16, att_hid_size=16, num_review_steps_0=3,
                     num_review_steps=3, top_words_count=20, seq_length=5)
    cfg.caption_model = 'recurrent_fusion_model'
    model = R.setup(cfg)
    model.load_state_dict(O.seeded_params(cfg, 0))
    crit = R.ReviewNetEnsembleCriterion(cfg)
    fc, att, labels, masks, top = O.synthetic_batch(cfg, 3, seed=1)
    B, S, V1 = 3, model._decoder_steps(labels), 51
    assert model.last_distill is None

    def call(teacher, **kw):
        return model.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=teacher, **kw)
    for shape in ((B, S, V1 - 1), (B + 1, S, V1), (B, S - 1, V1), (B * S, V1)):
        with pytest.raises(R._native.RfnError, match='shape'):
            call(torch.zeros(shape))
    with pytest.raises(R._native.RfnError, match='float32'):
        call(torch.zeros(B, S, V1, dtype=torch.float64))
    with pytest.raises(R._native.RfnError, match='float32'):
        call(torch.zeros(B, S, V1, dtype=torch.float16))
    with pytest.raises(R._native.RfnError, match='GPU'):     # a host tensor: there is no CPU path
        call(torch.zeros(B, S, V1))
    with pytest.raises(R._native.RfnError, match='tensor'):
        call([[0.0]])
    for kw in (dict(kd_alpha=-0.1), dict(kd_alpha=1.5), dict(kd_temperature=0.0), dict(kd_temperature=float('inf'))):
        with pytest.raises(R._native.RfnError, match='kd_'):
            call(torch.zeros(B, S, V1), **kw)
    model.ss_prob = 0.25
    with pytest.raises(R._native.RfnError, match='scheduled sampling'):
        call(torch.zeros(B, S, V1))
    model.ss_prob = 0.0
    assert model.last_distill is None                        # none of the refused calls got as far as a loss
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    assert callable(EnsembleDecoder.teacher_logits)
