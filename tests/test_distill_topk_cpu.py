"""CPU: the compact-teacher restatement (tests/distill_topk_cpu.py) against torch's float64 autograd on a -inf-filled dense
teacher; the rfn_kd_topk_* ABI is declared, exported and refuses bad calls before any launch; TopKTeacher and
forward_loss(teacher=TopKTeacher) refuse what they cannot honour without a GPU; decode.labels_from_seq against the loader's
rule."""
import os
import re

import numpy as np
import pytest
import torch

import distill_cpu as D
import distill_topk_cpu as DK
from test_distill_cpu import ITS, torch_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows(seed, B=3, T=4, V1=37, K=6):
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, T, V1)) * 3
    ids = np.stack([np.stack([g.permutation(V1)[:K] for _ in range(T)]) for _ in range(B)]).astype(np.int64)
    val = g.standard_normal((B, T, K)) * 3
    ids[0, 1, 2], ids[1, 0, 0], val[2, 3, 4] = -1, V1, -np.inf          # the three kinds of padding
    ids[2, 2, :], val[2, 2, 1:] = np.arange(K), -np.inf                 # a row with one live entry
    tgt = g.integers(-2, V1 + 2, (B, T))
    tgt[1, 2] = ids[1, 2, 3]                                             # a teacher id that is the row's target
    mask = g.choice([0.0, 1.0, 0.5], (B, T), p=[0.3, 0.5, 0.2])
    mask[0, 0], mask[1, 1], mask[1, 2], mask[2, 2] = 0.0, 1.0, 1.0, 1.0
    return x, ids, val, tgt, mask


@pytest.mark.parametrize('it', ITS)
@pytest.mark.parametrize('alpha', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_restatement_matches_torch_float64_autograd(it, alpha, eps):
    x, ids, val, tgt, mask = rows(1)
    got = DK.kd_topk_reference(x, ids, val, tgt, mask, eps, alpha, it)
    z = DK.dense_rows(ids, val, x.shape[2])
    assert np.isneginf(z).sum() >= z.size - ids.size and np.isfinite(z).any(-1).all()
    z[mask == 0] = 0.0                                       # torch's kl_div has no notion of a row that is not read
    loss, xe, kd, grad = torch_form(x, z, tgt, mask, eps, alpha, it)
    assert abs(got['loss'] - loss) <= 1e-12 * max(1.0, abs(loss))
    assert abs(got['xe'] - xe) <= 1e-12 * max(1.0, abs(xe)) and abs(got['kd'] - kd) <= 1e-12 * max(1.0, abs(kd))
    assert np.abs(got['grad'] - grad).max() <= 1e-12
    assert got['kd'] > 0 and np.isfinite(got['grad']).all() and (got['grad'][mask == 0] == 0).all()
    live = DK.live_entries(ids, val, x.shape[2])
    lse_t = np.array([[np.log(np.exp(val[b, t][live[b, t]] * it).sum()) for t in range(x.shape[1])] for b in range(x.shape[0])])
    assert np.abs(got['stats'][2] - lse_t)[mask != 0].max() <= 1e-12 and (got['stats'][2][mask == 0] == 0).all()


def test_masked_rows_of_the_teacher_are_never_looked_at():
    x, ids, val, tgt, mask = rows(2)
    clean = DK.kd_topk_reference(x, ids, val, tgt, mask, 0.1, 0.3, 0.5)
    ids2, val2 = ids.copy(), val.copy()
    ids2[mask == 0], val2[mask == 0] = 10 ** 6, np.nan
    got = DK.kd_topk_reference(x, ids2, val2, tgt, mask, 0.1, 0.3, 0.5)
    assert (mask == 0).sum() >= 2 and got['loss'] == clean['loss'] and np.array_equal(got['grad'], clean['grad'])


def test_a_full_teacher_is_the_dense_restatement_and_padding_is_minus_infinity():
    g = np.random.default_rng(3)
    B, T, V1 = 2, 3, 5
    x, z = g.standard_normal((B, T, V1)), g.standard_normal((B, T, V1))
    tgt, mask = g.integers(0, V1, (B, T)), np.array([[1.0, 0.0, 0.5], [1.0, 1.0, 0.0]])
    ids = np.stack([np.stack([g.permutation(V1) for _ in range(T)]) for _ in range(B)])
    val = np.take_along_axis(z, ids, axis=2)
    a, b = DK.kd_topk_reference(x, ids, val, tgt, mask, 0.1, 0.3, 0.5), D.kd_reference(x, z, tgt, mask, 0.1, 0.3, 0.5)
    assert a['loss'] == b['loss'] and a['kd'] == b['kd'] and np.array_equal(a['grad'], b['grad'])
    # K = 32 at V1 = 5: the rest is padding of all three kinds
    ids32, val32 = np.full((B, T, 32), -1), np.zeros((B, T, 32))
    ids32[:, :, 3:8], val32[:, :, 3:8] = ids, val
    ids32[:, :, 8:16], ids32[:, :, 16:], val32[:, :, 16:] = V1, 0, -np.inf
    c = DK.kd_topk_reference(x, ids32, val32, tgt, mask, 0.1, 0.3, 0.5)
    assert c['loss'] == b['loss'] and np.array_equal(c['grad'], b['grad'])


def test_topk_selection_order():
    x = np.array([[1.0, 3.0, 3.0, -1.0, 3.0, 0.5], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    ids, lp = DK.topk_rows(x, 4)
    assert ids.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]]      # value descending, token ascending among equals
    ref = torch.log_softmax(torch.tensor(x, dtype=torch.float64), 1).numpy()
    assert np.abs(lp - np.take_along_axis(ref, ids, 1)).max() <= 1e-14


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def native():
    import recurrent_fusion_network_amd._native as N
    return N


def test_both_symbols_are_declared_exported_and_bound():
    N = native()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rfn.h')).read(), flags=re.S)
    for name in ('rfn_kd_topk_fwd', 'rfn_kd_topk_bwd'):
        assert re.search(r'\bint %s\s*\(' % name, src), name
        assert name in N.EXPORTS and hasattr(N.lib, name) and getattr(N.lib, name).argtypes is not None
    assert N.lib.rfn_abi_version() == 9                      # additive: the ABI version stays


def fwd_call(N, ldl=51, B=3, T=4, V1=51, eps=0.1, i_sb=4 * 8, i_st=8, v_sb=4 * 8, v_st=8, K=8, alpha=0.3, it=0.5, logits=256,
             target=256, mask=256, t_ids=256, t_val=256, row_stats=256, scratch=256, loss_out=256, terms_out=256):
    return N.lib.rfn_kd_topk_fwd(logits, ldl, B, T, V1, target, 8, mask, 8, eps, t_ids, i_sb, i_st, t_val, v_sb, v_st, K, alpha, it,
                                 row_stats, scratch, loss_out, 0, terms_out, None)


def bwd_call(N, ldl=51, B=3, T=4, V1=51, eps=0.1, i_sb=4 * 8, i_st=8, v_sb=4 * 8, v_st=8, K=8, alpha=0.3, it=0.5, logits=256,
             target=256, mask=256, t_ids=256, t_val=256, row_stats=256):
    return N.lib.rfn_kd_topk_bwd(logits, ldl, B, T, V1, target, 8, mask, 8, eps, t_ids, i_sb, i_st, t_val, v_sb, v_st, K, alpha, it,
                                 row_stats, 1.0, None, None)


@pytest.mark.parametrize('call', [fwd_call, bwd_call])
def test_kd_topk_reject_bad_calls_without_launching(call):
    """Every pointer is the same dummy address: a refused call returns before it reads through any of them and before anything
    is launched."""
    N = native()
    SHAPE, ARG = -1, -5
    for bad in (dict(B=0), dict(T=0), dict(V1=0), dict(ldl=50), dict(eps=-0.1), dict(eps=1.0),           # rfn_xe_logits_*'s
                dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float('nan')),                           # the dense pair's
                dict(it=0.0), dict(it=-1.0), dict(it=float('inf')), dict(it=float('nan')),
                dict(K=0), dict(K=-1), dict(K=33),
                dict(i_sb=7), dict(i_sb=-7), dict(i_st=7), dict(i_st=0), dict(i_st=-7),
                dict(v_sb=7), dict(v_sb=-7), dict(v_st=7), dict(v_st=0), dict(v_st=-7),
                dict(K=32)):                                 # a legal K that the strides (8) no longer hold
        assert call(N, **bad) == SHAPE, bad
    names = ['logits', 'target', 'mask', 't_ids', 't_val', 'row_stats'] + (['scratch', 'loss_out'] if call is fwd_call else [])
    for name in names:
        assert call(N, **{name: None}) == ARG, name
    for bad in (dict(alpha=2.0), dict(K=33), dict(v_st=1)):  # the shape checks come first
        assert call(N, t_ids=None, **bad) == SHAPE and call(N, logits=None, **bad) == SHAPE, bad


# ---- the host -----------------------------------------------------------------------------------------------------------------
def test_topk_teacher_refuses_bad_arrays():
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.distill import TopKTeacher
    assert R.TopKTeacher is TopKTeacher
    B, T, K = 3, 4, 5
    ids, logp = torch.zeros(B, T, K, dtype=torch.int32), torch.zeros(B, T, K)
    t = TopKTeacher(ids, logp)
    assert tuple(t.shape) == (B, T, K) and t.k == K and len(t) == B and t.device == ids.device
    for bad_ids, bad_logp in ((ids[0], logp[0]), (ids, logp[:, :, :4]), (ids[:2], logp), (ids.view(B * T, K), logp.view(B * T, K))):
        with pytest.raises(ValueError, match='shape'):
            TopKTeacher(bad_ids, bad_logp)
    for bad_ids, bad_logp in ((ids.long(), logp), (ids, logp.double()), (ids, logp.half()), (logp, logp), (ids, ids)):
        with pytest.raises(ValueError, match='dtype'):
            TopKTeacher(bad_ids, bad_logp)
    with pytest.raises(ValueError, match='tensors'):
        TopKTeacher(ids.numpy(), logp)
    for k in (0, 33):
        with pytest.raises(ValueError, match='K = %d' % k):
            TopKTeacher(torch.zeros(B, T, k, dtype=torch.int32), torch.zeros(B, T, k))
    TopKTeacher(torch.zeros(B, T, 32, dtype=torch.int32), torch.zeros(B, T, 32))
    TopKTeacher(torch.zeros(B, T, 1, dtype=torch.int32), torch.zeros(B, T, 1))
    with pytest.raises(ValueError, match='device'):
        TopKTeacher(ids, torch.zeros(B, T, K, device='meta'))
    with pytest.raises(ValueError, match='unit stride'):
        TopKTeacher(ids, torch.zeros(B, T, 2 * K)[:, :, ::2])
    with pytest.raises(ValueError, match='overlap'):
        TopKTeacher(ids, torch.zeros(B, 1, K).expand(B, T, K))
    # strided in the first two dimensions is fine: the transposed view of a time-major buffer, padded rows
    tm = TopKTeacher(torch.zeros(T, B, K, dtype=torch.int32).transpose(0, 1), torch.zeros(T + 1, B, K + 3)[:T, :, :K].transpose(0, 1))
    assert tm._abi()[1:3] == (K, B * K) and tm._abi()[4:] == (K + 3, B * (K + 3), K)
    # from_dense: k and dtype are refused before the device is asked for
    for k in (0, 33, 7):
        with pytest.raises(ValueError, match='k = %d' % k):
            TopKTeacher.from_dense(torch.zeros(B, T, 6 if k == 7 else 50), k)
    with pytest.raises(ValueError, match='float32'):
        TopKTeacher.from_dense(torch.zeros(B, T, 50, dtype=torch.float64), 4)
    with pytest.raises(R._native.RfnError, match='GPU'):
        TopKTeacher.from_dense(torch.zeros(B, T, 50), 4)


def test_topk_teacher_members_on_the_host():
    from recurrent_fusion_network_amd.distill import TopKTeacher
    V1 = 9
    ids = torch.tensor([[[3, 0, 8, -1], [2, 9, 5, 1]], [[4, 4, 1, 0], [7, 6, 5, 4]], [[0, 1, 2, 3], [8, -5, 100, 2]]], dtype=torch.int32)
    logp = -torch.arange(24, dtype=torch.float32).view(3, 2, 4) / 7
    logp[1, 0, 1] = float('-inf')                            # the second 4 of that row is padding: no duplicate
    t = TopKTeacher(ids, logp)
    z = t.dense(V1)
    assert tuple(z.shape) == (3, 2, V1) and z.is_contiguous()
    assert np.array_equal(z.double().numpy(), DK.dense_rows(ids.numpy(), logp.numpy(), V1))
    assert t.check(V1) is t
    sub = t[1:]
    assert tuple(sub.shape) == (2, 2, 4) and torch.equal(sub.ids, ids[1:]) and torch.equal(t[torch.tensor([2, 0])].logp, logp[[2, 0]])
    assert tuple(t[1].shape) == (1, 2, 4) and torch.equal(t[-1].ids, ids[2:])
    back = TopKTeacher.from_state_dict(t.state_dict())
    assert torch.equal(back.ids, ids) and torch.equal(back.logp, logp) and set(t.state_dict()) == {'ids', 'logp'}
    assert t.cpu().ids.device.type == 'cpu' and t.to('cpu').logp.dtype == torch.float32
    dup = ids.clone()
    dup[2, 0, 3] = 1
    with pytest.raises(ValueError, match='twice'):
        TopKTeacher(dup, logp).check(V1)
    dead = logp.clone()
    dead[0, 1, 0], dead[0, 1, 2], dead[0, 1, 3] = (float('-inf'),) * 3   # what is left of row (0, 1) is id 9 = V1: padding
    with pytest.raises(ValueError, match='no live entry'):
        TopKTeacher(ids, dead).check(V1)
    TopKTeacher(ids, dead).check(V1 + 1)                     # ... and live in a larger vocabulary


def test_forward_loss_refuses_a_bad_topk_teacher_without_a_gpu():
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    from recurrent_fusion_network_amd.distill import TopKTeacher
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    info = [dict(att_num=5, att_feat_size=24, fc_feat_size=24), dict(att_num=7, att_feat_size=40, fc_feat_size=32)]
    cfg = O.make_cfg(info, vocab_size=50, rnn_size=16, input_encoding_size=16, att_hid_size=16, num_review_steps_0=3,
                     num_review_steps=3, top_words_count=20, seq_length=5)
    cfg.caption_model = 'recurrent_fusion_model'
    model = R.setup(cfg)
    model.load_state_dict(O.seeded_params(cfg, 0))
    crit = R.ReviewNetEnsembleCriterion(cfg)
    fc, att, labels, masks, top = O.synthetic_batch(cfg, 3, seed=1)
    B, S, K = 3, model._decoder_steps(labels), 4

    def teacher(b=B, s=S):
        return TopKTeacher(torch.zeros(b, s, K, dtype=torch.int32), torch.zeros(b, s, K))

    def call(t, **kw):
        return model.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=t, **kw)
    for t in (teacher(b=B + 1), teacher(s=S - 1)):           # wrong batch size, T < S
        with pytest.raises(R._native.RfnError, match='shape'):
            call(t)
    with pytest.raises(R._native.RfnError, match='GPU'):     # a host teacher: there is no CPU path
        call(teacher())
    with pytest.raises(R._native.RfnError, match='GPU'):
        call(teacher(s=S + 2))                               # T > S is fine as a shape
    for kw in (dict(kd_alpha=-0.1), dict(kd_alpha=1.5), dict(kd_temperature=0.0), dict(kd_temperature=float('inf'))):
        with pytest.raises(R._native.RfnError, match='kd_'):
            call(teacher(), **kw)
    model.ss_prob = 0.25
    with pytest.raises(R._native.RfnError, match='scheduled sampling'):
        call(teacher())
    model.ss_prob = 0.0
    model.dedup_seq_per_img = 5
    with pytest.raises(R._native.RfnError, match='dedup_seq_per_img'):
        call(teacher())
    model.dedup_seq_per_img = 0
    assert model.last_distill is None                        # none of the refused calls got as far as a loss
    assert callable(EnsembleDecoder.teacher_topk)


# ---- sequence-level distillation: decoded ids -> labels and masks ---------------------------------------------------------------
def test_labels_from_seq_against_the_loaders_rule():
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.decode import labels_from_seq
    assert R.labels_from_seq is labels_from_seq
    seq = torch.tensor([[0, 0, 0, 0, 0, 0],                  # length 0
                        [4, 9, 2, 7, 1, 3],                  # full length: no 0 at all
                        [5, 6, 0, 8, 9, 0],                  # tokens after the first 0
                        [0, 3, 3, 3, 3, 3],                  # length 0 with a tail
                        [7, 0, 0, 0, 0, 0],
                        [1, 2, 3, 4, 5, 0]])
    for dtype in (torch.int64, torch.int32):
        for S in (None, 6, 9):                               # seq_length larger than S'
            labels, masks = labels_from_seq(seq.to(dtype), S)
            want_l, want_m = DK.labels_masks(seq.numpy(), S)
            assert labels.dtype == torch.int64 and masks.dtype == torch.float32
            assert tuple(labels.shape) == tuple(masks.shape) == (6, (S or 6) + 2)
            assert np.array_equal(labels.numpy(), want_l) and np.array_equal(masks.numpy(), want_m)
    labels, masks = labels_from_seq(seq)
    assert labels[:, 0].eq(0).all() and masks.sum(1).tolist() == [2.0, 8.0, 4.0, 2.0, 3.0, 7.0]
    assert labels[2].tolist() == [0, 5, 6, 0, 0, 0, 0, 0]
    g = np.random.default_rng(0)
    rnd = g.integers(0, 4, (64, 7))                          # many zeros at random places
    labels, masks = labels_from_seq(torch.tensor(rnd), 8)
    want_l, want_m = DK.labels_masks(rnd, 8)
    assert np.array_equal(labels.numpy(), want_l) and np.array_equal(masks.numpy(), want_m)
    with pytest.raises(ValueError, match='seq_length'):
        labels_from_seq(seq, 5)
    for bad in (seq.float(), seq[0], seq.numpy()):
        with pytest.raises(ValueError, match='integer'):
            labels_from_seq(bad)
