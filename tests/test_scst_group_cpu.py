"""CPU: the multi-sample self-critical reward's restatement (tests/scst_group_cpu.py) has the properties include/rfn.h states,
and the host side of the new entry points (rfn_decoder_*_ex, rfn_dec_attn_bwd_ex, rfn_dec_du_ex, rfn_rowgroup_sum,
rfn_scst_reward_group) validates its arguments -- no kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scst_group_cpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('rfn_decoder_ws_bytes_ex', 'rfn_decoder_fwd_ex', 'rfn_decoder_fwd_sampled_ex', 'rfn_decoder_bwd_ex',
               'rfn_dec_attn_bwd_ex', 'rfn_dec_du_ex', 'rfn_rowgroup_sum', 'rfn_scst_reward_group')
OK_DIMS = dict(M=2, R=16, A=16, E=16, T1=3, T2=3, K=20, V1=51, L=[5, 7], D=[24, 40], Fc=[24, 32])
SHAPE, UNSUPPORTED, ARG = -1, -2, -5


def test_two_draws_get_opposite_rewards_exactly():
    rng = np.random.default_rng(0)
    s = rng.random(14) * 3
    r = G.group_reward(s, None, 2, 5, cider_weight=0.7)
    assert r.shape == (14, 5)
    for k in range(7):
        assert np.array_equal(r[2 * k], -r[2 * k + 1]) and r[2 * k, 0] != 0.0
    assert np.array_equal(r[:, :1].repeat(5, 1), r)


@pytest.mark.parametrize('n', [2, 3, 5, 7])
def test_a_constant_group_gets_exactly_zero(n):
    # dyadic scores: the sum of n - 1 of them is exact, and its correctly rounded quotient by n - 1 is the score again
    for v in (0.0, 1.5, 0.375, 3.0):
        s = np.full(2 * n, v)
        r = G.group_reward(s, None, n, 3)
        assert np.array_equal(r, np.zeros((2 * n, 3))) and not np.signbit(r).any()      # the trailing + 0.0: never -0


def test_baseline_order_is_ascending_from_zero():
    s = np.array([1e16, 1.0, -1e16, 1.0])                      # ((0 + 1.0) + -1e16) + 1.0 for row 0, by hand
    want0 = s[0] - (((0.0 + 1.0) + -1e16) + 1.0) / 3.0
    want1 = s[1] - (((0.0 + 1e16) + -1e16) + 1.0) / 3.0
    d = G.loo_diff(s, 4)
    assert d[0] == want0 and d[1] == want1
    assert np.array_equal(G.loo_diff(s, 4, 'none'), s)


def test_a_nan_stays_inside_its_images_group():
    s = np.array([0.5, np.nan, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0])
    r = G.group_reward(s, None, 3, 2)
    assert np.isnan(r[:3]).all() and np.isfinite(r[3:]).all()
    clean = G.group_reward(np.where(np.isnan(s), 0.25, s), None, 3, 2)
    assert np.array_equal(r[3:], clean[3:])
    rn = G.group_reward(s, None, 3, 2, baseline='none')
    assert np.isnan(rn[1]).all() and np.isfinite(np.delete(rn, 1, 0)).all()        # without a baseline: the row alone


def test_weights_and_the_missing_scorer_behave_as_in_the_mixed_reward():
    rng = np.random.default_rng(3)
    c, b = rng.random(6), rng.random((6, 4))
    both = G.group_reward(c, b, 3, 4, cider_weight=0.5, bleu4_weight=2.0)
    dc, db = G.loo_diff(c, 3), G.loo_diff(b[:, 3], 3)
    assert np.array_equal(both[:, 0], ((db * 2.0) + (dc * 0.5)) + 0.0)
    assert np.array_equal(G.group_reward(c, None, 3, 4, cider_weight=0.5)[:, 0], ((0.0 * 0.0) + (dc * 0.5)) + 0.0)
    assert np.array_equal(G.group_reward(None, b, 3, 4, bleu4_weight=2.0)[:, 0], ((db * 2.0) + 0.0) + 0.0)
    # a missing scorer is 0 * weight: an infinite weight on it poisons the reward as the reference's product would
    with np.errstate(invalid='ignore'):
        assert np.isnan(G.group_reward(c, None, 3, 4, bleu4_weight=np.inf)).all()
    # -0 becomes +0 through the trailing + 0.0
    z = G.group_reward(np.array([1.0, 1.0]), None, 2, 1, cider_weight=-1.0)
    assert np.array_equal(z, [[0.0], [0.0]]) and not np.signbit(z).any()
    with pytest.raises(AssertionError):
        G.loo_diff(c, 4)
    with pytest.raises(AssertionError):
        G.loo_diff(c[:1], 1)


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def test_new_symbols_are_declared_exported_and_the_abi_version_stays():
    N = native()
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    assert 'multi-sample self-critical' in src
    declared = set(re.findall(r'\b(rfn_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    for s in NEW_SYMBOLS:
        assert s in declared and s in N.EXPORTS and hasattr(N.lib, s), s
    assert N.lib.rfn_abi_version() == 9                                   # additive: the ABI version stays


def test_workspace_query_with_rows_per_image():
    N = native()
    d = N.make_dims(**OK_DIMS)
    dp = C.byref(d)
    for B, S, train in ((3, 4, 1), (6, 2, 0), (12, 5, 1)):
        assert N.lib.rfn_decoder_ws_bytes_ex(dp, B, S, train, 1) == N.lib.rfn_decoder_ws_bytes(dp, B, S, train) > 0
    assert N.lib.rfn_decoder_ws_bytes_ex(dp, 6, 4, 1, 4) == 0              # n does not divide B
    assert N.lib.rfn_decoder_ws_bytes_ex(dp, 6, 4, 1, 0) == 0
    assert N.lib.rfn_decoder_ws_bytes_ex(dp, 0, 4, 1, 1) == 0
    # inference workspace: Pd (T2, rows, A) and U (T2, rows, GD) shrink from B rows to B / n images, nothing else changes;
    # each of the two slabs is rounded up to 256 bytes
    whole, third = N.lib.rfn_decoder_ws_bytes_ex(dp, 12, 4, 0, 1), N.lib.rfn_decoder_ws_bytes_ex(dp, 12, 4, 0, 3)
    saved = 4 * OK_DIMS['T2'] * (12 - 4) * (OK_DIMS['A'] + 4 * OK_DIMS['R'])
    assert 0 < whole - third and abs((whole - third) - saved) <= 2 * 256


def test_entry_points_refuse_bad_rows_per_image_before_launching():
    N = native()
    d = N.make_dims(**OK_DIMS)
    un = N.make_dims(path_flags=N.PATH_OPT_DEC_UNHOISTED, **OK_DIMS)
    P = C.c_void_p(0x10000)
    size = N.lib.rfn_decoder_ws_bytes(C.byref(d), 6, 4, 1)

    def fwd(dd, B, n):
        return N.lib.rfn_decoder_fwd_ex(C.byref(dd), B, 4, P, P, P, P, P, 4, P, P, size, 1, 0, n, None)

    def sampled(dd, B, n):
        return N.lib.rfn_decoder_fwd_sampled_ex(C.byref(dd), B, 4, P, P, P, P, P, 4, 1.0, 1.0, P, P, P, P, size, 1, 0, n, None)

    def bwd(dd, B, n):
        return N.lib.rfn_decoder_bwd_ex(C.byref(dd), B, 4, P, P, P, P, P, 4, P, P, P, P, P, P, P, size, 0, n, None)

    for f in (fwd, sampled, bwd):
        assert f(d, 6, 4) == SHAPE and f(d, 6, 0) == SHAPE and f(d, 6, -2) == SHAPE, f.__name__
        assert f(un, 6, 2) == UNSUPPORTED, f.__name__
        assert f(un, 6, 4) == SHAPE, f.__name__                            # the shape is checked first
    assert N.lib.rfn_decoder_fwd_ex(C.byref(d), 6, 4, P, P, P, P, P, 4, P, None, size, 1, 0, 2, None) == ARG
    # the logits-only form (log_prob NULL) is reached through rfn_decoder_logits: one row per image only
    assert N.lib.rfn_decoder_fwd_ex(C.byref(d), 6, 4, P, P, P, P, P, 4, None, P, size, 1, 0, 2, None) == ARG
    assert N.lib.rfn_decoder_bwd_ex(C.byref(d), 6, 4, P, P, P, P, P, 4, None, None, P, P, P, P, P, size, 0, 2, None) == ARG
    assert N.lib.rfn_decoder_fwd_ex(C.byref(d), 6, 4, P, P, P, P, P, 4, P, P, 16, 1, 0, 2, None) == -4      # workspace too small


def test_kernel_entry_points_refuse_bad_shapes_before_launching():
    N = native()
    p = 0x10000
    ab = lambda B, rd: N.lib.rfn_dec_attn_bwd_ex(p, 4, 4, p, p, p, p, 16, 16, p, 16, B, rd, 1, 4, 16, p, 4, 4, 0, p, p, None)  # noqa: E731
    assert ab(2, 0) == SHAPE and ab(0, 1) == SHAPE and ab(2, -1) == SHAPE
    assert N.lib.rfn_dec_attn_bwd_ex(p, 4, 4, p, p, p, None, 16, 16, p, 16, 2, 2, 1, 4, 16, p, 4, 4, 0, p, p, None) == ARG
    du = lambda B, rd: N.lib.rfn_dec_du_ex(p, p, 2, B, 2, 4, rd, p, 8, 4, None)  # noqa: E731
    assert du(6, 4) == SHAPE and du(6, 0) == SHAPE and du(0, 1) == SHAPE
    assert N.lib.rfn_dec_du_ex(p, None, 2, 6, 2, 4, 3, p, 8, 4, None) == ARG
    assert N.lib.rfn_dec_du_ex(p, p, 3277, 2, 5, 4, 2, p, 20, 4, None) == SHAPE          # 2 * S * L floats of LDS: over 64 KiB
    rs = N.lib.rfn_rowgroup_sum
    assert rs(p, 8, 0, p, 8, 4, 8, None) == SHAPE and rs(p, 8, 2, p, 8, 0, 8, None) == SHAPE and rs(p, 8, 2, p, 8, 4, 0, None) == SHAPE
    assert rs(p, 4, 2, p, 8, 4, 8, None) == SHAPE and rs(p, 8, 2, p, 4, 4, 8, None) == SHAPE                # a stride below cols
    assert rs(None, 8, 2, p, 8, 4, 8, None) == ARG and rs(p, 8, 2, None, 8, 4, 8, None) == ARG


def test_group_reward_entry_point_refuses_bad_calls_before_launching():
    N = native()
    f = N.lib.rfn_scst_reward_group
    w = C.c_double(1.0)
    assert f(256, w, None, w, 6, 1, 4, 1, 256, None, None) == SHAPE                  # n = 1 with leave-one-out
    assert f(256, w, None, w, 6, 4, 4, 1, 256, None, None) == SHAPE                  # B % n != 0
    assert f(256, w, None, w, 6, 4, 4, 0, 256, None, None) == SHAPE
    assert f(256, w, None, w, 6, 0, 4, 0, 256, None, None) == SHAPE                  # n < 1
    assert f(256, w, None, w, 0, 2, 4, 1, 256, None, None) == SHAPE
    assert f(256, w, None, w, 6, 2, 0, 1, 256, None, None) == SHAPE
    assert f(256, w, None, w, 6, 2, 4, 2, 256, None, None) == SHAPE                  # baseline is 0 or 1
    assert f(None, w, None, w, 6, 2, 4, 1, 256, None, None) == ARG                   # neither score
    assert f(256, w, 256, w, 6, 2, 4, 1, None, None, None) == ARG                    # neither output


def test_python_layer_checks_without_a_gpu():
    import torch
    from recurrent_fusion_network_amd import rewards as RW
    gen = torch.zeros(6, 4, dtype=torch.int64)
    gts, n_refs = torch.zeros(3, 2, 5, dtype=torch.int64), torch.ones(3, dtype=torch.int32)
    with pytest.raises(ValueError):
        RW.scst_group_reward(RW.CiderD(), gen, gts, n_refs, 4)                       # 6 rows are not 4 per image
    with pytest.raises(ValueError):
        RW.scst_group_reward(RW.CiderD(), gen, gts, n_refs, 1)                       # leave-one-out of one draw
    with pytest.raises(ValueError):
        RW.scst_group_reward(RW.CiderD(), gen, gts, n_refs, 3)                       # 2 images of rows, 3 of references
    with pytest.raises(ValueError):
        RW.scst_group_reward(RW.CiderD(), gen, gts, n_refs, 2, baseline='greedy')
    with pytest.raises(ValueError):
        RW.scst_group_reward(None, gen, gts, n_refs, 2)
    import types
    opt = types.SimpleNamespace(bleu4_weight=0, spice_weight=1, cider_weight=1.0, use_baseline=1)
    with pytest.raises(NotImplementedError):
        RW.get_self_critical_reward_group({'gts': []}, gen, 2, opt, scorer=RW.CiderD())
    opt.spice_weight, opt.bleu4_weight = 0, 0.5
    with pytest.raises(NotImplementedError):
        RW.get_self_critical_reward_group({'gts': []}, gen, 2, opt, scorer=RW.CiderD())      # BLEU-4 weight without its scorer
    opt.bleu4_weight = 0
    with pytest.raises(ValueError):
        RW.get_self_critical_reward_group({'gts': [np.zeros((1, 5), dtype=np.int64)] * 2}, gen, 2, opt, scorer=RW.CiderD())
