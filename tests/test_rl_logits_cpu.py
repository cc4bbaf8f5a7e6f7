"""CPU: the fp64 restatements of the policy-gradient loss from the logits and of the distinct-sample reward (tests/rl_logits_cpu.py)
against torch autograd in double on the reference's formula (misc/utils.py:50-72 written out with log_softmax), the properties
include/rfn.h states for rfn_scst_reward_distinct, and the argument checks of the new entry points through the C ABI with dummy
pointers -- no kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rl_logits_cpu as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('rfn_rl_logits_fwd', 'rfn_rl_logits_bwd', 'rfn_decoder_logits_fwd', 'rfn_decoder_logits_ex', 'rfn_decoder_logits_bwd',
               'rfn_scst_reward_distinct')
OK_DIMS = dict(M=2, R=16, A=16, E=16, T1=3, T2=3, K=20, V1=51, L=[5, 7], D=[24, 40], Fc=[24, 32])
SHAPE, UNSUPPORTED, WORKSPACE, ARG = -1, -2, -4, -5


def _reference(x, seq, reward, entropy_reg, old, ppo_clip):
    """ReviewNetRewardCriterion's policy + entropy terms (misc/utils.py:50-72) on log_softmax(x), torch double, autograd."""
    xd = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True)
    B, T, V1 = xd.shape
    seq = torch.from_numpy(seq)
    tok = torch.where((seq < 0) | (seq >= V1), torch.zeros_like(seq), seq)
    lp_all = torch.log_softmax(xd, 2)
    inp = lp_all.gather(2, tok.unsqueeze(2)).squeeze(2)
    rw = torch.from_numpy(np.asarray(reward, dtype=np.float64))
    mask0 = (seq > 0).double()
    mask = torch.cat([torch.ones(B, 1, dtype=torch.float64), mask0[:, :-1]], 1)
    ent = float(np.float32(entropy_reg))
    entropy = ent * (mask0 * (lp_all * torch.exp(lp_all)).sum(2)).sum() / B
    if old is None:
        pol = inp * rw
    else:
        clip = float(np.float32(ppo_clip))
        surr1 = torch.exp(inp) / (1e-5 + torch.exp(torch.from_numpy(np.asarray(old, dtype=np.float64)))) * rw
        surr2 = torch.clamp(surr1, 1.0 - clip, 1.0 + clip) * rw
        pol = torch.min(surr1, surr2)
    policy = -(pol * mask).sum() / B
    loss = policy + entropy
    loss.backward()
    return float(loss.detach()), float(policy.detach()), float(entropy.detach()), inp.detach().numpy(), xd.grad.numpy()


@pytest.mark.parametrize('ppo', [False, True], ids=['reinforce', 'ppo'])
@pytest.mark.parametrize('entropy_reg', [0.0, 0.01])
@pytest.mark.parametrize('shape', [(3, 4, 37), (4, 6, 64), (2, 1, 5)])
def test_restatement_equals_autograd_in_double(shape, entropy_reg, ppo):
    c = RL.make_case(*shape, seed=7)
    old = c['old'] if ppo else None
    got = RL.rl_logits(c['x'], c['seq'], c['reward'], entropy_reg, old, 0.2)
    loss, policy, entropy, inp, grad = _reference(c['x'], c['seq'], c['reward'], entropy_reg, old, 0.2)
    assert abs(got['loss'] - loss) < 1e-12 * max(1.0, abs(loss))
    assert abs(got['policy'] - policy) < 1e-12 * max(1.0, abs(policy)) and abs(got['entropy'] - entropy) < 1e-12
    assert float(np.abs(got['tok_lp'] - inp).max()) < 1e-12
    assert float(np.abs(got['grad'] - grad).max()) < 1e-12
    if entropy_reg:
        assert float(np.abs(got['Hm']).max()) > 0.0 and got['entropy'] != 0.0
    else:
        assert not got['Hm'].any() and got['entropy'] == 0.0
    # masked rows are exactly zero
    seq = c['seq']
    for b in range(shape[0]):
        for t in range(1, shape[1]):
            if seq[b, t - 1] <= 0 and seq[b, t] <= 0:
                assert not got['grad'][b, t].any() and got['rows'][b, t] == 0.0


def test_ppo_case_reaches_both_sides_of_the_clamp_and_its_inside():
    c = RL.make_case(4, 6, 64, seed=7)
    lp = RL.rl_logits(c['x'], c['seq'], c['reward'])['tok_lp']
    s1 = np.exp(lp) / (1e-5 + np.exp(c['old'].astype(np.float64))) * c['reward']
    mk = np.concatenate([np.ones((4, 1), bool), c['seq'][:, :-1] > 0], 1)
    assert (mk & (s1 < 0.8)).any() and (mk & (s1 > 0.8) & (s1 < 1.2)).any() and (mk & (s1 > 1.2)).any()
    assert (c['reward'] < 0).any() and (c['reward'] > 0).any() and (c['reward'] == 0).any()


def test_upstream_gradient_scales_the_gradient_only():
    c = RL.make_case(3, 4, 37, seed=1)
    a = RL.rl_logits(c['x'], c['seq'], c['reward'], 0.01, c['old'], 0.2, g=1.0)
    b = RL.rl_logits(c['x'], c['seq'], c['reward'], 0.01, c['old'], 0.2, g=0.5)
    assert a['loss'] == b['loss'] and np.allclose(a['grad'] * 0.5, b['grad'], rtol=1e-15, atol=0)


# ---- the reward of a distinct-sample set ------------------------------------------------------------------------------------------
def test_distinct_reward_order_is_ascending_from_zero_and_scaled_by_n():
    w = np.array([0.5, 0.25, 1e-3, 0.0])                       # the threshold row weighs 0
    s = np.array([1.0, 3.0, 2.0, 100.0])
    wsum = ((0.0 + 0.5) + 0.25) + 1e-3
    q = w[:3] / wsum
    base = ((0.0 + q[0] * s[0]) + q[1] * s[1]) + q[2] * s[2]
    r = RL.distinct_reward(s, None, w, 4, 3)
    assert r.shape == (4, 3) and np.array_equal(r[:, :1].repeat(3, 1), r)
    for j in range(3):
        assert r[j, 0] == (q[j] * (s[j] - base)) * 4.0
    assert r[3, 0] == 0.0 and not np.signbit(r[3, 0])
    rn = RL.distinct_reward(s, None, w, 4, 3, baseline='none')
    assert np.array_equal(rn[:3, 0], (q * s[:3]) * 4.0) and rn[3, 0] == 0.0
    # the coefficients of an image sum to ~0 under the weighted baseline: sum_j q_j (s_j - base) = base - base
    assert abs(r[:, 0].sum()) < 1e-12


def test_distinct_reward_dead_rows_dead_images_and_one_live_row():
    s = np.arange(9, dtype=np.float64) + 1.0
    w = np.array([0.4, 0.0, -1.0,        # one weighted row: its coefficient is q * (s - q * s) = 0 with q = 1
                  0.0, 0.0, 0.0,         # a dead image
                  0.3, 0.6, np.nan])     # a NaN weight is no weight
    r = RL.distinct_reward(s, None, w, 3, 2)
    assert np.array_equal(r[:6], np.zeros((6, 2)))
    assert r[6, 0] != 0.0 and r[7, 0] != 0.0 and r[8, 0] == 0.0
    rn = RL.distinct_reward(s, None, w, 3, 2, baseline='none')
    assert rn[0, 0] == (1.0 * s[0]) * 3.0 and not rn[1:6].any()
    # an infinite weight sum: zeros
    assert not RL.distinct_reward(s[:3], None, np.array([np.inf, 1.0, 0.0]), 3, 1).any()


def test_distinct_reward_nan_scores_poison_their_own_image_only_and_only_when_weighted():
    w = np.array([0.5, 0.5, 0.0, 0.5, 0.25, 0.0])
    s = np.array([1.0, np.nan, 2.0, 1.0, 2.0, np.nan])         # weighted NaN in image 0, zero-weight NaN in image 1
    r = RL.distinct_reward(s, None, w, 3, 2)
    assert np.isnan(r[0]).all() and np.isnan(r[1]).all() and not r[2].any()
    clean = RL.distinct_reward(np.where(np.isnan(s), 7.0, s), None, w, 3, 2)
    assert np.array_equal(r[3:], clean[3:]) and np.isfinite(r[3:]).all() and not r[5].any()
    rn = RL.distinct_reward(s, None, w, 3, 2, baseline='none')
    assert np.isfinite(rn[0]).all() and np.isnan(rn[1]).all()          # without a baseline: the row alone


def test_distinct_reward_mixes_the_scores_as_the_group_reward_does():
    rng = np.random.default_rng(3)
    c, b, w = rng.random(6), rng.random((6, 4)), rng.random(6)
    s = RL.mixed_score(c, b, 6, 0.5, 2.0)
    assert np.array_equal(s, ((b[:, 3] * 2.0) + (c * 0.5)) + 0.0)
    assert np.array_equal(RL.distinct_reward(c, b, w, 3, 1, 0.5, 2.0), RL.distinct_reward(s, None, w, 3, 1, 1.0, 0.0))
    assert np.array_equal(RL.mixed_score(None, b, 6, 0.5, 2.0), ((b[:, 3] * 2.0) + (0.0 * 0.5)) + 0.0)
    with pytest.raises(ValueError, match='n >= 3'):
        RL.distinct_reward(c, None, w, 2, 1)
    assert RL.distinct_reward(c, None, w, 2, 1, baseline='none').shape == (6, 1)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def native():
    import recurrent_fusion_network_amd._native as N
    return N


def test_new_symbols_are_declared_exported_and_the_abi_version_stays():
    N = native()
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    assert 'policy-gradient loss from the logits' in src and 'Kool' in src
    declared = set(re.findall(r'\b(rfn_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    for s in NEW_SYMBOLS:
        assert s in declared and s in N.EXPORTS and getattr(N.lib, s).argtypes is not None, s
    assert N.lib.rfn_abi_version() == 9 == N.ABI_VERSION                  # additive: the ABI version stays


def test_rl_logits_entry_points_refuse_bad_calls_before_launching():
    N = native()
    p = 0x10000

    def fwd(B=3, T=4, V1=50, ldl=52, ld_tl=4, logits=p, seq=p, reward=p, old=None, ppo=0, stats=p, tok_lp=p, scratch=p, loss=p):
        return N.lib.rfn_rl_logits_fwd(logits, ldl, B, T, V1, seq, 4, reward, 4, 0.01, old, 4, ppo, 0.2, stats, tok_lp, ld_tl, scratch,
                                       loss, 0, None, None)

    def bwd(B=3, T=4, V1=50, ldl=52, logits=p, seq=p, reward=p, old=None, ppo=0, stats=p):
        return N.lib.rfn_rl_logits_bwd(logits, ldl, B, T, V1, seq, 4, reward, 4, 0.01, old, 4, ppo, 0.2, stats, 1.0, None, None)

    for f in (fwd, bwd):
        for bad in (dict(B=0), dict(T=0), dict(V1=0), dict(B=-1), dict(ldl=49)):
            assert f(**bad) == SHAPE, (f.__name__, bad)
        for bad in (dict(logits=None), dict(seq=None), dict(reward=None), dict(stats=None), dict(ppo=1)):
            assert f(**bad) == ARG, (f.__name__, bad)
        assert f(B=0, logits=None) == SHAPE                                # the shape checks come first
    assert fwd(ld_tl=3) == SHAPE
    for bad in (dict(tok_lp=None), dict(scratch=None), dict(loss=None)):
        assert fwd(**bad) == ARG, bad


def test_decoder_logits_pair_checks_its_arguments_before_launching():
    N = native()
    d = N.make_dims(**OK_DIMS)
    un = N.make_dims(path_flags=N.PATH_OPT_DEC_UNHOISTED, **OK_DIMS)
    P = C.c_void_p(0x10000)
    size = N.lib.rfn_decoder_ws_bytes_ex(C.byref(d), 6, 4, 1, 2)
    assert 0 < size <= N.lib.rfn_decoder_ws_bytes_ex(C.byref(d), 6, 4, 1, 1) + 4 * 3 * 3 * 16 + 1024

    def fwd(dd, B, n, ws=P, size=size, ids=P):
        return N.lib.rfn_decoder_logits_fwd(C.byref(dd), B, 4, P, P, P, P, ids, 4, ws, size, 1, 0, n, None)

    def bwd(dd, B, n, ws=P, size=size, ids=P):
        return N.lib.rfn_decoder_logits_bwd(C.byref(dd), B, 4, P, P, ids, 4, P, P, P, P, ws, size, 0, n, None)

    for f in (fwd, bwd):
        assert f(d, 6, 4) == SHAPE and f(d, 6, 0) == SHAPE and f(d, 0, 1) == SHAPE, f.__name__
        assert f(un, 6, 2) == UNSUPPORTED and f(un, 6, 4) == SHAPE, f.__name__
        assert f(d, 6, 2, ws=None) == ARG and f(d, 6, 2, ids=None) == ARG, f.__name__
        assert f(d, 6, 2, size=16) == WORKSPACE, f.__name__
    # where the rows lie: behind everything the layout puts in front of them, inside the workspace; NULL on a bad query
    base = 0x100000
    at = N.lib.rfn_decoder_logits_ex(C.byref(d), 6, 4, 1, 2, base)
    assert base < at < base + size
    assert N.lib.rfn_decoder_logits_ex(C.byref(d), 6, 4, 1, 1, base) == N.lib.rfn_decoder_logits(C.byref(d), 6, 4, 1, base)
    assert N.lib.rfn_decoder_logits_ex(C.byref(d), 6, 4, 1, 1, base) > at                       # Pd and U shrink to the images
    assert not N.lib.rfn_decoder_logits_ex(C.byref(d), 6, 4, 1, 4, base) and not N.lib.rfn_decoder_logits_ex(C.byref(d), 6, 4, 1, 2, None)
    # the old entry points keep refusing the logits-only form with n > 1
    assert N.lib.rfn_decoder_fwd_ex(C.byref(d), 6, 4, P, P, P, P, P, 4, None, P, size, 1, 0, 2, None) == ARG
    assert N.lib.rfn_decoder_bwd_ex(C.byref(d), 6, 4, P, P, P, P, P, 4, None, None, P, P, P, P, P, size, 0, 2, None) == ARG


def test_distinct_reward_entry_point_refuses_bad_calls_before_launching():
    N = native()
    f = N.lib.rfn_scst_reward_distinct
    w = C.c_double(1.0)
    p = 256
    assert f(p, w, None, w, p, 6, 2, 4, 1, p, None, None) == SHAPE                   # the weighted baseline needs n >= 3
    assert f(p, w, None, w, p, 6, 1, 4, 1, p, None, None) == SHAPE
    assert f(p, w, None, w, p, 6, 4, 4, 1, p, None, None) == SHAPE                   # B % n != 0
    assert f(p, w, None, w, p, 6, 0, 4, 0, p, None, None) == SHAPE
    assert f(p, w, None, w, p, 0, 3, 4, 1, p, None, None) == SHAPE
    assert f(p, w, None, w, p, 6, 3, 0, 1, p, None, None) == SHAPE
    assert f(p, w, None, w, p, 6, 3, 4, 2, p, None, None) == SHAPE                   # baseline is 0 or 1
    assert f(None, w, None, w, p, 6, 3, 4, 1, p, None, None) == ARG                  # neither score
    assert f(p, w, None, w, None, 6, 3, 4, 1, p, None, None) == ARG                  # no weights
    assert f(p, w, p, w, p, 6, 3, 4, 1, None, None, None) == ARG                     # neither output


def test_python_layer_checks_without_a_gpu():
    import types
    from recurrent_fusion_network_amd import rewards as RW
    gen = torch.zeros(6, 4, dtype=torch.int64)
    gts, n_refs = torch.zeros(3, 2, 5, dtype=torch.int64), torch.ones(3, dtype=torch.int32)
    w2, w3 = torch.ones(3, 2, dtype=torch.float64), torch.ones(2, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match='n >= 3'):
        RW.scst_distinct_reward(RW.CiderD(), gen, w2, gts, n_refs, 2)
    with pytest.raises(ValueError, match='per image'):
        RW.scst_distinct_reward(RW.CiderD(), gen, w2, gts, n_refs, 4)
    with pytest.raises(ValueError, match='images of references'):
        RW.scst_distinct_reward(RW.CiderD(), gen, w3, gts, n_refs, 3)
    with pytest.raises(ValueError, match='weighted'):
        RW.scst_distinct_reward(RW.CiderD(), gen, w3, gts[:2], n_refs[:2], 3, baseline='loo')
    with pytest.raises(ValueError, match='scorer'):
        RW.scst_distinct_reward(None, gen, w3, gts[:2], n_refs[:2], 3)
    with pytest.raises(ValueError, match='one entry per row'):
        RW.scst_distinct_reward(RW.CiderD(), gen, torch.ones(5, dtype=torch.float64), gts[:2], n_refs[:2], 3)
    opt = types.SimpleNamespace(bleu4_weight=0, spice_weight=0, cider_weight=1.0, use_baseline=1)
    with pytest.raises(ValueError, match='images'):
        RW.get_self_critical_reward_distinct({'gts': [np.zeros((1, 5), dtype=np.int64)] * 3}, gen, {'weight': w3}, opt,
                                             scorer=RW.CiderD())
    with pytest.raises(ValueError, match='n >= 3'):
        RW.get_self_critical_reward_distinct({'gts': [np.zeros((1, 5), dtype=np.int64)] * 3}, gen, {'weight': w2}, opt,
                                             scorer=RW.CiderD())
