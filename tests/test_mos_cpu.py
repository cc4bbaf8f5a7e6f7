"""CPU: the restatement of the mixture-of-softmaxes head (tests/mos_cpu.py) against the reference module's recorded output
(tests/golden/mos_ref.npz, tools/make_mos_golden.py) and against torch fp64 autograd; the new symbols of the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

import mos_cpu as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIERS = {'t0': (5, 24, 3, 37), 't1': (4, 32, 10, 301)}      # rows, R = E, K, V1


def golden_tier(name):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'mos_ref.npz'))
    pre = name + '.'
    t = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    h, prob = t.pop('h'), t.pop('prob')
    return t, h, prob


@pytest.mark.parametrize('name', sorted(TIERS))
def test_restatement_reproduces_the_reference_module(name):
    rows, R, K, V1 = TIERS[name]
    P, h, prob = golden_tier(name)
    assert sorted(P) == sorted(MC.param_names(K))          # the archive lists its members by name
    assert P['prior.weight'].shape == (K, R) and P['latent.%d.0.weight' % (K - 1)].shape == (R, R)
    assert P['latent.0.0.bias'].shape == (R,) and P['decoder.weight'].shape == (V1, R) and P['decoder.bias'].shape == (V1,)
    assert h.shape == (rows, R) and prob.shape == (rows, V1) and prob.dtype == torch.float32
    logp = MC.log_prob(P, h)
    live = prob >= 1e-30
    assert int(live.sum()) > rows * V1 // 2
    err = (logp - torch.log(prob.double()))[live].abs().max()
    assert float(err) <= 1e-5, float(err)


@pytest.mark.parametrize('name', sorted(TIERS))
def test_rows_sum_to_one(name):
    P, h, _ = golden_tier(name)
    s = torch.exp(MC.log_prob(P, h)).sum(1)
    assert float((s - 1.0).abs().max()) <= 1e-12


def test_log_sum_exp_form_is_finite_where_the_linear_form_underflows():
    R, K, V1 = 16, 3, 41
    P = MC.random_params(R, R, K, V1, 5)
    P['decoder.weight'] *= 30.0
    P['decoder.bias'] *= 30.0
    h = torch.randn(4, R, generator=torch.Generator().manual_seed(6))
    P['prior.weight'][0] = -100.0 * h[0] / float(h[0] @ h[0])      # prior logit -100 on row 0
    f = MC.forward_parts(P, h)
    assert abs(float(f['c'][0, 0]) + 100.0) < 1e-4           # f32 weights
    assert bool(torch.isfinite(f['logp']).all())
    x32 = f['x'].float()
    lin = (torch.softmax(f['c'].float(), 1).t().unsqueeze(2) * torch.softmax(x32, 2)).sum(0)
    assert int((lin == 0).sum()) > 0, 'the case is meant to underflow in linear f32 space'


@pytest.mark.parametrize('rows,R,K,V1', [(5, 24, 3, 37), (3, 16, 1, 19), (4, 32, 10, 61)])
def test_restatement_backward_equals_autograd(rows, R, K, V1):
    P = MC.random_params(R, R, K, V1, 11 + K)
    g = torch.Generator().manual_seed(12)
    h = torch.randn(rows, R, generator=g)
    G = torch.randn(rows, V1, generator=g)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    h64 = h.double().requires_grad_(True)
    f = MC.forward_parts(P64, h64)
    keep = [f['x'], f['c']]
    for t in keep:
        t.retain_grad()
    (f['logp'] * G.double()).sum().backward()
    b = MC.backward(P, h, G)

    def close(a, ref):
        assert float((a - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    close(b['dx'], f['x'].grad)
    close(b['dc'], f['c'].grad)
    close(b['d_h'], h64.grad)
    for k in MC.param_names(K):
        close(b['grads'][k], P64[k].grad)
    if K == 1:
        assert float(b['dc'].abs().max()) == 0.0


def test_loss_form_matches_the_criterion_on_log_probs():
    B, T, R, K, V1 = 3, 4, 16, 2, 23
    P = MC.random_params(R, R, K, V1, 21)
    g = torch.Generator().manual_seed(22)
    h = torch.randn(T * B, R, generator=g)
    target = torch.randint(0, V1, (B, T), generator=g)
    target[0, 1] = V1 + 4                                   # clamped to 0
    mask = (torch.rand(B, T, generator=g) > 0.3).float()
    for eps in (0.0, 0.1):
        h64 = h.double().requires_grad_(True)
        logp = MC.log_prob(P, h64)
        G = MC.loss_G(B, T, V1, target, mask, eps)
        ref = (G * logp).sum()
        assert abs(float(MC.loss(P, h, B, T, target, mask, eps)) - float(ref.detach())) <= 1e-12
        ref.backward()
        assert float((MC.backward(P, h, G)['d_h'] - h64.grad).abs().max()) <= 1e-12


def test_new_symbols_are_declared_and_exported():
    import recurrent_fusion_network_amd._native as N
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    assert re.search(r'^#define RFN_ABI_VERSION 9$', src, flags=re.M)
    assert N.ABI_VERSION == 9 and N.lib.rfn_abi_version() == 9
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for s in ['rfn_mos_param_count', 'rfn_mos_param_name', 'rfn_mos_param_shape', 'rfn_mos_ws_bytes', 'rfn_mos_fwd',
              'rfn_mos_loss_fwd', 'rfn_mos_bwd', 'rfn_mos_loss_bwd', 'rfn_decoder_fwd_hidden', 'rfn_decoder_hidden',
              'rfn_decoder_bwd_hidden']:
        assert re.search(r'\b%s\s*\(' % s, code), '%s is not declared in rfn.h' % s
        assert s in N.EXPORTS and hasattr(N.lib, s), s
    assert 'typedef struct rfn_mos_dims' in code


def test_parameter_table_and_limits():
    import ctypes as C
    import recurrent_fusion_network_amd._native as N
    md = N.mos_dims(24, 24, 3, 37)
    assert N.mos_param_names(md) == MC.param_names(3)
    shapes = [N.mos_param_shape(md, i) for i in range(9)]
    assert shapes == [(3, 24), (24, 24), (24, 1), (24, 24), (24, 1), (24, 24), (24, 1), (37, 24), (37, 1)]
    for K in (0, 17):
        bad = N.mos_dims(24, 24, K, 37)
        assert N.lib.rfn_mos_param_count(C.byref(bad)) == -1            # RFN_ERR_SHAPE
        assert N.lib.rfn_mos_ws_bytes(C.byref(bad), 5, 0) == 0
    assert N.lib.rfn_mos_param_count(C.byref(N.mos_dims(8, 8, 16, 9))) == 35
    # the workspace grows with the rows, and the train form adds the backward's slabs
    w0, w1 = N.lib.rfn_mos_ws_bytes(C.byref(md), 5, 0), N.lib.rfn_mos_ws_bytes(C.byref(md), 500, 0)
    assert 0 < w0 < w1 < N.lib.rfn_mos_ws_bytes(C.byref(md), 500, 1)
    assert w1 >= 4 * 3 * 500 * (37 + 24)
