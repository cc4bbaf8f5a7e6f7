"""GPU: the mixture-of-softmaxes kernels through the C ABI (rfn_mos_fwd / _loss_fwd / _bwd / _loss_bwd) against the fp64
restatement tests/mos_cpu.py, on inputs of the scale test_xe_logits_kernels_against_float64 uses (expert logits of standard
deviation ~3).  Tolerances are that test's -- the same arithmetic class: log-probs and log-sum-exps 1e-5 absolute, loss 1e-5
relative, d x 1e-6 absolute; d_h, d c and the parameter gradients follow the project's gradient rule 1e-7 + 2e-5 * max|ref|."""
import os

import numpy as np
import pytest
import torch

import mos_cpu as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def grad_close(got, ref, what):
    tol = 1e-7 + 2e-5 * float(ref.abs().max())
    err = float((got.double().cpu() - ref).abs().max())
    assert err <= tol, '%s: %.3e > %.3e' % (what, err, tol)


class Head:
    """One head on the device: parameters in slot order, a train-size workspace, zeroed gradient buffers."""

    def __init__(self, dev, rows, R, K, V1, P):
        N = native()
        self.N, self.dev, self.rows, self.K, self.V1, self.R = N, dev, rows, K, V1, R
        self.md = N.mos_dims(R, R, K, V1)
        self.names = N.mos_param_names(self.md)
        assert self.names == MC.param_names(K)
        self.P = P
        self.prm = [P[k].float().contiguous().to(dev) for k in self.names]
        self.ws = N.mos_workspace(self.md, rows, True, dev)
        self.grd = [torch.full_like(p, float('nan')) for p in self.prm]          # every slot must be overwritten
        self.d_h = torch.full((rows, R), float('nan'), device=dev)

    def fwd(self, h, **kw):
        logp = torch.empty(self.rows, self.V1, device=self.dev)
        self.N.mos_fwd(self.md, h, self.prm, logp, self.ws, train=True, **kw)
        return logp

    def x(self):
        return self.N.mos_ws_x(self.md, self.rows, self.ws)

    def check_grads(self, b, tag):
        grad_close(self.d_h, b['d_h'], tag + ' d_h')
        grad_close(self.N.mos_ws_dc(self.md, self.rows, self.ws), b['dc'], tag + ' dc')
        for k, g in zip(self.names, self.grd):
            grad_close(g.view(b['grads'][k].shape), b['grads'][k], tag + ' ' + k)


def case_inputs(rows, R, K, V1, seed):
    P = MC.random_params(R, R, K, V1, seed)
    g = torch.Generator().manual_seed(seed + 1)
    h = torch.randn(rows, R, generator=g)
    G = torch.randn(rows, V1, generator=g) * 0.01
    return P, h, G


# scalar path (V1 % 4 != 0), vector path with K > 8 and a ragged last tile of rows, K = 1, the headline widths
SHAPES = [(5, 24, 3, 37), (7, 32, 2, 301), (33, 64, 10, 1024), (1, 32, 1, 50), (3, 512, 3, 9488)]


@pytest.mark.parametrize('rows,R,K,V1', SHAPES)
def test_head_forward_and_backward_against_float64(dev, rows, R, K, V1):
    N = native()
    P, h, G = case_inputs(rows, R, K, V1, 40 + K)
    f = MC.forward_parts(P, h)
    assert 1.5 < float(f['x'].std()) < 6.0                   # the scale the tolerances were set for
    hd = Head(dev, rows, R, K, V1, P)
    hg = h.to(dev)
    logp = hd.fwd(hg)
    print('logp err %.3e' % float((logp.double().cpu() - f['logp']).abs().max()))
    assert float((logp.double().cpu() - f['logp']).abs().max()) <= 1e-5
    assert float((N.mos_ws_lse(hd.md, rows, hd.ws).double().cpu() - f['lse']).abs().max()) <= 1e-5
    assert float((N.mos_ws_logpi(hd.md, rows, hd.ws).double().cpu() - f['logpi']).abs().max()) <= 1e-5
    assert float((torch.exp(logp.double()).sum(1) - 1.0).abs().max()) <= 1e-5
    if K == 1:      # one expert: its log-softmax, and the prior gets no gradient at all
        ls = torch.empty(rows, V1, device=dev)
        N.check(N.lib.rfn_log_softmax_fwd(hd.x().data_ptr(), V1, rows, V1, rows, V1, 0, ls.data_ptr(), N.stream_ptr()))
        assert float((logp - ls).abs().max()) <= 1e-5
    b = MC.backward(P, h, G)
    N.mos_bwd(hd.md, hg, hd.prm, G.to(dev), hd.d_h, hd.grd, hd.ws)
    dx = hd.x().double().cpu()
    print('dx err %.3e' % float((dx - b['dx']).abs().max()))
    assert float((dx - b['dx']).abs().max()) <= 1e-6
    hd.check_grads(b, 'two-call')
    if K == 1:
        assert float(N.mos_ws_dc(hd.md, rows, hd.ws).abs().max()) == 0.0


def test_strided_hidden_rows(dev):
    """h with a row stride above R (a slice of a wider buffer) gives the bits of the packed rows, both ways."""
    N = native()
    rows, R, K, V1 = 6, 24, 3, 44
    P, h, G = case_inputs(rows, R, K, V1, 77)
    a, b2 = Head(dev, rows, R, K, V1, P), Head(dev, rows, R, K, V1, P)
    wide = torch.zeros(rows, R + 8, device=dev)
    wide[:, :R] = h.to(dev)
    la, lb = a.fwd(h.to(dev)), b2.fwd(wide[:, :R])
    assert torch.equal(la, lb)
    N.mos_bwd(a.md, h.to(dev), a.prm, G.to(dev), a.d_h, a.grd, a.ws)
    N.mos_bwd(b2.md, wide[:, :R], b2.prm, G.to(dev), b2.d_h, b2.grd, b2.ws)
    assert torch.equal(a.d_h, b2.d_h) and all(torch.equal(x, y) for x, y in zip(a.grd, b2.grd))


def test_small_prior_and_large_logits_stay_finite(dev):
    """A prior logit of -100 and expert logits scaled by 30: log(sum_k pi_k softmax(x_k)) underflows in linear f32 space, the
    log-sum-exp form does not.  Tolerance: every term of a_kv has magnitude up to M = max|x| + max|lse| + max|log pi|, an f32 of
    that size carries 2^-24 * M of rounding, and the E-term dot product behind x adds about sqrt(E) of those: 1e-5 + 16 * 2^-24 * M."""
    rows, R, K, V1 = 4, 32, 3, 64
    P = MC.random_params(R, R, K, V1, 5)
    P['decoder.weight'] *= 30.0
    P['decoder.bias'] *= 30.0
    h = torch.randn(rows, R, generator=torch.Generator().manual_seed(6))
    P['prior.weight'][0] = -100.0 * h[0] / float(h[0] @ h[0])
    f = MC.forward_parts(P, h)
    lin = (torch.softmax(f['c'].float(), 1).t().unsqueeze(2) * torch.softmax(f['x'].float(), 2)).sum(0)
    assert int((lin == 0).sum()) > 0
    M = float(f['x'].abs().max() + f['lse'].abs().max() + f['logpi'].abs().max())
    for v1 in (V1, V1 - 1):          # vector and scalar path
        Pv = dict(P)
        Pv['decoder.weight'], Pv['decoder.bias'] = P['decoder.weight'][:v1], P['decoder.bias'][:v1]
        fv = MC.forward_parts(Pv, h)
        logp = Head(dev, rows, R, K, v1, Pv).fwd(h.to(dev))
        assert bool(torch.isfinite(logp).all())
        assert float((logp.double().cpu() - fv['logp']).abs().max()) <= 1e-5 + 16 * 2.0 ** -24 * M


@pytest.mark.parametrize('V1', [37, 64])
def test_time_major_rows_land_in_batch_major_layout(dev, V1):
    B, S, R, K = 3, 4, 24, 3
    P, h, G = case_inputs(S * B, R, K, V1, 60)
    hd = Head(dev, S * B, R, K, V1, P)
    flat = hd.fwd(h.to(dev))
    out = torch.full((B, S, V1), float('nan'), device=dev)
    hd.N.mos_fwd(hd.md, h.to(dev), hd.prm, out, hd.ws, inner=B, s_inner=S * V1, s_outer=V1, train=True)
    assert torch.equal(out, flat.view(S, B, V1).transpose(0, 1))
    # and the backward reads d_logp through the same remap
    Gd = G.to(dev)
    hd.N.mos_bwd(hd.md, h.to(dev), hd.prm, Gd, hd.d_h, hd.grd, hd.ws)
    ref_dh, ref_g = hd.d_h.clone(), [g.clone() for g in hd.grd]
    hd.fwd(h.to(dev))
    hd.N.mos_bwd(hd.md, h.to(dev), hd.prm, Gd.view(S, B, V1).transpose(0, 1).contiguous(), hd.d_h, hd.grd, hd.ws,
                 inner=B, s_inner=S * V1, s_outer=V1)
    assert torch.equal(hd.d_h, ref_dh) and all(torch.equal(x, y) for x, y in zip(hd.grd, ref_g))


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('R,K,V1', [(24, 3, 37), (64, 10, 1024)])
def test_loss_form_against_head_plus_criterion(dev, R, K, V1, eps):
    N = native()
    B, T = 5, 4
    rows = B * T
    P, h, _ = case_inputs(rows, R, K, V1, 80 + K)
    g = torch.Generator().manual_seed(9)
    target = torch.randint(0, V1, (B, T + 2), generator=g)
    target[1, 2] = V1 + 3                                    # clamped to 0, as rfn_xe_logits_* does
    mask = (torch.rand(B, T + 2, generator=g) > 0.3).float()
    mask[2, 1:] = 0.0                                        # a wholly masked-out image
    mask[0, 1] = 1.0
    tg, mk = target.to(dev), mask.to(dev)
    hg = h.to(dev)
    st = N.stream_ptr()
    # the two-call form: head, then the criterion on (B, T, V1) log-probs
    two = Head(dev, rows, R, K, V1, P)
    logp = torch.empty(B, T, V1, device=dev)
    N.mos_fwd(two.md, hg, two.prm, logp, two.ws, inner=B, s_inner=T * V1, s_outer=V1, train=True)
    scratch, loss2, dlogp = torch.empty(rows, device=dev), torch.zeros(1, device=dev), torch.empty_like(logp)
    N.check(N.lib.rfn_xe_loss(logp.data_ptr(), B, T, V1, tg[:, 1:].data_ptr(), tg.stride(0), mk[:, 1:].data_ptr(), mk.stride(0),
                              eps, 1.0, scratch.data_ptr(), loss2.data_ptr(), 0, dlogp.data_ptr(), st))
    N.mos_bwd(two.md, hg, two.prm, dlogp, two.d_h, two.grd, two.ws, inner=B, s_inner=T * V1, s_outer=V1)
    # the loss form
    one = Head(dev, rows, R, K, V1, P)
    loss1 = torch.full((1,), float('nan'), device=dev)
    N.mos_loss_fwd(one.md, B, T, hg, one.prm, tg[:, 1:], mk[:, 1:], eps, scratch, loss1, one.ws)
    ref = float(MC.loss(P, h, B, T, target[:, 1:], mask[:, 1:], eps))
    print('loss %.7f two-call %.7f fp64 %.7f' % (float(loss1), float(loss2), ref))
    assert abs(float(loss1) - float(loss2)) <= 1e-5 * max(1.0, abs(float(loss2)))
    assert abs(float(loss1) - ref) <= 1e-5 * max(1.0, abs(ref))
    gdev = torch.full((1,), 0.5, device=dev)
    N.mos_loss_bwd(one.md, B, T, hg, one.prm, tg[:, 1:], mk[:, 1:], eps, 2.0, gdev, one.d_h, one.grd, one.ws)     # 2.0 * 0.5 = 1
    b = MC.backward(P, h, MC.loss_G(B, T, V1, target[:, 1:], mask[:, 1:], eps))
    dx = one.x().double().cpu()
    print('dx err %.3e' % float((dx - b['dx']).abs().max()))
    assert float((dx - b['dx']).abs().max()) <= 1e-6
    one.check_grads(b, 'loss form')
    two.check_grads(b, 'two-call')
    # masked-out rows (time-major r = t * B + b): exactly zero in d x, d c and d_h
    dead = (mask[:, 1:T + 1].t().reshape(-1) == 0).nonzero().flatten()
    assert dead.numel() >= T
    dead = dead.to(dev)
    assert float(one.x()[:, dead].abs().max()) == 0.0
    assert float(N.mos_ws_dc(one.md, rows, one.ws)[dead].abs().max()) == 0.0
    assert float(one.d_h[dead].abs().max()) == 0.0


@pytest.mark.parametrize('name,shape', [('t0', (5, 24, 3, 37)), ('t1', (4, 32, 10, 301))])
def test_golden_tiers(dev, name, shape):
    rows, R, K, V1 = shape
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'mos_ref.npz'))
    pre = name + '.'
    P = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    h, prob = P.pop('h'), P.pop('prob')
    logp = Head(dev, rows, R, K, V1, P).fwd(h.to(dev)).double().cpu()
    live = prob >= 1e-30
    assert float((logp - torch.log(prob.double()))[live].abs().max()) <= 1e-5


def test_bad_calls_are_refused(dev):
    import ctypes as C
    N = native()
    rows, R, K, V1 = 4, 16, 2, 20
    P, h, G = case_inputs(rows, R, K, V1, 3)
    hd = Head(dev, rows, R, K, V1, P)
    logp = torch.empty(rows, V1, device=dev)
    args = lambda md, ws_bytes: (C.byref(md), rows, h.to(dev).data_ptr(), R, N.ptr_array(hd.prm), rows, V1, 0,   # noqa: E731
                                 logp.data_ptr(), hd.ws.data_ptr(), ws_bytes, 0, N.stream_ptr())
    assert N.lib.rfn_mos_fwd(*args(N.mos_dims(R, R, 17, V1), hd.ws.numel())) == -1           # RFN_ERR_SHAPE
    assert N.lib.rfn_mos_fwd(*args(hd.md, 1024)) == -4                                       # RFN_ERR_WORKSPACE
    small = N.mos_workspace(hd.md, rows, False, dev)
    assert N.lib.rfn_mos_bwd(C.byref(hd.md), rows, h.to(dev).data_ptr(), R, N.ptr_array(hd.prm), G.to(dev).data_ptr(), rows, V1, 0,
                             hd.d_h.data_ptr(), N.ptr_array(hd.grd), small.data_ptr(), small.numel(), N.stream_ptr()) == -4
