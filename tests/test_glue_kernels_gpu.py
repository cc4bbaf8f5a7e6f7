"""The streaming kernels between the GEMMs (csrc/rfn_cell.hip, csrc/rfn_glue.hip, rfn_logsoftmax.hip, rfn_criteria.hip,
rfn_adam.hip, rfn_pick.hip, rfn_gather_rows), swept over the shapes and alignments at which each of them changes its code
path, through the C ABI, against plain restatements.

Every output buffer is pre-filled with NaN (integers: a sentinel), leading dimensions are wider than the rows, and the
padding as well as the elements past the end are checked unchanged.

Tolerances
----------
* data movers and selections (embed forward, gather, fill, copy, max over steps, picked ids, masks): bit-equal.
* fixed-order sums of given floats (colsum, embed backward): n * 2^-24 * sum|x_i| per output element, the worst case of
  ANY summation order of n floats -- derived, not tuned.  axpby: 2^-23 * (|alpha x| + |beta y|) (two roundings, or one
  when the compiler contracts).
* statements of bit-identity the sources make (grouped == per-group calls, _multi_coef == _multi == per bucket, vector
  == scalar embed backward) are asserted as bit-identity.
* kernels with transcendentals are compared with fp64 torch.  Where tests/test_kernels_gpu.py already states a tolerance
  for the same kernel at the same input scale it is reused:
      LSTM without dropout, unit-normal gates   h, c 1e-6; d gates, d c_prev 2e-6   (test_lstm_forward_backward)
      rfn_xe_loss_ex / rfn_multilabel_margin_grouped   loss 1e-5 * max(1, |ref|), gradients 1e-7
                                                                                    (test_criteria_match_torch)
      rfn_rl_loss_ex   loss 1e-5 * max(1, |ref|), d input 1e-6, d logprobs_all 1e-7
                                                                     (test_rl_reward_criterion_matches_oracle)
      rfn_multinomial_pick   2e-6 of the total mass around the fp64 CDF bracket
                                                         (test_multinomial_pick_is_the_inverse_cdf_of_its_uniform)
  The criteria keep that test's B = 6, T = 5, its log_softmax(randn) log-probs and unit-normal predictions, so every term
  and gradient has the scale it has there (gradients <= gscale / B); the device-side gscale_dev = 0.37 only shrinks them.
* a new regime (another V1, dropout scaling, other Adam settings) gets no invented number: the same operation is done in
  plain fp32 torch on the CPU, its max error against the fp64 reference is the YARDSTICK -- the reference's own fp32
  error, not the kernel's --, and the kernel is allowed 4x that (another fixed summation tree; device expf / logf /
  tanhf at 1-2 ulp against libm's < 1).  `python tests/test_glue_kernels_gpu.py` (no GPU) re-measures the table:

  vocabulary log-softmax, 64 rows per V1 (lsm_rows): unit-normal * 3 logits (a row of them holds -inf entries) and
  logits near +-80; backward of given float32 log-probs with unit-normal g.  yardstick (bound = 4x):
      V1      fwd scale 3   fwd +-80    bwd scale 3   bwd +-80
      1       0             0           0             0
      3       4.72e-07      1.46e-05    3.58e-07      2.95e-07
      255     2.05e-06      1.52e-05    2.11e-06      2.96e-07
      256     1.97e-06      1.49e-05    2.17e-06      3.1e-07
      1024    1.99e-06      1.51e-05    5.88e-06      2.54e-07
      1028    2.02e-06      1.48e-05    5.32e-06      2.74e-07
      9489    2.1e-06       1.5e-05     6.8e-06       2.28e-07
      10240   2.4e-06       1.55e-05    6.27e-06      2.32e-07
      10244   2.39e-06      1.5e-05     8.69e-06      2.06e-07

  LSTM with dropout (h is o * tanh(c) / (1 - p)), shapes (7, 48) and (5, 300), maxout 0 and 1, unit-normal inputs:
      p       h             d gates / d c_prev
      0.1     1.64e-07      3.05e-07
      0.5     2.03e-07      3.53e-07

  Adam, one step from unit-normal p, m ~ 0.1 * randn, v ~ (0.1 * randn)^2, g ~ 2 * randn * grad_scale 0.5, lr 5e-4,
  betas (0.9, 0.999), eps 1e-8, 100 000 elements:
      clip   wd     step    p           m           v
      1      0      1       2.18e-07    2.87e-08    1.14e-08
      1      1e-05  1       2.09e-07    3.22e-08    1.41e-08
      1e+09  0      1       2.18e-07    3.73e-08    1.34e-08
      1e+09  1e-05  1       2.09e-07    5.27e-08    1.41e-08
      1      0      1000    2.27e-07    2.87e-08    1.14e-08
      1      1e-05  1000    2.19e-07    3.22e-08    1.41e-08
      1e+09  0      1000    2.27e-07    3.73e-08    1.34e-08
      1e+09  1e-05  1000    2.19e-07    5.27e-08    1.41e-08
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import philox_cpu as PH

pytestmark = pytest.mark.gpu

NAN = float('nan')
INF = float('inf')
U = 2.0 ** -24
STAGE2 = 1 << 20                                   # rfn.h RFN_DROP_OFFSET_STAGE2
HI_SEED, HI_OFFSET = 2 ** 63 + 1, 2 ** 33 + 7
ERR_SHAPE, ERR_ARG = -1, -5

# ---- measured yardsticks (see the docstring; re-measure with `python tests/test_glue_kernels_gpu.py`) ------------------
LSM_V1 = [1, 3, 255, 256, 1024, 1028, 9489, 10240, 10244]
LSM_YARD = {
    # V1: (fwd scale 3, fwd +-80, bwd scale 3, bwd +-80)
    1: (0, 0, 0, 0),
    3: (4.72e-07, 1.46e-05, 3.58e-07, 2.95e-07),
    255: (2.05e-06, 1.52e-05, 2.11e-06, 2.96e-07),
    256: (1.97e-06, 1.49e-05, 2.17e-06, 3.1e-07),
    1024: (1.99e-06, 1.51e-05, 5.88e-06, 2.54e-07),
    1028: (2.02e-06, 1.48e-05, 5.32e-06, 2.74e-07),
    9489: (2.1e-06, 1.5e-05, 6.8e-06, 2.28e-07),
    10240: (2.4e-06, 1.55e-05, 6.27e-06, 2.32e-07),
    10244: (2.39e-06, 1.5e-05, 8.69e-06, 2.06e-07),
}
LSTM_DROP_YARD = {
    # p: (h, d gates / d c_prev)
    0.1: (1.64e-07, 3.05e-07),
    0.5: (2.03e-07, 3.53e-07),
}
ADAM_CASES = [(1.0, 0.0, 1), (1.0, 1e-5, 1), (1e9, 0.0, 1), (1e9, 1e-5, 1),
              (1.0, 0.0, 1000), (1.0, 1e-5, 1000), (1e9, 0.0, 1000), (1e9, 1e-5, 1000)]
ADAM_YARD = {
    # (clip, wd, step): (p, m, v)
    (1, 0, 1): (2.18e-07, 2.87e-08, 1.14e-08),
    (1, 1e-05, 1): (2.09e-07, 3.22e-08, 1.41e-08),
    (1e+09, 0, 1): (2.18e-07, 3.73e-08, 1.34e-08),
    (1e+09, 1e-05, 1): (2.09e-07, 5.27e-08, 1.41e-08),
    (1, 0, 1000): (2.27e-07, 2.87e-08, 1.14e-08),
    (1, 1e-05, 1000): (2.19e-07, 3.22e-08, 1.41e-08),
    (1e+09, 0, 1000): (2.27e-07, 3.73e-08, 1.34e-08),
    (1e+09, 1e-05, 1000): (2.19e-07, 5.27e-08, 1.41e-08),
}


def N():
    import recurrent_fusion_network_amd._native as n
    return n


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def pad2d(t, ld, dev, lead=0):
    """`t` (rows, w) as columns [lead, lead + w) of a NaN-filled (rows, ld) device buffer -> (buffer, view)."""
    buf = torch.full((t.shape[0], ld), NAN, device=dev)
    view = buf[:, lead:lead + t.shape[1]]
    view.copy_(t)
    return buf, view


def nan2d(rows, w, ld, dev, lead=0):
    buf = torch.full((rows, ld), NAN, device=dev)
    return buf, buf[:, lead:lead + w]


def pad_is_nan(buf, lead, w):
    m = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    m[:, lead:lead + w] = False
    return bool(torch.isnan(buf[m]).all())


def within(got, ref, bound):
    """|got - ref| <= bound element-wise (bound a tensor or a number); NaN anywhere fails."""
    d = (got.detach().double().cpu() - ref.detach().double().cpu()).abs()
    return bool((d <= bound).all())


def key_tensor(seed, dev):
    return torch.tensor([seed - 2 ** 64 if seed >= 2 ** 63 else seed], dtype=torch.int64, device=dev)


# =================================================================================================================
# 1. dropout mask == the Philox restatement
# =================================================================================================================
MASK_KEYS = [(0, 0), (0x123456789ABCDEF0, 5), (11, STAGE2 + 3), (HI_SEED, HI_OFFSET)]


@pytest.mark.parametrize('p', [0.0, 0.3, 0.999])
@pytest.mark.parametrize('seed,offset', MASK_KEYS)
def test_dropout_mask_is_the_documented_philox_stream(dev, seed, offset, p):
    n, cnt = N(), 1000
    st = n.stream_ptr()
    want = torch.from_numpy(PH.keep_mask(seed, offset, cnt, p))
    buf = torch.full((cnt + 8,), NAN, device=dev)
    n.check(n.lib.rfn_dropout_mask(seed, offset, cnt, p, buf.data_ptr(), st))
    assert torch.equal(buf[:cnt].cpu(), want) and bool(torch.isnan(buf[cnt:]).all())
    if p == 0.0:
        assert bool((buf[:cnt] == 1.0).all())
    # the key read from device memory: same bits, and the mask follows what is stored there
    key = key_tensor(seed, dev)
    buf2 = torch.full((cnt + 8,), NAN, device=dev)
    n.check(n.lib.rfn_dropout_mask_dev(key.data_ptr(), offset, cnt, p, buf2.data_ptr(), st))
    assert torch.equal(buf2[:cnt].cpu(), want) and bool(torch.isnan(buf2[cnt:]).all())
    other = 0x0FEDCBA987654321
    key.copy_(key_tensor(other, dev))
    n.check(n.lib.rfn_dropout_mask_dev(key.data_ptr(), offset, cnt, p, buf2.data_ptr(), st))
    want2 = torch.from_numpy(PH.keep_mask(other, offset, cnt, p))
    assert torch.equal(buf2[:cnt].cpu(), want2)
    if p == 0.3:
        assert not torch.equal(want, want2)


def test_dropout_mask_argument_errors(dev):
    n = N()
    st = n.stream_ptr()
    buf = torch.full((16,), NAN, device=dev)
    key = key_tensor(11, dev)
    assert n.lib.rfn_dropout_mask(11, 0, 16, 1.0, buf.data_ptr(), st) == ERR_SHAPE
    assert n.lib.rfn_dropout_mask(11, 0, 0, 0.3, buf.data_ptr(), st) == ERR_SHAPE
    assert n.lib.rfn_dropout_mask(11, 0, 16, 0.3, None, st) == ERR_ARG
    assert n.lib.rfn_dropout_mask_dev(key.data_ptr(), 0, 16, 1.0, buf.data_ptr(), st) == ERR_SHAPE
    assert n.lib.rfn_dropout_mask_dev(key.data_ptr(), 0, 0, 0.3, buf.data_ptr(), st) == ERR_SHAPE
    assert n.lib.rfn_dropout_mask_dev(None, 0, 16, 0.3, buf.data_ptr(), st) == ERR_ARG
    assert n.lib.rfn_dropout_mask_dev(key.data_ptr(), 0, 16, 0.3, None, st) == ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())            # nothing was launched


# =================================================================================================================
# 2. LSTM epilogue
# =================================================================================================================
def lstm_inputs(B, R, maxout, seed=0):
    GW = (5 if maxout else 4) * R
    sums, c0 = rnd(B, GW, seed=seed + 1), rnd(B, R, seed=seed + 2)
    if maxout:
        k = min(3, R)
        sums[:, 4 * R:4 * R + k] = sums[:, 3 * R:3 * R + k]      # exact ties: torch.max(a, b) splits their gradient evenly
    return sums, c0, rnd(B, R, seed=seed + 3), rnd(B, R, seed=seed + 4)


def lstm_ref(sums, c0, dh, dcn, R, maxout, keep=None, p=0.0, dtype=torch.float64):
    """The gate math under autograd (dtype = float64: the reference; float32: the yardstick).
    -> h, c, d gates, d c_prev.  keep: (B, R) 0/1 mask, h = o * tanh(c) * keep / (1 - float32(p))."""
    sr, cr = sums.to(dtype).requires_grad_(True), c0.to(dtype).requires_grad_(True)
    sig = torch.sigmoid(sr[:, :3 * R])
    g = torch.max(sr[:, 3 * R:4 * R], sr[:, 4 * R:5 * R]) if maxout else torch.tanh(sr[:, 3 * R:4 * R])
    c1 = sig[:, R:2 * R] * cr + sig[:, :R] * g
    h1 = sig[:, 2 * R:3 * R] * torch.tanh(c1)
    if keep is not None:
        h1 = h1 * keep.to(dtype) * torch.tensor(1.0, dtype=dtype).div(torch.tensor(1.0 - float(np.float32(p)), dtype=dtype))
    loss = (h1 * dh.to(dtype)).sum()
    if dcn is not None:
        loss = loss + (c1 * dcn.to(dtype)).sum()
    loss.backward()
    return h1.detach(), c1.detach(), sr.grad, cr.grad


def run_lstm(n, dev, sums, c0, dh, dcn, R, maxout, p=0.0, seed=0, offset=0, strided=False, alias=False):
    """One rfn_lstm_fwd + rfn_lstm_bwd.  strided: the gates are a column slice of a wider buffer and every other operand
    has its own leading dimension > R; alias: c_next overwrites c_prev and dc_prev overwrites dc_next (rfn_cell.hip).
    -> h, c_next, d gates, d c_prev (device views), after checking every padding column."""
    B, GW = sums.shape
    st = n.stream_ptr()
    k = (lambda i: R + i) if strided else (lambda i: R)
    gbuf, gv = pad2d(sums, GW + 7 if strided else GW, dev, 3 if strided else 0)
    cpbuf, cpv = pad2d(c0, k(1), dev)
    if alias:
        cnbuf, cnv = cpbuf, cpv
    else:
        cnbuf, cnv = nan2d(B, R, k(2), dev)
    hbuf, hv = nan2d(B, R, k(3), dev)
    n.check(n.lib.rfn_lstm_fwd(gv.data_ptr(), gbuf.shape[1], cpv.data_ptr(), cpbuf.shape[1], cnv.data_ptr(), cnbuf.shape[1],
                               hv.data_ptr(), hbuf.shape[1], B, R, maxout, p, seed, offset, st))
    h, c1 = hv.clone(), cnv.clone()
    assert pad_is_nan(gbuf, 3 if strided else 0, GW) and pad_is_nan(cpbuf, 0, R) and pad_is_nan(cnbuf, 0, R)
    assert pad_is_nan(hbuf, 0, R)
    if alias:                                    # the backward still needs c_prev: a fresh copy, as the path keeps per step
        cpbuf, cpv = pad2d(c0, k(1), dev)
    dhbuf, dhv = pad2d(dh, k(4), dev)
    dcnbuf, dcnv = pad2d(dcn, k(5), dev) if dcn is not None else (None, None)
    if alias and dcn is not None:
        dcpbuf, dcpv = dcnbuf, dcnv
    else:
        dcpbuf, dcpv = nan2d(B, R, k(6), dev)
    n.check(n.lib.rfn_lstm_bwd(gv.data_ptr(), gbuf.shape[1], cpv.data_ptr(), cpbuf.shape[1], cnv.data_ptr(), cnbuf.shape[1],
                               dhv.data_ptr(), dhbuf.shape[1], n.ptr(dcnv), dcnbuf.shape[1] if dcn is not None else R,
                               dcpv.data_ptr(), dcpbuf.shape[1], B, R, maxout, p, seed, offset, st))
    assert pad_is_nan(gbuf, 3 if strided else 0, GW) and pad_is_nan(dcpbuf, 0, R) and pad_is_nan(dhbuf, 0, R)
    assert torch.equal(cnv, c1) and torch.equal(dhv.cpu(), dh)            # read-only operands
    return h, c1, gv, dcpv


LSTM_SHAPES = [(1, 1), (3, 5), (7, 48), (5, 300)]          # (5, 300): more than one 256-thread block, ragged tail


@pytest.mark.parametrize('variant', ['packed', 'strided', 'aliased', 'strided_aliased', 'no_dc_next'])
@pytest.mark.parametrize('maxout', [0, 1])
@pytest.mark.parametrize('B,R', LSTM_SHAPES)
def test_lstm_epilogue_layouts_match_fp64(dev, B, R, maxout, variant):
    n = N()
    sums, c0, dh, dcn = lstm_inputs(B, R, maxout)
    if variant == 'no_dc_next':
        dcn = None
    h64, c64, dg64, dcp64 = lstm_ref(sums, c0, dh, dcn, R, maxout)
    h, c1, dg, dcp = run_lstm(n, dev, sums, c0, dh, dcn, R, maxout, strided='strided' in variant, alias='aliased' in variant)
    assert maxerr(h, h64) < 1e-6 and maxerr(c1, c64) < 1e-6
    assert maxerr(dg, dg64) < 2e-6 and maxerr(dcp, dcp64) < 2e-6
    if maxout:                                               # the tie columns really were ties
        k = min(3, R)
        assert torch.equal(dg[:, 3 * R:3 * R + k], dg[:, 4 * R:4 * R + k])


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('maxout', [0, 1])
@pytest.mark.parametrize('B,R', [(7, 48), (5, 300)])
def test_lstm_dropout_applies_the_restated_mask_forward_and_backward(dev, B, R, maxout, p):
    n = N()
    sums, c0, dh, dcn = lstm_inputs(B, R, maxout)
    keep = torch.from_numpy(PH.keep_mask(HI_SEED, HI_OFFSET, B * R, p)).view(B, R)
    assert 0 < int(keep.sum()) < B * R
    h64, c64, dg64, dcp64 = lstm_ref(sums, c0, dh, dcn, R, maxout, keep, p)
    h, c1, dg, dcp = run_lstm(n, dev, sums, c0, dh, dcn, R, maxout, p, HI_SEED, HI_OFFSET, strided=True)
    yh, yb = LSTM_DROP_YARD[p]
    assert bool((h.cpu()[keep == 0] == 0).all()) and bool((h.cpu()[keep == 1] != 0).all())
    print('lstm dropout p=%g: h err %.3g (bound %.3g), bwd err %.3g (bound %.3g)'
          % (p, maxerr(h, h64), 4 * yh, max(maxerr(dg, dg64), maxerr(dcp, dcp64)), 4 * yb))
    assert maxerr(h, h64) <= 4 * yh
    assert maxerr(c1, c64) < 1e-6                           # c is never dropped
    h0, c0n, _, _ = run_lstm(n, dev, sums, c0, dh, dcn, R, maxout, 0.0, strided=True)
    assert torch.equal(c1, c0n)                             # ... not by a bit
    assert maxerr(dg, dg64) <= 4 * yb and maxerr(dcp, dcp64) <= 4 * yb


@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('layout', ['slabs', 'interleaved'])
@pytest.mark.parametrize('maxout', [0, 1])
@pytest.mark.parametrize('G', [1, 3])
def test_lstm_grouped_calls_equal_single_calls_with_offset_plus_g(dev, G, maxout, layout, p):
    """rfn_lstm_fwd_grouped / rfn_lstm_bwd_grouped: group g is the single call on its slice with dropout stream offset + g.
    slabs: (G, B, .) back to back; interleaved: column slices of (B, G * .) -- the concatenated-state layout (gs = R)."""
    n = N()
    st = n.stream_ptr()
    B, R = 5, 70                                            # 350 units: two blocks per group
    GW = (5 if maxout else 4) * R
    seed, offset = HI_SEED, HI_OFFSET
    ins = [lstm_inputs(B, R, maxout, seed=10 * g) for g in range(G)]

    def pack(parts, w):
        """-> (buffer, [view per group], ld, group stride in floats)"""
        if layout == 'slabs':
            buf = torch.full((G, B, w), NAN, device=dev)
            views = [buf[g] for g in range(G)]
            ld, gs = w, B * w
        else:
            buf = torch.full((B, G * w), NAN, device=dev)
            views = [buf[:, g * w:(g + 1) * w] for g in range(G)]
            ld, gs = G * w, w
        for v, t in zip(views, parts):
            if t is not None:
                v.copy_(t)
        return buf, views, ld, gs

    def state():
        return (pack([i[0] for i in ins], GW), pack([i[1] for i in ins], R), pack([None] * G, R), pack([None] * G, R),
                pack([i[2] for i in ins], R), pack([i[3] for i in ins], R), pack([None] * G, R))
    # grouped
    (gb, gv, ldg, gsg), (cpb, cpv, ldc, gsc), (cnb, cnv, _, _), (hb, hv, ldh, gsh), (dhb, dhv, lddh, gsdh), \
        (dcnb, dcnv, lddc, gsdc), (dcpb, dcpv, _, _) = state()
    n.check(n.lib.rfn_lstm_fwd_grouped(gb.data_ptr(), ldg, cpb.data_ptr(), ldc, cnb.data_ptr(), ldc, hb.data_ptr(), ldh, B, R,
                                       maxout, p, seed, offset, G, gsg, gsc, gsc, gsh, st))
    act = gb.clone()
    n.check(n.lib.rfn_lstm_bwd_grouped(gb.data_ptr(), ldg, cpb.data_ptr(), ldc, cnb.data_ptr(), ldc, dhb.data_ptr(), lddh,
                                       dcnb.data_ptr(), lddc, dcpb.data_ptr(), lddc, B, R, maxout, p, seed, offset, G, gsg, gsc,
                                       gsdh, gsdc, st))
    # per-group single calls on the same layout
    (gb2, gv2, _, _), (cpb2, cpv2, _, _), (cnb2, cnv2, _, _), (hb2, hv2, _, _), (dhb2, dhv2, _, _), (dcnb2, dcnv2, _, _), \
        (dcpb2, dcpv2, _, _) = state()
    for g in range(G):
        n.check(n.lib.rfn_lstm_fwd(gv2[g].data_ptr(), ldg, cpv2[g].data_ptr(), ldc, cnv2[g].data_ptr(), ldc, hv2[g].data_ptr(),
                                   ldh, B, R, maxout, p, seed, offset + g, st))
    act2 = gb2.clone()
    for g in range(G):
        n.check(n.lib.rfn_lstm_bwd(gv2[g].data_ptr(), ldg, cpv2[g].data_ptr(), ldc, cnv2[g].data_ptr(), ldc, dhv2[g].data_ptr(),
                                   lddh, dcnv2[g].data_ptr(), lddc, dcpv2[g].data_ptr(), lddc, B, R, maxout, p, seed,
                                   offset + g, st))
    for a, b in ((act, act2), (cnb, cnb2), (hb, hb2), (gb, gb2), (dcpb, dcpb2)):
        assert not bool(torch.isnan(a).any()) and torch.equal(a, b)
    # and they are right: group g against fp64 through the mask of offset + g
    for g in range(G):
        keep = torch.from_numpy(PH.keep_mask(seed, offset + g, B * R, p)).view(B, R) if p > 0 else None
        h64, c64, dg64, dcp64 = lstm_ref(*ins[g], R, maxout, keep, p)
        assert maxerr(cnv[g], c64) < 1e-6
        if p > 0:
            yh, yb = LSTM_DROP_YARD[p]
            assert maxerr(hv[g], h64) <= 4 * yh and maxerr(gv[g], dg64) <= 4 * yb and maxerr(dcpv[g], dcp64) <= 4 * yb
        else:
            assert maxerr(hv[g], h64) < 1e-6 and maxerr(gv[g], dg64) < 2e-6 and maxerr(dcpv[g], dcp64) < 2e-6
        if p > 0:
            assert torch.equal((hv[g] == 0).cpu(), keep == 0)
            if g > 0:
                assert not torch.equal(keep, torch.from_numpy(PH.keep_mask(seed, offset, B * R, p)).view(B, R))
                assert not torch.equal((hv[g] == 0).cpu(), (hv[0] == 0).cpu())


# =================================================================================================================
# 3. column sums and small fills
# =================================================================================================================
@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('rows,cols', [(0, 5), (1, 1), (63, 17), (259, 16), (130, 8195)])   # 8195: the 64-column template
def test_colsum_shapes(dev, rows, cols, accumulate):
    n = N()
    X = rnd(max(rows, 1), cols, seed=rows + cols)
    xbuf, xv = pad2d(X, cols + 3, dev)
    out = torch.full((cols + 4,), NAN, device=dev)
    prior = rnd(cols, seed=5)
    if accumulate:
        out[:cols] = prior.to(dev)
    n.check(n.lib.rfn_colsum_f32(xv.data_ptr(), cols + 3, rows, cols, out.data_ptr(), accumulate, n.stream_ptr()))
    assert bool(torch.isnan(out[cols:]).all())
    Xr = X[:rows].double()
    ref = Xr.sum(0) + (prior.double() if accumulate else 0.0)
    mag = Xr.abs().sum(0) + (prior.double().abs() if accumulate else 0.0)
    assert within(out[:cols], ref, (rows + accumulate) * U * mag)
    if rows == 0:
        assert torch.equal(out[:cols].cpu(), prior if accumulate else torch.zeros(cols))


@pytest.mark.parametrize('cols', [1, 64, 65, 130])
@pytest.mark.parametrize('ngroups', [1, 3, 65])              # 65: the second launch
def test_colsum_grouped(dev, ngroups, cols):
    n = N()
    st = n.stream_ptr()
    for rows in (0, 1, 15, 16, 17, 100):
        ldx = cols + 3
        gstride = max(rows, 1) * ldx + 5
        flat = torch.full((ngroups * gstride,), NAN, device=dev)
        X = rnd(ngroups, max(rows, 1), cols, seed=rows + 7 * cols)
        for g in range(ngroups):
            flat[g * gstride:g * gstride + max(rows, 1) * ldx].view(max(rows, 1), ldx)[:, :cols].copy_(X[g])
        Xr = X[:, :rows].double()
        ref, bound = Xr.sum(1), rows * U * Xr.abs().sum(1)
        for mode in ('none', 'full', 'some'):
            o1 = torch.full((ngroups, cols + 2), NAN, device=dev)
            o2 = torch.full((ngroups, cols + 2), NAN, device=dev)
            has2 = [mode == 'full' or (mode == 'some' and g % 2 == 0) for g in range(ngroups)]
            p1 = n.ptr_array([o1[g] for g in range(ngroups)])
            p2 = n.ptr_array([o2[g] if has2[g] else None for g in range(ngroups)])
            if mode == 'none':
                n.check(n.lib.rfn_colsum_grouped_f32(flat.data_ptr(), gstride, ldx, rows, cols, p1, ngroups, st))
            else:
                n.check(n.lib.rfn_colsum_grouped2_f32(flat.data_ptr(), gstride, ldx, rows, cols, p1, p2, ngroups, st))
            assert within(o1[:, :cols], ref, bound), (rows, mode)
            assert bool(torch.isnan(o1[:, cols:]).all()) and bool(torch.isnan(o2[:, cols:]).all())
            for g in range(ngroups):
                if has2[g]:
                    assert torch.equal(o2[g, :cols], o1[g, :cols])
                else:
                    assert bool(torch.isnan(o2[g]).all())
    o1 = torch.full((ngroups, cols), NAN, device=dev)
    ptrs = n.ptr_array([o1[g] if g != ngroups - 1 else None for g in range(ngroups)])
    assert n.lib.rfn_colsum_grouped_f32(flat.data_ptr(), gstride, ldx, rows, cols, ptrs, ngroups, st) == ERR_ARG
    assert n.lib.rfn_colsum_grouped2_f32(flat.data_ptr(), gstride, ldx, rows, cols, ptrs, None, ngroups, st) == ERR_ARG


@pytest.mark.parametrize('ngroups', [1, 64, 65, 130])
def test_fill_and_copy_small(dev, ngroups):
    n = N()
    st = n.stream_ptr()
    for cnt in (1, 63, 64, 65, 200):
        dst = torch.full((ngroups, cnt + 3), NAN, device=dev)
        n.check(n.lib.rfn_fill_small_f32(n.ptr_array([dst[g] for g in range(ngroups)]), ngroups, cnt, 1.25, st))
        assert bool((dst[:, :cnt] == 1.25).all()) and bool(torch.isnan(dst[:, cnt:]).all())
        src = rnd(ngroups, cnt + 1, seed=cnt).to(dev)
        dst = torch.full((ngroups, cnt + 3), NAN, device=dev)
        n.check(n.lib.rfn_copy_small_f32(n.ptr_array([dst[g] for g in range(ngroups)]),
                                         n.ptr_array([src[g] for g in range(ngroups)]), ngroups, cnt, st))
        assert torch.equal(dst[:, :cnt], src[:, :cnt]) and bool(torch.isnan(dst[:, cnt:]).all())
    one = torch.zeros(4, device=dev)
    assert n.lib.rfn_fill_small_f32(n.ptr_array([one, None]), 2, 4, 0.0, st) == ERR_ARG
    assert n.lib.rfn_copy_small_f32(n.ptr_array([one, one]), n.ptr_array([one, None]), 2, 4, st) == ERR_ARG


# =================================================================================================================
# 4. embedding
# =================================================================================================================
@pytest.mark.parametrize('layout', ['step_batch', 'rows'])
@pytest.mark.parametrize('E', [1, 127, 128, 129, 512])
def test_embed_forward(dev, E, layout):
    n = N()
    V1, B, S = 23, 5, 4
    W = rnd(V1, E, seed=E)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, V1, (B, S + 2), generator=g)
    ids[1, 1], ids[2, 3] = -1, V1                           # out of range: read row 0 (the kernel never faults)
    rows = S * B
    obuf, ov = nan2d(rows, E, E + 3, dev)
    Wd, idd = W.to(dev), ids.to(dev)
    if layout == 'step_batch':                              # row r = (step, batch) reads ids[batch, step]
        by_row = ids[:, :S].t().reshape(-1)
        n.check(n.lib.rfn_embed_fwd(Wd.data_ptr(), E, V1, idd.data_ptr(), B, S + 2, 1, rows, ov.data_ptr(), E + 3, n.stream_ptr()))
    else:
        by_row = ids.reshape(-1)[:rows]
        n.check(n.lib.rfn_embed_fwd(Wd.data_ptr(), E, V1, idd.data_ptr(), rows, 1, 0, rows, ov.data_ptr(), E + 3, n.stream_ptr()))
    safe = torch.where((by_row < 0) | (by_row >= V1), torch.zeros_like(by_row), by_row)
    assert int((safe != by_row).sum()) >= 1
    assert torch.equal(ov.cpu(), W[safe]) and pad_is_nan(obuf, 0, E)


EMB_V1 = 40
# E, ldo - E, rows, inner, hot   (rows % inner == 0: memory-order scan with mod = rows / inner, else row order)
EMB_BWD = [
    (20, 0, 20, 5, 0),        # vector path, memory order, mod 4
    (516, 0, 20, 7, 0),       # vector path, two e0 chunks, row order
    (3, 0, 300, 75, 0),       # scalar path (E % 4), mod 4, two scan rounds
    (130, 0, 300, 7, 0),      # scalar path, two e0 chunks, row order
    (20, 1, 320, 5, 0),       # scalar path by ldo % 4, mod 64
    (20, 4, 1100, 7, 700),    # hot token: mid-scan drains, five scan rounds, row order
    (516, 0, 1120, 16, 700),  # hot token, two chunks, mod 70
    (3, 0, 1120, 16, 700),    # hot token on the scalar path
    (20, 0, 0, 5, 0),         # no rows: all of dW is zero
]


def emb_ids(rows, inner, hot, seed):
    """ids per logical row: token 0 `hot` times, token 1 exactly 8 times and token 2 exactly 9 times (the drain depth
    edge), tokens 3 and >= EMB_V1 - 3 never; placed as row r -> ids2d[r % inner, r // inner] (ld = outer + 2)."""
    g = torch.Generator().manual_seed(seed)
    fixed = [0] * hot + ([1] * 8 + [2] * 9 if rows >= 17 + hot else [])
    rest = torch.randint(4, EMB_V1 - 3, (rows - len(fixed),), generator=g).tolist()
    by_row = torch.tensor(fixed + rest, dtype=torch.long)[torch.randperm(rows, generator=g)] if rows else torch.zeros(0, dtype=torch.long)
    outer = (rows + inner - 1) // inner
    ids2d = torch.full((inner, outer + 2), 3, dtype=torch.long)          # unread slots name the never-used token 3
    for r in range(rows):
        ids2d[r % inner, r // inner] = by_row[r]
    return by_row, ids2d


@pytest.mark.parametrize('E,ldx,rows,inner,hot', EMB_BWD)
def test_embed_backward_paths(dev, E, ldx, rows, inner, hot):
    n = N()
    st = n.stream_ptr()
    V1, ldo = EMB_V1, E + ldx
    by_row, ids2d = emb_ids(rows, inner, hot, seed=rows + E)
    idd = ids2d.to(dev)
    dout = rnd(max(rows, 1), E, seed=E + 1)

    def run(misalign):
        flat = torch.full((max(rows, 1) * ldo + 8,), NAN, device=dev)
        v = flat[misalign:misalign + max(rows, 1) * ldo].view(max(rows, 1), ldo)[:, :E]
        v.copy_(dout)
        dW = torch.full((V1 * E + 4,), NAN, device=dev)
        n.check(n.lib.rfn_embed_bwd(v.data_ptr(), ldo, idd.data_ptr(), inner, ids2d.shape[1], 1, rows, E, V1, dW.data_ptr(), st))
        assert bool(torch.isnan(dW[V1 * E:]).all())
        return dW[:V1 * E].view(V1, E)
    dW = run(0)
    d64 = dout[:rows].double()
    ref = torch.zeros(V1, E, dtype=torch.float64).index_add_(0, by_row, d64)
    mag = torch.zeros(V1, E, dtype=torch.float64).index_add_(0, by_row, d64.abs())
    cnt = torch.bincount(by_row, minlength=V1).double()
    if rows >= 17 + hot:
        assert int(cnt[1]) == 8 and int(cnt[2]) == 9 and int(cnt[0]) == hot
    assert int(cnt[3]) == 0 and int(cnt[V1 - 1]) == 0
    assert within(dW, ref, cnt[:, None] * U * mag)
    assert bool((dW.cpu()[cnt == 0] == 0).all())             # tokens without a match: exact zero rows
    assert torch.equal(run(0), dW)                           # deterministic
    if E % 4 == 0 and ldo % 4 == 0:                          # the scalar template adds in the same queue order
        assert torch.equal(run(1), dW)


# =================================================================================================================
# 5. vocabulary log-softmax
# =================================================================================================================
def lsm_rows(V1, seed, rows=4):
    """rows - 2 rows of 3 * randn, one more with -inf entries, and a last row of logits near +-80."""
    x = rnd(rows, V1, seed=seed, scale=3.0)
    if V1 >= 3:
        x[rows - 2, 1] = x[rows - 2, V1 - 1] = -INF
    x[rows - 1] = torch.where(rnd(V1, seed=seed + 1) > 0, 80.0, -80.0) + rnd(V1, seed=seed + 2)
    return x, rnd(rows, V1, seed=seed + 3)


def lsm_bwd_ref(lp, g, dtype):
    """rfn.h: d logits = g - exp(logp) * sum_v g, a function of the GIVEN log-probs (float32 values, taken as exact)."""
    lp, g = lp.to(dtype), g.to(dtype)
    return g - torch.exp(lp) * g.sum(1, keepdim=True)


@pytest.mark.parametrize('variant', ['aligned', 'ld_plus_1', 'offset_1'])
@pytest.mark.parametrize('mapping', ['rows', 'transposed'])
@pytest.mark.parametrize('V1', LSM_V1)
def test_log_softmax_forward_backward_paths(dev, V1, mapping, variant):
    """Register path (V1 % 4 == 0, <= 10240, aligned): a partly filled slot at 1028, exact capacity at 10240; everything
    else, `ld_plus_1` (ldl = ldd = V1 + 1) and `offset_1` (outputs one float off 16 bytes) take the three-pass scalar form."""
    n = N()
    st = n.stream_ptr()
    Bq, S = 2, 2
    rows = Bq * S
    x, g = lsm_rows(V1, seed=V1)
    lp64 = torch.log_softmax(x.double(), 1)
    ld = V1 + 1 if variant == 'ld_plus_1' else V1
    off = 1 if variant == 'offset_1' else 0
    xbuf, xv = pad2d(x, ld, dev)
    flat = torch.full((rows * V1 + 8,), NAN, device=dev)
    out = flat[off:off + rows * V1]
    if mapping == 'rows':
        inner, s_in, s_out = rows, V1, 0
        perm = torch.arange(rows)
    else:                                                   # row r = (s, b) -> out[b, s, :]
        inner, s_in, s_out = Bq, S * V1, V1
        perm = torch.tensor([(r % Bq) * S + r // Bq for r in range(rows)])
    n.check(n.lib.rfn_log_softmax_fwd(xv.data_ptr(), ld, rows, V1, inner, s_in, s_out, out.data_ptr(), st))
    assert pad_is_nan(xbuf, 0, V1) and bool(torch.isnan(flat[:off]).all()) and bool(torch.isnan(flat[off + rows * V1:]).all())
    lp = out.view(rows, V1).cpu()[perm]                     # back to logits-row order
    yf3, yf80, yb3, yb80 = LSM_YARD[V1]
    neg = torch.isinf(x)
    assert torch.equal(torch.isinf(lp) & (lp < 0), neg) and bool(torch.isfinite(lp[~neg]).all())
    e = (lp.double() - lp64).abs().masked_fill(neg, 0.0)
    print('log_softmax V1=%d: fwd err %.3g / %.3g (bounds %.3g / %.3g)' % (V1, float(e[:-1].max()), float(e[-1].max()), 4 * yf3, 4 * yf80))
    assert float(e[:-1].max()) <= 4 * yf3 and float(e[-1].max()) <= 4 * yf80
    # backward from the kernel's own log-probs, g in the same (mapped) layout
    gflat = torch.full((rows * V1 + 8,), NAN, device=dev)
    gout = gflat[off:off + rows * V1]
    gout.view(rows, V1)[perm] = g.to(dev)
    dbuf, dv = nan2d(rows, V1, ld, dev)
    n.check(n.lib.rfn_log_softmax_bwd(gout.data_ptr(), out.data_ptr(), rows, V1, inner, s_in, s_out, dv.data_ptr(), ld, st))
    assert pad_is_nan(dbuf, 0, V1)
    eb = (dv.double().cpu() - lsm_bwd_ref(lp, g, torch.float64)).abs()
    print('log_softmax V1=%d: bwd err %.3g / %.3g (bounds %.3g / %.3g)' % (V1, float(eb[:-1].max()), float(eb[-1].max()), 4 * yb3, 4 * yb80))
    assert float(eb[:-1].max()) <= 4 * yb3 and float(eb[-1].max()) <= 4 * yb80


@pytest.mark.parametrize('V1', [3, 1028, 10244])
def test_log_softmax_topk_lists_the_best_of_the_forward_bits(dev, V1):
    n = N()
    st = n.stream_ptr()
    W, rows = 5, 4
    x, _ = lsm_rows(V1, seed=V1)
    x = x[:3].contiguous()                                  # scale-3 rows, the last with -inf entries
    rows = 3
    if V1 >= 1028:
        x[0, 900] = x[0, 17] = x[0].max() + 1.0             # tied best: the lower token first
        x[1, 1027] = x[1, 1026]
    else:
        x[0, 2] = x[0, 0]
    xd = x.to(dev)
    lp = torch.full((rows, V1), NAN, device=dev)
    n.check(n.lib.rfn_log_softmax_fwd(xd.data_ptr(), V1, rows, V1, rows, V1, 0, lp.data_ptr(), st))
    topv = torch.full((rows, W), NAN, device=dev)
    topi = torch.full((rows, W), -7, dtype=torch.int32, device=dev)
    n.check(n.lib.rfn_log_softmax_topk(xd.data_ptr(), V1, rows, V1, W, topv.data_ptr(), topi.data_ptr(), st))
    cols = min(W, V1)
    lpc, tv, ti = lp.cpu(), topv.cpu(), topi.cpu().long()
    assert bool(torch.isnan(tv[:, cols:]).all()) and bool((ti[:, cols:] == -7).all())
    lp64 = torch.log_softmax(x.double(), 1)
    for r in range(rows):
        order = sorted(range(V1), key=lambda v: (-float(lpc[r, v]), v))[:cols]     # value descending, token ascending
        assert ti[r, :cols].tolist() == order
        assert torch.equal(tv[r, :cols], lpc[r, order])                            # the bits the forward writes
        # ... which are the best of the fp64 log-probs, to the forward's tolerance
        best64 = torch.sort(lp64[r], descending=True).values[:cols]
        fin = torch.isfinite(best64)
        assert torch.equal(torch.isfinite(tv[r, :cols]), fin)
        assert float((tv[r, :cols].double()[fin] - best64[fin]).abs().max()) <= 4 * LSM_YARD[V1][0]
    if V1 >= 1028:
        assert ti[0, :2].tolist() == [17, 900]


# =================================================================================================================
# 6. max over steps, axpby, div, state mean, gather
# =================================================================================================================
@pytest.mark.parametrize('B,K', [(5, 51), (4, 64), (1, 257)])
@pytest.mark.parametrize('T', [1, 6])
@pytest.mark.parametrize('G', [1, 3])
def test_max_over_steps_grouped(dev, G, T, B, K):
    n = N()
    st = n.stream_ptr()
    X = rnd(G, T, B, K, seed=T + K)
    if T > 1:
        X[:, 3, :, ::5] = X[:, 1, :, ::5] = X.max() + 1.0    # ties: the first step attaining the maximum
    Xd = X.to(dev)
    out = torch.full((G * B * K + 4,), NAN, device=dev)
    arg = torch.full((G * B * K + 4,), -7, dtype=torch.int32, device=dev)
    n.check(n.lib.rfn_max_over_steps_fwd_grouped(Xd.data_ptr(), T, B, K, out.data_ptr(), arg.data_ptr(), G, st))
    mref = X.max(1).values
    aref = (X == mref.unsqueeze(1)).float().argmax(1)       # first maximum
    assert torch.equal(out[:G * B * K].view(G, B, K).cpu(), mref) and bool(torch.isnan(out[G * B * K:]).all())
    assert torch.equal(arg[:G * B * K].view(G, B, K).cpu().long(), aref) and bool((arg[G * B * K:] == -7).all())
    if T > 1:
        assert int(aref[0, 0, 0]) == 1
    out2 = torch.full((G, B, K), NAN, device=dev)
    n.check(n.lib.rfn_max_over_steps_fwd_grouped(Xd.data_ptr(), T, B, K, out2.data_ptr(), None, G, st))     # arg = NULL
    assert torch.equal(out2.cpu(), mref)
    dout = rnd(G, B, K, seed=9).to(dev)
    dX = torch.full((G * T * B * K + 4,), NAN, device=dev)
    n.check(n.lib.rfn_max_over_steps_bwd_grouped(dout.data_ptr(), arg.data_ptr(), T, B, K, dX.data_ptr(), G, st))
    ref = torch.zeros(G, T, B, K).scatter_(1, aref.unsqueeze(1), dout.cpu().unsqueeze(1))
    assert torch.equal(dX[:G * T * B * K].view(G, T, B, K).cpu(), ref) and bool(torch.isnan(dX[G * T * B * K:]).all())
    dX0 = torch.full((G, T, B, K), NAN, device=dev)
    n.check(n.lib.rfn_max_over_steps_bwd_grouped(None, arg.data_ptr(), T, B, K, dX0.data_ptr(), G, st))      # dout = NULL
    assert bool((dX0 == 0).all())
    # the G single calls
    o1 = torch.full((G, B, K), NAN, device=dev)
    a1 = torch.full((G, B, K), -7, dtype=torch.int32, device=dev)
    d1 = torch.full((G, T, B, K), NAN, device=dev)
    for g in range(G):
        n.check(n.lib.rfn_max_over_steps_fwd(Xd[g].data_ptr(), T, B, K, o1[g].data_ptr(), a1[g].data_ptr(), st))
        n.check(n.lib.rfn_max_over_steps_bwd(dout[g].data_ptr(), a1[g].data_ptr(), T, B, K, d1[g].data_ptr(), st))
    assert torch.equal(o1.view(-1), out[:G * B * K]) and torch.equal(a1.view(-1), arg[:G * B * K])
    assert torch.equal(d1.view(-1), dX[:G * T * B * K])


@pytest.mark.parametrize('rows,cols', [(5, 51), (1, 257)])    # 255 and 257 elements around one block
def test_axpby_div_and_state_mean(dev, rows, cols):
    n = N()
    st = n.stream_ptr()
    x, y = rnd(rows, cols, seed=1), rnd(rows, cols, seed=2)
    alpha, beta = 1.7, -0.3
    a32, b32 = float(np.float32(alpha)), float(np.float32(beta))
    xbuf, xv = pad2d(x, cols + 1, dev)
    ybuf, yv = pad2d(y, cols + 2, dev)
    n.check(n.lib.rfn_axpby_2d(alpha, xv.data_ptr(), cols + 1, beta, yv.data_ptr(), cols + 2, rows, cols, st))
    ref = a32 * x.double() + b32 * y.double()
    assert within(yv, ref, 2 * U * ((a32 * x.double()).abs() + (b32 * y.double()).abs())) and pad_is_nan(ybuf, 0, cols)
    ybuf, yv = pad2d(y, cols + 2, dev)
    n.check(n.lib.rfn_axpby_2d(alpha, None, 0, beta, yv.data_ptr(), cols + 2, rows, cols, st))               # x = NULL
    assert within(yv, b32 * y.double(), 2 * U * (b32 * y.double()).abs()) and pad_is_nan(ybuf, 0, cols)
    ybuf, yv = nan2d(rows, cols, cols + 2, dev)
    n.check(n.lib.rfn_axpby_2d(alpha, xv.data_ptr(), cols + 1, 0.0, yv.data_ptr(), cols + 2, rows, cols, st))  # beta = 0 over NaN
    assert within(yv, a32 * x.double(), 2 * U * (a32 * x.double()).abs()) and pad_is_nan(ybuf, 0, cols)
    # IEEE division, compared with the CPU's
    ybuf, yv = pad2d(y, cols + 2, dev)
    n.check(n.lib.rfn_div_2d(yv.data_ptr(), cols + 2, rows, cols, 3.0, st))
    assert torch.equal(yv.cpu(), y / 3.0) and pad_is_nan(ybuf, 0, cols)
    assert n.lib.rfn_div_2d(yv.data_ptr(), cols + 2, rows, cols, 0.0, st) == ERR_SHAPE
    # state mean: sum in slice order, then divide
    for G in (1, 3):
        for npairs in (1, 2):
            srcs = [rnd(rows, G * cols, seed=20 + k) for k in range(npairs)]
            sb = [pad2d(s_, G * cols + 1, dev) for s_ in srcs]
            ob = [nan2d(rows, cols, cols + 1, dev) for _ in range(npairs)]
            n.check(n.lib.rfn_mean_over_groups(npairs, n.ptr_array([b[1] for b in sb]), G * cols + 1, cols, G,
                                               n.ptr_array([b[1] for b in ob]), cols + 1, rows, cols, st))
            for s_, (buf, v) in zip(srcs, ob):
                acc = s_[:, :cols].clone()
                for i in range(1, G):
                    acc = acc + s_[:, i * cols:(i + 1) * cols]
                assert torch.equal(v.cpu(), acc / float(G)) and pad_is_nan(buf, 0, cols)


@pytest.mark.parametrize('R', [1, 33, 512])
@pytest.mark.parametrize('rows', [1, 37])
def test_gather_rows(dev, rows, R):
    n = N()
    src = rnd(9, R, seed=R)
    order = torch.randint(0, 9, (rows,), generator=torch.Generator().manual_seed(rows), dtype=torch.int32)
    if rows > 2:
        order[2] = order[0]                                 # a repeated source row
    dst = torch.full((rows * R + 4,), NAN, device=dev)
    sd, od = src.to(dev), order.to(dev)
    n.check(n.lib.rfn_gather_rows(sd.data_ptr(), dst.data_ptr(), od.data_ptr(), rows, R, n.stream_ptr()))
    assert torch.equal(dst[:rows * R].view(rows, R).cpu(), src[order.long()]) and bool(torch.isnan(dst[rows * R:]).all())
    assert n.lib.rfn_gather_rows(sd.data_ptr(), sd.data_ptr(), od.data_ptr(), rows, R, n.stream_ptr()) == ERR_ARG


# =================================================================================================================
# 7. criteria
# =================================================================================================================
GS = float(np.float32(0.37))                                # the device-side upstream gradient


@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('V1', [50, 301])
def test_xe_loss_ex(dev, V1, eps):
    n = N()
    st = n.stream_ptr()
    B, T = 6, 5
    lp = torch.log_softmax(rnd(B, T, V1, seed=1), 2)
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(0, V1, (B, T + 2), generator=g)
    labels[0, 2], labels[3, 1] = -3, V1                     # out of range: treated as token 0
    mask = (torch.rand(B, T + 2, generator=g) > 0.3).float()
    target, mk = labels[:, 1:], mask[:, 1:]                 # strided views (ld = T + 2), as the trainer passes them
    tsafe = torch.where((target < 0) | (target >= V1), torch.zeros_like(target), target)[:, :T]
    lpr = lp.double().requires_grad_(True)
    oh = torch.zeros(B, T, V1, dtype=torch.float64).scatter_(2, tsafe.unsqueeze(2), 1.0)
    q = oh * (1 - float(np.float32(eps))) + float(np.float32(eps)) / V1 if eps > 0 else oh
    ref = (-(lpr * q).sum(2) * mk[:, :T].double()).sum() / B
    ref.backward()
    rloss, rgrad = float(ref.detach()), lpr.grad * GS
    lpd, td, md = lp.to(dev), labels.to(dev)[:, 1:], mask.to(dev)[:, 1:]
    gdev = torch.tensor([0.37], device=dev)
    scratch = torch.full((B * T,), NAN, device=dev)

    def call(loss_out, acc, dlogp):
        n.check(n.lib.rfn_xe_loss_ex(lpd.data_ptr(), B, T, V1, td.data_ptr(), T + 2, md.data_ptr(), T + 2, eps,
                                     1.0, gdev.data_ptr(), scratch.data_ptr(), n.ptr(loss_out), acc,
                                     n.ptr(dlogp), st))
    loss = torch.tensor([1.5, NAN], device=dev)
    d = torch.full((B * T * V1 + 4,), NAN, device=dev)
    call(loss, 1, d)                                        # both outputs, the loss accumulated onto 1.5
    assert abs(float(loss[0]) - (1.5 + rloss)) < 1e-5 * max(1.0, abs(1.5 + rloss)) and bool(torch.isnan(loss[1]))
    assert maxerr(d[:B * T * V1].view(B, T, V1), rgrad) < 1e-7 and bool(torch.isnan(d[B * T * V1:]).all())
    loss2 = torch.tensor([NAN, NAN], device=dev)
    call(loss2, 0, None)                                    # the loss alone, overwriting
    assert abs(float(loss2[0]) - rloss) < 1e-5 * max(1.0, abs(rloss)) and bool(torch.isnan(loss2[1]))
    d2 = torch.full((B * T * V1 + 4,), NAN, device=dev)
    call(None, 0, d2)                                       # the gradient alone
    assert torch.equal(d2[:B * T * V1], d[:B * T * V1]) and bool(torch.isnan(d2[B * T * V1:]).all())


@pytest.mark.parametrize('entropy_reg', [0.0, 0.01])
@pytest.mark.parametrize('use_ppo', [0, 1])
def test_rl_loss_ex(dev, use_ppo, entropy_reg):
    """T_all = T + 1 steps per caption in a strided logprobs_all: the extra d_logprobs_all row is written as exact zeros, the
    gradients carry gscale_dev[0], and the step after an END still counts (mask = [1, (seq > 0)[:, :-1]])."""
    from types import SimpleNamespace
    from oracle import rfn_oracle as O
    n = N()
    st = n.stream_ptr()
    B, T, V1 = 6, 5, 301
    g = torch.Generator().manual_seed(5 + use_ppo)
    lp_all = torch.log_softmax(torch.randn(B, T + 1, V1, generator=g), 2)
    seq = torch.randint(1, V1, (B, T), generator=g)
    seq[1, 2:] = 0                                          # END mid-row: step 2 is still in `mask`, not in `mask0`
    seq[2, 1] = 0                                           # an END followed by tokens
    seq[4, 0:] = 0
    inp = lp_all[:, :T].gather(2, seq.unsqueeze(2)).squeeze(2).clone()
    old = inp + 0.3 * torch.randn(B, T, generator=g)
    reward = torch.randn(B, 1, generator=g).expand(B, T).contiguous() * 2.0
    cfg = SimpleNamespace(use_ppo=use_ppo, ppo_clip=0.2)
    ir, lr = inp.double().requires_grad_(True), lp_all.double().requires_grad_(True)
    ref = O.rl_criterion(cfg, ir, seq, reward.double(), lr, float(np.float32(entropy_reg)), [torch.zeros(B, 2, dtype=torch.float64)],
                         -torch.ones(B, 2, dtype=torch.long), 0.0, old.double())
    ref.backward()
    rloss = float(ref.detach())
    ld = V1 + 3
    lpbuf = torch.full((B, T + 1, ld), NAN, device=dev)
    lpbuf[:, :, :V1] = lp_all.to(dev)
    dlp = torch.full((B, T + 1, ld), NAN, device=dev)
    ib, iv = pad2d(inp, T + 1, dev)
    ob, ov = pad2d(old, T + 2, dev)
    rb, rv = pad2d(reward, T + 3, dev)
    db, dv = nan2d(B, T, T + 4, dev)
    sq = torch.full((B, T + 2), 9, dtype=torch.long, device=dev)
    sq[:, :T] = seq.to(dev)
    gdev = torch.tensor([0.37], device=dev)
    scratch = torch.full((B * T,), NAN, device=dev)
    loss = torch.tensor([NAN, NAN], device=dev)
    n.check(n.lib.rfn_rl_loss_ex(iv.data_ptr(), T + 1, sq.data_ptr(), T + 2, rv.data_ptr(), T + 3, lpbuf.data_ptr(), (T + 1) * ld, ld,
                                 B, T, T + 1, V1, entropy_reg, ov.data_ptr(), T + 2, use_ppo, 0.2, gdev.data_ptr(),
                                 scratch.data_ptr(), loss.data_ptr(), 0, dv.data_ptr(), T + 4, dlp.data_ptr(), (T + 1) * ld, ld, st))
    assert abs(float(loss[0]) - rloss) < 1e-5 * max(1.0, abs(rloss)) and bool(torch.isnan(loss[1]))
    assert maxerr(dv, ir.grad * GS) < 1e-6 and pad_is_nan(db, 0, T)
    assert maxerr(dlp[:, :T, :V1], lr.grad[:, :T] * GS) < 1e-7
    assert bool((dlp[:, T, :V1] == 0).all()) and bool(torch.isnan(dlp[:, :, V1:]).all())
    assert float(ir.grad[1, 3].abs()) == 0 and (use_ppo or float(ir.grad[1, 2].abs()) > 0)   # the step after END counts, the next does not
    if entropy_reg > 0:
        assert float(lr.grad[1, 2].abs().max()) == 0 and float(lr.grad[1, 1].abs().max()) > 0


@pytest.mark.parametrize('K', [1, 50, 300])
@pytest.mark.parametrize('nheads', [1, 3, 9])
def test_multilabel_margin_grouped(dev, nheads, K):
    import torch.nn.functional as F
    n = N()
    st = n.stream_ptr()
    B, scale, gscale = 6, 0.7, 1.3
    preds = [rnd(B, K, seed=30 + h) for h in range(nheads)]
    g = torch.Generator().manual_seed(4)
    top = -torch.ones(B, K, dtype=torch.long)
    for b in range(B):
        if b == 0:
            continue                                        # no target (leading -1)
        k = K if b == 1 else min(K, b)                      # row 1 names all K classes
        top[b, :k] = torch.randperm(K, generator=g)[:k]
    if K >= 3:
        top[2, 1] = top[2, 0]                               # a duplicated target
    s32, g32 = float(np.float32(scale)), float(np.float32(gscale))
    prs = [p.double().requires_grad_(True) for p in preds]
    ref = torch.zeros((), dtype=torch.float64)
    for pr in prs:                                          # head after head
        ref = ref + s32 * F.multilabel_margin_loss(pr, top)
    ref.backward()
    rloss = float(ref.detach())
    pd, topd = [p.to(dev) for p in preds], top.to(dev)
    dps = [torch.full((B * K + 4,), NAN, device=dev) for _ in range(nheads)]
    skip = 1 if nheads >= 3 else -1                         # a NULL entry in dpreds
    gdev = torch.tensor([0.37], device=dev)
    scratch = torch.full((nheads * B,), NAN, device=dev)
    loss = torch.tensor([2.5, NAN], device=dev)
    n.check(n.lib.rfn_multilabel_margin_grouped(nheads, n.ptr_array(pd), B, K, topd.data_ptr(), scale, gscale,
                                                gdev.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 1,
                                                n.ptr_array([None if h == skip else dps[h] for h in range(nheads)]), st))
    assert abs(float(loss[0]) - (2.5 + rloss)) < 1e-5 * max(1.0, abs(2.5 + rloss)) and bool(torch.isnan(loss[1]))
    for h in range(nheads):
        if h == skip:
            assert bool(torch.isnan(dps[h]).all())
            continue
        assert maxerr(dps[h][:B * K].view(B, K), prs[h].grad * (g32 * GS)) < 1e-7 and bool(torch.isnan(dps[h][B * K:]).all())
    assert float(prs[0].grad[0].abs().max()) == 0           # the row without targets
    loss2 = torch.tensor([NAN], device=dev)
    n.check(n.lib.rfn_multilabel_margin_grouped(nheads, n.ptr_array(pd), B, K, topd.data_ptr(), scale, gscale, None,
                                                scratch.data_ptr(), loss2.data_ptr(), 0, None, st))          # dpreds = NULL
    assert abs(float(loss2[0]) - rloss) < 1e-5 * max(1.0, abs(rloss))


def test_multilabel_margin_rejects_what_does_not_fit_in_lds(dev):
    n = N()
    B, K = 2, 5000
    pred = torch.zeros(B, K, device=dev)
    top = -torch.ones(B, K, dtype=torch.long, device=dev)
    scratch, loss = torch.zeros(B, device=dev), torch.full((1,), NAN, device=dev)
    assert n.lib.rfn_multilabel_margin_grouped(1, n.ptr_array([pred]), B, K, top.data_ptr(), 1.0, 1.0, None, scratch.data_ptr(),
                                               loss.data_ptr(), 0, None, n.stream_ptr()) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all())


# =================================================================================================================
# 8. Adam
# =================================================================================================================
LR, B1, B2, EPS, GSCALE = (float(np.float32(v)) for v in (5e-4, 0.9, 0.999, 1e-8, 0.5))


def adam_state(cnt, seed=0):
    return rnd(cnt, seed=seed + 1), rnd(cnt, seed=seed + 2, scale=2.0), rnd(cnt, seed=seed + 3, scale=0.1), rnd(cnt, seed=seed + 4, scale=0.1) ** 2


def adam_ref(p, g, m, v, clip, wd, step, dtype):
    """The documented update (rfn.h: rfn_adam_step), every scalar the float the call receives."""
    t = lambda x: torch.tensor(float(np.float32(x)), dtype=dtype)                                           # noqa: E731
    p, g, m, v = (x.to(dtype) for x in (p, g, m, v))
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    g = torch.clamp(g * t(GSCALE), -t(clip), t(clip)) + t(wd) * p
    m = t(B1) * m + (1 - t(B1)) * g
    v = t(B2) * v + (1 - t(B2)) * g * g
    p = p - t(LR / bc1) * m / (torch.sqrt(v) * t(1.0 / math.sqrt(bc2)) + t(EPS))
    return p, m, v


@pytest.mark.parametrize('clip,wd,step', ADAM_CASES)
def test_adam_step_matches_the_documented_formula(dev, clip, wd, step):
    n = N()
    st = n.stream_ptr()
    yp, ym, yv = ADAM_YARD[(clip, wd, step)]
    for cnt in (1, 3, 4, 5, 1023):
        for off in (0, 1):                                  # off = 1: four bytes off 16 -> the scalar path
            p, g, m, v = adam_state(cnt, seed=cnt)
            if clip == 1.0 and cnt >= 5:
                assert bool(((g * 0.5).abs() > 1.0).any())  # the clip is active
            rp, rm, rv = adam_ref(p, g, m, v, clip, wd, step, torch.float64)
            bufs = []
            for t in (p, g, m, v):
                b = torch.full((cnt + 8,), NAN, device=dev)
                b[off:off + cnt] = t.to(dev)
                bufs.append(b)
            pv, gv, mv, vv = (b[off:off + cnt] for b in bufs)
            n.check(n.lib.rfn_adam_step(pv.data_ptr(), gv.data_ptr(), mv.data_ptr(), vv.data_ptr(), cnt, LR, B1, B2, EPS, wd,
                                        clip, GSCALE, step, st))
            assert maxerr(pv, rp) <= 4 * yp and maxerr(mv, rm) <= 4 * ym and maxerr(vv, rv) <= 4 * yv, (cnt, off)
            assert torch.equal(gv.cpu(), g)
            for b in bufs:
                assert bool(torch.isnan(b[:off]).all()) and bool(torch.isnan(b[off + cnt:]).all())


def test_adam_grid_stride_second_trip_and_coefficient_form(dev):
    """The grid is capped at 4096 blocks of 256: a vector bucket of 4 * 2^20 + 8 floats and a scalar (misaligned) one of
    2^20 + 300 need a second trip of the grid-stride loop.  Per-bucket calls, the one-launch form and the form that reads
    its step coefficients from device memory give the same bits."""
    n = N()
    st = n.stream_ptr()
    sizes = [4 * 2 ** 20 + 8, 2 ** 20 + 300]
    gen = torch.Generator(device=dev).manual_seed(0)

    def randn(cnt, scale):
        return torch.randn(cnt + 4, device=dev, generator=gen) * scale
    base = [[randn(s_, 1.0), randn(s_, 2.0), randn(s_, 0.1), randn(s_, 0.1) ** 2] for s_ in sizes]
    offs = [0, 1]

    def fresh():
        cp = [[t.clone() for t in b] for b in base]
        return cp, [[t[o:o + s_] for t in b] for b, o, s_ in zip(cp, offs, sizes)]
    step, clip, wd = 1, 1.0, 1e-5
    bufs1, v1 = fresh()
    for (p, g, m, v), s_ in zip(v1, sizes):
        n.check(n.lib.rfn_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), s_, LR, B1, B2, EPS, wd, clip, GSCALE,
                                    step, st))
    bufs2, v2 = fresh()
    cols = lambda vs, i: n.ptr_array([x[i] for x in vs])                                                       # noqa: E731
    nn_ = (C.c_int64 * 2)(*sizes)
    n.check(n.lib.rfn_adam_step_multi(2, cols(v2, 0), cols(v2, 1), cols(v2, 2), cols(v2, 3), nn_, LR, B1, B2, EPS, wd, clip,
                                      GSCALE, step, st))
    bufs3, v3 = fresh()
    # the coefficients, computed on the host in double and rounded to float (rfn.h: rfn_adam_step_multi_coef)
    coef = torch.tensor([float(np.float32(LR / (1.0 - B1 ** step))), float(np.float32(1.0 / math.sqrt(1.0 - B2 ** step)))],
                        dtype=torch.float32, device=dev)
    n.check(n.lib.rfn_adam_step_multi_coef(2, cols(v3, 0), cols(v3, 1), cols(v3, 2), cols(v3, 3), nn_, coef.data_ptr(), B1, B2,
                                           EPS, wd, clip, GSCALE, st))
    for k in range(2):
        for i in (0, 2, 3):
            assert torch.equal(bufs1[k][i], bufs2[k][i]) and torch.equal(bufs1[k][i], bufs3[k][i]), (k, i)
        assert torch.equal(bufs1[k][1], base[k][1])                                  # g is read-only
        o, s_ = offs[k], sizes[k]
        for i in (0, 2, 3):                                                           # the last elements took the second trip
            assert bool((v1[k][i][-8:] != base[k][i][o + s_ - 8:o + s_]).all())
            assert torch.equal(bufs1[k][i][o + s_:], base[k][i][o + s_:]) and torch.equal(bufs1[k][i][:o], base[k][i][:o])
        # head and tail against the formula (the first elements of trip one, the last of trip two)
        for sl in (slice(0, 64), slice(s_ - 64, s_)):
            ins = [base[k][i][o:o + s_][sl].cpu() for i in range(4)]
            rp, rm, rv = adam_ref(*ins, clip, wd, step, torch.float64)
            yp, ym, yv = ADAM_YARD[(1.0, 1e-5, 1)]
            assert maxerr(v1[k][0][sl], rp) <= 4 * yp and maxerr(v1[k][2][sl], rm) <= 4 * ym and maxerr(v1[k][3][sl], rv) <= 4 * yv
    assert n.lib.rfn_adam_step_multi_coef(2, cols(v3, 0), cols(v3, 1), cols(v3, 2), cols(v3, 3), nn_, None, B1, B2, EPS, wd, clip,
                                          GSCALE, st) == ERR_ARG


# =================================================================================================================
# 9. picks
# =================================================================================================================
def first_max(row):
    """torch.max's order: the first NaN if there is one, else the first maximum."""
    a = row.numpy()
    nan = np.isnan(a)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(a))


@pytest.mark.parametrize('V1', [1, 2, 255, 257, 9488])
def test_greedy_pick_ties_strides_and_degenerate_rows(dev, V1):
    n = N()
    st = n.stream_ptr()
    B = 9
    lp = torch.log_softmax(rnd(B, V1, seed=V1), 1)
    top = float(lp.max()) + 1.0
    if V1 >= 2:
        lp[1, V1 - 2] = lp[1, V1 - 1] = top                # adjacent lanes
    if V1 > 256:
        lp[2, 0] = lp[2, 256] = top                        # one thread's two entries
        lp[8, 256] = top
        lp[8, 0] = lp[8, 3]
    if V1 > 200:
        lp[3, 200] = lp[3, 70] = top                       # two waves
    lp[4, :] = -INF                                        # nothing to choose from: token 0
    if V1 >= 2:
        lp[5, V1 - 1] = NAN                                # NaN ranks above everything: the first NaN
        lp[5, V1 // 2] = NAN
        lp[5, 0] = top
    else:
        lp[5, 0] = NAN
    lp[6, 0] = top                                         # END
    lp[7, ::3] = -INF
    if V1 == 1:
        lp[7, 0] = 0.0
    want = torch.tensor([first_max(lp[b]) for b in range(B)])
    assert int(want[4]) == 0 and int(want[5]) == (V1 // 2 if V1 >= 2 else 0)
    lbuf, lv = pad2d(lp, V1 + 2, dev)
    nxt = torch.full((B + 2,), -7, dtype=torch.long, device=dev)
    seq = torch.full((B, 4), -7, dtype=torch.long, device=dev)
    slp = torch.full((B, 3), NAN, device=dev)
    unf = torch.full((3, B + 2), -7, dtype=torch.int32, device=dev)
    n.check(n.lib.rfn_greedy_pick(lv.data_ptr(), V1 + 2, B, V1, 1, nxt.data_ptr(), seq[:, 1].data_ptr(), 4, slp[:, 1].data_ptr(), 3,
                                  None, unf[1].data_ptr(), st))
    got = nxt[:B].cpu()
    assert bool(((got >= 0) & (got < V1)).all())
    assert torch.equal(got, want) and bool((nxt[B:] == -7).all())
    assert torch.equal(unf[1, :B].cpu(), (want > 0).int()) and bool((unf[1, B:] == -7).all()) and bool((unf[0] == -7).all())
    assert torch.equal(seq[:, 1].cpu(), want) and bool((seq[:, [0, 2, 3]] == -7).all())      # t = 1: seq = it * (it > 0) = it
    val = lp[torch.arange(B), want]
    got_lp = slp[:, 1].cpu()
    assert torch.equal(torch.isnan(got_lp), torch.isnan(val)) and bool(torch.isnan(got_lp[5]))
    assert torch.equal(got_lp[~torch.isnan(val)], val[~torch.isnan(val)])
    assert bool(torch.isnan(slp[:, [0, 2]]).all())
    # t = 2: the finished flags chain
    n.check(n.lib.rfn_greedy_pick(lv.data_ptr(), V1 + 2, B, V1, 2, nxt.data_ptr(), seq[:, 2].data_ptr(), 4, slp[:, 2].data_ptr(), 3,
                                  unf[1].data_ptr(), unf[2].data_ptr(), st))
    assert torch.equal(nxt[:B].cpu(), want) and torch.equal(unf[2, :B].cpu(), (want > 0).int())
    assert torch.equal(seq[:, 2].cpu(), want) and bool((seq[:, [0, 3]] == -7).all())


def test_pick_record_bookkeeping_over_three_steps(dev):
    n = N()
    st = n.stream_ptr()
    B, V1 = 6, 37
    lp = torch.log_softmax(rnd(B, V1, seed=2), 1)
    lbuf, lv = pad2d(lp, V1 + 1, dev)
    given = torch.tensor([[5, 0, -1, V1, 36, 7],            # step 1: rows 1, 2, 3 end (0, and the out-of-range ids read as 0)
                          [0, 9, 4, 4, 36, 8],              # step 2: row 0 ends; rows 1-3 stay finished
                          [3, 3, 3, 3, 0, 9]])              # step 3: row 4 ends
    seq = torch.full((B, 5), -7, dtype=torch.long, device=dev)
    slp = torch.full((B, 5), NAN, device=dev)
    unf = torch.full((4, B), -7, dtype=torch.int32, device=dev)
    alive = torch.ones(B, dtype=torch.bool)
    for t in (1, 2, 3):
        ids = given[t - 1].to(dev)                          # `given` aliases next_ids
        n.check(n.lib.rfn_pick_record(lv.data_ptr(), V1 + 1, B, V1, t, ids.data_ptr(), ids.data_ptr(), seq[:, t].data_ptr(), 5,
                                      slp[:, t].data_ptr(), 5, None if t == 1 else unf[t - 1].data_ptr(), unf[t].data_ptr(), st))
        it = given[t - 1].clone()
        it[(it < 0) | (it >= V1)] = 0
        alive = alive & (it > 0)
        assert torch.equal(ids.cpu(), it)                   # next_ids: the raw (range-checked) token
        assert torch.equal(unf[t].cpu(), alive.int())
        assert torch.equal(seq[:, t].cpu(), it * alive.long())
        assert torch.equal(slp[:, t].cpu(), lp[torch.arange(B), it])
    assert alive.tolist() == [False, False, False, False, False, True]
    assert bool((seq[:, [0, 4]] == -7).all()) and bool(torch.isnan(slp[:, [0, 4]]).all()) and pad_is_nan(lbuf, 0, V1)
    assert n.lib.rfn_pick_record(lv.data_ptr(), V1 + 1, B, V1, 2, ids.data_ptr(), ids.data_ptr(), seq.data_ptr(), 5, slp.data_ptr(), 5,
                                 None, unf[0].data_ptr(), st) == ERR_ARG


@pytest.mark.parametrize('V1', [5, 257, 9488])
def test_multinomial_pick_edges(dev, V1):
    """The acceptance rule of test_multinomial_pick_is_the_inverse_cdf_of_its_uniform at the ends of u, with impossible
    tokens, and the coin mask."""
    n = N()
    st = n.stream_ptr()
    B = 16
    g = torch.Generator().manual_seed(V1)
    logits = torch.randn(B, V1, generator=g) * 3.0
    dead = torch.arange(1, V1, 3)
    logits[:, dead] = -INF                                  # never chosen
    logits[3, 0] = -INF                                     # u = 0 must skip a dead first token
    logits[4, V1 - 1] = -INF                                # u -> 1 must stop at the last token with mass
    logp = torch.log_softmax(logits.double(), 1).float()
    lbuf, lv = pad2d(logp, V1 + 5, dev)
    u = torch.rand(B, generator=g)
    u[0::4] = 0.0
    u[1::4] = float(np.nextafter(np.float32(1), np.float32(0)))
    u[3], u[4] = 0.0, float(np.nextafter(np.float32(1), np.float32(0)))
    ids = torch.full((B, 3), -7, dtype=torch.long, device=dev)
    ud = u.to(dev)                                          # named: a temporary's memory could be reused before the launch runs
    n.check(n.lib.rfn_multinomial_pick(lv.data_ptr(), V1 + 5, B, V1, 1.0, ud.data_ptr(), None, 1.0, ids[:, 1].data_ptr(), 3, st))
    got = ids.cpu()
    assert bool((got[:, [0, 2]] == -7).all())
    cdf = torch.cumsum(torch.exp(logp.double()), 1)
    tgt = u.double() * cdf[:, -1]
    for b in range(B):
        v = int(got[b, 1])
        assert 0 <= v < V1 and math.isfinite(float(logits[b, v])), (b, v)
        lo = float(cdf[b, v - 1]) if v > 0 else 0.0
        tol = 2e-6 * float(cdf[b, -1])
        assert lo - tol <= float(tgt[b]) <= float(cdf[b, v]) + tol, (b, v, lo, float(tgt[b]), float(cdf[b, v]))
    # scheduled sampling: rows with coin >= keep_prob keep the id they hold
    coin = torch.tensor([0.1, 0.9] * (B // 2)).to(dev)
    ids2 = torch.full((B, 3), -7, dtype=torch.long, device=dev)
    n.check(n.lib.rfn_multinomial_pick(lv.data_ptr(), V1 + 5, B, V1, 1.0, ud.data_ptr(), coin.data_ptr(), 0.5,
                                       ids2[:, 1].data_ptr(), 3, st))
    assert torch.equal(ids2[0::2], ids[0::2]) and bool((ids2[1::2] == -7).all())


# =================================================================================================================
# the yardsticks of the docstring: fp32 CPU against fp64, no GPU needed
# =================================================================================================================
def measure_yardsticks():
    print('log-softmax: V1 -> (fwd scale 3, fwd +-80, bwd scale 3, bwd +-80)')
    for V1 in LSM_V1:
        y = [0.0] * 4
        for draw in range(16):
            x, g = lsm_rows(V1, seed=1000 + 7 * draw)
            lp64, lp32 = torch.log_softmax(x.double(), 1), torch.log_softmax(x, 1)
            d64, d32 = lsm_bwd_ref(lp32, g, torch.float64), lsm_bwd_ref(lp32, g, torch.float32)
            e = (lp32.double() - lp64).abs().masked_fill(torch.isinf(x), 0.0)
            eb = (d32.double() - d64).abs()
            y = [max(a, float(b)) for a, b in zip(y, (e[:-1].max(), e[-1].max(), eb[:-1].max(), eb[-1].max()))]
        print('    %d: (%.3g, %.3g, %.3g, %.3g),' % (V1, *y))
    print('LSTM with dropout: p -> (h, d gates / d c_prev)')
    for p in (0.1, 0.5):
        yh = yb = 0.0
        for B, R in ((7, 48), (5, 300)):
            for maxout in (0, 1):
                ins = lstm_inputs(B, R, maxout)
                keep = torch.from_numpy(PH.keep_mask(HI_SEED, HI_OFFSET, B * R, p)).view(B, R)
                r64 = lstm_ref(*ins, R, maxout, keep, p, torch.float64)
                r32 = lstm_ref(*ins, R, maxout, keep, p, torch.float32)
                yh = max(yh, maxerr(r32[0], r64[0]))
                yb = max(yb, maxerr(r32[2], r64[2]), maxerr(r32[3], r64[3]))
        print('    %g: (%.3g, %.3g),' % (p, yh, yb))
    print('Adam: (clip, wd, step) -> (p, m, v)')
    for clip, wd, step in ADAM_CASES:
        st_ = adam_state(100000, seed=77)
        r64 = adam_ref(*st_, clip, wd, step, torch.float64)
        r32 = adam_ref(*st_, clip, wd, step, torch.float32)
        print('    (%r, %r, %d): (%.3g, %.3g, %.3g),' % (clip, wd, step, *(maxerr(a, b) for a, b in zip(r32, r64))))


if __name__ == '__main__':
    measure_yardsticks()
