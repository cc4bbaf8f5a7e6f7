"""The attention kernels (csrc/rfn_attn.hip, csrc/rfn_attn_small_body.h) swept over the shapes, strides and pointer
alignments at which a launcher picks another instantiation or a kernel's loop takes another trip, through the C ABI,
against a plain fp64 restatement on the CPU (attn_ref of tests/test_kernels_gpu.py and the backward formulas of rfn.h).

Constants restated from the sources (nothing is imported from the C side):
    ATT_THREADS 256, ATT_WAVES 4; score forward: SC_ROWS 16 rows per block, A chunks of 256 (16-B loads) / 64 (scalar);
    context forward: 1024 (vector) / 256 (scalar) columns per block, rows unrolled by 4 plus a remainder loop, the
    softmax's `l = tid` loops take a second trip at L > 256, dynamic LDS L floats (+ a static red[4] in the two-launch
    form); dalpha: 64 rows per block, 4 rows per wave walked together, D chunks of 256 / 64, LDS D floats rounded up to 4;
    score backward: SB_WAVES 16 (1024 threads), SB_UNROLL 4 -> 64 rows per sweep, `l = tid` loops trip again at L > 1024,
    LDS floats (2 + 2 * 16) * Ap + 16 + L, fused (2 + 2 * 16) * Ap + 16 + 2 * Lp + Dp (Xp = X rounded up to 4), refused above
    150 KiB, opt-in above 48 KiB; every other launcher refuses above 64 KiB; fused small-L: L <= 1024 (ATS_MAX_L), LDS
    2 * Ap + L (forward), 2 * Ap + Dp + 2 * Lp (backward), rows in pairs l, l + 4, d att_seq loop of 1024 float4 per trip
    clamped at n4 - 1, A loop of 1024 columns per trip (vector) / 256 (scalar).  RFN_MAX_ENC 8.

Conventions: every operand is carved out of a larger NaN-filled device buffer with at least 8 floats in front and behind;
after a call everything outside an output's elements (guards, padding between rows, the tail) must hold the same bits,
everything inside must have been written, and no input may have changed.  Layouts, per operand: packed; padded4 (row and
batch strides + 4 floats: still 16-B loads); ld_plus_1 (strides + 1: scalar instantiation); offset_1 (base + 1 float,
strides multiples of 4: the rfn_aligned16 fallback); time_major (stride_b = R, stride_l = B * R); `soff`: the operands
that are only ever read or written as scalars (hproj, w_out, b_out, alpha, dalpha, dz with an odd lddz) one float off.

Tolerances
----------
* what the sources state as bit-identity is asserted as bit-identity: two-launch forward == split pair, fused backward
  == dalpha + score backward, grouped / heterogeneous == one call per encoder (taking the same instantiation: one
  encoder that breaks the 16-B conditions puts every encoder of a heterogeneous launch on the scalar kernels, and the
  per-encoder comparison call is then made on a misaligned att_seq), in place == out of place, row b of a B-row call ==
  that row alone.
* exact consequences of the formulas are asserted exactly (L = 1, saturated tanh, equal scores).
* unit-normal operands with w_out at scale 0.3 are the regime of test_attention_forward_backward, whose tolerances are
  reused unchanged: alpha 2e-6, z 1e-5, dproj 2e-5, dhproj 1e-4, dw_part.sum(0) 1e-4 * max(1, max|ref|), d att_seq 1e-5.
  dalpha on its own (not stated there) is a dot product of D floats: (D + 1) * 2^-24 * sum_d |x dz|, the worst case of
  any summation order -- derived, not tuned.
* a new value regime gets no invented number: the same operation in plain fp32 torch on the CPU (the header's
  1 - 2 / (e^2x + 1) tanh, the rfn.h backward formulas), its max error against fp64 is the YARDSTICK, and the kernel is
  allowed 4x that (another summation tree; device expf / rcp at 1-2 ulp).  `python tests/test_attention_edges_gpu.py`
  (no GPU) re-measures the table.  Regimes: small = proj, hproj * 0.01; sat = proj * 30; peak = one row per batch row
  with proj + hproj = 30 * sign(w) and sum|w| = 240 (its score leads by > 120: every other alpha underflows to 0);
  shift+ / shift- = b_out = +-1e4.  Yardsticks (alpha, z, dproj, dhproj, dw, d att_seq):

      regime  (B, L, A, D)       alpha      z          dproj      dhproj     dw         d att_seq
      small   (2, 17, 64, 36)    1.5e-08    1.08e-07   7.59e-08   6.62e-08   1.85e-07   1.3e-07
      small   (2, 5, 30, 18)     3.12e-08   1.02e-07   9.84e-08   6.31e-08   2.2e-07    1.07e-07
      small   (2, 65, 260, 20)   8.75e-09   6.79e-08   6.25e-08   9.76e-08   8.62e-08   1.23e-07
      sat     (2, 17, 64, 36)    1.24e-07   3.95e-07   1.05e-07   1.05e-07   7.83e-07   5.32e-07
      sat     (2, 5, 30, 18)     6.75e-08   2.36e-07   1.32e-07   2.18e-07   5.29e-07   2.11e-07
      sat     (2, 65, 260, 20)   2.4e-07    7.18e-07   1.08e-07   1.43e-07   1.07e-06   3.52e-07
      peak    (2, 17, 64, 36)    1.82e-81   0          8.97e-80   8.97e-80   1.09e-80   1.19e-07
      peak    (2, 5, 30, 18)     6e-82      0          2.28e-80   1.79e-80   1.36e-81   1.19e-07
      peak    (2, 65, 260, 20)   6.66e-95   0          7.29e-94   1.18e-93   6.2e-94    1.19e-07
      shift+  (2, 17, 64, 36)    9.75e-05   0.000233   0.000208   0.000234   0.000618   0.000202
      shift+  (2, 5, 30, 18)     7.94e-05   0.000272   8.52e-05   7.16e-05   0.000494   0.000174
      shift+  (2, 65, 260, 20)   8.28e-05   0.000257   0.000185   0.000121   0.00075    0.000181
      shift-  (2, 17, 64, 36)    9.75e-05   0.000233   0.000208   0.000234   0.000618   0.000202
      shift-  (2, 5, 30, 18)     7.94e-05   0.000272   8.52e-05   7.16e-05   0.000494   0.000174
      shift-  (2, 65, 260, 20)   8.28e-05   0.000257   0.000185   0.000121   0.00075    0.000181
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')
U = 2.0 ** -24
GUARD = 8
ERR_SHAPE, ERR_ARG = -1, -5
MAX_ENC = 8                                        # rfn.h RFN_MAX_ENC
LDS_64K, LDS_150K, LDS_48K = 64 * 1024 // 4, 150 * 1024 // 4, 48 * 1024 // 4   # in floats
TOL = dict(alpha=2e-6, z=1e-5, dproj=2e-5, dhp=1e-4, dw=1e-4, dx=1e-5)          # test_attention_forward_backward

REGIMES = ['small', 'sat', 'peak', 'shift+', 'shift-']
REGIME_SHAPES = [(2, 17, 64, 36), (2, 5, 30, 18), (2, 65, 260, 20)]
# ---- measured yardsticks (see the docstring; re-measure with `python tests/test_attention_edges_gpu.py`) ---------------
YARD = {
    # (regime, (B, L, A, D)): (alpha, z, dproj, dhproj, dw, d att_seq)
    ('small', (2, 17, 64, 36)): (1.5e-08, 1.08e-07, 7.59e-08, 6.62e-08, 1.85e-07, 1.3e-07),
    ('small', (2, 5, 30, 18)): (3.12e-08, 1.02e-07, 9.84e-08, 6.31e-08, 2.2e-07, 1.07e-07),
    ('small', (2, 65, 260, 20)): (8.75e-09, 6.79e-08, 6.25e-08, 9.76e-08, 8.62e-08, 1.23e-07),
    ('sat', (2, 17, 64, 36)): (1.24e-07, 3.95e-07, 1.05e-07, 1.05e-07, 7.83e-07, 5.32e-07),
    ('sat', (2, 5, 30, 18)): (6.75e-08, 2.36e-07, 1.32e-07, 2.18e-07, 5.29e-07, 2.11e-07),
    ('sat', (2, 65, 260, 20)): (2.4e-07, 7.18e-07, 1.08e-07, 1.43e-07, 1.07e-06, 3.52e-07),
    ('peak', (2, 17, 64, 36)): (1.82e-81, 0, 8.97e-80, 8.97e-80, 1.09e-80, 1.19e-07),
    ('peak', (2, 5, 30, 18)): (6e-82, 0, 2.28e-80, 1.79e-80, 1.36e-81, 1.19e-07),
    ('peak', (2, 65, 260, 20)): (6.66e-95, 0, 7.29e-94, 1.18e-93, 6.2e-94, 1.19e-07),
    ('shift+', (2, 17, 64, 36)): (9.75e-05, 0.000233, 0.000208, 0.000234, 0.000618, 0.000202),
    ('shift+', (2, 5, 30, 18)): (7.94e-05, 0.000272, 8.52e-05, 7.16e-05, 0.000494, 0.000174),
    ('shift+', (2, 65, 260, 20)): (8.28e-05, 0.000257, 0.000185, 0.000121, 0.00075, 0.000181),
    ('shift-', (2, 17, 64, 36)): (9.75e-05, 0.000233, 0.000208, 0.000234, 0.000618, 0.000202),
    ('shift-', (2, 5, 30, 18)): (7.94e-05, 0.000272, 8.52e-05, 7.16e-05, 0.000494, 0.000174),
    ('shift-', (2, 65, 260, 20)): (8.28e-05, 0.000257, 0.000185, 0.000121, 0.00075, 0.000181),
}


def N():
    import recurrent_fusion_network_amd._native as n
    return n


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def up4(v):
    return (v + 3) // 4 * 4


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# =================================================================================================================
# operands carved out of guarded buffers
# =================================================================================================================
class Op:
    """A logical tensor placed with element strides `strides` at GUARD + off floats into a NaN-filled device buffer."""

    def __init__(self, t, dev, strides=None, off=0):
        shape = tuple(t.shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.insert(0, acc)
                acc *= s
        span = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        self.buf = torch.full((GUARD + off + span + GUARD,), NAN, device=dev)
        self.v = self.buf.as_strided(shape, tuple(strides), GUARD + off)
        self.v.copy_(t.to(dev))
        self.strides = tuple(strides)
        self.mask = torch.ones(self.buf.shape, dtype=torch.bool, device=dev)
        self.mask.as_strided(shape, tuple(strides), GUARD + off).fill_(False)
        self.snap = self.buf.clone()
        assert (self.ptr % 16 == 0) == (off % 4 == 0)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def outside_ok(self):
        """guards, padding and the tail hold the bits they held when the operand was made"""
        return torch.equal(self.buf.view(torch.int32)[self.mask], self.snap.view(torch.int32)[self.mask])

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.snap.view(torch.int32))

    def written(self):
        return not bool(torch.isnan(self.v).any())

    def get(self):
        return self.v.detach().cpu().clone()

    def freeze(self):
        """an output that now serves as an input: from here on it must not change at all"""
        self.snap = self.buf.clone()
        return self


def lay3(B, L, R, variant):
    """strides and base offset of a (B, L, R) operand"""
    if variant == 'packed':
        return (L * R, R, 1), 0
    if variant == 'padded4':
        return (L * (R + 4) + 4, R + 4, 1), 0
    if variant == 'ld_plus_1':
        return (L * (R + 1) + 1, R + 1, 1), 0
    if variant == 'offset_1':
        return (L * up4(R), up4(R), 1), 1
    if variant == 'time_major':
        return (R, B * R, 1), 0
    raise ValueError(variant)


def lay2(R, variant):
    """leading dimension and base offset of a (B, R) operand"""
    return {'packed': (R, 0), 'time_major': (R, 0), 'padded4': (R + 4, 0), 'ld_plus_1': (R + 1, 0),
            'offset_1': (up4(R), 1)}[variant]


def op3(t, dev, variant='packed'):
    st, off = lay3(t.shape[0], t.shape[1], t.shape[2], variant)
    return Op(t, dev, st, off)


def op2(t, dev, variant='packed'):
    ld, off = lay2(t.shape[1], variant)
    return Op(t, dev, (ld, 1), off)


def nans(*shape):
    return torch.full(shape, NAN)


def finish(outs, ins):
    torch.cuda.synchronize()
    for o in outs:
        assert o.outside_ok(), 'a kernel wrote outside its output'
    for i in ins:
        assert i.unchanged(), 'a kernel wrote into an input'


# =================================================================================================================
# references
# =================================================================================================================
def make_inputs(B, L, A, D, seed=0, bo=True):
    return dict(proj=rnd(B, L, A, seed=seed + 1), hp=rnd(B, A, seed=seed + 2), w=rnd(A, seed=seed + 3, scale=0.3),
                bo=rnd(1, seed=seed + 4) if bo else None, x=rnd(B, L, D, seed=seed + 5), dz=rnd(B, D, seed=seed + 6),
                base=rnd(B, L, A, seed=seed + 7), xbase=rnd(B, L, D, seed=seed + 8))


def rows(d, b):
    """batch row b of a set of inputs, as a B = 1 problem"""
    return {k: (v if v is None or k in ('w', 'bo') else v[b:b + 1].clone()) for k, v in d.items()}


def attn_all(d, dtype=torch.float64, fast_tanh=False, alpha=None):
    """Forward and backward of the whole attention from the formulas in rfn.h, in `dtype`.  alpha: use these weights in
    the backward (the kernels' backward takes the forward's float32 alpha) instead of the ones computed here."""
    proj, hp, w, x, dz = [d[k].to(dtype) for k in ('proj', 'hp', 'w', 'x', 'dz')]
    p = proj + hp[:, None, :]
    e = 1.0 - 2.0 / (torch.exp(2.0 * p) + 1.0) if fast_tanh else torch.tanh(p)
    s = e @ w
    if d['bo'] is not None:
        s = s + d['bo'].to(dtype)
    ex = torch.exp(s - s.max(1, keepdim=True)[0])
    al = ex / ex.sum(1, keepdim=True)
    z = (al[:, :, None] * x).sum(1)
    a2 = al if alpha is None else alpha.to(dtype)
    dal = (x * dz[:, None, :]).sum(2)
    ds = a2 * (dal - (a2 * dal).sum(1, keepdim=True))
    dproj = ds[:, :, None] * w * (1.0 - e * e)
    return dict(alpha=al, z=z, dal=dal, dproj=dproj, dhp=dproj.sum(1), dwp=(ds[:, :, None] * e).sum(1),
                dx=a2[:, :, None] * dz[:, None, :])


def regime_inputs(regime, B, L, A, D):
    d = make_inputs(B, L, A, D, seed=100)
    if regime == 'small':
        d['proj'], d['hp'] = d['proj'] * 0.01, d['hp'] * 0.01
    elif regime == 'sat':
        d['proj'] = d['proj'] * 30.0
    elif regime == 'peak':
        d['w'] = d['w'] * (240.0 / float(d['w'].abs().sum()))
        sg = torch.where(d['w'] >= 0, torch.ones(A), -torch.ones(A))
        for b in range(B):
            d['proj'][b, (3 * b + 1) % L] = 30.0 * sg - d['hp'][b]
    elif regime == 'shift+':
        d['bo'] = torch.tensor([1e4])
    elif regime == 'shift-':
        d['bo'] = torch.tensor([-1e4])
    else:
        raise ValueError(regime)
    return d


def measure_yardstick(regime, shape):
    d = regime_inputs(regime, *shape)
    r64, r32 = attn_all(d), attn_all(d, torch.float32, fast_tanh=True)
    if regime == 'peak':                          # every other weight is below the smallest float32
        top = r64['alpha'].max(1, keepdim=True)[0]
        assert float(r64['alpha'][r64['alpha'] < top].max()) < 1e-46
    out = []
    for k in ('alpha', 'z', 'dproj', 'dhp', 'dwp', 'dx'):
        a, b = r32[k].double(), r64[k]
        if k == 'dwp':
            a, b = a.sum(0), b.sum(0)
        if k == 'dx':                             # accumulated onto a given target, as rfn_attn_small_bwd does
            a, b = (d['xbase'] + r32[k]).double(), d['xbase'].double() + b
        out.append(float((a - b).abs().max()))
    return tuple(out)


def print_table():
    lines = []
    for regime in REGIMES:
        for shape in REGIME_SHAPES:
            y = measure_yardstick(regime, shape)
            lines.append("    ('%s', %s): (%s)," % (regime, shape, ', '.join('%.3g' % v for v in y)))
    print('\n'.join(lines))


# =================================================================================================================
# runners: one forward / backward of one encoder in a given layout, every guard checked
# =================================================================================================================
def run_fwd(n, dev, d, form='pair', lp='packed', lx='packed', lz='packed', soff=0):
    """-> alpha, z (CPU).  form: pair (scores_fwd + context_fwd), fused (rfn_attn_fwd), small (rfn_attn_small_fwd)."""
    B, L, A = d['proj'].shape
    D = d['x'].shape[2]
    st = n.stream_ptr()
    P, X = op3(d['proj'], dev, lp), op3(d['x'], dev, lx)
    HP, W = Op(d['hp'], dev, off=soff), Op(d['w'], dev, off=soff)
    BO = Op(d['bo'], dev, off=soff) if d['bo'] is not None else None
    AL, Z = Op(nans(B, L), dev, off=soff), op2(nans(B, D), dev, lz)
    bo = BO.ptr if BO else None
    outs = [AL, Z]
    if form == 'pair':
        n.check(n.lib.rfn_attn_scores_fwd(P.ptr, P.strides[0], P.strides[1], HP.ptr, W.ptr, bo, B, L, A, AL.ptr, st))
        n.check(n.lib.rfn_attn_context_fwd(X.ptr, X.strides[0], X.strides[1], AL.ptr, B, L, D, Z.ptr, Z.strides[0], st))
    elif form == 'fused':
        RAW = Op(nans(B, L), dev, off=soff)
        outs.append(RAW)
        n.check(n.lib.rfn_attn_fwd(P.ptr, P.strides[0], P.strides[1], HP.ptr, W.ptr, bo, X.ptr, X.strides[0], X.strides[1],
                                   B, L, A, D, RAW.ptr, AL.ptr, Z.ptr, Z.strides[0], st))
    elif form == 'small':
        pa = lambda *ops: n.ptr_array([o.v if o is not None else None for o in ops])  # noqa: E731
        n.check(n.lib.rfn_attn_small_fwd(1, pa(P), P.strides[0], P.strides[1], pa(HP), pa(W), pa(BO), pa(X), X.strides[0],
                                         X.strides[1], B, L, A, D, pa(AL), pa(Z), Z.strides[0], st))
    else:
        raise ValueError(form)
    finish(outs, [P, X, HP, W] + ([BO] if BO else []))
    return AL.get(), Z.get()


def run_bwd(n, dev, d, alpha, form='pair', lp='packed', lx='packed', ldp='packed', ldz='packed', soff=0, acc=0,
            inplace=False, ldhp='packed', ldwp='packed', ldx='packed', want_dx=True):
    """-> dict(dproj, dhp, dwp[, dal][, dx]) on the CPU.  form: pair (context_bwd_dalpha + scores_bwd), fused
    (rfn_attn_bwd), small (rfn_attn_small_bwd, one encoder; d att_seq accumulated onto d['xbase'] when want_dx).
    acc: dproj is accumulated onto d['base'].  inplace: dproj is the proj buffer itself (layout lp)."""
    B, L, A = d['proj'].shape
    D = d['x'].shape[2]
    st = n.stream_ptr()
    P, X = op3(d['proj'], dev, lp), op3(d['x'], dev, lx)
    HP, W, AL = Op(d['hp'], dev, off=soff), Op(d['w'], dev, off=soff), Op(alpha, dev, off=soff)
    DZ = Op(d['dz'], dev, (D + 1, 1), 1) if soff else op2(d['dz'], dev, ldz)     # soff: an odd lddz, one float off
    DP = P if inplace else op3(d['base'] if acc else nans(B, L, A), dev, ldp)
    DHP = Op(nans(B, A), dev, off=1 if ldhp == 'offset_1' else 0)
    DWP = Op(nans(B, A), dev, off=1 if ldwp == 'offset_1' else 0)
    outs, ins = [DP, DHP, DWP], [X, HP, W, AL, DZ] + ([] if inplace else [P])
    res = {}
    if form == 'pair':
        DAL = Op(nans(B, L), dev, off=soff)
        n.check(n.lib.rfn_attn_context_bwd_dalpha(X.ptr, X.strides[0], X.strides[1], DZ.ptr, DZ.strides[0], B, L, D,
                                                  DAL.ptr, st))
        n.check(n.lib.rfn_attn_scores_bwd(P.ptr, P.strides[0], P.strides[1], HP.ptr, W.ptr, AL.ptr, DAL.ptr, B, L, A, DP.ptr,
                                          DP.strides[0], DP.strides[1], acc, DHP.ptr, DWP.ptr, st))
        outs.append(DAL)
    elif form == 'fused':
        n.check(n.lib.rfn_attn_bwd(P.ptr, P.strides[0], P.strides[1], HP.ptr, W.ptr, AL.ptr, X.ptr, X.strides[0],
                                   X.strides[1], DZ.ptr, DZ.strides[0], B, L, A, D, DP.ptr, DP.strides[0], DP.strides[1], acc,
                                   DHP.ptr, DWP.ptr, st))
    elif form == 'small':
        pa = lambda *ops: n.ptr_array([o.v for o in ops])  # noqa: E731
        DX = None
        if want_dx:                                # d att_seq shares att_seq's strides; only its base may differ
            offx = {'packed': 1 if lx == 'offset_1' else 0, 'offset_1': 1, 'aligned': 0}[ldx]
            DX = Op(d['xbase'], dev, X.strides, offx)
            outs.append(DX)
        n.check(n.lib.rfn_attn_small_bwd(1, pa(P), P.strides[0], P.strides[1], pa(HP), pa(W), pa(AL), pa(X), X.strides[0],
                                         X.strides[1], pa(DZ), DZ.strides[0], B, L, A, D, pa(DP), DP.strides[0],
                                         DP.strides[1], acc, pa(DHP), pa(DWP), pa(DX) if DX else None, st))
        if DX:
            res['dx'] = DX.get()
    else:
        raise ValueError(form)
    finish(outs, ins)
    for o in outs:
        assert o.written()
    res.update(dproj=DP.get(), dhp=DHP.get(), dwp=DWP.get())
    if form == 'pair':
        res['dal'] = DAL.get()
    return res


def check_fwd_fp64(al, z, ref):
    assert maxerr(al, ref['alpha']) < TOL['alpha']
    assert maxerr(z, ref['z']) < TOL['z']


def check_bwd_fp64(got, ref, d, acc=0):
    """ref: attn_all(d, alpha=<the float32 alpha the kernel was given>)"""
    base = d['base'].double() if acc else 0.0
    assert maxerr(got['dproj'], ref['dproj'] + base) < TOL['dproj']
    assert maxerr(got['dhp'], ref['dhp']) < TOL['dhp']
    gw = ref['dwp'].sum(0)
    assert maxerr(got['dwp'].double().sum(0), gw) < TOL['dw'] * max(1.0, float(gw.abs().max()))
    if 'dx' in got:
        assert maxerr(got['dx'], ref['dx'] + d['xbase'].double()) < TOL['dx']
    if 'dal' in got:
        D = d['x'].shape[2]
        mag = (d['x'].double().abs() * d['dz'].double().abs()[:, None, :]).sum(2)
        assert bool(((got['dal'].double() - ref['dal']).abs() <= (D + 1) * U * mag).all())


def same_results(a, b, keys=('dproj', 'dhp', 'dwp')):
    return all(same_bits(a[k], b[k]) for k in keys)


# =================================================================================================================
# 1. score forward: 16 rows per block; A chunks of 256 (vector) / 64 (scalar)
# =================================================================================================================
SCORE_CASES = [
    # B, L, A, proj layout, soff          -- vector instantiation
    (2, 1, 64, 'packed', 0), (2, 15, 256, 'padded4', 0), (3, 16, 260, 'packed', 0), (2, 17, 1028, 'packed', 0),
    (2, 33, 64, 'time_major', 0), (2, 33, 256, 'packed', 1), (2, 17, 260, 'padded4', 1),
    # scalar instantiation: A % 4, an odd stride, a misaligned base
    (2, 1, 3, 'packed', 0), (2, 15, 65, 'padded4', 0), (2, 16, 1, 'packed', 0), (2, 17, 64, 'ld_plus_1', 0),
    (2, 33, 256, 'offset_1', 0), (2, 15, 260, 'ld_plus_1', 0), (1, 16, 1028, 'offset_1', 0), (3, 33, 3, 'time_major', 1),
    (2, 1, 256, 'offset_1', 0),
]


@pytest.mark.parametrize('B,L,A,lp,soff', SCORE_CASES)
def test_score_forward_edges(dev, B, L, A, lp, soff):
    n, D = N(), 4
    d = make_inputs(B, L, A, D, seed=B + L + A)
    ref = attn_all(d)
    al, z = run_fwd(n, dev, d, 'pair', lp=lp, soff=soff)
    assert not bool(torch.isnan(al).any()) and not bool(torch.isnan(z).any())
    check_fwd_fp64(al, z, ref)
    if L == 1:
        assert bool((al == 1.0).all())
    for b in range(B):                             # one block per (row, 16 scores): row b alone gives the same bits
        al1, _ = run_fwd(n, dev, rows(d, b), 'pair', lp=lp, soff=soff)
        assert same_bits(al1[0], al[b])


# =================================================================================================================
# 2. context forward and the two-launch form: 4-row unroll + remainder; 1024 / 256 columns per block; L > 256
# =================================================================================================================
CONTEXT_CASES = [
    # B, L, A, D, lp, lx, lz, soff          -- vector context
    (2, 1, 8, 4, 'packed', 'packed', 'packed', 0), (2, 2, 8, 256, 'packed', 'padded4', 'padded4', 0),
    (2, 3, 8, 1024, 'packed', 'packed', 'packed', 0), (2, 4, 8, 1028, 'packed', 'packed', 'padded4', 0),
    (3, 5, 64, 256, 'time_major', 'time_major', 'packed', 0), (2, 9, 8, 1028, 'padded4', 'padded4', 'packed', 0),
    (2, 257, 4, 4, 'packed', 'packed', 'packed', 0), (2, 5, 8, 256, 'packed', 'packed', 'packed', 1),
    (2, 9, 3, 1024, 'ld_plus_1', 'packed', 'packed', 0),          # scalar scores, vector context
    # scalar context: D % 4, att_seq only, z only
    (2, 1, 3, 1, 'packed', 'packed', 'packed', 0), (2, 2, 8, 255, 'packed', 'packed', 'packed', 0),
    (2, 3, 8, 257, 'packed', 'padded4', 'packed', 0), (2, 4, 8, 256, 'packed', 'ld_plus_1', 'packed', 0),
    (2, 5, 8, 1024, 'packed', 'offset_1', 'packed', 0), (2, 9, 8, 1028, 'packed', 'packed', 'ld_plus_1', 0),
    (2, 257, 8, 4, 'packed', 'packed', 'offset_1', 0), (2, 1, 8, 1028, 'packed', 'time_major', 'ld_plus_1', 1),
    (2, 257, 4, 1, 'packed', 'packed', 'packed', 0),
]


@pytest.mark.parametrize('B,L,A,D,lp,lx,lz,soff', CONTEXT_CASES)
def test_context_forward_and_two_launch_form_edges(dev, B, L, A, D, lp, lx, lz, soff):
    n = N()
    d = make_inputs(B, L, A, D, seed=L + D)
    ref = attn_all(d)
    kw = dict(lp=lp, lx=lx, lz=lz, soff=soff)
    al, z = run_fwd(n, dev, d, 'pair', **kw)
    assert not bool(torch.isnan(al).any()) and not bool(torch.isnan(z).any())
    check_fwd_fp64(al, z, ref)
    al2, z2 = run_fwd(n, dev, d, 'fused', **kw)
    assert same_bits(al2, al) and same_bits(z2, z)
    if L == 1:
        assert bool((al == 1.0).all()) and same_bits(z, d['x'][:, 0])
    for b in range(B):
        for form in ('pair', 'fused'):
            al1, z1 = run_fwd(n, dev, rows(d, b), form, **kw)
            assert same_bits(al1[0], al[b]) and same_bits(z1[0], z[b])


# =================================================================================================================
# 3. dalpha: 64 rows per block, 4 rows per wave together (rows past the end re-read the last valid one)
# =================================================================================================================
DALPHA_CASES = [
    # B, L, D, lx, ldz / soff
    (2, 1, 4, 'packed', 0), (2, 3, 252, 'padded4', 0), (2, 4, 256, 'packed', 0), (2, 5, 260, 'packed', 1),
    (2, 63, 512, 'packed', 0), (2, 64, 516, 'time_major', 0), (3, 65, 256, 'padded4', 1),
    (2, 1, 1, 'packed', 0), (2, 3, 4, 'ld_plus_1', 0), (2, 4, 252, 'offset_1', 0), (2, 5, 1, 'packed', 1),
    (2, 63, 260, 'ld_plus_1', 0), (2, 64, 257, 'packed', 0), (2, 65, 512, 'offset_1', 0), (2, 65, 516, 'ld_plus_1', 1),
    (2, 3, 256, 'offset_1', 0),
]


@pytest.mark.parametrize('B,L,D,lx,soff', DALPHA_CASES)
def test_dalpha_edges(dev, B, L, D, lx, soff):
    n, st = N(), N().stream_ptr()
    d = make_inputs(B, L, 4, D, seed=L * 7 + D)

    def run(dd):
        Bq = dd['x'].shape[0]
        X = op3(dd['x'], dev, lx)
        DZ = Op(dd['dz'], dev, (D + 1, 1), 1) if soff else op2(dd['dz'], dev, 'padded4')
        DAL = Op(nans(Bq, L), dev, off=soff)
        n.check(n.lib.rfn_attn_context_bwd_dalpha(X.ptr, X.strides[0], X.strides[1], DZ.ptr, DZ.strides[0], Bq, L, D,
                                                  DAL.ptr, st))
        finish([DAL], [X, DZ])
        assert DAL.written()
        return DAL.get()
    dal = run(d)
    want = (d['x'].double() * d['dz'].double()[:, None, :]).sum(2)
    mag = (d['x'].double().abs() * d['dz'].double().abs()[:, None, :]).sum(2)
    assert bool(((dal.double() - want).abs() <= (D + 1) * U * mag).all())
    for b in range(B):
        assert same_bits(run(rows(d, b))[0], dal[b])


# =================================================================================================================
# 4. d att_seq += alpha * dz on a non-zero target
# =================================================================================================================
@pytest.mark.parametrize('B,L,D,lx,soff', [(2, 1, 1, 'packed', 0), (2, 5, 255, 'padded4', 0), (2, 5, 256, 'packed', 0),
                                           (2, 1, 257, 'ld_plus_1', 0), (3, 5, 256, 'offset_1', 0),
                                           (2, 5, 256, 'time_major', 1), (2, 1, 256, 'padded4', 1)])
def test_dseq_accumulates_in_every_layout(dev, B, L, D, lx, soff):
    n, st = N(), N().stream_ptr()
    d = make_inputs(B, L, 4, D, seed=L + D)
    alpha = torch.softmax(rnd(B, L, seed=9), 1)

    def run(al, dz, base):
        Bq = al.shape[0]
        AL = Op(al, dev, off=soff)
        DZ = Op(dz, dev, (D + 1, 1), 1) if soff else op2(dz, dev, 'packed')
        DX = op3(base, dev, lx)
        n.check(n.lib.rfn_attn_context_bwd_dseq(AL.ptr, DZ.ptr, DZ.strides[0], Bq, L, D, DX.ptr, DX.strides[0], DX.strides[1],
                                                st))
        finish([DX], [AL, DZ])
        return DX.get()
    got = run(alpha, d['dz'], d['xbase'])
    want = d['xbase'].double() + alpha.double()[:, :, None] * d['dz'].double()[:, None, :]
    assert maxerr(got, want) < TOL['dx']
    # one multiply-add per element: at most two roundings whatever the compiler contracts
    assert bool(((got.double() - want).abs() <= 2 * 2 * U * (want.abs() + d['xbase'].double().abs())).all())
    for b in range(B):
        assert same_bits(run(alpha[b:b + 1], d['dz'][b:b + 1], d['xbase'][b:b + 1])[0], got[b])


# =================================================================================================================
# 5. score backward and the fused backward: 64 rows per sweep, L > 1024, A chunks, both mixed instantiations, LDS opt-in
# =================================================================================================================
# LDS floats of the score backward: 34 * Ap + 16 + L, fused 34 * Ap + 16 + 2 * Lp + Dp; the opt-in starts above 48 KiB = 12288
# floats.  At L = 17, D = 8: A = 356 stays below in both forms (12137 / 12168), A = 360 below in the split form (12273) and above
# in the fused one (12304), A = 364 above in both (12409 / 12440).
assert 34 * 356 + 16 + 2 * up4(17) + 8 <= LDS_48K and 34 * 360 + 16 + 17 <= LDS_48K < 34 * 360 + 16 + 2 * up4(17) + 8
assert LDS_48K < 34 * 364 + 16 + 17
BWD_CASES = [
    # B, L, A, D, lp, lx, ldp, soff, acc          -- <VEC = true, vec_x = 1>
    (2, 1, 64, 8, 'packed', 'packed', 'packed', 0, 0), (2, 15, 256, 8, 'padded4', 'padded4', 'padded4', 0, 1),
    (2, 16, 260, 260, 'packed', 'packed', 'packed', 0, 0), (2, 17, 360, 8, 'packed', 'packed', 'packed', 0, 1),
    (2, 17, 356, 8, 'padded4', 'packed', 'packed', 0, 0),
    (2, 17, 364, 8, 'packed', 'packed', 'packed', 1, 0), (2, 63, 64, 260, 'time_major', 'time_major', 'packed', 0, 0),
    (3, 64, 64, 8, 'packed', 'packed', 'padded4', 0, 1), (2, 65, 256, 8, 'packed', 'packed', 'time_major', 1, 0),
    (1, 1030, 64, 8, 'packed', 'packed', 'packed', 0, 1),
    # <VEC = true, vec_x = 0>: D % 4, an odd att_seq stride, a misaligned att_seq
    (2, 17, 64, 18, 'packed', 'packed', 'packed', 0, 0), (2, 65, 256, 8, 'packed', 'ld_plus_1', 'packed', 0, 1),
    (2, 16, 260, 260, 'packed', 'offset_1', 'packed', 0, 0), (2, 63, 64, 18, 'padded4', 'padded4', 'padded4', 1, 1),
    # <VEC = false, vec_x = 1>: A % 4, proj only, dproj only
    (2, 15, 65, 8, 'packed', 'packed', 'packed', 0, 0), (2, 17, 3, 260, 'packed', 'padded4', 'packed', 0, 1),
    (2, 64, 64, 8, 'ld_plus_1', 'packed', 'packed', 0, 0), (2, 16, 256, 8, 'offset_1', 'packed', 'packed', 0, 1),
    (2, 65, 260, 8, 'packed', 'packed', 'ld_plus_1', 0, 1), (2, 63, 64, 260, 'packed', 'packed', 'offset_1', 0, 0),
    (2, 17, 364, 8, 'packed', 'packed', 'offset_1', 0, 0), (2, 1, 1, 8, 'packed', 'packed', 'packed', 0, 0),
    # <VEC = false, vec_x = 0>
    (2, 1, 3, 18, 'packed', 'packed', 'packed', 0, 0), (2, 15, 1, 18, 'ld_plus_1', 'ld_plus_1', 'ld_plus_1', 1, 1),
    (1, 1030, 65, 18, 'packed', 'packed', 'packed', 0, 0), (2, 16, 360, 18, 'offset_1', 'offset_1', 'offset_1', 0, 0),
    (2, 64, 30, 20, 'packed', 'packed', 'packed', 0, 0),
]


@pytest.mark.parametrize('B,L,A,D,lp,lx,ldp,soff,acc', BWD_CASES)
def test_score_backward_and_fused_backward_edges(dev, B, L, A, D, lp, lx, ldp, soff, acc):
    n = N()
    d = make_inputs(B, L, A, D, seed=L + A + D)
    al, _ = run_fwd(n, dev, d, 'pair')
    ref = attn_all(d, alpha=al)
    kw = dict(lp=lp, lx=lx, ldp=ldp, soff=soff)
    pair = run_bwd(n, dev, d, al, 'pair', acc=acc, **kw)
    check_bwd_fp64(pair, ref, d, acc)
    fused = run_bwd(n, dev, d, al, 'fused', acc=acc, **kw)
    assert same_results(fused, pair)
    if L == 1:                                     # alpha = 1, ds = 1 * (dalpha - dalpha) = 0
        for k in ('dproj', 'dhp', 'dwp'):
            assert bool((fused[k].double() - (d['base'].double() if acc and k == 'dproj' else 0.0) == 0).all())
    # in place: the layout of dproj is then proj's, so compare with an out-of-place run in that layout
    kw2 = dict(kw, ldp=lp)
    plain = run_bwd(n, dev, d, al, 'fused', **kw2)
    for form in ('pair', 'fused'):
        assert same_results(run_bwd(n, dev, d, al, form, inplace=True, **kw2), plain)
    for b in range(B):
        one = run_bwd(n, dev, rows(d, b), al[b:b + 1], 'fused', acc=acc, **kw)
        assert all(same_bits(one[k][0], fused[k][b]) for k in ('dproj', 'dhp', 'dwp'))


# =================================================================================================================
# 6. grouped and heterogeneous launches against one call per encoder
# =================================================================================================================
def run_multi(n, dev, ds, B, A, het, bo_null=False, x_off=None, acc=0, inplace=False):
    """ds: per-encoder inputs.  het: rfn_attn_fwd_het / _bwd_het (contiguous maps), else the grouped entries.
    x_off: index of the encoder whose att_seq sits one float off.  -> per encoder (alpha, z, backward dict)."""
    G, st = len(ds), n.stream_ptr()
    Ls, Ds = [d['proj'].shape[1] for d in ds], [d['x'].shape[2] for d in ds]
    P = [op3(d['proj'], dev) for d in ds]
    X = [Op(d['x'], dev, off=1 if g == x_off else 0) for g, d in enumerate(ds)]
    HP, W, BO = [Op(d['hp'], dev) for d in ds], [Op(d['w'], dev) for d in ds], [Op(d['bo'], dev) for d in ds]
    DZ = [Op(d['dz'], dev) for d in ds]
    RAW, AL = [Op(nans(B, L), dev) for L in Ls], [Op(nans(B, L), dev) for L in Ls]
    Z = [Op(nans(B, D), dev) for D in Ds]
    DP = P if inplace else [Op(d['base'] if acc else nans(B, L, A), dev) for d, L in zip(ds, Ls)]
    DHP, DWP = [Op(nans(B, A), dev) for _ in ds], [Op(nans(B, A), dev) for _ in ds]
    pa = lambda ops: n.ptr_array([o.v for o in ops])  # noqa: E731
    bo = None if bo_null else pa(BO)
    La, Da = (C.c_int * G)(*Ls), (C.c_int * G)(*Ds)
    if het:
        n.check(n.lib.rfn_attn_fwd_het(G, pa(P), pa(HP), pa(W), bo, pa(X), B, La, A, Da, pa(RAW), pa(AL), pa(Z), st))
    else:
        n.check(n.lib.rfn_attn_fwd_grouped(G, pa(P), Ls[0] * A, A, pa(HP), pa(W), bo, pa(X), Ls[0] * Ds[0], Ds[0], B, Ls[0],
                                           A, Ds[0], pa(RAW), pa(AL), pa(Z), Ds[0], st))
    finish(RAW + AL + Z, P + X + HP + W + BO)
    assert all(o.written() for o in RAW + AL + Z)
    AL = [o.freeze() for o in AL]
    if het:
        n.check(n.lib.rfn_attn_bwd_het(G, pa(P), pa(HP), pa(W), pa(AL), pa(X), pa(DZ), B, La, A, Da, pa(DP), acc, pa(DHP),
                                       pa(DWP), st))
    else:
        n.check(n.lib.rfn_attn_bwd_grouped(G, pa(P), Ls[0] * A, A, pa(HP), pa(W), pa(AL), pa(X), Ls[0] * Ds[0], Ds[0],
                                           pa(DZ), Ds[0], B, Ls[0], A, Ds[0], pa(DP), Ls[0] * A, A, acc, pa(DHP), pa(DWP), st))
    finish(DP + DHP + DWP, X + HP + W + DZ + AL)
    assert all(o.written() for o in DP + DHP + DWP)
    return [(AL[g].get(), Z[g].get(), dict(dproj=DP[g].get(), dhp=DHP[g].get(), dwp=DWP[g].get())) for g in range(G)]


HET_CASES = [
    # Ls, Ds, A, b_out NULL, encoder with a misaligned att_seq
    ((17, 3, 64), (1028, 6, 256), 64, False, None),          # one scalar encoder among vector ones: D = 6
    ((17, 3, 64), (1028, 6, 256), 30, True, None),           # ... and scalar scores
    ((5, 1030), (1028, 8), 64, False, None),                 # the widest and the longest map on different encoders
    ((17, 3, 64), (1028, 8, 256), 64, False, 1),             # a misaligned pointer forces every encoder onto the scalar grid
    ((1, 2, 3, 4, 5, 9, 16, 17), (4, 8, 1028, 256, 260, 12, 16, 20), 64, True, None),     # RFN_MAX_ENC encoders, all vector
    ((1, 2, 3, 4, 5, 9, 16, 17), (4, 8, 1, 256, 260, 12, 16, 300), 3, False, None),       # ... all scalar
]


@pytest.mark.parametrize('Ls,Ds,A,bo_null,x_off', HET_CASES)
def test_heterogeneous_launch_equals_per_encoder_calls(dev, Ls, Ds, A, bo_null, x_off):
    n, B = N(), 2
    ds = [make_inputs(B, L, A, D, seed=10 * g + L) for g, (L, D) in enumerate(zip(Ls, Ds))]
    got = run_multi(n, dev, ds, B, A, het=True, bo_null=bo_null, x_off=x_off)
    # all or nothing: one encoder off the 16-B conditions puts the context kernel and the dalpha part of every encoder on
    # the scalar instantiation; the per-encoder call takes the same one when its att_seq is misaligned
    scalar_x = x_off is not None or any(D % 4 for D in Ds)
    lx = 'offset_1' if scalar_x else 'packed'
    for g, d in enumerate(ds):
        dd = dict(d, bo=None) if bo_null else d
        al, z, bw = got[g]
        check_fwd_fp64(al, z, attn_all(dd))
        al1, z1 = run_fwd(n, dev, dd, 'fused', lx=lx)
        assert same_bits(al1, al) and same_bits(z1, z)
        check_bwd_fp64(bw, attn_all(dd, alpha=al), dd)
        assert same_results(run_bwd(n, dev, dd, al, 'fused', lx=lx), bw)
    inpl = run_multi(n, dev, ds, B, A, het=True, bo_null=bo_null, x_off=x_off, inplace=True)
    accd = run_multi(n, dev, ds, B, A, het=True, bo_null=bo_null, x_off=x_off, acc=1)
    for g, d in enumerate(ds):
        assert same_results(inpl[g][2], got[g][2])
        assert maxerr(accd[g][2]['dproj'], attn_all(dict(d, bo=None) if bo_null else d, alpha=got[g][0])['dproj']
                      + d['base'].double()) < TOL['dproj']


@pytest.mark.parametrize('G,L,A,D', [(MAX_ENC, 17, 64, 260), (2, 5, 30, 18), (3, 65, 260, 1028)])
def test_grouped_launch_equals_per_encoder_calls(dev, G, L, A, D):
    n, B = N(), 2
    ds = [make_inputs(B, L, A, D, seed=10 * g + 3) for g in range(G)]
    got = run_multi(n, dev, ds, B, A, het=False)
    inpl = run_multi(n, dev, ds, B, A, het=False, inplace=True)
    for g, d in enumerate(ds):
        al, z, bw = got[g]
        check_fwd_fp64(al, z, attn_all(d))
        al1, z1 = run_fwd(n, dev, d, 'fused')
        assert same_bits(al1, al) and same_bits(z1, z)
        check_bwd_fp64(bw, attn_all(d, alpha=al), d)
        assert same_results(run_bwd(n, dev, d, al, 'fused'), bw)
        assert same_results(inpl[g][2], bw)


# =================================================================================================================
# 7. fused small-L forward
# =================================================================================================================
SMALL_FWD_CASES = [
    # B, L, A, D, lp, lx, lz, soff
    (2, 1, 256, 256, 'packed', 'packed', 'packed', 0), (2, 3, 260, 516, 'padded4', 'padded4', 'padded4', 0),
    (3, 4, 256, 1, 'time_major', 'time_major', 'packed', 0), (2, 5, 260, 257, 'packed', 'packed', 'packed', 1),
    (2, 9, 256, 516, 'packed', 'ld_plus_1', 'ld_plus_1', 0), (1, 1024, 260, 1, 'packed', 'packed', 'packed', 0),
    (2, 1, 3, 1, 'packed', 'packed', 'packed', 0), (2, 3, 65, 257, 'padded4', 'offset_1', 'offset_1', 0),
    (2, 4, 256, 256, 'ld_plus_1', 'packed', 'packed', 0), (2, 5, 260, 516, 'offset_1', 'packed', 'packed', 0),
    (2, 9, 65, 256, 'time_major', 'time_major', 'padded4', 1), (1, 1024, 3, 4, 'packed', 'packed', 'packed', 0),
]


@pytest.mark.parametrize('B,L,A,D,lp,lx,lz,soff', SMALL_FWD_CASES)
def test_small_forward_edges(dev, B, L, A, D, lp, lx, lz, soff):
    n = N()
    d = make_inputs(B, L, A, D, seed=L + A + D)
    kw = dict(lp=lp, lx=lx, lz=lz, soff=soff)
    al, z = run_fwd(n, dev, d, 'small', **kw)
    assert not bool(torch.isnan(al).any()) and not bool(torch.isnan(z).any())
    check_fwd_fp64(al, z, attn_all(d))
    if L == 1:
        assert bool((al == 1.0).all()) and same_bits(z, d['x'][:, 0])
    for b in range(B):
        al1, z1 = run_fwd(n, dev, rows(d, b), 'small', **kw)
        assert same_bits(al1[0], al[b]) and same_bits(z1[0], z[b])


def run_small_groups(n, dev, ds, B, L, A, D, bo_null=False, acc=0, with_dx=True):
    """G encoders in one small forward + backward, thoughts time-major side by side as stage II lays them out:
    att_seq of encoder g = columns [g * D, (g + 1) * D) of an (L, B, G * D) buffer.  -> per encoder (alpha, z, bwd)."""
    G, st = len(ds), n.stream_ptr()
    xall = torch.cat([d['x'].transpose(0, 1) for d in ds], 2)              # (L, B, G * D)
    XA, DXA = Op(xall, dev), Op(torch.cat([d['xbase'].transpose(0, 1) for d in ds], 2), dev)
    ZA, DZA = Op(nans(B, G * D), dev), Op(torch.cat([d['dz'] for d in ds], 1), dev)
    P = [op3(d['proj'], dev) for d in ds]
    HP, W, BO = [Op(d['hp'], dev) for d in ds], [Op(d['w'], dev) for d in ds], [Op(d['bo'], dev) for d in ds]
    AL = [Op(nans(B, L), dev) for _ in ds]
    DP = [Op(d['base'] if acc else nans(B, L, A), dev) for d in ds]
    DHP, DWP = [Op(nans(B, A), dev) for _ in ds], [Op(nans(B, A), dev) for _ in ds]
    pa = lambda ops: n.ptr_array([o.v for o in ops])  # noqa: E731
    cols = lambda o: n.ptr_array([o.v[..., g * D:] for g in range(G)])  # noqa: E731
    n.check(n.lib.rfn_attn_small_fwd(G, pa(P), L * A, A, pa(HP), pa(W), None if bo_null else pa(BO), cols(XA), G * D,
                                     B * G * D, B, L, A, D, pa(AL), cols(ZA), G * D, st))
    finish(AL + [ZA], P + HP + W + BO + [XA])
    assert all(o.written() for o in AL + [ZA])
    AL = [o.freeze() for o in AL]
    n.check(n.lib.rfn_attn_small_bwd(G, pa(P), L * A, A, pa(HP), pa(W), pa(AL), cols(XA), G * D, B * G * D, cols(DZA), G * D,
                                     B, L, A, D, pa(DP), L * A, A, acc, pa(DHP), pa(DWP), cols(DXA) if with_dx else None, st))
    finish(DP + DHP + DWP + [DXA], P + HP + W + AL + [XA, DZA])
    assert all(o.written() for o in DP + DHP + DWP)
    if not with_dx:
        assert DXA.unchanged()
    z, dx = ZA.get(), DXA.get()
    return [(AL[g].get(), z[:, g * D:(g + 1) * D],
             dict(dproj=DP[g].get(), dhp=DHP[g].get(), dwp=DWP[g].get(), dx=dx[:, :, g * D:(g + 1) * D].transpose(0, 1)))
            for g in range(G)]


@pytest.mark.parametrize('G,L,A,D,bo_null', [(3, 5, 256, 256, False), (3, 9, 65, 257, True), (MAX_ENC, 4, 64, 4, False)])
def test_small_groups_equal_per_encoder_calls(dev, G, L, A, D, bo_null):
    n, B = N(), 2
    ds = [make_inputs(B, L, A, D, seed=7 * g + L) for g in range(G)]
    got = run_small_groups(n, dev, ds, B, L, A, D, bo_null=bo_null)
    nodx = run_small_groups(n, dev, ds, B, L, A, D, bo_null=bo_null, with_dx=False, acc=1)
    # one encoder alone, its thoughts time-major in a buffer of their own: rows of width D for G * D, the same alignment class
    for g, d in enumerate(ds):
        dd = dict(d, bo=None) if bo_null else d
        al, z, bw = got[g]
        check_fwd_fp64(al, z, attn_all(dd))
        ref = attn_all(dd, alpha=al)
        check_bwd_fp64(bw, ref, dd)
        al1, z1 = run_fwd(n, dev, dd, 'small', lx='time_major')
        assert same_bits(al1, al) and same_bits(z1, z)
        one = run_bwd(n, dev, dd, al, 'small', lx='time_major')
        assert same_results(one, bw, ('dproj', 'dhp', 'dwp', 'dx'))
        assert maxerr(nodx[g][2]['dproj'], ref['dproj'] + d['base'].double()) < TOL['dproj']


# =================================================================================================================
# 8. fused small-L backward: rows in pairs l, l + 4; d att_seq loop clamped at n4 - 1 once L * D / 4 > 1024; A > 1024
# =================================================================================================================
SMALL_BWD_CASES = [
    # B, L, A, D, layouts (lp, lx, ldp, ldhp, ldwp, ldx), soff, acc, d att_seq      -- vector instantiation
    (2, 1, 64, 8, {}, 0, 0, True), (2, 4, 1024, 8, {'lp': 'padded4', 'lx': 'padded4', 'ldp': 'padded4'}, 0, 1, True),
    (2, 5, 1028, 8, {}, 0, 0, False), (2, 8, 64, 512, {}, 0, 0, True), (2, 8, 64, 516, {}, 0, 1, True),
    (3, 9, 64, 16, {'lp': 'time_major', 'lx': 'time_major'}, 0, 0, True), (2, 12, 64, 8, {'ldp': 'time_major'}, 0, 1, False),
    (2, 13, 64, 260, {}, 0, 0, True),
    # scalar instantiation, one operand at a time
    (2, 8, 64, 516, {'lp': 'offset_1'}, 0, 0, True), (2, 13, 64, 8, {'lp': 'ld_plus_1'}, 0, 1, True),
    (2, 8, 64, 512, {'lx': 'offset_1', 'ldx': 'aligned'}, 0, 0, True), (2, 5, 1028, 8, {'lx': 'ld_plus_1'}, 0, 0, True),
    (2, 9, 64, 8, {'ldp': 'offset_1'}, 0, 1, True), (2, 4, 1024, 8, {'ldp': 'ld_plus_1'}, 0, 0, False),
    (2, 12, 64, 8, {'ldhp': 'offset_1'}, 0, 0, True), (2, 8, 64, 8, {'ldwp': 'offset_1'}, 0, 1, True),
    (2, 8, 64, 516, {'ldx': 'offset_1'}, 0, 0, True), (2, 1, 64, 8, {'ldx': 'offset_1'}, 0, 0, True),
    (2, 13, 64, 8, {}, 1, 0, True),                # dz with an odd lddz (and the scalar operands one float off)
    (2, 1, 3, 8, {}, 0, 0, True), (2, 5, 64, 18, {}, 0, 1, True), (2, 9, 3, 1, {}, 0, 0, False),
    (2, 4, 1028, 8, {'lp': 'offset_1'}, 0, 0, True), (2, 12, 1024, 6, {}, 0, 0, True),
]


@pytest.mark.parametrize('B,L,A,D,lay,soff,acc,want_dx', SMALL_BWD_CASES)
def test_small_backward_edges(dev, B, L, A, D, lay, soff, acc, want_dx):
    n = N()
    d = make_inputs(B, L, A, D, seed=L + A + D)
    al, _ = run_fwd(n, dev, d, 'small')
    ref = attn_all(d, alpha=al)
    kw = dict(lay, soff=soff, want_dx=want_dx)
    got = run_bwd(n, dev, d, al, 'small', acc=acc, **kw)
    check_bwd_fp64(got, ref, d, acc)
    if L == 1:
        for k in ('dproj', 'dhp', 'dwp'):
            assert bool((got[k] == 0).all())
    kw2 = dict(kw, ldp=lay.get('lp', 'packed'))
    keys = ('dproj', 'dhp', 'dwp') + (('dx',) if want_dx else ())
    plain = run_bwd(n, dev, d, al, 'small', **kw2)
    assert same_results(run_bwd(n, dev, d, al, 'small', inplace=True, **kw2), plain, keys)
    for b in range(B):
        one = run_bwd(n, dev, rows(d, b), al[b:b + 1], 'small', acc=acc, **kw)
        assert all(same_bits(one[k][0], got[k][b]) for k in keys)


# =================================================================================================================
# 9. exact consequences of the formulas; a NaN stays in its batch row
# =================================================================================================================
@pytest.mark.parametrize('L,A,D,lp', [(17, 64, 36, 'packed'), (5, 30, 18, 'packed'), (65, 64, 8, 'offset_1')])
def test_saturated_tanh_and_equal_scores_are_exact(dev, L, A, D, lp):
    n, B = N(), 2
    d = make_inputs(B, L, A, D, seed=L)
    # proj + hproj pinned at +-30, where 1 - 2 / (e^60 + 1) is exactly 1 in float32: 1 - e^2 = 0
    d['hp'] = torch.zeros(B, A)
    d['proj'] = torch.where(d['proj'] >= 0, torch.full((B, L, A), 30.0), torch.full((B, L, A), -30.0))
    for ff, fb in (('pair', 'pair'), ('fused', 'fused'), ('small', 'small')):
        al, _ = run_fwd(n, dev, d, ff, lp=lp)
        got = run_bwd(n, dev, d, al, fb, lp=lp)
        assert bool((got['dproj'] == 0).all()) and bool((got['dhp'] == 0).all())
        assert not bool(torch.isnan(got['dwp']).any())
    # equal scores (w_out = 0): alpha = 1 * (1 / sum of L ones), every one the float32 quotient 1 / L
    d = make_inputs(B, L, A, D, seed=L)
    d['w'] = torch.zeros(A)
    want = float(np.float32(1.0) / np.float32(L))
    for form in ('pair', 'fused', 'small'):
        al, z = run_fwd(n, dev, d, form, lp=lp)
        assert bool((al == want).all())


@pytest.mark.parametrize('L,A,D', [(17, 64, 36), (5, 30, 18)])
def test_a_nan_row_leaves_the_other_rows_alone(dev, L, A, D):
    n, B = N(), 3
    d = make_inputs(B, L, A, D, seed=L + 1)
    bad = dict(d, proj=d['proj'].clone())
    bad['proj'][1, L // 2, A // 2] = NAN
    for form in ('pair', 'fused', 'small'):
        al, z = run_fwd(n, dev, d, form)
        al2, z2 = run_fwd(n, dev, bad, form)
        assert bool(torch.isnan(al2[1]).any())
        for b in (0, 2):
            assert same_bits(al2[b], al[b]) and same_bits(z2[b], z[b])
        keys = ('dproj', 'dhp', 'dwp') + (('dx',) if form == 'small' else ())
        bw, bw2 = run_bwd_nocheck(n, dev, d, al, form), run_bwd_nocheck(n, dev, bad, al, form)
        for b in (0, 2):
            assert all(same_bits(bw2[k][b], bw[k][b]) for k in keys)


def run_bwd_nocheck(n, dev, d, al, form):
    """run_bwd for inputs that hold a NaN (its `everything was written` check counts NaNs)"""
    B, L, A = d['proj'].shape
    D, st = d['x'].shape[2], n.stream_ptr()
    P, X, HP, W, AL, DZ = [Op(t, dev) for t in (d['proj'], d['x'], d['hp'], d['w'], al, d['dz'])]
    DP, DHP, DWP, DAL, DX = Op(nans(B, L, A), dev), Op(nans(B, A), dev), Op(nans(B, A), dev), Op(nans(B, L), dev), Op(d['xbase'], dev)
    if form == 'pair':
        n.check(n.lib.rfn_attn_context_bwd_dalpha(X.ptr, L * D, D, DZ.ptr, D, B, L, D, DAL.ptr, st))
        n.check(n.lib.rfn_attn_scores_bwd(P.ptr, L * A, A, HP.ptr, W.ptr, AL.ptr, DAL.ptr, B, L, A, DP.ptr, L * A, A, 0, DHP.ptr,
                                          DWP.ptr, st))
    elif form == 'fused':
        n.check(n.lib.rfn_attn_bwd(P.ptr, L * A, A, HP.ptr, W.ptr, AL.ptr, X.ptr, L * D, D, DZ.ptr, D, B, L, A, D, DP.ptr, L * A,
                                   A, 0, DHP.ptr, DWP.ptr, st))
    else:
        pa = lambda o: n.ptr_array([o.v])  # noqa: E731
        n.check(n.lib.rfn_attn_small_bwd(1, pa(P), L * A, A, pa(HP), pa(W), pa(AL), pa(X), L * D, D, pa(DZ), D, B, L, A, D, pa(DP),
                                         L * A, A, 0, pa(DHP), pa(DWP), pa(DX), st))
    finish([DP, DHP, DWP, DAL, DX], [P, X, HP, W, AL, DZ])
    return dict(dproj=DP.get(), dhp=DHP.get(), dwp=DWP.get(), dx=DX.get())


# =================================================================================================================
# 10. new value regimes against 4x the fp32 restatement's own error
# =================================================================================================================
@pytest.mark.parametrize('shape', REGIME_SHAPES)
@pytest.mark.parametrize('regime', REGIMES)
def test_value_regimes_within_four_yardsticks(dev, regime, shape):
    n = N()
    B, L, A, D = shape
    d = regime_inputs(regime, *shape)
    ya, yz, ydp, ydh, ydw, ydx = YARD[(regime, shape)]
    ref = attn_all(d)
    for ff, fb in (('pair', 'pair'), ('fused', 'fused'), ('small', 'small')):
        al, z = run_fwd(n, dev, d, ff)
        got = run_bwd(n, dev, d, al, fb)
        # the kernel's backward is given the kernel's own alpha, as the restatement's backward uses its own
        errs = dict(alpha=maxerr(al, ref['alpha']), z=maxerr(z, ref['z']), dproj=maxerr(got['dproj'], ref['dproj']),
                    dhp=maxerr(got['dhp'], ref['dhp']), dw=maxerr(got['dwp'].double().sum(0), ref['dwp'].sum(0)))
        if 'dx' in got:
            errs['dx'] = maxerr(got['dx'], ref['dx'] + d['xbase'].double())
        print(regime, shape, ff, ' '.join('%s %.3g' % kv for kv in errs.items()))
        assert all(bool(torch.isfinite(v).all()) for v in list(got.values()) + [al, z])
        assert errs['alpha'] <= 4 * ya and errs['z'] <= 4 * yz
        assert errs['dproj'] <= 4 * ydp and errs['dhp'] <= 4 * ydh and errs['dw'] <= 4 * ydw
        if 'dx' in got:
            assert errs['dx'] <= 4 * ydx
        if regime == 'peak':                       # exact zeros wherever alpha underflowed
            dead = al == 0
            assert int(dead.sum()) == B * (L - 1)
            assert bool((got['dproj'][dead] == 0).all())
            if 'dx' in got:
                assert same_bits(got['dx'][dead], d['xbase'][dead])


# =================================================================================================================
# 11. limits: the largest accepted size runs and is right, the next one is refused before any launch
# =================================================================================================================
def refused(n, outs, rc, want=ERR_SHAPE):
    torch.cuda.synchronize()
    assert rc == want
    for o in outs:
        assert o.unchanged()


def test_context_length_limit(dev):
    """dynamic LDS of the context kernel: L floats <= 64 KiB -> L = 16384 runs (in the two-launch form next to its static
    red[4]), L = 16385 is refused with nothing launched, the raw-score scratch included."""
    n, st = N(), N().stream_ptr()
    B, A, D, L = 1, 4, 4, LDS_64K
    d = make_inputs(B, L, A, D, seed=5)
    ref = attn_all(d)
    for form in ('pair', 'fused'):
        al, z = run_fwd(n, dev, d, form)
        assert not bool(torch.isnan(al).any())
        check_fwd_fp64(al, z, ref)
    L1 = L + 1
    P, X, HP, W = Op(rnd(B, L1, A), dev), Op(rnd(B, L1, D), dev), Op(d['hp'], dev), Op(d['w'], dev)
    AL, RAW, Z = Op(torch.softmax(rnd(B, L1), 1), dev), Op(nans(B, L1), dev), Op(nans(B, D), dev)
    refused(n, [Z], n.lib.rfn_attn_context_fwd(X.ptr, L1 * D, D, AL.ptr, B, L1, D, Z.ptr, D, st))
    AL2 = Op(nans(B, L1), dev)
    refused(n, [Z, RAW, AL2], n.lib.rfn_attn_fwd(P.ptr, L1 * A, A, HP.ptr, W.ptr, None, X.ptr, L1 * D, D, B, L1, A, D, RAW.ptr,
                                                 AL2.ptr, Z.ptr, D, st))
    La, Da = (C.c_int * 1)(L1), (C.c_int * 1)(D)
    pa = lambda o: n.ptr_array([o.v])  # noqa: E731
    refused(n, [Z, RAW, AL2], n.lib.rfn_attn_fwd_het(1, pa(P), pa(HP), pa(W), None, pa(X), B, La, A, Da, pa(RAW), pa(AL2),
                                                     pa(Z), st))


def test_dalpha_width_limit(dev):
    n, st = N(), N().stream_ptr()
    B, L, D = 1, 2, LDS_64K                        # LDS: D floats rounded up to 4
    d = make_inputs(B, L, 4, D, seed=6)
    X, DZ, DAL = Op(d['x'], dev), Op(d['dz'], dev), Op(nans(B, L), dev)
    n.check(n.lib.rfn_attn_context_bwd_dalpha(X.ptr, L * D, D, DZ.ptr, D, B, L, D, DAL.ptr, st))
    finish([DAL], [X, DZ])
    want = (d['x'].double() * d['dz'].double()[:, None, :]).sum(2)
    mag = (d['x'].double().abs() * d['dz'].double().abs()[:, None, :]).sum(2)
    assert bool(((DAL.get().double() - want).abs() <= (D + 1) * U * mag).all())
    D1 = D + 1
    X, DZ, DAL = Op(rnd(B, L, D1), dev), Op(rnd(B, D1), dev), Op(nans(B, L), dev)
    refused(n, [DAL], n.lib.rfn_attn_context_bwd_dalpha(X.ptr, L * D1, D1, DZ.ptr, D1, B, L, D1, DAL.ptr, st))


def test_score_forward_width_limit(dev):
    n, st = N(), N().stream_ptr()
    B, L, A = 1, 3, LDS_64K // 2                   # LDS: 2 * Ap floats
    d = make_inputs(B, L, A, 4, seed=7)
    d['w'] = d['w'] * 0.1                          # keep the scores at the scale the tolerances are stated for
    al, z = run_fwd(n, dev, d, 'fused')
    check_fwd_fp64(al, z, attn_all(d))
    A1 = A + 1
    P, HP, W, AL = Op(rnd(B, L, A1), dev), Op(rnd(B, A1), dev), Op(rnd(A1), dev), Op(nans(B, L), dev)
    refused(n, [AL], n.lib.rfn_attn_scores_fwd(P.ptr, L * A1, A1, HP.ptr, W.ptr, None, B, L, A1, AL.ptr, st))


def test_score_backward_lds_limit(dev):
    """34 * Ap + 16 + L floats (score backward), 34 * Ap + 16 + 2 * Lp + Dp (fused) <= 150 KiB = 38400 floats."""
    n, st = N(), N().stream_ptr()
    B, A = 1, 1128
    L, Lf, D = LDS_150K - 34 * A - 16, 4, 24
    assert (L, 34 * A + 16 + 2 * Lf + D) == (32, LDS_150K)
    d = make_inputs(B, L, A, 4, seed=8)
    d['w'] = d['w'] * 0.3
    al, _ = run_fwd(n, dev, d, 'pair')
    check_bwd_fp64(run_bwd(n, dev, d, al, 'pair'), attn_all(d, alpha=al), d)
    d = make_inputs(B, Lf, A, D, seed=9)
    d['w'] = d['w'] * 0.3
    al, _ = run_fwd(n, dev, d, 'pair')
    check_bwd_fp64(run_bwd(n, dev, d, al, 'fused'), attn_all(d, alpha=al), d)
    # one row / one column more
    L1 = L + 1
    P, HP, W, AL, DAL = Op(rnd(B, L1, A), dev), Op(rnd(B, A), dev), Op(rnd(A), dev), Op(rnd(B, L1), dev), Op(rnd(B, L1), dev)
    DP, DHP, DWP = Op(nans(B, L1, A), dev), Op(nans(B, A), dev), Op(nans(B, A), dev)
    refused(n, [DP, DHP, DWP], n.lib.rfn_attn_scores_bwd(P.ptr, L1 * A, A, HP.ptr, W.ptr, AL.ptr, DAL.ptr, B, L1, A, DP.ptr, L1 * A,
                                                         A, 0, DHP.ptr, DWP.ptr, st))
    D1 = D + 1
    X, DZ = Op(rnd(B, Lf, D1), dev), Op(rnd(B, D1), dev)
    refused(n, [DP, DHP, DWP], n.lib.rfn_attn_bwd(P.ptr, Lf * A, A, HP.ptr, W.ptr, AL.ptr, X.ptr, Lf * D1, D1, DZ.ptr, D1, B, Lf, A,
                                                  D1, DP.ptr, Lf * A, A, 0, DHP.ptr, DWP.ptr, st))


def test_small_attention_limits(dev):
    """L <= 1024; forward LDS 2 * Ap + L floats, backward 2 * Ap + Dp + 2 * Lp floats, both <= 64 KiB = 16384 floats."""
    n, st = N(), N().stream_ptr()
    pa = lambda o: n.ptr_array([o.v]) if o is not None else None  # noqa: E731

    def small_fwd_rc(B, L, A, D):
        P, HP, W, X = Op(rnd(B, L, A), dev), Op(rnd(B, A), dev), Op(rnd(A), dev), Op(rnd(B, L, D), dev)
        AL, Z = Op(nans(B, L), dev), Op(nans(B, D), dev)
        return [AL, Z], n.lib.rfn_attn_small_fwd(1, pa(P), L * A, A, pa(HP), pa(W), None, pa(X), L * D, D, B, L, A, D, pa(AL),
                                                 pa(Z), D, st)

    def small_bwd_rc(B, L, A, D):
        P, HP, W, X = Op(rnd(B, L, A), dev), Op(rnd(B, A), dev), Op(rnd(A), dev), Op(rnd(B, L, D), dev)
        AL, DZ, DX = Op(rnd(B, L), dev), Op(rnd(B, D), dev), Op(rnd(B, L, D), dev)
        DP, DHP, DWP = Op(nans(B, L, A), dev), Op(nans(B, A), dev), Op(nans(B, A), dev)
        return [DP, DHP, DWP, DX], n.lib.rfn_attn_small_bwd(1, pa(P), L * A, A, pa(HP), pa(W), pa(AL), pa(X), L * D, D, pa(DZ), D,
                                                            B, L, A, D, pa(DP), L * A, A, 0, pa(DHP), pa(DWP), pa(DX), st)
    # the longest row (forward and backward); L = 1024 itself runs in test_small_forward_edges too
    d = make_inputs(1, 1024, 8, 4, seed=11)
    al, z = run_fwd(n, dev, d, 'small')
    check_fwd_fp64(al, z, attn_all(d))
    check_bwd_fp64(run_bwd(n, dev, d, al, 'small'), attn_all(d, alpha=al), d)
    refused(n, *small_fwd_rc(1, 1025, 8, 4))
    refused(n, *small_bwd_rc(1, 1025, 8, 4))
    # forward LDS: A = 8188, L = 8 -> 16384 floats
    A, L = 8188, 8
    assert 2 * up4(A) + L == LDS_64K
    d = make_inputs(1, L, A, 4, seed=12)
    d['w'] = d['w'] * 0.1
    al, z = run_fwd(n, dev, d, 'small')
    check_fwd_fp64(al, z, attn_all(d))
    refused(n, *small_fwd_rc(1, L + 1, A, 4))
    # backward LDS: A = 8184, D = 8, L = 4 -> 16384 floats
    A, D, L = 8184, 8, 4
    assert 2 * up4(A) + up4(D) + 2 * up4(L) == LDS_64K
    d = make_inputs(1, L, A, D, seed=13)
    d['w'] = d['w'] * 0.1
    al, _ = run_fwd(n, dev, d, 'small')
    check_bwd_fp64(run_bwd(n, dev, d, al, 'small'), attn_all(d, alpha=al), d)
    refused(n, *small_bwd_rc(1, L, A, D + 1))
    refused(n, *small_bwd_rc(1, L + 1, A, D))


# =================================================================================================================
# 12. rfn_attn_bwd_grouped_ks: layout and offsets of the plane images
# =================================================================================================================
@pytest.mark.parametrize('L', [1, 17])
@pytest.mark.parametrize('col0', ['0', 'A', 'mp-A'])
def test_plane_image_backward_layout_and_offsets(dev, L, col0):
    n, st = N(), N().stream_ptr()
    G, B, A, D = 2, 2, 64, 8
    K, cols = B * L, 3 * A
    mp = (cols + 255) // 256 * 256                 # 256 > the 192 columns used
    c0 = {'0': 0, 'A': A, 'mp-A': mp - A}[col0]
    ds = [make_inputs(B, L, A, D, seed=3 * g + L) for g in range(G)]
    al = [torch.softmax(rnd(B, L, seed=40 + g), 1) for g in range(G)]
    P, HP, W = [Op(d['proj'], dev) for d in ds], [Op(d['hp'], dev) for d in ds], [Op(d['w'], dev) for d in ds]
    X, DZ, AL = [Op(d['x'], dev) for d in ds], [Op(d['dz'], dev) for d in ds], [Op(a, dev) for a in al]
    DP, DHP, DWP = [Op(nans(B, L, A), dev) for _ in ds], [Op(nans(B, A), dev) for _ in ds], [Op(nans(B, A), dev) for _ in ds]
    DHP2, DWP2 = [Op(nans(B, A), dev) for _ in ds], [Op(nans(B, A), dev) for _ in ds]
    pa = lambda ops: n.ptr_array([o.v for o in ops])  # noqa: E731
    n.check(n.lib.rfn_attn_bwd_grouped(G, pa(P), L * A, A, pa(HP), pa(W), pa(AL), pa(X), L * D, D, pa(DZ), D, B, L, A, D, pa(DP),
                                       L * A, A, 0, pa(DHP), pa(DWP), st))
    nbytes = n.lib.rfn_x3_image_bytes(cols, K)
    k_pad = nbytes // (6 * mp)
    assert nbytes == k_pad * mp * 6 and k_pad >= K
    imgs = [torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev) for _ in range(G)]
    before = [i.clone() for i in imgs]

    def call(A_=A, mp_=mp, c0_=c0, proj=None):
        return n.lib.rfn_attn_bwd_grouped_ks(G, proj or pa(P), L * A_, A_, pa(HP), pa(W), pa(AL), pa(X), L * D, D, pa(DZ), D, B, L,
                                             A_, D, n.ptr_array(imgs), mp_, c0_, pa(DHP2), pa(DWP2), st)
    # refused before any launch
    Pm = [Op(d['proj'], dev, off=1) for d in ds]
    for rc in (call(c0_=c0 + 2), call(mp_=mp + 2), call(A_=A - 2), call(proj=pa(Pm)), call(c0_=mp - A + 4)):
        torch.cuda.synchronize()
        assert rc == ERR_SHAPE
        assert all(torch.equal(i, b) for i, b in zip(imgs, before)) and all(o.unchanged() for o in DHP2 + DWP2)
    n.check(call())
    finish(DHP2 + DWP2, P + HP + W + X + DZ + AL)
    for g in range(G):
        w16 = imgs[g].view(torch.int16).view(k_pad, 3, mp)
        b16 = before[g].view(torch.int16).view(k_pad, 3, mp)
        keep = torch.ones(k_pad, 3, mp, dtype=torch.bool, device=dev)
        keep[:K, :, c0:c0 + A] = False
        assert torch.equal(w16[keep], b16[keep])   # every other column and row of the image is untouched
        planes = (w16[:K, :, c0:c0 + A].to(torch.int32) << 16).view(torch.float32).double().sum(1).cpu()
        want = DP[g].get().reshape(K, A).double()
        # the bound test_x3_gpu.py states: the two instantiations contract 1 - t * t differently, one rounding apart
        assert float((planes - want).abs().max()) <= 1.2e-7 * float(want.abs().max())
        for u, v in ((DHP[g].get(), DHP2[g].get()), (DWP[g].get(), DWP2[g].get())):
            assert float((u - v).abs().max()) <= 1e-6 * float(u.abs().max())


# =================================================================================================================
# 13. argument errors: nothing is launched
# =================================================================================================================
def test_argument_errors_launch_nothing(dev):
    n, st = N(), N().stream_ptr()
    B, L, A, D = 2, 5, 8, 8
    d = make_inputs(B, L, A, D)
    P, X, HP, W, BO, DZ = [Op(d[k], dev) for k in ('proj', 'x', 'hp', 'w', 'bo', 'dz')]
    AL, DAL = Op(torch.softmax(rnd(B, L), 1), dev), Op(rnd(B, L), dev)
    o_al, o_raw, o_z, o_dal = Op(nans(B, L), dev), Op(nans(B, L), dev), Op(nans(B, D), dev), Op(nans(B, L), dev)
    o_dp, o_dhp, o_dwp, o_dx = Op(nans(B, L, A), dev), Op(nans(B, A), dev), Op(nans(B, A), dev), Op(d['xbase'], dev)
    outs = [o_al, o_raw, o_z, o_dal, o_dp, o_dhp, o_dwp, o_dx]
    lib = n.lib
    p1 = lambda o: n.ptr_array([o.v if o is not None else None])  # noqa: E731
    La, Da = (C.c_int * 1)(L), (C.c_int * 1)(D)
    bad = lambda v: (C.c_int * 1)(v)  # noqa: E731

    def variants(args, ptr_idx, ext_idx, null):
        """every required pointer NULL in turn -> ERR_ARG; every extent 0 and -1 in turn -> ERR_SHAPE"""
        for i in ptr_idx:
            a = list(args)
            a[i] = null(a[i])
            yield a, ERR_ARG
        for i in ext_idx:
            for v in (0, -1):
                a = list(args)
                a[i] = bad(v) if isinstance(a[i], C.Array) else v
                yield a, ERR_SHAPE

    none = lambda a: None  # noqa: E731
    arr_none = lambda a: n.ptr_array([None])  # noqa: E731
    table = [
        (lib.rfn_attn_scores_fwd, [P.ptr, L * A, A, HP.ptr, W.ptr, BO.ptr, B, L, A, o_al.ptr, st], (0, 3, 4, 9), (6, 7, 8), none),
        (lib.rfn_attn_context_fwd, [X.ptr, L * D, D, AL.ptr, B, L, D, o_z.ptr, D, st], (0, 3, 7), (4, 5, 6), none),
        (lib.rfn_attn_fwd, [P.ptr, L * A, A, HP.ptr, W.ptr, BO.ptr, X.ptr, L * D, D, B, L, A, D, o_raw.ptr, o_al.ptr, o_z.ptr, D, st],
         (0, 3, 4, 6, 13, 14, 15), (9, 10, 11, 12), none),
        (lib.rfn_attn_context_bwd_dalpha, [X.ptr, L * D, D, DZ.ptr, D, B, L, D, o_dal.ptr, st], (0, 3, 8), (5, 6, 7), none),
        (lib.rfn_attn_context_bwd_dseq, [AL.ptr, DZ.ptr, D, B, L, D, o_dx.ptr, L * D, D, st], (0, 1, 6), (3, 4, 5), none),
        (lib.rfn_attn_scores_bwd, [P.ptr, L * A, A, HP.ptr, W.ptr, AL.ptr, DAL.ptr, B, L, A, o_dp.ptr, L * A, A, 0, o_dhp.ptr,
                                   o_dwp.ptr, st], (0, 3, 4, 5, 6, 10, 14, 15), (7, 8, 9), none),
        (lib.rfn_attn_bwd, [P.ptr, L * A, A, HP.ptr, W.ptr, AL.ptr, X.ptr, L * D, D, DZ.ptr, D, B, L, A, D, o_dp.ptr, L * A, A, 0,
                            o_dhp.ptr, o_dwp.ptr, st], (0, 3, 4, 5, 6, 9, 15, 19, 20), (11, 12, 13, 14), none),
    ]
    grouped = [
        (lib.rfn_attn_fwd_grouped, [1, p1(P), L * A, A, p1(HP), p1(W), p1(BO), p1(X), L * D, D, B, L, A, D, p1(o_raw), p1(o_al),
                                    p1(o_z), D, st], (1, 4, 5, 7, 14, 15, 16), (10, 11, 12, 13)),
        (lib.rfn_attn_bwd_grouped, [1, p1(P), L * A, A, p1(HP), p1(W), p1(AL), p1(X), L * D, D, p1(DZ), D, B, L, A, D, p1(o_dp),
                                    L * A, A, 0, p1(o_dhp), p1(o_dwp), st], (1, 4, 5, 6, 7, 10, 16, 20, 21), (12, 13, 14, 15)),
        (lib.rfn_attn_fwd_het, [1, p1(P), p1(HP), p1(W), p1(BO), p1(X), B, La, A, Da, p1(o_raw), p1(o_al), p1(o_z), st],
         (1, 2, 3, 5, 10, 11, 12), (6, 7, 8, 9)),
        (lib.rfn_attn_bwd_het, [1, p1(P), p1(HP), p1(W), p1(AL), p1(X), p1(DZ), B, La, A, Da, p1(o_dp), 0, p1(o_dhp), p1(o_dwp),
                                st], (1, 2, 3, 4, 5, 6, 11, 13, 14), (7, 8, 9, 10)),
        (lib.rfn_attn_small_fwd, [1, p1(P), L * A, A, p1(HP), p1(W), p1(BO), p1(X), L * D, D, B, L, A, D, p1(o_al), p1(o_z), D, st],
         (1, 4, 5, 7, 14, 15), (10, 11, 12, 13)),
        (lib.rfn_attn_small_bwd, [1, p1(P), L * A, A, p1(HP), p1(W), p1(AL), p1(X), L * D, D, p1(DZ), D, B, L, A, D, p1(o_dp), L * A,
                                  A, 0, p1(o_dhp), p1(o_dwp), p1(o_dx), st], (1, 4, 5, 6, 7, 10, 16, 20, 21), (12, 13, 14, 15)),
    ]
    count = 0
    for fn, args, ptr_idx, ext_idx, null in table:
        for a, want in variants(args, ptr_idx, ext_idx, null):
            assert fn(*a) == want, (fn.__name__, a, want)
            count += 1
    for fn, args, ptr_idx, ext_idx in grouped:
        for null in (none, arr_none):              # the host array itself missing / its entry NULL
            for a, want in variants(args, ptr_idx, ext_idx, null):
                assert fn(*a) == want, (fn.__name__, a, want)
                count += 1
        for ng in (0, MAX_ENC + 1):
            assert fn(*([ng] + args[1:])) == ERR_SHAPE, fn.__name__
    # the raw-score scratch must not be alpha
    assert lib.rfn_attn_fwd(P.ptr, L * A, A, HP.ptr, W.ptr, BO.ptr, X.ptr, L * D, D, B, L, A, D, o_al.ptr, o_al.ptr, o_z.ptr, D,
                            st) == ERR_ARG
    assert lib.rfn_attn_fwd_grouped(1, p1(P), L * A, A, p1(HP), p1(W), p1(BO), p1(X), L * D, D, B, L, A, D, p1(o_al), p1(o_al),
                                    p1(o_z), D, st) == ERR_ARG
    assert lib.rfn_attn_fwd_het(1, p1(P), p1(HP), p1(W), p1(BO), p1(X), B, La, A, Da, p1(o_al), p1(o_al), p1(o_z), st) == ERR_ARG
    torch.cuda.synchronize()
    assert count > 150
    for o in outs:
        assert o.unchanged()


if __name__ == '__main__':
    print_table()
