"""The hoisted decoder cell (csrc/rfn_deccell.hip, csrc/rfn_deccell_body.h; C ABI rfn_dec_cell_fwd, rfn_dec_attn_bwd,
rfn_dec_du) swept over the shapes, strides and pointer alignments at which a launcher picks another kernel or a loop takes
another trip.  The cases, the model of the launchers that says which kernel a case reaches, the inputs and the yardsticks
are in tests/deccell_cases.py (tests/test_deccell_cases_cpu.py proves the coverage without a GPU); the number of compute
units the launchers size their blocks by is read from the device.

Conventions (those of tests/test_attention_edges_gpu.py, whose Op carves the operands): every operand lies in a NaN-filled
device buffer with 8 floats in front and behind; after a call everything outside an output's elements must hold the same
bits, every output element must have been written, no input may have changed.  A refused call must leave every output as
it was.

What is asserted
* fp64 parity with the reference's un-hoisted formulas (ref_cell of tests/test_deccell_gpu.py; autograd through them for
  the backward) at that file's tolerances in its regime; in a new regime (L > 17, A > 512, GD > 2560, saturated, small,
  b_out = +-1e4) 4 x the fp32 yardstick of tests/deccell_cases.py (YARD_FWD / YARD_BWD there).
* what the sources state as bit-identity, as bit-identity: a row's gates, c, alpha, h (with and without dropout) on the fast
  kernel at 1 / 2 / 4 threads per unit, on the general kernel with 16-byte score reads at 64 / 128 / 256 threads, inside any
  batch; the same units in another block; in place == out of place; b_out NULL == b_out {0}; alpha == rfn_attn_small_fwd's;
  U = 0, b_z = 0 == rfn_lstm_fwd's gates (c, h to rounding: see the test); dhproj / dw_part whatever accumulate; row b == that row
  alone; the two dU kernels.  (The fast backward body and dec_attn_bwd_k<true, true> are the same formulas but not the same
  bits -- the compiler's contraction differs -- and are held to fp64 and to each other at the tolerance: see test_backward_edges.)
* accumulate: dproj is prior + overwrite to half an ulp of each (one fma: see test_backward_edges), not in bits.
* exact consequences: L = 1 -> alpha 1 and a zero attention gradient; w_out = 0 -> alpha = fl(1 / L); maxout ties -> 0.5;
  dgates = 0 -> zero gradients; the kept units are rfn_dropout_mask's over b * R + unit at an offset above 2^32.
* rfn_dec_du against the worst case of any summation order, (S + 1) * 2^-24 * sum_s |alpha * dgates| per element.

Layouts: packed, padded4, ld_plus_1, offset_1, time_major for the operands with strides; `soff` puts b_z, b_out, alpha (and
rfn_dec_du's alpha and dgates) one float off; hproj and w_out have offsets of their own (hp_off, w_off), because one float
there is what moves a forward or backward call off its fast kernel.

A departure from tests/test_attention_edges_gpu.py, stated plainly: that file measures a yardstick on the very inputs of its
case; here a yardstick is the maximum over 16 freshly drawn batch rows of the case's shape (YARD_ROWS of tests/deccell_cases.py),
while the device runs the case's own 1 to 7 rows.  The bar is therefore not the fp32 error on the inputs the kernel sees, and it
is larger than the figure those few rows alone give: with two softmax rows (A = 516, L = 2) the maximum of the fp32 error came
out at a tenth of its 16-row value.  The dropped-term check of tests/test_deccell_cases_cpu.py holds at 4 x these yardsticks.
"""
import numpy as np
import pytest
import torch

import deccell_cases as DC
from test_attention_edges_gpu import ERR_ARG, ERR_SHAPE, N, Op, finish, maxerr, nans, op2, op3, same_bits
from test_deccell_gpu import ref_cell

pytestmark = pytest.mark.gpu

NG_KEYS = ('gates', 'c', 'h', 'alpha')


def cus_of(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def dd(t):
    return t.double()


def held(name, key, err, bar):
    print('%-16s %-6s err %.3g  allowed %.3g' % (name, key, err, bar))
    return err < bar


# =================================================================================================================
# forward runner
# =================================================================================================================
def run_cell(n, dev, c, d, inplace=False, h_old=False, bo_zero=False, drop=None, seed=DC.DROP_SEED, offset=DC.DROP_OFF,
             expect=0, override=None, null=None):
    """One rfn_dec_cell_fwd of resolved case `c` on inputs `d`, every guard checked.  inplace: c_next is c_prev.  h_old: h_next is
    a buffer that holds finite values (the previous h of a decoder that steps in place).  bo_zero: a NULL b_out is replaced by
    {0}.  override: ABI scalars to replace (L, A, drop_p, row_div); null: name of a pointer passed as NULL; expect: the return
    code -- a refused call must leave every output untouched.  -> dict(gates, c, h, alpha) on the CPU"""
    B, L, A, R, mo = c['B'], c['L'], c['A'], c['R'], c['maxout']
    p = c['drop'] if drop is None else drop
    P, UO = op3(d['proj'], dev, c['lp']), op3(d['U'], dev, c['lu'])
    so = c['soff']                                 # the operands only ever read or written as scalars, one float off
    HP, W, BZ = Op(d['hp'], dev, off=c['hp_off']), Op(d['w'], dev, off=c['w_off']), Op(d['bz'], dev, off=so)
    bo = d['bo'] if d['bo'] is not None else (torch.zeros(1) if bo_zero else None)
    BO = Op(bo, dev, off=so) if bo is not None else None
    G, C0 = op2(d['gin'], dev, c['lg']), op2(d['c0'], dev, c['lcp'])
    C1 = C0 if inplace else op2(nans(B, R), dev, c['lcn'])
    H1 = op2(DC.rnd(B, R, seed=77) if h_old else nans(B, R), dev, c['lh'])
    AL = Op(nans(B, L), dev, off=so)
    ptr = dict(proj=P.ptr, hproj=HP.ptr, w_out=W.ptr, b_out=BO.ptr if BO else None, U=UO.ptr, bz=BZ.ptr, gates=G.ptr,
               c_prev=C0.ptr, c_next=C1.ptr, h_next=H1.ptr, alpha=AL.ptr)
    if null:
        ptr[null] = None
    s = dict(dict(L=L, A=A, drop_p=p, row_div=c['row_div'], B=B), **(override or {}))
    rc = n.lib.rfn_dec_cell_fwd(ptr['proj'], P.strides[0], P.strides[1], ptr['hproj'], ptr['w_out'], ptr['b_out'], ptr['U'],
                                UO.strides[0], UO.strides[1], ptr['bz'], ptr['gates'], G.strides[0], ptr['c_prev'], C0.strides[0],
                                ptr['c_next'], C1.strides[0], ptr['h_next'], H1.strides[0], ptr['alpha'], s['B'], s['L'], s['A'], R, mo,
                                s['row_div'], s['drop_p'], seed, offset, n.stream_ptr())
    assert rc == expect, (rc, expect)
    ins = [P, UO, HP, W, BZ] + ([BO] if BO else []) + ([] if inplace else [C0])
    if rc != 0:
        finish([], ins + [G, C1, H1, AL])
        return None
    finish([G, C1, H1, AL], ins)
    assert C1.written() and H1.written() and AL.written() and G.written()
    return dict(gates=G.get(), c=C1.get(), h=H1.get(), alpha=AL.get())


def keep_mask(n, dev, B, R, p, seed=DC.DROP_SEED, offset=DC.DROP_OFF):
    keep = torch.empty(B * R, device=dev)
    n.check(n.lib.rfn_dropout_mask(seed, offset, B * R, p, keep.data_ptr(), n.stream_ptr()), 'mask')
    return keep.view(B, R).cpu()


def check_cell(n, dev, c, d, out):
    """fp64 parity of one forward: the existing tolerances in their regime, 4 x the yardstick elsewhere"""
    B, R, mo, p = c['B'], c['R'], c['maxout'], c['drop']
    if c['regime'] == 'std':
        vx = dd(d['v']).repeat_interleave(c['row_div'], 0)[:B]
        bo = dd(d['bo']) if d['bo'] is not None else torch.zeros(1, dtype=torch.float64)
        alpha, sig, g, c1, h1, sums = ref_cell(vx, dd(d['Wa']), dd(d['ba']), dd(d['hp']), dd(d['w']), bo, dd(d['Wz']), dd(d['bz']),
                                               dd(d['gin']), dd(d['c0']), mo)
        ref, bar = dict(alpha=alpha, sig=sig, g=g, c=c1, h=h1), DC.TOL
    else:
        ref = DC.cell_formulas(d)
        sums = ref['pre']
        bar = dict(zip(DC.FWD_KEYS, (DC.YARD_FACTOR * y for y in DC.YARD_FWD[c['name']])))
    gates = out['gates']
    got = dict(alpha=out['alpha'], sig=gates[:, :3 * R], g=gates[:, 3 * R:4 * R], c=out['c'], h=out['h'])
    hbar = bar['h']
    if p > 0:                                      # h = dropout(o tanh c): the published mask, the kept units scaled by 1 / (1 - p)
        keep = keep_mask(n, dev, B, R, p)
        assert 0.5 < float(keep.mean()) < 0.95
        ref = dict(ref, h=ref['h'] * keep.double() / (1.0 - p))
        hbar = bar['h'] / (1.0 - p)
        assert torch.equal(out['h'] == 0, (keep == 0) | (ref['h'] == 0))
    ok = [held(c['name'], k, maxerr(got[k], ref[k]), hbar if k == 'h' else bar[k]) for k in DC.FWD_KEYS]
    assert all(ok), dict(zip(DC.FWD_KEYS, ok))
    if mo:                                         # chunk 4 keeps the selector: 1 / 0 where the candidates differ, 0.5 on a tie
        s3, s4 = sums[:, 3 * R:4 * R], sums[:, 4 * R:]
        clear = (s3 - s4).abs() > 1e-4
        sel = torch.where(s3 > s4, 1.0, 0.0)
        assert torch.equal(gates[:, 4 * R:][clear].double(), sel[clear])
        assert float((gates[:, 4 * R:4 * R + 3] - 0.5).abs().max()) == 0.0
    if c['L'] == 1:
        assert bool((out['alpha'] == 1.0).all())


def same_out(a, b, keys=NG_KEYS, rows=None):
    for k in keys:
        x, y = (a[k], b[k]) if rows is None else (a[k][:rows], b[k][:rows])
        if not same_bits(x, y):
            return False
    return True


# =================================================================================================================
# 1. forward: every instantiation and layout against fp64; in place, NULL b_out
# =================================================================================================================
@pytest.mark.parametrize('name', [c['name'] for c in DC.FWD_CASES])
def test_forward_edges(dev, name):
    n = N()
    c, plan, _ = DC.fwd_geometry(DC.FWD_BY_NAME[name], cus_of(dev))
    assert plan['kernel'] != 'refused'
    d = DC.fwd_inputs(c)
    out = run_cell(n, dev, c, d)
    check_cell(n, dev, c, d, out)
    # the free-running decoders step in place: c_next is c_prev, h_next the buffer of the previous h
    assert same_out(run_cell(n, dev, c, d, inplace=True), out)
    assert same_out(run_cell(n, dev, c, d, h_old=True), out)
    if d['bo'] is None:
        assert same_out(run_cell(n, dev, c, d, bo_zero=True), out)


# =================================================================================================================
# 2. a row's bits depend neither on the kernel, nor on the threads per unit, nor on the block size, nor on the batch
# =================================================================================================================
@pytest.mark.parametrize('maxout', [0, 1])
@pytest.mark.parametrize('drop', [0.0, DC.DROP_P])
def test_a_rows_bits_do_not_depend_on_kernel_threads_per_unit_block_size_or_batch(dev, maxout, drop):
    n, cus = N(), cus_of(dev)
    base = None
    want = [('cus', 0, 0, 'fast', 1), ('half', 0, 0, 'fast', 2), (2, 0, 0, 'fast', 4), (5, 0, 0, 'fast', 4),
            ('cus', 1, 0, 'general', 256), ('half', 0, 1, 'general', 128), (2, 1, 0, 'general', 64), (3, 1, 1, 'general', 64)]
    outs = []
    for Bs, hp_off, w_off, kernel, width in want:
        c, plan, _ = DC.fwd_geometry(DC.F('row', Bs, 8, 512, 256, maxout=maxout, hp_off=hp_off, w_off=w_off, drop=drop, lh='padded4'),
                                     cus)
        assert plan['kernel'] == kernel and plan.get('tpu', plan.get('ub')) == width and plan.get('vecA', True)
        d = DC.fwd_inputs(c)
        if base is None:
            base = {k: d[k][:2].clone() for k in ('hp', 'gin', 'c0')}
        for k, v in base.items():                  # rows 0 and 1 of every batch are the same two rows
            d[k][:2] = v
        outs.append(run_cell(n, dev, c, d))
    for o in outs[1:]:
        assert same_out(o, outs[0], rows=2)
    if drop:
        assert bool((outs[0]['h'][:2] == 0).any())


@pytest.mark.parametrize('maxout', [0, 1])
@pytest.mark.parametrize('hp_off', [0, 1])
def test_a_units_bits_do_not_depend_on_the_block_it_sits_in(dev, maxout, hp_off):
    """units 256..511 of an R = 512 call against the same units re-laid as an R = 256 call (without dropout: its counter is
    b * R + unit)"""
    n, cus, NG = N(), cus_of(dev), 5 if maxout else 4
    c, plan, _ = DC.fwd_geometry(DC.F('wide', 3, 8, 256, 512, maxout=maxout, row_div=2, hp_off=hp_off), cus)
    assert plan['kernel'] == ('general' if hp_off else 'fast') and plan['blocks'] == 8
    d = DC.fwd_inputs(c)
    big = run_cell(n, dev, c, d)
    cols = torch.cat([torch.arange(g * 512 + 256, g * 512 + 512) for g in range(NG)])
    c2 = dict(c, R=256)
    d2 = dict(d, U=d['U'][:, :, cols].contiguous(), bz=d['bz'][cols].contiguous(), gin=d['gin'][:, cols].contiguous(),
              c0=d['c0'][:, 256:].contiguous())
    small = run_cell(n, dev, c2, d2)
    assert same_bits(small['gates'], big['gates'][:, cols]) and same_bits(small['alpha'], big['alpha'])
    assert same_bits(small['c'], big['c'][:, 256:]) and same_bits(small['h'], big['h'][:, 256:])


# =================================================================================================================
# 3. alpha is rfn_attn_small_fwd's; with U = 0 and b_z = 0 the cell is rfn_lstm_fwd
# =================================================================================================================
@pytest.mark.parametrize('name', ['fast_r512_L2', 'fast_L3', 'L9', 'A516', 'scal_small', 'scal_tm_A256', 'scal_off_A260', 'L9_r512'])
def test_alpha_is_the_alpha_of_the_small_attention(dev, name):
    """`the arithmetic of attn_small_fwd_body`: both entries decide on 16-byte score reads from A and proj alone, so the same
    proj puts both on the same path (row_div = 1 here: the small attention has no shared rows)"""
    n = N()
    c, plan, _ = DC.fwd_geometry(dict(DC.FWD_BY_NAME[name], row_div=1), cus_of(dev))
    d = DC.fwd_inputs(c)
    B, L, A = c['B'], c['L'], c['A']
    out = run_cell(n, dev, c, d)
    P, HP, W = op3(d['proj'], dev, c['lp']), Op(d['hp'], dev, off=c['hp_off']), Op(d['w'], dev, off=c['w_off'])
    BO = Op(d['bo'], dev) if d['bo'] is not None else None
    X, AL, Z = Op(DC.rnd(B, L, 4, seed=5), dev), Op(nans(B, L), dev), Op(nans(B, 4), dev)
    pa = lambda *ops: n.ptr_array([o.v if o is not None else None for o in ops])  # noqa: E731
    n.check(n.lib.rfn_attn_small_fwd(1, pa(P), P.strides[0], P.strides[1], pa(HP), pa(W), pa(BO), pa(X), 4 * L, 4, B, L, A, 4,
                                     pa(AL), pa(Z), 4, n.stream_ptr()))
    finish([AL, Z], [P, HP, W, X])
    assert same_bits(AL.get(), out['alpha'])


@pytest.mark.parametrize('name', ['fast_4_4', 'fast_4_1', 'fast_5_2', 'fast_5_4_L1', 'gen_5_drop', 'gen_128', 'scal_odd_L9', 'r130_ub64'])
@pytest.mark.parametrize('drop', [0.0, DC.DROP_P])
def test_with_no_context_the_cell_is_the_lstm_epilogue(dev, name, drop):
    """U = 0, b_z = 0: the pre-activation is exactly the incoming gate sum and the update is rfn_lstm_fwd's formulas: the gate
    activations (the maxout selector included) are the same bits, with dropout and with maxout, and so is the kept set.  c
    and h are NOT the same bits: the compiler contracts `fg * cprev + ig * gg` as fma(ig, gg, fl(fg * cprev)) in lstm_fwd_k and
    as fma(fg, cprev, fl(ig * gg)) in the decoder-cell kernels (read in the gfx950 assembly of both), one rounding apart; the
    sources and rfn.h claim no more than that, and both are held to the fp64 tolerances of c and h."""
    n = N()
    c, plan, _ = DC.fwd_geometry(DC.FWD_BY_NAME[name], cus_of(dev))
    B, R, mo = c['B'], c['R'], c['maxout']
    d = DC.fwd_inputs(c)
    d = dict(d, U=torch.zeros_like(d['U']), bz=torch.zeros_like(d['bz']))
    out = run_cell(n, dev, c, d, drop=drop)
    G, C0 = op2(d['gin'], dev, c['lg']), op2(d['c0'], dev, c['lcp'])
    C1, H1 = op2(nans(B, R), dev, c['lcn']), op2(nans(B, R), dev, c['lh'])
    n.check(n.lib.rfn_lstm_fwd(G.ptr, G.strides[0], C0.ptr, C0.strides[0], C1.ptr, C1.strides[0], H1.ptr, H1.strides[0], B, R, mo,
                               drop, DC.DROP_SEED, DC.DROP_OFF, n.stream_ptr()))
    finish([G, C1, H1], [C0])
    assert same_bits(G.get(), out['gates'])
    ref = DC.cell_formulas(d)
    keep = keep_mask(n, dev, B, R, drop).double() if drop else 1.0
    for c1, h1 in ((C1.get(), H1.get()), (out['c'], out['h'])):
        assert maxerr(c1, ref['c']) < DC.TOL['c'] and maxerr(h1 * (1.0 - drop), ref['h'] * keep) < DC.TOL['h']
    assert torch.equal(H1.get() == 0, out['h'] == 0)


# =================================================================================================================
# 4. exact consequences; dropout
# =================================================================================================================
@pytest.mark.parametrize('name', ['fast_L3', 'fast_5_1', 'L9', 'L257', 'scal_small'])
def test_equal_scores_give_the_float32_quotient(dev, name):
    n = N()
    c, _, _ = DC.fwd_geometry(DC.FWD_BY_NAME[name], cus_of(dev))
    d = DC.fwd_inputs(c)
    out = run_cell(n, dev, c, dict(d, w=torch.zeros_like(d['w'])))
    q = float(np.float32(1.0) / np.float32(c['L']))
    assert bool((out['alpha'] == q).all()), (float(out['alpha'].min()), q)


@pytest.mark.parametrize('name', ['fast_L4_drop', 'gen_5_drop', 'scal_odd_L9'])
def test_without_dropout_the_seed_does_not_matter_and_with_it_it_does(dev, name):
    n = N()
    c, _, _ = DC.fwd_geometry(DC.FWD_BY_NAME[name], cus_of(dev))
    d = DC.fwd_inputs(c)
    a, b = run_cell(n, dev, c, d, drop=0.0), run_cell(n, dev, c, d, drop=0.0, seed=99, offset=5)
    assert same_out(a, b)
    p1, p2 = run_cell(n, dev, c, d), run_cell(n, dev, c, d, seed=99)
    assert same_out(p1, p2, keys=('gates', 'c', 'alpha')) and not same_bits(p1['h'], p2['h'])
    assert same_out(p1, a, keys=('gates', 'c', 'alpha'))
    # the counter is b * R + unit whatever ldh is: another ldh, same kept set
    p3 = run_cell(n, dev, dict(c, lh='packed' if c['lh'] != 'packed' else 'padded4'), d)
    assert same_out(p3, p1)


# =================================================================================================================
# 5. forward limits and refusals
# =================================================================================================================
def test_forward_limits_and_refusals(dev):
    n, cus = N(), cus_of(dev)
    c, _, _ = DC.fwd_geometry(DC.F('lim', 2, 2, 4, 4, maxout=1), cus)
    d = DC.fwd_inputs(c)
    assert run_cell(n, dev, c, d) is not None
    for ov in (dict(L=0), dict(L=1025), dict(drop_p=1.0), dict(drop_p=-0.25), dict(row_div=0), dict(B=0), dict(A=0)):
        run_cell(n, dev, c, d, override=ov, expect=ERR_SHAPE)
    for name in ('proj', 'hproj', 'w_out', 'U', 'bz', 'gates', 'c_prev', 'c_next', 'h_next', 'alpha'):
        run_cell(n, dev, c, d, null=name, expect=ERR_ARG)
    # the general kernel's LDS: 2 * up4(A) + L floats; A = 8188, L = 8 is exactly 64 KiB (case A8188_lds runs it), A = 8192 is over
    big, plan, _ = DC.fwd_geometry(DC.F('over', 1, 8, 8192, 4), cus)
    assert plan['kernel'] == 'refused' and DC.fwd_geometry(DC.FWD_BY_NAME['A8188_lds'], cus)[1]['lds'] == DC.LDS_FLOATS
    run_cell(n, dev, big, DC.fwd_inputs(big), expect=ERR_SHAPE)
    # L = 1024 runs (case L1024); L = 1025 on buffers that hold 1025 rows is refused
    over, plan, _ = DC.fwd_geometry(DC.F('over', 1, 1025, 4, 4), cus)
    assert plan['kernel'] == 'refused'
    run_cell(n, dev, over, DC.fwd_inputs(over), expect=ERR_SHAPE)


# =================================================================================================================
# backward runner
# =================================================================================================================
def run_bwd(n, dev, c, d, acc=None, expect=0, override=None, null=None):
    B, L, A, GD = d['proj'].shape[0], c['L'], c['A'], c['GD']
    acc = c['acc'] if acc is None else acc
    P, UO = op3(d['proj'], dev, c['lp']), op3(d['U'], dev, c['lu'])
    HP, W, AL = Op(d['hp'], dev, off=c['hp_off']), Op(d['w'], dev, off=c['w_off']), Op(d['alpha'], dev, off=c['soff'])
    DG = op2(d['dg'], dev, c['lg'])
    DP = op3(d['base'] if acc else nans(B, L, A), dev, c['ldp'])
    DHP, DWP = Op(nans(B, A), dev, off=c['dhp_off']), Op(nans(B, A), dev, off=c['dwp_off'])
    ptr = dict(proj=P.ptr, hproj=HP.ptr, w_out=W.ptr, alpha=AL.ptr, U=UO.ptr, dgates=DG.ptr, dproj=DP.ptr, dhproj=DHP.ptr,
               dw_part=DWP.ptr)
    if null:
        ptr[null] = None
    s = dict(dict(L=L, A=A, B=B, GD=GD), **(override or {}))
    rc = n.lib.rfn_dec_attn_bwd(ptr['proj'], P.strides[0], P.strides[1], ptr['hproj'], ptr['w_out'], ptr['alpha'], ptr['U'],
                                UO.strides[0], UO.strides[1], ptr['dgates'], DG.strides[0], s['B'], s['L'], s['A'], s['GD'],
                                ptr['dproj'], DP.strides[0], DP.strides[1], acc, ptr['dhproj'], ptr['dw_part'], n.stream_ptr())
    assert rc == expect, (rc, expect)
    ins = [P, UO, HP, W, AL, DG]
    if rc != 0:
        finish([], ins + [DP, DHP, DWP])
        return None
    finish([DP, DHP, DWP], ins)
    assert DP.written() and DHP.written() and DWP.written()
    return dict(dproj=DP.get(), dhp=DHP.get(), dwp=DWP.get())


def check_bwd(c, d, got, acc):
    base = dd(d['base']) if acc else 0.0
    if c['regime'] == 'std':
        ref = DC.bwd_autograd(d)
        scale = max(1.0, float(ref['dproj'].abs().max()))
        bar = dict(dproj=DC.TOL['dproj'] * scale, dhp=DC.TOL['dhp'] * scale, dw=DC.TOL['dw'] * max(1.0, float(ref['dw'].abs().max())))
    else:
        ref = DC.bwd_formulas(d)
        bar = dict(zip(DC.BWD_KEYS, (DC.YARD_FACTOR * y for y in DC.YARD_BWD[c['name']])))
    errs = dict(dproj=maxerr(got['dproj'], ref['dproj'] + base), dhp=maxerr(got['dhp'], ref['dhp']),
                dw=maxerr(dd(got['dwp']).sum(0), ref['dw']))
    ok = [held(c['name'], k, errs[k], bar[k]) for k in DC.BWD_KEYS]
    assert all(ok), dict(zip(DC.BWD_KEYS, ok))


def row_of(d, b):
    return {k: (v if k in ('w', 'bo', 'Wz') else v[b:b + 1].clone()) for k, v in d.items()}


# =================================================================================================================
# 6. backward: five kernels, every layout, both accumulate values, every trip
# =================================================================================================================
@pytest.mark.parametrize('name', [c['name'] for c in DC.BWD_CASES])
def test_backward_edges(dev, name):
    n = N()
    c = DC.BWD_BY_NAME[name]
    plan, _ = DC.bwd_geometry(c)
    assert plan['kernel'] != 'refused'
    d = DC.bwd_inputs(c)
    ow, ac = run_bwd(n, dev, c, d, acc=0), run_bwd(n, dev, c, d, acc=1)
    check_bwd(c, d, ow if c['acc'] == 0 else ac, c['acc'])
    # accumulate adds the gradient to what was there; dhproj and dw_part do not depend on it.  The sum is NOT fl(prior + the
    # overwrite result) in bits: `acc ? ov + dpre : dpre` with dpre = ds * w * (1 - t * t) is contracted, so the accumulating
    # form adds the exact last product with one rounding, fma(ds * w, 1 - t * t, prior), where the overwrite form rounds the
    # product.  The two therefore differ by at most half an ulp of each: u * (|accumulated| + |overwritten|), u = 2^-24 --
    # derived, and a thousand times tighter than the fp64 tolerance both are held to above and below.
    gap = (dd(ac['dproj']) - (dd(d['base']) + dd(ow['dproj']))).abs()
    assert bool((gap <= DC.U24 * (1 + 2.0 ** -20) * (dd(ac['dproj']).abs() + dd(ow['dproj']).abs())).all())
    if c['regime'] == 'std':                       # (a yardstick is measured for the case's own accumulate value)
        check_bwd(c, d, ac if c['acc'] == 0 else ow, 1 - c['acc'])
    assert same_bits(ac['dhp'], ow['dhp']) and same_bits(ac['dwp'], ow['dwp'])
    got = ac if c['acc'] else ow
    for b in range(c['B']):                        # one block per row
        one = run_bwd(n, dev, c, row_of(d, b))
        assert all(same_bits(one[k][0], got[k][b]) for k in ('dproj', 'dhp', 'dwp')), b
    if c['L'] == 1:                                # alpha = 1: ds = 1 * (d alpha - 1 * d alpha) = 0
        assert bool((d['alpha'] == 1.0).all())
        assert all(bool((ow[k] == 0).all()) for k in ('dproj', 'dhp', 'dwp'))
    zero = run_bwd(n, dev, c, dict(d, dg=torch.zeros_like(d['dg'])), acc=0)
    assert all(bool((zero[k] == 0).all()) for k in ('dproj', 'dhp', 'dwp'))
    if plan['kernel'] == 'fast':                   # hproj one float off: fast_ok fails, vec and vecu hold
        c2 = dict(c, hp_off=1) if c['L'] % 2 else dict(c, w_off=1)
        assert DC.bwd_geometry(c2)[0]['kernel'] == 'vec_vecu'
        # Same formulas, NOT the same bits, not even dproj: the compiler contracts `1 - t * t`, `ds * w * (1 - t * t)` and the
        # `ah += dpre` / `ov + dpre` sums into fmas differently in the two kernels (in dec_attn_bwd_k<true, true> even from one
        # vector element to the next: read in the gfx950 assembly), and the fast body adds the two row halves separately.  Each
        # is held to fp64 and the pair to the same tolerance.
        vv = run_bwd(n, dev, c2, d)
        check_bwd(c, d, vv, c['acc'])
        scale = max(1.0, float(got['dproj'].abs().max()))
        assert maxerr(vv['dproj'], got['dproj']) < DC.TOL['dproj'] * scale and maxerr(vv['dhp'], got['dhp']) < DC.TOL['dhp'] * scale
        dw = dd(got['dwp']).sum(0)
        assert maxerr(dd(vv['dwp']).sum(0), dw) < DC.TOL['dw'] * max(1.0, float(dw.abs().max()))


def test_backward_refusals_launch_nothing(dev):
    n = N()
    c = DC.Bk('lim', 2, 2, 4, 8)
    d = DC.bwd_inputs(c)
    assert run_bwd(n, dev, c, d) is not None
    for ov in (dict(L=1025), dict(L=0), dict(B=0), dict(A=0), dict(GD=0)):
        run_bwd(n, dev, c, d, override=ov, expect=ERR_SHAPE)
    for name in ('proj', 'hproj', 'w_out', 'alpha', 'U', 'dgates', 'dproj', 'dhproj', 'dw_part'):
        run_bwd(n, dev, c, d, null=name, expect=ERR_ARG)
    # LDS: 2 * up4(A) + 2 * up4(L) + 32 floats; at L = 1, A = 8172 is exactly 64 KiB and runs, A = 8176 is refused
    for A, expect in ((8172, 0), (8176, ERR_SHAPE)):
        cb = DC.Bk('lds', 1, 1, A, 8)
        assert (DC.bwd_geometry(cb)[0]['kernel'] == 'refused') == (expect != 0)
        got = run_bwd(n, dev, cb, DC.bwd_inputs(cb), expect=expect)
        if got is not None:
            assert all(bool((got[k] == 0).all()) for k in ('dproj', 'dhp', 'dwp'))
    over = DC.Bk('over', 1, 1025, 4, 8)
    run_bwd(n, dev, over, DC.bwd_inputs(over), expect=ERR_SHAPE)


# =================================================================================================================
# 7. rfn_dec_du
# =================================================================================================================
def run_du(n, dev, S, B, L, GD, lay, al, dg, expect=0, soff=0):
    AL, DG = Op(al, dev, off=soff), Op(dg, dev, off=soff)
    DU = op3(torch.full((B, L, GD), 7.0), dev, lay)
    rc = n.lib.rfn_dec_du(AL.ptr, DG.ptr, S, B, L, GD, DU.ptr, DU.strides[0], DU.strides[1], n.stream_ptr())
    assert rc == expect, (rc, expect)
    if rc != 0:
        finish([], [AL, DG, DU])
        return None
    finish([DU], [AL, DG])                         # nothing outside rows l < L and columns c < GD has changed
    return DU.get()


def du_data(S, B, L, GD):
    return torch.softmax(DC.rnd(S, B, L, seed=1), 2), DC.rnd(S, B, GD, seed=2)


def du_held(got, al, dg, S):
    ref = torch.einsum('sbl,sbg->blg', dd(al), dd(dg))
    mag = torch.einsum('sbl,sbg->blg', dd(al).abs(), dd(dg).abs())
    err = (dd(got) - ref).abs()
    print('dec_du S=%d max err / bound %.3g' % (S, float((err / ((S + 1) * DC.U24 * mag).clamp_min(1e-300)).max())))
    return bool((err <= (S + 1) * DC.U24 * mag).all())


@pytest.mark.parametrize('S,B,L,GD,lay', DC.DU_CASES)
def test_du_edges(dev, S, B, L, GD, lay):
    n = N()
    plan, _ = DC.du_geometry(S, B, L, GD, lay)
    al, dg = du_data(S, B, L, GD)
    got = run_du(n, dev, S, B, L, GD, lay, al, dg)
    assert du_held(got, al, dg, S)
    if plan['kernel'] == 'vector':                 # the scalar kernel on the same data (dU one float off): the same bits
        assert DC.du_geometry(S, B, L, GD, 'offset_1')[0]['kernel'] == 'scalar'
        assert same_bits(run_du(n, dev, S, B, L, GD, 'offset_1', al, dg), got)


@pytest.mark.parametrize('S,B,L,GD,lay', DC.DU_SOFF_CASES)
def test_du_with_alpha_and_dgates_one_float_off_takes_the_scalar_kernel_and_gives_the_same_bits(dev, S, B, L, GD, lay):
    n = N()
    assert DC.du_geometry(S, B, L, GD, lay)[0]['kernel'] == 'vector' and DC.du_geometry(S, B, L, GD, lay, soff=1)[0]['kernel'] == 'scalar'
    al, dg = du_data(S, B, L, GD)
    got = run_du(n, dev, S, B, L, GD, lay, al, dg, soff=1)
    assert du_held(got, al, dg, S)
    assert same_bits(run_du(n, dev, S, B, L, GD, lay, al, dg), got)


def test_du_refuses_a_row_whose_alpha_does_not_fit_lds_on_the_vector_path_only(dev):
    n = N()
    S, B, L, GD = DC.DU_LIMIT
    al, dg = du_data(S, B, L, GD)
    assert DC.du_geometry(S, B, L, GD, 'packed')[0]['kernel'] == 'refused'
    run_du(n, dev, S, B, L, GD, 'packed', al, dg, expect=ERR_SHAPE)
    assert DC.du_geometry(S, B, L, GD, 'offset_1')[0]['kernel'] == 'scalar'
    assert du_held(run_du(n, dev, S, B, L, GD, 'offset_1', al, dg), al, dg, S)
    # one step fewer fits: S * L = 16380 floats
    assert DC.du_geometry(S - 1, B, L, GD, 'packed')[0]['kernel'] == 'vector'
    assert du_held(run_du(n, dev, S - 1, B, L, GD, 'packed', al[:S - 1].contiguous(), dg[:S - 1].contiguous()), al[:S - 1], dg[:S - 1], S - 1)
    for bad in (dict(S=0), dict(L=0), dict(GD=0), dict(B=0)):
        a = dict(dict(S=2, B=1, L=2, GD=4), **bad)
        t = torch.zeros(64, device=dev)
        assert n.lib.rfn_dec_du(t.data_ptr(), t.data_ptr(), a['S'], a['B'], a['L'], a['GD'], t.data_ptr(), 8, 4, n.stream_ptr()) == ERR_SHAPE
    t = torch.zeros(64, device=dev)
    for i in range(3):
        p = [t.data_ptr()] * 3
        p[i] = None
        assert n.lib.rfn_dec_du(p[0], p[1], 2, 1, 2, 4, p[2], 8, 4, n.stream_ptr()) == ERR_ARG
