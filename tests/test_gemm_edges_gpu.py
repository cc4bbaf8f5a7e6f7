"""The f32 GEMM entry family (csrc/rfn_gemm.hip: rfn_gemm_f32, _ws, _opt, _tk, _lstm) swept over the shapes, strides, pointer
alignments, flags, workspaces and ticket counts at which gemm_entry / launch_tile / launch_cfg pick another kernel or a
kernel's loop takes another trip, through the C ABI, against a plain fp64 product on the CPU.  The cases and a Python model
of the host's decisions live in tests/gemm_cases.py (its docstring restates the constants; nothing is imported from the C
side); tests/test_gemm_cases_cpu.py proves without a GPU that the table reaches every branch named below.

Conventions: every operand (A, B, bias, C, a_colsum, the LSTM state, the workspace, the tickets) is carved out of a larger
device buffer: float buffers NaN-filled with at least 8 floats in front and behind, tickets int32 with a sentinel in the
guard words and zeros inside.  After a call the guards, the padding between rows and the tails must hold their bits, every
output element must have been written, no input may have changed, the tickets are zero again, and the workspace was written
exactly where the model says (all of [0, (M N + M [a_colsum]) G splitk) floats, nothing behind) -- which also pins the K
split the device really took to the model's.  A NaN guard next to an operand also catches an over-read that reaches a
stored value.  Layouts per operand: packed; padded4 (ld + 4: still float4); ld_plus_1 (scalar staging); offset_1 (base + 1
float, ld % 4 == 0: the rfn_aligned16 fallback); soff: bias, a_colsum and the LSTM state one float off.

Tolerances -- no invented numbers
---------------------------------
* what the sources state as bit-identity is asserted as bit-identity: unsplit, the flags 0 / NO_DMA / LDS_LEAN / both (tail
  rounds included: a tile's shape does not enter the k order); under a K split LDS_LEAN == default always, NO_DMA == default
  wherever the model says both cut the same K ranges (its 32-deep register kernel cannot start mid-step: against the 16-deep
  default of the layouts other than [row][k] x [row][k] the ranges differ whenever 0 < (K / 32) mod s <= s / 2) and within
  the yardstick otherwise; in-kernel ticket finish == separate reduce; repeated calls; rfn_gemm_f32_lstm == rfn_gemm_f32_ws
  + rfn_lstm_fwd_grouped; a workspace that is too small or misaligned == no workspace.
* hard cap: against fp64 every element stays within (K_total + nseg + splitk + 2) * 2^-24 * (|A||B|^T + sum|bias| + |C_prev|),
  the worst case of any association (derived, loose).
* yardstick: the same product accumulated sequentially in k order in plain fp32 on the CPU, max error against fp64, measured
  per case and committed in gemm_cases.YARD; the kernel gets 4 x that for another association (32x32x2 MFMA pairs, split
  ranges).  A dropped or doubled term is ~1 in size, four orders of magnitude above any yardstick (checked on the CPU).

Out of scope: rfn_gemm_x3.hip (its own sweep: tests/test_x3_edges_gpu.py) and rfn_cell_gemm (tests/test_cellgemm_gpu.py); operands of >= 4 GiB
(the span32 fallback); any timing.
"""
import ctypes as C
import pytest
import torch

import gemm_cases as GC
from gemm_cases import FLAG_SETS, MIB, OPT_LEAN, OPT_NO_DMA, but, plan

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 8
SENTINEL = 0x5A5A5A5A
WS_TAIL = 4096                                      # guard floats behind a workspace: more than any a_colsum slab here
ERR_SHAPE, ERR_ARG = -1, -5


def N():
    import recurrent_fusion_network_amd._native as n
    return n


def ids(cases):
    return [c.name.replace(' ', '_') for c in cases]


# =================================================================================================================
# operands carved out of guarded buffers
# =================================================================================================================
class Op:
    """A logical tensor (or, given a shape, a NaN-filled output) placed with element strides `strides` at GUARD + off
    floats into a NaN-filled device buffer."""

    def __init__(self, t, dev, strides=None, off=0):
        shape = tuple(t) if isinstance(t, (tuple, list)) else tuple(t.shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.insert(0, acc)
                acc *= s
        span = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if all(shape) else 0
        self.buf = torch.full((GUARD + off + span + GUARD,), NAN, device=dev)
        self.v = self.buf.as_strided(shape, tuple(strides), GUARD + off)
        if not isinstance(t, (tuple, list)):
            self.v.copy_(t.to(dev))
        self.strides = tuple(strides)
        self.mask = torch.ones(self.buf.shape, dtype=torch.bool, device=dev)
        self.mask.as_strided(shape, tuple(strides), GUARD + off).fill_(False)
        self.snap = self.buf.clone()
        self.ptr = self.buf.data_ptr() + 4 * (GUARD + off)          # also for an operand without elements (K = 0)
        assert (self.ptr % 16 == 0) == (off % 4 == 0)

    def outside_ok(self):
        """guards, padding and the tail hold the bits they held when the operand was made"""
        return torch.equal(self.buf.view(torch.int32)[self.mask], self.snap.view(torch.int32)[self.mask])

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int32), self.snap.view(torch.int32))

    def written(self):
        return not bool(torch.isnan(self.v).any())

    def get(self):
        return self.v.detach().cpu().clone()

    def same_bits(self, other):
        return torch.equal(self.buf.view(torch.int32), other.buf.view(torch.int32))


class Workspace:
    """`nbytes` of NaN-filled scratch at GUARD + off floats into a NaN-filled buffer, WS_TAIL guard floats behind it"""

    def __init__(self, dev, nbytes, off=0):
        assert nbytes % 4 == 0
        self.nbytes, self.n, self.off = nbytes, nbytes // 4, GUARD + off
        self.buf = torch.full((self.off + self.n + WS_TAIL,), NAN, device=dev)
        self.nanbits = int(torch.full((1,), NAN).view(torch.int32)[0])

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def reset(self):
        self.buf.fill_(NAN)

    def check(self, used):
        """the first `used` floats were all written, nothing else was"""
        b = self.buf.view(torch.int32)
        assert used <= self.n
        assert bool((b[:self.off] == self.nanbits).all()) and bool((b[self.off + used:] == self.nanbits).all()), \
            'the workspace was written outside the floats the split needs'
        assert not bool(torch.isnan(self.buf[self.off:self.off + used]).any()), 'part of the split workspace was never written'


class Tickets:
    def __init__(self, dev, n, spare=0):
        """n counters handed to the library; `spare` more zeros behind them that it must not touch"""
        self.n = n
        self.buf = torch.full((GUARD + n + spare + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
        self.buf[GUARD:GUARD + n + spare] = 0
        self.snap = self.buf.clone()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def check(self):
        assert torch.equal(self.buf, self.snap), 'a ticket was left non-zero, or a word outside the n_tickets counters was written'


_WS = {}


def workspace(dev, nbytes, off=0):
    """one buffer per size for the whole module (the big one is 256 MiB), NaN-filled again for every call"""
    key = (nbytes, off)
    if key not in _WS:
        _WS[key] = Workspace(dev, nbytes, off)
    _WS[key].reset()
    return _WS[key]


_INPUTS = {}


def inputs(c):
    k = GC.yard_key(c)
    if k not in _INPUTS:
        if len(_INPUTS) > 4:
            _INPUTS.clear()
        _INPUTS[k] = GC.make_inputs(c)
    return _INPUTS[k]


# =================================================================================================================
# the runner: one call of one case, every guard checked
# =================================================================================================================
class Run:
    pass


def build_problems(n, dev, c, inp):
    """operands of the case on the device -> (ctypes problem array, outputs C, a_colsum, inputs)"""
    arr = (n.GemmProblem * max(1, c.G))()
    Cs, CSs, ins = [], [], []
    ldc, offc = GC.lay2(c.N, c.layC)
    for g in range(c.G):
        Cg = Op(inp['prev'][g] if c.acc else (c.M, c.N), dev, (ldc, 1), offc)
        Cs.append(Cg)
        arr[g].C, arr[g].ldc, arr[g].nseg = Cg.ptr, ldc, len(c.Ks)
        arr[g].a_colsum = None
        if c.colsum:
            CSs.append(Op(inp['csprev'][g] if c.acc else (c.M,), dev, off=c.soff))
            arr[g].a_colsum = CSs[-1].ptr
        for s, K in enumerate(c.Ks):
            A, B = inp['A'][g][s], inp['B'][g][s]
            lda, offa = GC.lay2(K if c.ak else c.M, c.layA)
            ldb, offb = GC.lay2(K if c.bk else c.N, c.layB)
            Ao = Op(A if c.ak else A.t(), dev, (lda, 1), offa)
            Bo = Op(B if c.bk else B.t(), dev, (ldb, 1), offb)
            ins += [Ao, Bo]
            sg = arr[g].seg[s]
            sg.A, sg.lda, sg.a_kfast, sg.B, sg.ldb, sg.b_kfast, sg.K = Ao.ptr, lda, c.ak, Bo.ptr, ldb, c.bk, K
            sg.bias = None
            if inp['bias'][g][s] is not None:
                bo = Op(inp['bias'][g][s], dev, off=c.soff)
                ins.append(bo)
                sg.bias = bo.ptr
    return arr, Cs, CSs, ins


def run(n, dev, c, tk=None, rc=0, check_ws=True):
    """One rfn_gemm_f32_tk call of case c (tk: a Tickets object to draw on).  Asserts the return code, every guard, that
    every output was written (rc = 0) or nothing was (otherwise), that no input changed, that the tickets are zero again
    and that the workspace was written exactly where the model says.  -> Run with the outputs still on the device."""
    inp = inputs(c)
    p = plan(c)
    arr, Cs, CSs, ins = build_problems(n, dev, c, inp)
    ws = workspace(dev, c.ws, c.ws_off) if c.ws else None
    got = n.lib.rfn_gemm_f32_tk(c.M, c.N, c.G, arr, c.acc, ws.ptr if ws else None, c.ws, c.flags, tk.ptr if tk else None,
                                tk.n if tk else 0, n.stream_ptr())
    torch.cuda.synchronize()
    assert got == rc, 'return code %d, expected %d' % (got, rc)
    for o in ins:
        assert o.unchanged(), 'a kernel wrote into an input'
    for o in Cs + CSs:
        if rc == 0 and p['kind'] == 'run':
            assert o.outside_ok(), 'a kernel wrote outside its output'
            assert o.written(), 'an output element was never written'
        else:
            assert o.unchanged(), 'a refused or empty call wrote into an output'
        o.snap = None
    if tk:
        tk.check()
    if ws and check_ws:
        ws.check(p.get('ws_floats', 0))
    r = Run()
    r.C, r.cs, r.plan, r.case = Cs, CSs, p, c
    return r


def same(a, b):
    return all(x.same_bits(y) for x, y in zip(a.C + a.cs, b.C + b.cs))


def check_fp64(r, splitk=None):
    c, inp = r.case, inputs(r.case)
    yc, ys = GC.yard(c)
    sk = r.plan['splitk'] if splitk is None else splitk
    for g in range(c.G):
        ref, mag = GC.ref_group(c, inp, g)
        GC.check_product(r.C[g].get(), ref, mag, c, sk, yc)
        if c.colsum:
            ref, mag = GC.ref_colsum(c, inp, g)
            GC.check_product(r.cs[g].get(), ref, mag, c, sk, ys, 'a_colsum')


def with_tickets(n, dev, c, base):
    """the in-kernel finish on exactly as many counters as output tiles, three launches in a row on the same counters, and
    on one counter fewer (the separate reduce again; the counters beyond n_tickets stay untouched): all == `base`"""
    tiles = base.plan['tiles']
    assert plan(but(c, tickets=0))['finish'] == 'ticket' and plan(but(c, tickets=-1))['finish'].startswith('reduce')
    tk = Tickets(dev, tiles)
    for _ in range(3):
        assert same(run(n, dev, c, tk=tk), base), 'the in-kernel finish differs from the separate reduce'
    if tiles > 1:
        assert same(run(n, dev, c, tk=Tickets(dev, tiles - 1, spare=1)), base)


# =================================================================================================================
# 1. 64 x 64 tile and block bookkeeping
# =================================================================================================================
@pytest.mark.parametrize('c', GC.TILE_CASES, ids=ids(GC.TILE_CASES))
def test_tile_and_block_bookkeeping(dev, c):
    """accumulate = 0 on a NaN-filled C: every element is written; accumulate = 1 on C = 0.25: every element is visited
    exactly once (a second visit adds the product twice, ~1 against a yardstick of 1e-6)"""
    r = run(N(), dev, c)
    assert r.plan['tile'] == 64 and r.plan['splitk'] == 1
    check_fp64(r)


# =================================================================================================================
# 2. K edges, segments, biases, groups, operand layouts
# =================================================================================================================
@pytest.mark.parametrize('c', GC.K_CASES, ids=ids(GC.K_CASES))
def test_k_edges_segments_and_layouts(dev, c):
    check_fp64(run(N(), dev, c))


@pytest.mark.parametrize('c', GC.K0_REFUSED, ids=ids(GC.K0_REFUSED))
def test_an_empty_segment_among_others_is_refused(dev, c):
    """The tile kernels count a K = 0 segment as zero K steps but spend a load on it: before the refusal, K = [32, 0, 32]
    returned A0 B0^T plus every bias, silently (reproduced on the MI355X: error ~ 20 against fp64, with the empty segment
    first or in the middle; an empty LAST segment came out right).  rfn.h now states the K rule: K = 0 only when every
    segment of the problem is empty; every position is refused alike."""
    run(N(), dev, c, rc=ERR_SHAPE)


# =================================================================================================================
# 3. big tile, >= 384 tiles: the three big kernels and the ragged LDS-DMA form, unsplit: the flags are bit-identical
# =================================================================================================================
@pytest.mark.parametrize('c', GC.BIG_CASES, ids=ids(GC.BIG_CASES))
def test_big_tile_kernels_agree_bit_for_bit(dev, c):
    n = N()
    base = run(n, dev, c)
    assert base.plan['tile'] == 128 and base.plan['splitk'] == 1
    check_fp64(base)
    for f in FLAG_SETS[1:]:
        assert same(run(n, dev, but(c, flags=f)), base), 'flags %d change the bits of an unsplit product' % f


@pytest.mark.parametrize('c', GC.TAIL_CASES, ids=ids(GC.TAIL_CASES))
def test_tail_rounds(dev, c):
    """half-height and quarter tiles of the last round; ragged: some tail parts lie wholly outside the matrix"""
    n = N()
    base = run(n, dev, c)
    check_fp64(base)
    for f in (OPT_NO_DMA, OPT_LEAN):
        assert same(run(n, dev, but(c, flags=f)), base)
        torch.cuda.empty_cache()
    del base
    torch.cuda.empty_cache()


# =================================================================================================================
# 4. the 64 x 64 K split
# =================================================================================================================
@pytest.mark.parametrize('c', GC.SPLIT64_CASES, ids=ids(GC.SPLIT64_CASES))
def test_small_tile_k_split(dev, c):
    n = N()
    base = run(n, dev, c)
    assert base.plan['tile'] == 64 and base.plan['splitk'] > 1
    check_fp64(base)
    assert same(run(n, dev, c), base), 'a repeated call gives other bits'
    assert GC.same_ranges(c, OPT_NO_DMA)            # both kernels step by 32
    assert same(run(n, dev, but(c, flags=OPT_NO_DMA)), base), 'LDS-DMA and register staging differ'
    with_tickets(n, dev, c, base)


# =================================================================================================================
# 5. the medium big-tile split: M = N = 512, K = 11456
# =================================================================================================================
@pytest.mark.parametrize('ak,bk', GC.KLAYS)
def test_medium_big_tile_split(dev, ak, bk):
    n = N()
    for c in [c for c in GC.MEDIUM_CASES + GC.MEDIUM_RAGGED_CASES if (c.ak, c.bk) == (ak, bk)]:
        base = run(n, dev, c)
        assert base.plan['tile'] == 128
        check_fp64(base)
        split = base.plan['splitk'] > 1
        if split:
            with_tickets(n, dev, c, base)
        for f in FLAG_SETS[1:]:
            cf = but(c, flags=c.flags | f)
            r = run(n, dev, cf)
            if not (f & OPT_NO_DMA):
                assert GC.same_ranges(c, f)
            if GC.same_ranges(c, f):
                assert same(r, base), '%s: flags %d change the bits' % (c.name, f)
            else:                                   # NO_DMA against a 16-deep default: other K ranges, re-association only
                check_fp64(r)
            if split:
                assert same(run(n, dev, cf, tk=Tickets(dev, base.plan['tiles'])), r)


# =================================================================================================================
# 6. the a_colsum rider
# =================================================================================================================
@pytest.mark.parametrize('c', GC.COLSUM_CASES, ids=ids(GC.COLSUM_CASES))
def test_a_colsum_rider(dev, c):
    n = N()
    base = run(n, dev, c)
    check_fp64(base)
    assert same(run(n, dev, c), base)
    if base.plan['splitk'] > 1:
        with_tickets(n, dev, c, base)
    else:
        for f in FLAG_SETS[1:]:
            assert same(run(n, dev, but(c, flags=f)), base)


# =================================================================================================================
# 7. workspace boundaries
# =================================================================================================================
@pytest.mark.parametrize('c', GC.WS_CASES, ids=ids(GC.WS_CASES))
def test_workspace_boundaries(dev, c):
    """run() checks that exactly the model's floats of the workspace were written: all of them, and nothing behind --
    in particular nothing beyond ws_bytes when cap == the split the host wants, and nothing at all when the workspace is
    too small or misaligned, whose results are then the bits of a call without one"""
    n = N()
    r = run(n, dev, c)
    check_fp64(r)
    if r.plan['splitk'] == 1:
        assert same(run(n, dev, but(c, ws=0, ws_off=0)), r)
    else:
        with_tickets(n, dev, c, r)


# =================================================================================================================
# 8. rfn_gemm_f32_lstm
# =================================================================================================================
@pytest.mark.parametrize('c', GC.LSTM_CASES, ids=ids(GC.LSTM_CASES))
def test_gate_gemm_with_lstm_update(dev, c):
    """split and unsplit == rfn_gemm_f32_ws followed by rfn_lstm_fwd_grouped, bit for bit, as rfn.h states; gate buffers
    equally spaced with a padded group stride, the state buffers guarded (and one float off with soff)"""
    n, st = N(), N().stream_ptr()
    inp = inputs(c)
    M, R, G = c.M, c.N // 4, c.G
    ldc, _ = GC.lay2(c.N, c.layC)
    gsC = M * ldc + 8
    gen = torch.Generator().manual_seed(5)
    cprev = torch.randn(G, M, R, generator=gen)
    ldst, gss = R + 3, M * (R + 3) + 5              # scalar-accessed: any stride will do
    seed, off = 4242, 8
    outs = []
    for fused in (False, True):
        cc = but(c, G=1)                            # the operands of every group, C replaced by one equally spaced buffer
        Call = Op((G, M, c.N), dev, (gsC, ldc, 1))
        CP = Op(cprev, dev, (gss, ldst, 1), c.soff)
        CN, HN = Op((G, M, R), dev, (gss, ldst, 1), c.soff), Op((G, M, R), dev, (gss, ldst, 1), c.soff)
        arr = (n.GemmProblem * G)()
        ins = [CP]
        for g in range(G):
            a1, _, _, i1 = build_problems(n, dev, cc, dict(A=[inp['A'][g]], B=[inp['B'][g]], bias=[inp['bias'][g]],
                                                           prev=[inp['prev'][g]], csprev=[inp['csprev'][g]]))
            arr[g] = a1[0]
            arr[g].C = Call.ptr + 4 * g * gsC
            ins += i1
        ws = workspace(dev, c.ws) if c.ws else None
        wp, wb = (ws.ptr, c.ws) if ws else (None, 0)
        if fused:
            lu = n.GemmLstm()
            lu.c_prev, lu.c_next, lu.h_next = CP.ptr, CN.ptr, HN.ptr
            lu.ldcp = lu.ldcn = lu.ldh = ldst
            lu.gs_cprev = lu.gs_cnext = lu.gs_h = gss
            lu.drop_p, lu.seed, lu.offset = c.drop, seed, off
            n.check(n.lib.rfn_gemm_f32_lstm(M, R, G, arr, wp, wb, c.flags, C.byref(lu), st))
        else:
            n.check(n.lib.rfn_gemm_f32_ws(M, c.N, G, arr, 0, wp, wb, st))
            n.check(n.lib.rfn_lstm_fwd_grouped(Call.ptr, ldc, CP.ptr, ldst, CN.ptr, ldst, HN.ptr, ldst, M, R, 0, c.drop, seed, off,
                                               G, gsC, gss, gss, gss, st))
        torch.cuda.synchronize()
        for o in ins:
            assert o.unchanged()
        for o in (Call, CN, HN):
            assert o.outside_ok() and o.written()
        p = plan(c, lstm=True)
        assert (p['splitk'] > 1) == (c.name.split()[1] == 'split')
        if ws:
            ws.check(p['ws_floats'])
        outs.append((Call, CN, HN))
    for a, b in zip(*outs):
        assert a.same_bits(b), 'rfn_gemm_f32_lstm differs from rfn_gemm_f32_ws + rfn_lstm_fwd_grouped'
    if c.drop > 0:
        zeros = float((outs[1][2].v == 0).float().mean())
        assert 0.0 < zeros < 0.7
    gates = outs[1][0].v                            # activations: three sigmoids and a tanh
    assert bool((gates[..., :3 * R] >= 0).all()) and bool((gates.abs() <= 1).all())


# =================================================================================================================
# 9. refusals and empty calls
# =================================================================================================================
def test_empty_calls_return_ok_and_write_nothing(dev):
    n = N()
    c = GC.case('empty', 68, 72, [36], ws=GC.WS_8)
    for M, Nn in ((0, 72), (68, 0), (-1, 72), (68, -3)):
        inp = inputs(c)
        arr, Cs, _, ins = build_problems(n, dev, c, inp)
        ws, tk = workspace(dev, c.ws), Tickets(dev, 4)
        assert n.lib.rfn_gemm_f32_tk(M, Nn, 1, arr, 0, ws.ptr, c.ws, 0, tk.ptr, tk.n, n.stream_ptr()) == 0
        torch.cuda.synchronize()
        assert all(o.unchanged() for o in Cs + ins)
        ws.check(0)
        tk.check()


REFUSALS = [
    ('ngroups 0', ERR_SHAPE), ('ngroups 9', ERR_SHAPE), ('nseg 0', ERR_SHAPE), ('nseg 9', ERR_SHAPE), ('null C', ERR_SHAPE),
    ('null A', ERR_ARG), ('null B', ERR_ARG), ('K < 0', ERR_ARG), ('mixed segments', ERR_SHAPE), ('mixed groups', ERR_SHAPE),
    ('null problems', ERR_SHAPE),
]


@pytest.mark.parametrize('what,code', REFUSALS, ids=[w.replace(' ', '_') for w, _ in REFUSALS])
def test_refusals_write_nothing(dev, what, code):
    n = N()
    c = GC.case('refusal', 68, 72, [800, 36], G=2, ws=GC.WS_8, colsum=False)
    inp = inputs(c)
    arr, Cs, _, ins = build_problems(n, dev, c, inp)
    G = 2
    if what == 'ngroups 0':
        G = 0
    elif what == 'ngroups 9':
        G = 9
        big = (n.GemmProblem * 9)()
        for g in range(9):
            big[g] = arr[g % 2]
        arr = big
    elif what == 'nseg 0':
        arr[1].nseg = 0
    elif what == 'nseg 9':
        arr[1].nseg = 9
    elif what == 'null C':
        arr[1].C = None
    elif what == 'null A':
        arr[1].seg[1].A = None
    elif what == 'null B':
        arr[0].seg[1].B = None
    elif what == 'K < 0':
        arr[1].seg[0].K = -4
    elif what == 'mixed segments':
        arr[0].seg[1].a_kfast = 0
    elif what == 'mixed groups':
        arr[1].seg[0].b_kfast, arr[1].seg[1].b_kfast = 0, 0
    elif what == 'null problems':
        arr = None
    ws, tk = workspace(dev, c.ws), Tickets(dev, 8)
    assert n.lib.rfn_gemm_f32_tk(c.M, c.N, G, arr, 0, ws.ptr, c.ws, 0, tk.ptr, tk.n, n.stream_ptr()) == code
    torch.cuda.synchronize()
    assert all(o.unchanged() for o in Cs + ins)
    ws.check(0)
    tk.check()


@pytest.mark.parametrize('what,code', [('null lstm', ERR_ARG), ('null c_prev', ERR_ARG), ('null c_next', ERR_ARG),
                                       ('null h_next', ERR_ARG), ('R 0', ERR_ARG), ('drop_p 1', ERR_SHAPE),
                                       ('drop_p < 0', ERR_SHAPE)])
def test_bad_lstm_fields_are_refused(dev, what, code):
    n = N()
    c = GC.case('refusal lstm', 6, 160, [192, 128], ws=GC.WS_8)
    M, R = c.M, c.N // 4
    arr, Cs, _, ins = build_problems(n, dev, c, inputs(c))
    CP, CN, HN = Op(torch.zeros(M, R), dev), Op((M, R), dev), Op((M, R), dev)
    lu = n.GemmLstm()
    lu.c_prev, lu.c_next, lu.h_next = CP.ptr, CN.ptr, HN.ptr
    lu.ldcp = lu.ldcn = lu.ldh = R
    lu.drop_p, lu.seed, lu.offset = 0.0, 1, 0
    if what == 'null c_prev':
        lu.c_prev = None
    elif what == 'null c_next':
        lu.c_next = None
    elif what == 'null h_next':
        lu.h_next = None
    elif what == 'R 0':
        R = 0
    elif what == 'drop_p 1':
        lu.drop_p = 1.0
    elif what == 'drop_p < 0':
        lu.drop_p = -0.5
    ws = workspace(dev, c.ws)
    ref = None if what == 'null lstm' else C.byref(lu)
    assert n.lib.rfn_gemm_f32_lstm(M, R, 1, arr, ws.ptr, c.ws, 0, ref, n.stream_ptr()) == code
    torch.cuda.synchronize()
    assert all(o.unchanged() for o in Cs + ins + [CP, CN, HN])
    ws.check(0)
