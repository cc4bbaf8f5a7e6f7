"""Case table of the f32 GEMM sweep (tests/test_gemm_edges_gpu.py) and a plain-Python restatement of the decisions that
gemm_entry / launch_tile / launch_cfg of csrc/rfn_gemm.hip take for a call: float4 or scalar staging, tile size, kernel
(LDS-DMA, its ragged form, register-staged FAST, bounds-checked register-staged), K step, K split, the K ranges of the
split and which of them are empty, the kind of finish (rfn_gemm_reduce_k<true/false>, rfn_gemm_reduce_lstm_k, in-kernel
tickets) and the tail round.  Nothing is imported from the C side and nothing here needs a GPU:
tests/test_gemm_cases_cpu.py asserts that the table reaches every branch, so an edit of a constant that silently moves
a case off its branch fails there.

Constants restated from csrc/rfn_gemm.hip and include/rfn.h:
    RFN_GEMM_MAXSEG 8, RFN_GEMM_MAXGROUP 8; big tile 128 x 128, small tile 64 x 64, GEMM_BAND_ROWS 8, 8 XCDs;
    K steps: register-staged 32 (both tiles), 64 x 64 LDS-DMA 32, big LDS-DMA 32 ([row][k] x [row][k]) / 16 (other layouts),
    RFN_GEMM_OPT_LDS_LEAN LDS-DMA 16 -- whose K RANGES are cut in the default kernel's step of the layout;
    big tile from 384 tiles; medium gate: 16 <= tiles <= 1023, >= 6e9 flop, a workspace; cost model of the split: rounds of
    512 blocks at 3.9 us per 32-deep step, a last round of <= 256 blocks at 0.6, 6 us + s * (M N G * 4 / 4e6) us for the
    reduce, a deeper split has to buy 3 %, s <= 16, s <= cap, s <= iters32 / 8; RFN_GEMM_OPT_FORCE_SPLIT bits 8-12;
    64 x 64 split: 768 / tiles, >= 4 steps per range, <= 16, <= cap; cap = (ws_bytes >> 20) * 2^18 / ((M N + M) G);
    a workspace counts from 1 MiB and 16-B aligned; tail round: q = tiles / 8 per XCD, S = (CUs / 8) * blocks per CU slots
    (MI355X: 32 * 2 = 64 or 32 * 3 = 96), tail = q mod S, taken when q / S >= 2 and 0 < 2 * tail <= S, quarter tiles when
    4 * tail <= S.

Tolerances (see the GPU test's docstring): the element-wise worst-case bound HARD CAP, and per case the YARDSTICK: the same
product accumulated sequentially in k order in plain fp32 on this CPU (acc += A[:, k:k+1] * B[:, k]; then the biases in
segment order, then the previous C), max error against fp64; the kernel gets 4 x that for its other association (32x32x2
MFMA pairs: two interleaved chains per element; K ranges added afterwards).  `python tests/gemm_cases.py` re-measures the
table below and prints it.
"""
import zlib

import numpy as np
import torch

U = 2.0 ** -24
MAXSEG = MAXGROUP = 8
BIG, SMALL, BAND, XCDS = 128, 64, 8, 8
OPT_LEAN, OPT_NO_DMA = 1, 2
MIB = 1 << 20
ERR_SHAPE, ERR_ARG = -1, -5
LAYOUTS = ('packed', 'padded4', 'ld_plus_1', 'offset_1')
KLAYS = ((1, 1), (1, 0), (0, 1), (0, 0))            # (a_kfast, b_kfast)
YARD_FACTOR = 4.0


def force(s):
    return (s & 31) << 8


def cdiv(a, b):
    return (a + b - 1) // b


def up4(v):
    return (v + 3) // 4 * 4


def lay2(cols, variant):
    """leading dimension and base offset (floats) of a row-major operand with `cols` columns"""
    return {'packed': (cols, 0), 'padded4': (cols + 4, 0), 'ld_plus_1': (cols + 1, 0), 'offset_1': (up4(cols), 1)}[variant]


class Case(dict):
    """One call.  M, N, Ks (K of every segment), ak / bk (a_kfast / b_kfast), G groups, bias: which segments carry one,
    acc, layA / layB / layC, soff: bias, a_colsum and the LSTM state one float off, colsum: the a_colsum rider,
    ws: workspace bytes (0: none), ws_off: its base offset in floats, flags, tickets: None or the number of counters
    relative to the tile count (0: exactly as many, -1: one fewer), cprev: 'rand' | 'quarter' | 'nan'."""
    __getattr__ = dict.__getitem__


def case(name, M, N, Ks, ak=1, bk=1, G=1, bias='all', acc=0, layA='packed', layB='packed', layC='packed', soff=0,
         colsum=False, ws=0, ws_off=0, flags=0, tickets=None, cprev='rand'):
    Ks = list(Ks)
    if bias == 'all':
        bias = [True] * len(Ks)
    elif bias == 'none':
        bias = [False] * len(Ks)
    elif bias == 'some':
        bias = [s % 2 == 0 for s in range(len(Ks))]
    return Case(name=name, M=M, N=N, Ks=Ks, ak=ak, bk=bk, G=G, bias=list(bias), acc=acc, layA=layA, layB=layB, layC=layC,
                soff=soff, colsum=colsum, ws=ws, ws_off=ws_off, flags=flags, tickets=tickets, cprev=cprev)


def but(c, **kw):
    d = Case(c)
    d.update(kw)
    return d


# =================================================================================================================
# the model
# =================================================================================================================
def k_ranges(Ks, BK, splitk, unit=None):
    """[(first k, last k + 1)] of every K range in the flattened k space of the segments, as gemm_tile / gemm_tile_dma
    cut them: per = ceil(steps / splitk) steps of BK -- counted in steps of `unit` (>= BK) when the kernel's ranges follow
    another kernel's step.  Steps never straddle segments (a segment's last step is short)."""
    unit = unit or BK
    ru = unit // BK if unit > BK else 1
    steps = []                                      # (k begin, k end) of every BK step
    base = 0
    for K in Ks:
        for i in range(cdiv(K, BK)):
            steps.append((base + i * BK, base + min(K, (i + 1) * BK)))
        base += K
    total = len(steps)
    if splitk <= 1:
        return [(0, base)]
    per = cdiv(total // ru, splitk) * ru
    out = []
    for ks in range(splitk):
        b, e = min(total, ks * per), min(total, ks * per + per)
        out.append((steps[b][0], steps[e - 1][1]) if e > b else (base, base))
    return out


def split_cost_model(big, iters32, cap, M, N, G):
    part_us = float(M) * N * G * 4.0 / 4.0e6
    want, best, s = 1, 1e30, 1
    while s <= 16 and s <= cap and (s == 1 or s <= iters32 // 8):
        nb = big * s
        full, rem = nb // 512, nb % 512
        t = 3.9 * (float(full) + (0.0 if rem == 0 else 1.0 if rem > 256 else 0.6)) * float((iters32 + s - 1) // s)
        if s > 1:
            t += 6.0 + s * part_us
        if t < best * 0.97:
            best, want = t, s
        s += 1
    return want


def plan(c, slots=64, lstm=False):
    """What the library does with the call: a dict with kind ('noop' | 'refused' | 'run') and, for a run, vec, tile, kernel
    ('dma' | 'dma_ragged' | 'fast' | 'reg'), BK, unit (the step its K ranges are counted in), splitk, ranges, empty (number
    of empty K ranges), finish ('none' | 'reduce_v4' | 'reduce_scalar' | 'lstm' | 'ticket'), tail (0 | 2 | 4), tiles, nblk,
    ws_floats (floats of the workspace the launch writes)."""
    M, N, G, Ks, ak, bk = c.M, c.N, c.G, c.Ks, c.ak, c.bk
    if M <= 0 or N <= 0:
        return dict(kind='noop')
    if G < 1 or G > MAXGROUP or len(Ks) < 1 or len(Ks) > MAXSEG:
        return dict(kind='refused', code=ERR_SHAPE)
    if any(K < 0 for K in Ks):
        return dict(kind='refused', code=ERR_ARG)
    if any(K == 0 for K in Ks) and any(K > 0 for K in Ks):
        return dict(kind='refused', code=ERR_SHAPE)
    vec = True
    for K in Ks:
        lda, offa = lay2(K if ak else M, c.layA)
        ldb, offb = lay2(K if bk else N, c.layB)
        vec = vec and offa % 4 == 0 and lda % 4 == 0 and (K % 4 == 0 if ak else M % 4 == 0)
        vec = vec and offb % 4 == 0 and ldb % 4 == 0 and (K % 4 == 0 if bk else N % 4 == 0)
    part = c.ws >= MIB and c.ws_off % 4 == 0
    ws_mib = c.ws >> 20
    big = cdiv(M, BIG) * cdiv(N, BIG) * G
    iters32 = sum(cdiv(K, 32) for K in Ks)
    flops = sum(2.0 * M * N * K * G for K in Ks)
    lean, no_dma = bool(c.flags & OPT_LEAN), bool(c.flags & OPT_NO_DMA)
    cap = ws_mib * (1 << 18) // ((M * N + M) * G)
    big_split, big_unsplit = 1, False
    if big <= 1023 and part and big >= 16 and flops >= 6e9:
        want = split_cost_model(big, iters32, cap, M, N, G)
        forced = (c.flags >> 8) & 31
        if 1 <= forced <= cap and forced <= iters32:
            want = forced
        big_split = want if want >= 2 else 1
        big_unsplit = want == 1 and ((cap >= 2 and iters32 // 8 >= 2) or forced == 1)
    p = dict(kind='run', vec=vec, cap=cap)
    if big >= 384 or big_split > 1 or big_unsplit:
        tile, splitk = BIG, big_split
        kdiv = all(K > 0 and K % 32 == 0 for K in Ks)
        fast = vec and kdiv and M % BIG == 0 and N % BIG == 0
        dma_ok = vec and (fast or (kdiv and ak and bk))
        if dma_ok and not c.colsum and not no_dma:
            kernel = 'dma' if fast else 'dma_ragged'
            unit = 32 if (ak and bk) else 16
            BK = 16 if lean else unit
        else:
            kernel, BK, unit = ('fast' if fast else 'reg'), 32, 32
        two_body = vec and ak and bk and kernel != 'reg'          # FAST && AK && BKF && VEC (&& DMA or one stage)
    else:
        tile, splitk = SMALL, 1
        if part:
            tiles = cdiv(M, SMALL) * cdiv(N, SMALL) * G
            want = min(768 // tiles, iters32 // 4, 16, cap)
            splitk = want if want >= 2 else 1
        ok = vec and ((ak and bk) or (M % 64 == 0 and N % 64 == 0)) and not c.colsum and not no_dma
        ok = ok and all(K > 0 and K % 32 == 0 for K in Ks)
        kernel = ('dma' if M % 64 == 0 and N % 64 == 0 else 'dma_ragged') if ok else 'reg'
        BK = unit = 32
        two_body = False
    tiles = cdiv(M, tile) * cdiv(N, tile) * G
    nblk = tiles * splitk
    tail = 0
    if two_body and splitk == 1 and nblk % XCDS == 0:
        q = nblk // XCDS
        t = q % slots
        if q // slots >= 2 and t > 0 and 2 * t <= slots:
            tail = 4 if 4 * t <= slots else 2
    ranges = k_ranges(Ks, BK, splitk, unit)
    finish = 'none'
    if splitk > 1:
        n_tickets = None if c.tickets is None else tiles + c.tickets
        if lstm:
            finish = 'lstm'
        elif n_tickets is not None and n_tickets > 0 and tiles <= n_tickets:
            finish = 'ticket'
        else:
            ldc, offc = lay2(N, c.layC)
            v4 = N % 4 == 0 and offc % 4 == 0 and ldc % 4 == 0 and not (c.soff and any(c.bias))
            finish = 'reduce_v4' if v4 else 'reduce_scalar'
    p.update(tile=tile, kernel=kernel, BK=BK, unit=unit, splitk=splitk, ranges=ranges, tiles=tiles, nblk=nblk, tail=tail,
             empty=sum(1 for b, e in ranges if e <= b) if splitk > 1 else 0, finish=finish,
             tiles_m=cdiv(M, tile), nc=cdiv(N, tile) * G,
             ws_floats=(M * N * G * splitk + (M * G * splitk if c.colsum else 0)) if splitk > 1 else 0)
    return p


def same_ranges(c, flags):
    """do the calls with `flags` and with the default flags cut the same K ranges (-> bit-identical results)?"""
    p0, p1 = plan(but(c, flags=c.flags & ~3)), plan(but(c, flags=(c.flags & ~3) | flags))
    return p0['splitk'] == p1['splitk'] and p0['ranges'] == p1['ranges']


# =================================================================================================================
# inputs and references
# =================================================================================================================
def make_inputs(c, groups=None):
    """Logical operands on the CPU: A[g][s] (M, K_s), B[g][s] (N, K_s), bias[g][s] (N,) or None, prev[g] (M, N),
    csprev[g] (M,).  Seeded by the case's name and shape, so that every layout of a shape gets the same values."""
    gen = torch.Generator().manual_seed(zlib.crc32(('%d %d %s' % (c.M, c.N, c.Ks)).encode()))
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    out = dict(A=[], B=[], bias=[], prev=[], csprev=[])
    for g in range(c.G if groups is None else groups):
        out['A'].append([r(c.M, K) for K in c.Ks])
        out['B'].append([r(c.N, K) for K in c.Ks])
        out['bias'].append([r(c.N) if hb else None for hb in c.bias])
        out['prev'].append(torch.full((c.M, c.N), 0.25) if c.cprev == 'quarter' else r(c.M, c.N))
        out['csprev'].append(r(c.M))
    return out


def ref_group(c, inp, g):
    """fp64 result of group g and the magnitude sum |A||B|^T + sum |bias| + |C_prev| of the hard cap"""
    ref = torch.zeros(c.M, c.N, dtype=torch.float64)
    mag = torch.zeros(c.M, c.N, dtype=torch.float64)
    for s in range(len(c.Ks)):
        A, B = inp['A'][g][s].double(), inp['B'][g][s].double()
        ref += A @ B.t()
        mag += A.abs() @ B.abs().t()
        if inp['bias'][g][s] is not None:
            ref += inp['bias'][g][s].double()
            mag += inp['bias'][g][s].double().abs()
    if c.acc:
        ref += inp['prev'][g].double()
        mag += inp['prev'][g].double().abs()
    return ref, mag


def ref_colsum(c, inp, g):
    ref = torch.zeros(c.M, dtype=torch.float64)
    mag = torch.zeros(c.M, dtype=torch.float64)
    for s in range(len(c.Ks)):
        ref += inp['A'][g][s].double().sum(1)
        mag += inp['A'][g][s].double().abs().sum(1)
    if c.acc:
        ref += inp['csprev'][g].double()
        mag += inp['csprev'][g].double().abs()
    return ref, mag


def seq_fp32_group(c, inp, g):
    """the yardstick's product: one fp32 accumulator per element, k in order, biases in segment order, then C_prev"""
    acc = np.zeros((c.M, c.N), dtype=np.float32)
    for s in range(len(c.Ks)):
        A, B = inp['A'][g][s].numpy(), inp['B'][g][s].numpy()
        for k in range(c.Ks[s]):
            acc += A[:, k:k + 1] * B[:, k]
    bsum = np.zeros((c.N,), dtype=np.float32)
    for s in range(len(c.Ks)):
        if inp['bias'][g][s] is not None:
            bsum += inp['bias'][g][s].numpy()
    acc = acc + bsum
    if c.acc:
        acc = acc + inp['prev'][g].numpy()
    return torch.from_numpy(acc)


def seq_fp32_colsum(c, inp, g):
    acc = np.zeros((c.M,), dtype=np.float32)
    for s in range(len(c.Ks)):
        A = inp['A'][g][s].numpy()
        for k in range(c.Ks[s]):
            acc += A[:, k]
    if c.acc:
        acc = acc + inp['csprev'][g].numpy()
    return torch.from_numpy(acc)


def yard_key(c):
    """cases that differ only in storage, flags, workspace or finish share their values and therefore their yardstick"""
    return '%dx%dx%s g%d b%s a%d %s' % (c.M, c.N, '+'.join(map(str, c.Ks)), c.G, ''.join('1' if b else '0' for b in c.bias),
                                         c.acc, c.cprev[0]) + (' cs' if c.colsum else '')


def measure_yardstick(c):
    """(C, a_colsum) yardsticks of a case: max error of the sequential fp32 product against fp64 over every group"""
    inp = make_inputs(c)
    yc = ys = 0.0
    for g in range(c.G):
        yc = max(yc, float((seq_fp32_group(c, inp, g).double() - ref_group(c, inp, g)[0]).abs().max()))
        if c.colsum:
            ys = max(ys, float((seq_fp32_colsum(c, inp, g).double() - ref_colsum(c, inp, g)[0]).abs().max()))
    return yc, ys


def check_product(got, ref, mag, c, splitk, yard, what='C'):
    """got (fp32, CPU) against the fp64 reference: the derived element-wise cap and 4 x the measured yardstick.
    -> (max error, worst fraction of the cap) for reporting."""
    assert not bool(torch.isnan(got).any()), '%s of %s holds a NaN' % (what, c.name)
    err = (got.double() - ref).abs()
    cap = (sum(c.Ks) + len(c.Ks) + splitk + 2) * U * mag
    worst = float(err.max()) if err.numel() else 0.0
    frac = float((err / cap.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= cap).all()), '%s of %s: %.3g of the worst-case bound' % (what, c.name, frac)
    assert worst <= YARD_FACTOR * yard, '%s of %s: max error %.3g > 4 x yardstick %.3g' % (what, c.name, worst, yard)
    return worst, frac


# =================================================================================================================
# the table
# =================================================================================================================
WS_BIG = 256 * MIB
WS_8 = 8 * MIB


def _tile_cases():
    """64 x 64 tile and block bookkeeping: tiles_m x (groups * tiles_n), ragged last tiles, K = 4 and 36, both accumulate
    modes: pins the XCD remap for nblk % 8 != 0 and a ragged last band of 8 row tiles."""
    out, i = [], 0
    for tm in (1, 7, 8, 9, 17):
        for G, tn in ((1, 1), (3, 1), (2, 4)):
            for K in (4, 36):
                for acc in (0, 1):
                    ak, bk = KLAYS[i % 4]
                    M = 64 * (tm - 1) + (37 if i % 2 else 64 if i % 3 == 0 else 20)
                    N = 64 * (tn - 1) + (21 if i % 4 < 2 else 48)
                    out.append(case('tile tm%d nc%d K%d acc%d' % (tm, G * tn, K, acc), M, N, [K], ak, bk, G,
                                    bias='all' if i % 3 else 'none', acc=acc, cprev='quarter' if acc else 'nan',
                                    layA=LAYOUTS[(i // 4) % 4] if i % 5 == 0 else 'packed',
                                    layC=LAYOUTS[(i // 2) % 4]))
                    i += 1
    return out


def _k_cases():
    out = []
    for ak, bk in KLAYS:
        for K in (1, 3, 4, 31, 32, 33, 36, 64, 68):
            out.append(case('k %d%d K%d' % (ak, bk, K), 68, 72, [K], ak, bk, bias='all', acc=K % 2))
    segsets = [[36, 4], [4, 32, 33], [32, 64, 32, 96], [1, 3, 4, 31, 32, 33, 36, 68], [32] * 8, [4, 8, 12, 16, 20, 24, 28, 36]]
    for i, Ks in enumerate(segsets):
        for j, (ak, bk) in enumerate(KLAYS):
            out.append(case('seg %d%d %s' % (ak, bk, '+'.join(map(str, Ks))), 68, 72, Ks, ak, bk, G=1 + (i + j) % 3,
                            bias=('all', 'some', 'none')[(i + j) % 3], acc=(i + j) % 2))
    for ak, bk in KLAYS:
        out.append(case('maxgroup %d%d' % (ak, bk), 68, 72, [32, 36], ak, bk, G=MAXGROUP, bias='some'))
    # operand layouts on each of A, B, C in turn, and the scalar-accessed riders one float off
    for ak, bk in KLAYS:
        for lay in LAYOUTS[1:]:
            for which in ('layA', 'layB', 'layC'):
                out.append(but(case('lay %d%d %s %s' % (ak, bk, which, lay), 68, 72, [32, 36], ak, bk, G=2, bias='some', acc=1),
                               **{which: lay}))
        out.append(case('lay %d%d soff' % (ak, bk), 68, 72, [32, 36], ak, bk, G=2, bias='all', soff=1))
    # all segments empty: C (+)= sum of the biases
    for ak, bk in ((1, 1), (0, 0)):
        for acc in (0, 1):
            out.append(case('k0 all %d%d acc%d' % (ak, bk, acc), 68, 72, [0, 0, 0], ak, bk, bias='some', acc=acc))
    return out


def _k0_refused():
    out = []
    for ak, bk in KLAYS:
        for Ks in ([0, 32, 32], [32, 0, 32], [32, 32, 0], [0, 36], [4, 0]):
            out.append(case('k0 %d%d %s' % (ak, bk, '+'.join(map(str, Ks))), 68, 72, Ks, ak, bk, bias='all'))
    return out


def _big_cases():
    """>= 384 big tiles: 8 groups of 768 x 1024 (6 x 8 tiles each) and ragged versions with as many tiles"""
    out = []
    for ak, bk in KLAYS:
        t = '%d%d' % (ak, bk)
        out += [case('big %s interior K32' % t, 768, 1024, [32], ak, bk, G=8, bias='all'),
                case('big %s interior K96 acc' % t, 768, 1024, [64, 32], ak, bk, G=8, bias='some', acc=1),
                case('big %s ragged K32' % t, 700, 900, [32], ak, bk, G=8, bias='all', acc=1, layC='ld_plus_1'),
                case('big %s odd K96' % t, 701, 901, [96], ak, bk, G=8, bias='none'),
                case('big %s K16' % t, 768, 1024, [16], ak, bk, G=8, bias='all'),
                case('big %s K40 ragged' % t, 700, 1024, [40], ak, bk, G=8, bias='all', layA='padded4'),
                case('big %s K7' % t, 768, 900, [7], ak, bk, G=8, bias='all', acc=1),
                case('big %s offset_1 A' % t, 768, 1024, [32], ak, bk, G=8, bias='all', layA='offset_1'),
                case('big %s offset_1 B ragged' % t, 700, 900, [32], ak, bk, G=8, bias='all', layB='offset_1', soff=1)]
    return out


def _tail_cases():
    out = []
    for tiles, (tm, tn) in ((208, (13, 16)), (220, (11, 20)), (242, (11, 22))):
        out.append(case('tail %d interior' % tiles, 128 * tm, 128 * tn, [32], G=8, bias='all'))
        out.append(case('tail %d ragged' % tiles, 128 * (tm - 1) + 8, 128 * (tn - 1) + 16, [32], G=8, bias='all'))
    return out


def _split64_cases():
    out = []
    for ak, bk in KLAYS:
        t = '%d%d' % (ak, bk)
        out += [case('s64 %s K2080' % t, 64, 64, [2080], ak, bk, ws=WS_8),
                case('s64 %s K800 acc' % t, 64, 64, [800], ak, bk, acc=1, ws=WS_8),
                case('s64 %s 3seg g3' % t, 64, 64, [64, 160, 96], ak, bk, G=3, bias='some', ws=WS_8),
                case('s64 %s ragged' % t, 52, 40, [800], ak, bk, acc=1, ws=WS_8),
                case('s64 %s N42' % t, 64, 42, [800], ak, bk, G=3, ws=WS_8),
                case('s64 %s offset_1 C' % t, 64, 64, [800], ak, bk, layC='offset_1', acc=1, ws=WS_8),
                case('s64 %s offset_1 bias' % t, 64, 64, [2080], ak, bk, soff=1, ws=WS_8),
                case('s64 %s K804' % t, 70, 68, [804], ak, bk, G=3, acc=1, ws=WS_8)]
    return out


def _medium_cases():
    """the smallest product the medium gate admits: 16 big tiles, 6.006e9 flop"""
    out = []
    for ak, bk in KLAYS:
        for s in (0, 1, 2, 3, 5, 7, 31):
            out.append(case('medium %d%d s%d' % (ak, bk, s), 512, 512, [11456], ak, bk, bias='all', ws=WS_BIG, flags=force(s)))
    return out


def _medium_ragged_cases():
    """the same gate with ragged tiles: the ragged LDS-DMA form ([row][k] x [row][k]) and the bounds-checked kernel, split"""
    return [case('medium ragged %d%d s3' % (ak, bk), 500, 508, [11840], ak, bk, bias='all', acc=1, ws=WS_BIG, flags=force(3))
            for ak, bk in KLAYS]


def _colsum_cases():
    out = []
    for bk in (0, 1):
        t = '0%d' % bk
        out += [case('cs %s vec' % t, 68, 72, [36], 0, bk, G=2, colsum=True),
                case('cs %s scalar M37 acc' % t, 37, 72, [36, 5], 0, bk, colsum=True, acc=1),
                case('cs %s ragged M' % t, 100, 72, [64], 0, bk, G=3, colsum=True, acc=1),
                case('cs %s split' % t, 68, 72, [800], 0, bk, G=2, colsum=True, ws=WS_8),
                case('cs %s split scalar M37 acc' % t, 37, 72, [801], 0, bk, colsum=True, acc=1, ws=WS_8),
                case('cs %s split interior' % t, 64, 64, [800], 0, bk, colsum=True, acc=1, ws=WS_8, soff=1),
                case('cs %s big' % t, 768, 1024, [40], 0, bk, G=8, colsum=True),
                case('cs %s big interior acc' % t, 768, 1024, [32], 0, bk, G=8, colsum=True, acc=1),
                case('cs %s big scalar' % t, 701, 1024, [32], 0, bk, G=8, colsum=True),
                case('cs %s medium s3' % t, 512, 512, [11456], 0, bk, colsum=True, ws=WS_BIG, flags=force(3))]
    return out


def _ws_cases():
    """M = N = 256: 65536 + 256 floats per K range.  2 MiB: cap = 7 (7.97), and 8 if the + M of the colsum slab were left
    out -- whose slab would then lie past ws_bytes.  1 MiB: cap = 3."""
    out = []
    for ak, bk, cs in ((1, 1, False), (0, 0, True), (0, 1, True)):
        t = '%d%d' % (ak, bk)
        out += [case('ws %s cap=want' % t, 256, 256, [896], ak, bk, colsum=cs, ws=2 * MIB),
                case('ws %s cap<want' % t, 256, 256, [1024], ak, bk, colsum=cs, ws=2 * MIB),
                case('ws %s 1 MiB less' % t, 256, 256, [896], ak, bk, colsum=cs, ws=1 * MIB),
                case('ws %s too small' % t, 256, 256, [896], ak, bk, colsum=cs, ws=MIB - 16),
                case('ws %s misaligned' % t, 256, 256, [896], ak, bk, colsum=cs, ws=2 * MIB, ws_off=1)]
    return out


def _lstm_cases():
    """gate GEMMs (N = 4R).  M * R is no multiple of 256 anywhere."""
    out = []
    for drop in (0.0, 0.3):
        out += [but(case('lstm unsplit p%g' % drop, 6, 160, [96, 64], G=3, bias='some'), drop=drop),
                but(case('lstm split p%g' % drop, 6, 160, [192, 128], G=3, bias='some', ws=WS_8, soff=1), drop=drop),
                but(case('lstm split g1 p%g' % drop, 37, 44, [801], G=1, bias='all', ws=WS_8), drop=drop),
                but(case('lstm split padded p%g' % drop, 70, 264, [256, 64], G=3, bias='all', ws=WS_8, layC='padded4'), drop=drop)]
    return out


TILE_CASES, K_CASES, K0_REFUSED = _tile_cases(), _k_cases(), _k0_refused()
BIG_CASES, TAIL_CASES, SPLIT64_CASES = _big_cases(), _tail_cases(), _split64_cases()
MEDIUM_CASES, COLSUM_CASES, WS_CASES, LSTM_CASES = _medium_cases(), _colsum_cases(), _ws_cases(), _lstm_cases()
MEDIUM_RAGGED_CASES = _medium_ragged_cases()
FP64_CASES = TILE_CASES + K_CASES + BIG_CASES + TAIL_CASES + SPLIT64_CASES + MEDIUM_CASES + MEDIUM_RAGGED_CASES + COLSUM_CASES + WS_CASES
ALL_CASES = FP64_CASES + K0_REFUSED + LSTM_CASES
FLAG_SETS = (0, OPT_NO_DMA, OPT_LEAN, OPT_NO_DMA | OPT_LEAN)

# ---- measured yardsticks: yard_key(case) -> (C, a_colsum); re-measure with `python tests/gemm_cases.py` -------------------
YARD = {
    '64x21x4 g1 b0 a0 n': (6.42e-07, 0),
    '37x21x4 g1 b1 a1 q': (5.86e-07, 0),
    '20x48x36 g1 b1 a0 n': (3.06e-06, 0),
    '37x48x36 g1 b0 a1 q': (5.78e-06, 0),
    '20x21x4 g3 b1 a0 n': (8.16e-07, 0),
    '37x21x4 g3 b1 a1 q': (8.17e-07, 0),
    '64x48x36 g3 b0 a0 n': (5.64e-06, 0),
    '37x48x36 g3 b1 a1 q': (5.66e-06, 0),
    '20x213x4 g2 b1 a0 n': (1e-06, 0),
    '37x213x4 g2 b0 a1 q': (7.26e-07, 0),
    '20x240x36 g2 b1 a0 n': (5.28e-06, 0),
    '37x240x36 g2 b1 a1 q': (5.88e-06, 0),
    '448x21x4 g1 b0 a0 n': (7.89e-07, 0),
    '421x21x4 g1 b1 a1 q': (1.01e-06, 0),
    '404x48x36 g1 b1 a0 n': (5.82e-06, 0),
    '421x48x36 g1 b0 a1 q': (5.9e-06, 0),
    '404x21x4 g3 b1 a0 n': (9.62e-07, 0),
    '421x21x4 g3 b1 a1 q': (1.37e-06, 0),
    '448x48x36 g3 b0 a0 n': (7.47e-06, 0),
    '421x48x36 g3 b1 a1 q': (6.96e-06, 0),
    '404x213x4 g2 b1 a0 n': (1.35e-06, 0),
    '421x213x4 g2 b0 a1 q': (1.27e-06, 0),
    '404x240x36 g2 b1 a0 n': (8.91e-06, 0),
    '421x240x36 g2 b1 a1 q': (7.87e-06, 0),
    '512x21x4 g1 b0 a0 n': (8.45e-07, 0),
    '485x21x4 g1 b1 a1 q': (1.2e-06, 0),
    '468x48x36 g1 b1 a0 n': (5.9e-06, 0),
    '485x48x36 g1 b0 a1 q': (6.96e-06, 0),
    '468x21x4 g3 b1 a0 n': (1.18e-06, 0),
    '485x21x4 g3 b1 a1 q': (1.2e-06, 0),
    '512x48x36 g3 b0 a0 n': (6.17e-06, 0),
    '485x48x36 g3 b1 a1 q': (7.59e-06, 0),
    '468x213x4 g2 b1 a0 n': (1.42e-06, 0),
    '485x213x4 g2 b0 a1 q': (1.58e-06, 0),
    '468x240x36 g2 b1 a0 n': (7.77e-06, 0),
    '485x240x36 g2 b1 a1 q': (7.34e-06, 0),
    '576x21x4 g1 b0 a0 n': (6.98e-07, 0),
    '549x21x4 g1 b1 a1 q': (8.83e-07, 0),
    '532x48x36 g1 b1 a0 n': (6.87e-06, 0),
    '549x48x36 g1 b0 a1 q': (6.4e-06, 0),
    '532x21x4 g3 b1 a0 n': (1.09e-06, 0),
    '549x21x4 g3 b1 a1 q': (1.22e-06, 0),
    '576x48x36 g3 b0 a0 n': (7.3e-06, 0),
    '549x48x36 g3 b1 a1 q': (8.22e-06, 0),
    '532x213x4 g2 b1 a0 n': (2.4e-06, 0),
    '549x213x4 g2 b0 a1 q': (1.16e-06, 0),
    '532x240x36 g2 b1 a0 n': (7.28e-06, 0),
    '549x240x36 g2 b1 a1 q': (7.25e-06, 0),
    '1088x21x4 g1 b0 a0 n': (1.07e-06, 0),
    '1061x21x4 g1 b1 a1 q': (1.49e-06, 0),
    '1044x48x36 g1 b1 a0 n': (6.06e-06, 0),
    '1061x48x36 g1 b0 a1 q': (6.85e-06, 0),
    '1044x21x4 g3 b1 a0 n': (1.32e-06, 0),
    '1061x21x4 g3 b1 a1 q': (1.49e-06, 0),
    '1088x48x36 g3 b0 a0 n': (7.03e-06, 0),
    '1061x48x36 g3 b1 a1 q': (7.21e-06, 0),
    '1044x213x4 g2 b1 a0 n': (1.98e-06, 0),
    '1061x213x4 g2 b0 a1 q': (1.23e-06, 0),
    '1044x240x36 g2 b1 a0 n': (8.03e-06, 0),
    '1061x240x36 g2 b1 a1 q': (8.66e-06, 0),
    '68x72x1 g1 b1 a1 r': (5.03e-07, 0),
    '68x72x3 g1 b1 a1 r': (8.06e-07, 0),
    '68x72x4 g1 b1 a0 r': (9.9e-07, 0),
    '68x72x31 g1 b1 a1 r': (3.79e-06, 0),
    '68x72x32 g1 b1 a0 r': (4.27e-06, 0),
    '68x72x33 g1 b1 a1 r': (4.44e-06, 0),
    '68x72x36 g1 b1 a0 r': (4.34e-06, 0),
    '68x72x64 g1 b1 a0 r': (9.14e-06, 0),
    '68x72x68 g1 b1 a0 r': (1.11e-05, 0),
    '68x72x36+4 g1 b11 a0 r': (5.94e-06, 0),
    '68x72x36+4 g2 b10 a1 r': (5.88e-06, 0),
    '68x72x36+4 g3 b00 a0 r': (7.56e-06, 0),
    '68x72x36+4 g1 b11 a1 r': (5.93e-06, 0),
    '68x72x4+32+33 g2 b101 a1 r': (1.07e-05, 0),
    '68x72x4+32+33 g3 b000 a0 r': (1.1e-05, 0),
    '68x72x4+32+33 g1 b111 a1 r': (9.73e-06, 0),
    '68x72x4+32+33 g2 b101 a0 r': (1.09e-05, 0),
    '68x72x32+64+32+96 g3 b0000 a0 r': (4.14e-05, 0),
    '68x72x32+64+32+96 g1 b1111 a1 r': (2.68e-05, 0),
    '68x72x32+64+32+96 g2 b1010 a0 r': (2.72e-05, 0),
    '68x72x32+64+32+96 g3 b0000 a1 r': (4.13e-05, 0),
    '68x72x1+3+4+31+32+33+36+68 g1 b11111111 a1 r': (2.1e-05, 0),
    '68x72x1+3+4+31+32+33+36+68 g2 b10101010 a0 r': (3.34e-05, 0),
    '68x72x1+3+4+31+32+33+36+68 g3 b00000000 a1 r': (2.52e-05, 0),
    '68x72x1+3+4+31+32+33+36+68 g1 b11111111 a0 r': (2.04e-05, 0),
    '68x72x32+32+32+32+32+32+32+32 g2 b10101010 a0 r': (3.16e-05, 0),
    '68x72x32+32+32+32+32+32+32+32 g3 b00000000 a1 r': (3.74e-05, 0),
    '68x72x32+32+32+32+32+32+32+32 g1 b11111111 a0 r': (2.9e-05, 0),
    '68x72x32+32+32+32+32+32+32+32 g2 b10101010 a1 r': (3.25e-05, 0),
    '68x72x4+8+12+16+20+24+28+36 g3 b00000000 a1 r': (2.02e-05, 0),
    '68x72x4+8+12+16+20+24+28+36 g1 b11111111 a0 r': (1.89e-05, 0),
    '68x72x4+8+12+16+20+24+28+36 g2 b10101010 a1 r': (2.37e-05, 0),
    '68x72x4+8+12+16+20+24+28+36 g3 b00000000 a0 r': (1.93e-05, 0),
    '68x72x32+36 g8 b10 a0 r': (1.12e-05, 0),
    '68x72x32+36 g2 b10 a1 r': (8.85e-06, 0),
    '68x72x32+36 g2 b11 a0 r': (8.73e-06, 0),
    '68x72x0+0+0 g1 b101 a0 r': (1.19e-07, 0),
    '68x72x0+0+0 g1 b101 a1 r': (3.58e-07, 0),
    '768x1024x32 g8 b1 a0 r': (8.24e-06, 0),
    '768x1024x64+32 g8 b10 a1 r': (2.53e-05, 0),
    '700x900x32 g8 b1 a1 r': (9.21e-06, 0),
    '701x901x96 g8 b0 a0 r': (2.36e-05, 0),
    '768x1024x16 g8 b1 a0 r': (4.73e-06, 0),
    '700x1024x40 g8 b1 a0 r': (1.07e-05, 0),
    '768x900x7 g8 b1 a1 r': (3.06e-06, 0),
    '700x900x32 g8 b1 a0 r': (9.11e-06, 0),
    '1664x2048x32 g8 b1 a0 r': (9.17e-06, 0),
    '1544x1936x32 g8 b1 a0 r': (9.79e-06, 0),
    '1408x2560x32 g8 b1 a0 r': (9.77e-06, 0),
    '1288x2448x32 g8 b1 a0 r': (9.51e-06, 0),
    '1408x2816x32 g8 b1 a0 r': (1.27e-05, 0),
    '1288x2704x32 g8 b1 a0 r': (9.49e-06, 0),
    '64x64x2080 g1 b1 a0 r': (0.000208, 0),
    '64x64x800 g1 b1 a1 r': (0.00011, 0),
    '64x64x64+160+96 g3 b101 a0 r': (4.68e-05, 0),
    '52x40x800 g1 b1 a1 r': (8.27e-05, 0),
    '64x42x800 g3 b1 a0 r': (0.000129, 0),
    '70x68x804 g3 b1 a1 r': (0.00011, 0),
    '512x512x11456 g1 b1 a0 r': (0.00194, 0),
    '500x508x11840 g1 b1 a1 r': (0.00256, 0),
    '68x72x36 g2 b1 a0 r cs': (5.38e-06, 3.34e-06),
    '37x72x36+5 g1 b11 a1 r cs': (5.21e-06, 2.87e-06),
    '100x72x64 g3 b1 a1 r cs': (1.03e-05, 3.84e-06),
    '68x72x800 g2 b1 a0 r cs': (0.000136, 8.14e-05),
    '37x72x801 g1 b1 a1 r cs': (0.000103, 3.83e-05),
    '64x64x800 g1 b1 a1 r cs': (0.00011, 5.19e-05),
    '768x1024x40 g8 b1 a0 r cs': (1.18e-05, 4.6e-06),
    '768x1024x32 g8 b1 a1 r cs': (9.01e-06, 3.1e-06),
    '701x1024x32 g8 b1 a0 r cs': (9.2e-06, 5.86e-06),
    '512x512x11456 g1 b1 a0 r cs': (0.00194, 0.000892),
    '256x256x896 g1 b1 a0 r': (0.000151, 0),
    '256x256x1024 g1 b1 a0 r': (0.000192, 0),
    '256x256x896 g1 b1 a0 r cs': (0.000151, 9.03e-05),
    '256x256x1024 g1 b1 a0 r cs': (0.000192, 0.000153),
}


def yard(c):
    return YARD[yard_key(c)]


def print_table():
    seen = {}
    for c in FP64_CASES:
        k = yard_key(c)
        if k not in seen:
            seen[k] = measure_yardstick(c)
            print("    %r: (%.3g, %.3g)," % (k, seen[k][0], seen[k][1]), flush=True)


if __name__ == '__main__':
    print_table()
