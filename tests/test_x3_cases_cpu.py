"""The tables of the bf16-plane GEMM sweep reach every branch they are meant to reach (tests/x3_cases.py: a plain-Python
restatement of the host side of csrc/rfn_gemm_x3.hip), the modelled tile walk computes every quarter of every tile exactly
once, and the tolerances tell a dropped plane product or a dropped 32-wide piece of K from rounding.  No GPU."""
import numpy as np
import pytest
import torch

import x3_cases as XC
from x3_cases import U


# =================================================================================================================
# branch coverage
# =================================================================================================================
def test_base_shapes_reach_every_epilogue_on_both_image_kinds():
    for kind in XC.KINDS:
        seen = {}
        for M, N, K in XC.BASE_SHAPES:
            for lay in XC.LAYOUTS:
                ldc, off = XC.lay2(N, lay)
                e = XC.epilogues(kind, M, N, ldc, off)
                for k, v in e.items():
                    if v:
                        seen.setdefault(k, set()).add(lay)
        assert seen['vector'] == {'packed', 'padded4'}, 'the 16-byte epilogue needs an aligned C and ldc % 4 == 0'
        assert seen['scalar'] == set(XC.LAYOUTS), 'ragged wave tiles (packed) and misaligned ones (ldc + 1, base + 1)'
        assert 'skip' in seen
    # a wave tile runs the scalar epilogue for alignment alone: an interior shape, every wave tile whole
    for kind in XC.KINDS:
        assert XC.epilogues(kind, 256, 256, 256) == {'skip': 0, 'vector': 8, 'scalar': 0}
        assert XC.epilogues(kind, 256, 256, 260) == {'skip': 0, 'vector': 8, 'scalar': 0}
        assert XC.epilogues(kind, 256, 256, 261) == {'skip': 0, 'vector': 0, 'scalar': 8}
        assert XC.epilogues(kind, 256, 256, 260, 1) == {'skip': 0, 'vector': 0, 'scalar': 8}
        assert XC.epilogues(kind, 256, 256, 256, accumulate=True) == {'skip': 0, 'vector': 0, 'scalar': 8}
    assert (256, 256, 40) in XC.EPILOGUE_SHAPES and all(s in XC.BASE_SHAPES for s in XC.EPILOGUE_SHAPES)
    # every epilogue shape but the interior one mixes both epilogues in one launch of an aligned C
    for M, N, K in XC.EPILOGUE_SHAPES[1:]:
        for kind in XC.KINDS:
            e = XC.epilogues(kind, M, N, N)
            assert e['vector'] and e['scalar'], (kind, M, N, e)


def test_wave_tile_edges_return_whole_wave_tiles_early():
    """M in {65, 129}, N in {68, 132}: rows 64 x 4 (fragment order) and 128 x 2 (k-slow), columns 128 x 2 and 64 x 4"""
    skips = {kind: {(M, N): XC.epilogues(kind, M, N, N)['skip'] for M, N, _ in XC.WAVE_EDGES} for kind in XC.KINDS}
    assert skips['frag'] == {(65, 68): 6, (65, 132): 4, (129, 68): 5, (129, 132): 2}
    assert skips['ks'] == {(65, 68): 6, (65, 132): 5, (129, 68): 4, (129, 132): 2}
    assert {s[0] for s in XC.TILE_EDGES} == {255, 256, 257} and {s[1] for s in XC.TILE_EDGES} == {252, 256, 260}
    assert {s[2] for s in XC.K_EDGES} == {31, 32, 33, 64, 65}
    assert XC.SMALL == [(1, 4, 1), (16, 16, 32), (17, 20, 33)]


def test_split_cases_and_slices():
    M, N, K = XC.SPLIT_SHAPE
    assert XC.k_pad(K) // XC.KC == 11 and N % 4 == 0 and M % 256 == 0
    assert XC.slices(K, 2) == [(0, 192), (192, 330)]
    assert XC.slices(K, 7) == [(0, 64), (64, 128), (128, 192), (192, 256), (256, 320), (320, 330), (330, 330)]
    assert XC.slices(K, 11)[-1] == (320, 330) and all(e > b for b, e in XC.slices(K, 11))
    assert [e > b for b, e in XC.slices(320, 7)] == [True] * 5 + [False] * 2          # nkc = 10, splitk = 7: two empty slices
    assert set(XC.SPLITKS) == {2, 3, 4, 7, 11}
    for sk in XC.SPLITKS:
        sl = XC.slices(K, sk)
        assert sl[0][0] == 0 and max(e for _, e in sl) == K
        assert all(a[1] == b[0] for a, b in zip(sl, sl[1:]))                           # contiguous, in order
        assert XC.gemm_refusal(M, N, K, M, N, N, sk) == XC.OK
        for kind in XC.KINDS:                       # raw partial tiles: vector for whole wave tiles, scalar at the ragged edge
            e = XC.epilogues(kind, M, N, N, splitk=sk)
            assert e['vector'] and e['scalar'] and e['skip']
    assert XC.gemm_refusal(M, N, K, M, N, N, 12) == XC.ERR_SHAPE
    names = [o[0] for o in XC.SPLIT_OPTS]
    assert names == ['plain', 'gm', 'bias', 'accumulate', 'ldc', 'all']
    assert XC.SPLIT_OPTS[-1][1:] == (256, True, True, 'padded4')
    m, n, k, gn, sk = XC.SPLIT_GN
    assert XC.cdiv(n, gn) == 2 and XC.gemm_refusal(m, n, k, m, gn, gn, sk) == XC.OK and XC.k_pad(k) // XC.KC == sk


@pytest.mark.parametrize('cus', [64, 256, 304])
def test_tail_shape_has_a_tail_under_three_tile_columns(cus):
    M, N, K = XC.tail_shape(cus)
    tm, tn = XC.cdiv(M, 256), XC.cdiv(N, 256)
    assert tn == 3 and tm == XC.cdiv(2 * cus + 1, 3) and M % 256 == 156 and N % 256 == 252 and M % 4 == 0
    assert XC.has_tail(M, N, cus) and not XC.has_tail(M, N, cus, splitk=2) and not XC.has_tail(300, N, cus)
    main = XC.main_tiles(tm * tn, cus)
    assert main == 2 * cus and 1 <= tm * tn - main <= 3
    assert XC.gemm_refusal(M, N, K, M, 256, 256, 1) == XC.OK                             # gn = 256 groups
    # the existing tail test walks 16 tile columns: whole groups of 4 only; here every index lies in the ragged group
    for kind in XC.KINDS:
        e = XC.epilogues(kind, M, N, 256, cus=cus, gn=256)
        assert e['vector'] and e['scalar'] and e['skip']


def test_walk_and_group_cases():
    assert [(XC.cdiv(M, 256), XC.cdiv(N, 256)) for M, N, _ in XC.WALK] == [(9, 5), (17, 3)]
    for M, N, _ in XC.WALK:                         # a ragged band together with a ragged column group
        assert XC.cdiv(M, 256) % XC.BAND_ROWS and XC.cdiv(N, 256) % XC.BAND_COLS
    by = {c[0]: c for c in XC.GROUP_CASES}
    _, M, N, K, gm, gn, bias = by['row groups 188 short']
    assert M % gm == 188 and gn is None
    _, M, N, K, gm, gn, bias = by['column groups 88 short bias']
    assert N % gn == 88 and gm is None and bias
    _, M, N, K, gm, gn, bias = by['both']
    assert M % gm == 188 and N % gn == 88
    _, M, N, K, gm, gn, bias = by['64 groups']
    assert XC.cdiv(M, gm) * XC.cdiv(N, gn) == XC.MAX_GROUPS and K == 8
    for _, M, N, K, gm, gn, bias in XC.GROUP_CASES:
        assert XC.gemm_refusal(M, N, K, gm or M, gn or N, gn or N, 1) == XC.OK
    assert XC.gemm_refusal(17 * 256, 4 * 256, 8, 256, 256, 256, 1) == XC.ERR_SHAPE       # 68 groups
    assert XC.gemm_refusal(256, 256, 32, 256, 100, 100, 1) == XC.ERR_SHAPE               # gn = 100: three column groups
    assert XC.gemm_refusal(1, 4, 8, 1, 4, 2 ** 22, 1) == XC.ERR_SHAPE and XC.gemm_refusal(1, 4, 8, 1, 4, 2 ** 22 - 4, 1) == XC.OK
    assert XC.gemm_refusal(64, 66, 64, 64, 66, 66, 2) == XC.ERR_ARG and XC.gemm_refusal(64, 64, 64, 64, 64, 64, 2, part=False) == XC.ERR_ARG


def test_image_writer_cases():
    assert XC.split_lanes(45, 48, 0) == {'vec', 'scalar'}                                # K = 45: one image mixes both
    assert XC.split_lanes(45, 45, 0) == XC.split_lanes(45, 49, 0) == XC.split_lanes(45, 48, 1) == {'scalar'}
    assert XC.split_lanes(32, 32, 0) == {'vec'} and XC.split_lanes(7, 8, 0) == {'scalar'}
    assert [XC.pad_launch(g, r) for g, r in ((2, 32), (8, 32), (3, 64), (64, 32))] == [True, False, True, False]
    assert XC.split_refusal(65, 32, 8) == XC.ERR_ARG and XC.split_refusal(2, 48, 8) == XC.ERR_SHAPE
    assert XC.split_refusal(64, 32, 8) == XC.OK and XC.split_refusal(1, 17, 8) == XC.OK
    assert XC.split_ks_refusal(65, 4, 8, 4) == XC.ERR_ARG and XC.split_ks_refusal(1, 8, 8, 6) == XC.ERR_SHAPE
    assert XC.split_ks_refusal(1, 9, 8, 4) == XC.ERR_SHAPE and XC.split_ks_refusal(1, 8, 8, 4, off=1) == XC.ERR_ARG
    assert XC.image_bytes(1, 1) == 256 * 32 * 6 and XC.image_bytes(257, 33) == 512 * 64 * 6 and XC.image_bytes(0, 5) == 0
    assert XC.part_floats(3, 5, 1) == 0 and XC.part_floats(3, 5, 2) == 30


def test_splitk_for_model():
    for cus in (64, 256, 304):
        for M in (1, 256, 257, 2048, 5000):
            for N in (4, 256, 1000, 4096):
                for K in (1, 2047, 2048, 4096, 50176, 200000):
                    s, nkc = XC.splitk_for(M, N, K, cus), XC.k_pad(K) // 32
                    tiles = XC.cdiv(M, 256) * XC.cdiv(N, 256)
                    assert 1 <= s <= nkc and (s == 1 or (tiles < cus and nkc // s >= 64))


# =================================================================================================================
# the tile walk
# =================================================================================================================
def test_the_tile_walk_is_a_bijection():
    """every (tiles_m, tiles_n) of 1..44 x 1..21 and every main_tiles the tail rule can give for some number of CUs: each
    quarter of each tile is computed exactly once -- by a whole-tile block or by one quarter block"""
    checked = 0
    for tm in range(1, 45):
        for tn in range(1, 22):
            tiles = tm * tn
            mains = {tiles} | {XC.main_tiles(tiles, cus) for cus in range(1, tiles // 2 + 1)}
            for main in mains:
                assert 0 < main <= tiles
                cover = XC.coverage(tm, tn, main)
                assert cover.min() == 1 and cover.max() == 1, (tm, tn, main)
                checked += 1
    assert checked > 5000
    for main in range(1, 925):                      # the XCD remap alone, every count
        assert np.array_equal(np.sort(XC.xcd_remap(main)), np.arange(main))
    # the walk of x3_tile_of, spelled out for 9 x 5 tiles: band 0 (8 rows): column groups {0..3}, {4}; band 1: one row
    tmv, tnv = XC.tile_of(np.arange(45), 9, 5)
    assert (tmv[0], tnv[0]) == (0, 0) and (tmv[3], tnv[3]) == (0, 3) and (tmv[4], tnv[4]) == (1, 0)
    assert (tmv[32], tnv[32]) == (0, 4) and (tmv[39], tnv[39]) == (7, 4)
    assert [(int(a), int(b)) for a, b in zip(tmv[40:], tnv[40:])] == [(8, 0), (8, 1), (8, 2), (8, 3), (8, 4)]


# =================================================================================================================
# detection
# =================================================================================================================
DETECT = [('normal', M, N, K) for M, N, K in XC.BASE_SHAPES + XC.WALK + [XC.SPLIT_SHAPE]] + [c[:4] for c in XC.VALUE_CASES]


def test_the_planes_are_an_exact_split():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4000, generator=g) * torch.exp(6 * torch.randn(4000, generator=g))
    x[:6] = torch.tensor([0.0, 1e-30, -3.0e38, 1.0 + 2.0 ** -23, 3.4e38, -1.0])
    p = XC.planes(x)
    assert torch.equal(p[0].double() + p[1].double() + p[2].double(), x.double())
    for q in p:                                     # each plane is a bf16 value
        assert bool(((q.view(torch.int32) & 0xFFFF) == 0).all())
    same = p[0] == x.bfloat16().float()             # the leading plane is the bf16 rounding, but 3.4e38 would round to inf: truncated
    assert bool(same[:4].all()) and bool(same[5:].all()) and float(p[0][4]) < float('inf')


@pytest.mark.parametrize('regime,M,N,K', DETECT, ids=['%s_%dx%dx%d' % c for c in DETECT])
def test_the_bars_tell_a_dropped_product_from_rounding(regime, M, N, K):
    """The reference alone passes: the six plane products of the exactly split operands, summed in fp64, stay inside the
    bar of the case and inside the hard cap.  With any one product left out, or one 32-wide piece of K, they leave the bar.
    (The 1 x 4 x 1 case has four outputs: a low plane can be zero there by chance, so it only checks the first half.)"""
    a, b, _, _ = XC.operands(M, N, K, regime)
    ref, mag = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
    bar = XC.bar(regime, M, N, K)
    good = XC.six_products(a, b)
    assert XC.rel_err(good, ref, mag) <= bar and XC.hard_cap_ok(good, ref, mag, K)
    assert XC.rel_err(good, ref, mag) <= 2 * U      # the three dropped products: 3 x 2^-24 at the most, in fact far less
    if M * N < 256:
        return
    for drop in XC.PRODUCTS:
        assert XC.rel_err(XC.six_products(a, b, drop=drop), ref, mag) > 1.2 * bar, (drop, bar / U)      # a fifth to spare
    for piece in {0, (K - 1) // 32}:
        assert XC.rel_err(XC.six_products(a, b, drop_piece=piece), ref, mag) > 1000 * bar


def test_every_regime_has_a_value_case_and_the_bars_are_the_stated_ones():
    assert {c[0] for c in XC.VALUE_CASES} == {'positive', 'wide'} and {c[4] > 1 for c in XC.VALUE_CASES} == {True, False}
    assert (XC.BAR_PLAIN, XC.BAR_BIAS, XC.BAR_TAIL) == (6 * U, 8 * U, 16 * U)
    assert XC.bar('normal', 70, 72, 33) == 6 * U and XC.bar('normal', 70, 72, 33, bias=True) == 8 * U
    for r, M, N, K, sk in XC.VALUE_CASES:
        assert XC.bar(r, M, N, K) == max(4 * XC.YARD[XC.value_key(r, M, N, K)], 6 * U)
        assert sk <= XC.k_pad(K) // 32


# =================================================================================================================
# yardsticks
# =================================================================================================================
def test_the_committed_yardsticks_are_the_measured_ones():
    """sequential fp32 in k order against fp64, re-measured here.  The fp32 side is bit-exact anywhere; the fp64 reference may
    associate differently under another BLAS, which moves the third digit at the most: equal to 1 %."""
    got = XC.yard_table()
    assert set(got) == set(XC.YARD), 'run `python tests/x3_cases.py` and commit the table'
    for k, v in got.items():
        assert abs(v - XC.YARD[k]) <= 0.01 * XC.YARD[k], (k, v, XC.YARD[k])
