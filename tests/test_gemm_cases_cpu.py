"""The case table of the f32 GEMM sweep reaches every branch it is meant to reach (tests/gemm_cases.py: a plain-Python
restatement of gemm_entry / launch_tile / launch_cfg), and its tolerances separate a wrong product from a right one.
No GPU: an edit of a tuning constant that silently moves a case off its branch fails here once the model follows it."""
import pytest
import torch

import gemm_cases as GC
from gemm_cases import OPT_LEAN, OPT_NO_DMA, but, plan


def plans(cases, **kw):
    return [plan(c, **kw) for c in cases]


def test_names_are_unique_and_every_case_has_a_yardstick():
    names = [c.name for c in GC.ALL_CASES]
    assert len(names) == len(set(names))
    keys = {GC.yard_key(c) for c in GC.FP64_CASES}
    assert keys == set(GC.YARD), 'run `python tests/gemm_cases.py` and commit the table'
    assert all(y[0] > 0 for y in GC.YARD.values())
    assert all((GC.yard(c)[1] > 0) == c.colsum for c in GC.FP64_CASES)


def test_tile_bookkeeping_cases():
    ps = plans(GC.TILE_CASES)
    assert all(p['tile'] == 64 and p['splitk'] == 1 for p in ps)
    assert {(p['tiles_m'], p['nc']) for p in ps} == {(tm, nc) for tm in (1, 7, 8, 9, 17) for nc in (1, 3, 8)}
    for tm in (1, 7, 8, 9, 17):
        for nc in (1, 3, 8):
            mine = [c for c, p in zip(GC.TILE_CASES, ps) if (p['tiles_m'], p['nc']) == (tm, nc)]
            assert {(c.Ks[0], c.acc) for c in mine} == {(4, 0), (4, 1), (36, 0), (36, 1)}
    assert any(p['nblk'] % 8 for p in ps) and any(p['nblk'] % 8 == 0 for p in ps)          # both arms of the XCD remap
    assert any(p['tiles_m'] % 8 and p['tiles_m'] > 8 for p in ps)                          # a ragged last band
    assert all(c.M % 64 or c.N % 64 for c in GC.TILE_CASES)                                # ragged last tiles
    assert all(c.cprev == ('quarter' if c.acc else 'nan') for c in GC.TILE_CASES)
    assert {(c.ak, c.bk) for c in GC.TILE_CASES} == set(GC.KLAYS)
    assert {c.layC for c in GC.TILE_CASES} == set(GC.LAYOUTS) and {p['vec'] for p in ps} == {True, False}


def test_k_edge_cases():
    cs = GC.K_CASES
    for lay in GC.KLAYS:
        mine = [c for c in cs if (c.ak, c.bk) == lay]
        assert {c.Ks[0] for c in mine if len(c.Ks) == 1} >= {1, 3, 4, 31, 32, 33, 36, 64, 68}
        assert {len(c.Ks) for c in mine} >= {1, 2, 3, 4, 8}
        assert any(c.G == GC.MAXGROUP for c in mine) and any(len(c.Ks) == GC.MAXSEG for c in mine)
        assert any(all(c.bias) for c in mine) and any(not any(c.bias) for c in mine)
        assert any(any(c.bias) and not all(c.bias) for c in mine)
        for which in ('layA', 'layB', 'layC'):
            assert {c[which] for c in mine} == set(GC.LAYOUTS)
        assert any(c.soff for c in mine)
        assert any(len(set(c.Ks)) > 1 for c in mine)
    # every reason for scalar staging: K % 4 (k-contiguous operands), an odd ld, a misaligned base
    assert any(not plan(c)['vec'] and c.Ks[0] % 4 and c.layA == c.layB == 'packed' for c in cs)
    assert any(not plan(c)['vec'] and 'ld_plus_1' in (c.layA, c.layB) for c in cs)
    assert any(not plan(c)['vec'] and 'offset_1' in (c.layA, c.layB) and all(K % 4 == 0 for K in c.Ks) for c in cs)
    assert any(plan(c)['vec'] and 'padded4' in (c.layA, c.layB) for c in cs)
    # K = 0
    assert any(c.Ks == [0, 0, 0] and plan(c)['kind'] == 'run' for c in cs)
    pos = set()
    for c in GC.K0_REFUSED:
        assert plan(c) == dict(kind='refused', code=GC.ERR_SHAPE)
        pos.add('first' if c.Ks[0] == 0 else 'last' if c.Ks[-1] == 0 else 'middle')
    assert pos == {'first', 'middle', 'last'} and {(c.ak, c.bk) for c in GC.K0_REFUSED} == set(GC.KLAYS)


def test_big_tile_cases():
    for lay in GC.KLAYS:
        mine = [c for c in GC.BIG_CASES if (c.ak, c.bk) == lay]
        got = set()
        for c in mine:
            for f in GC.FLAG_SETS:
                p = plan(but(c, flags=f))
                assert p['tile'] == 128 and p['tiles'] >= 384 and p['splitk'] == 1
                got.add((p['kernel'], p['BK'], p['vec']))
        want = {('dma', 16, True), ('fast', 32, True), ('reg', 32, True), ('reg', 32, False)}
        want.add(('dma', 32, True) if lay == (1, 1) else ('dma', 16, True))
        if lay == (1, 1):
            want |= {('dma_ragged', 32, True), ('dma_ragged', 16, True)}
        assert got == want, (lay, got)
        assert any(c.M % 2 and c.N % 2 for c in mine)                                      # odd ragged sizes
        assert any(not plan(c)['vec'] and c.Ks == [7] for c in mine) or lay == (0, 0)      # scalar staging through K = 7
        assert any(not plan(c)['vec'] and 'offset_1' in (c.layA, c.layB) for c in mine)    # ... and through offset_1
        assert {sum(c.Ks) for c in mine} >= {32, 96, 16, 40, 7}


@pytest.mark.parametrize('slots', [64, 96])
def test_tail_cases(slots):
    want = {208: 4, 220: 2, 242: 0}
    seen = set()
    for c in GC.TAIL_CASES:
        for f in (0, OPT_LEAN, OPT_NO_DMA):
            p = plan(but(c, flags=f), slots=slots)
            q = p['tiles'] // 8
            assert p['tiles'] % 8 == 0 and q in want and p['splitk'] == 1
            ragged = bool(c.M % 128)
            if p['kernel'] == 'reg':                # ragged under NO_DMA: the bounds-checked kernel has no tail form
                assert ragged and f == OPT_NO_DMA and p['tail'] == 0
            else:
                assert p['tail'] == want[q]
                seen.add((q, ragged, p['kernel']))
        if c.M % 128:                               # some tail parts lie wholly outside the matrix
            assert c.M % 128 <= 64 and c.N % 128 <= 64
    assert seen == {(q, r, k) for q in want for r, ks in ((False, ('dma', 'fast')), (True, ('dma_ragged',))) for k in ks}


def test_small_tile_split_cases():
    byname = {c.name: (c, plan(c)) for c in GC.SPLIT64_CASES}
    for lay in GC.KLAYS:
        t = '%d%d' % lay
        c, p = byname['s64 %s K2080' % t]
        assert p['tile'] == 64 and p['splitk'] == 16 and p['empty'] == 3 and p['ranges'][13:] == [(2080, 2080)] * 3
        c, p = byname['s64 %s K800 acc' % t]
        assert p['splitk'] == 6 and p['empty'] == 1
        c, p = byname['s64 %s 3seg g3' % t]
        cut = p['ranges'][0][1]
        assert p['splitk'] == 2 and c.Ks[0] < cut < c.Ks[0] + c.Ks[1] and c.G == 3
        assert byname['s64 %s ragged' % t][1]['splitk'] > 1
        kinds = {n_: p_['finish'] for n_, (c_, p_) in byname.items() if n_.startswith('s64 ' + t)}
        assert kinds['s64 %s K2080' % t] == 'reduce_v4'
        for n_ in ('N42', 'offset_1 C', 'offset_1 bias'):
            assert kinds['s64 %s %s' % (t, n_)] == 'reduce_scalar'
        mine = [c_ for c_, p_ in byname.values() if (c_.ak, c_.bk) == lay]
        assert {c_.G for c_ in mine} == {1, 3} and {c_.acc for c_ in mine} == {0, 1}
        for c_ in mine:
            assert plan(but(c_, tickets=0))['finish'] == 'ticket'
            assert GC.same_ranges(c_, OPT_NO_DMA) and plan(c_)['ws_floats'] * 4 <= c_.ws
    ks = {p['kernel'] for c, p in byname.values()}
    assert ks == {'dma', 'dma_ragged', 'reg'}
    assert {plan(but(c, flags=OPT_NO_DMA))['kernel'] for c, p in byname.values()} == {'reg'}


def test_medium_split_cases():
    coincide = set()
    for c in GC.MEDIUM_CASES:
        p = plan(c)
        forced = (c.flags >> 8) & 31
        assert p['tile'] == 128 and p['tiles'] == 16
        assert 2.0 * c.M * c.N * sum(c.Ks) >= 6e9 > 2.0 * c.M * c.N * (sum(c.Ks) - 32)        # the smallest K the gate admits
        if forced:
            assert p['splitk'] == forced
            assert p['empty'] == (1 if forced == 31 else 0)
        else:
            assert p['splitk'] > 1                  # the cost model's own choice is a split
        assert GC.same_ranges(c, OPT_LEAN)          # LDS_LEAN cuts the default kernel's ranges, whatever its own K step
        assert plan(but(c, flags=c.flags | OPT_LEAN))['BK'] == 16
        assert p['BK'] == (32 if (c.ak, c.bk) == (1, 1) else 16)
        same = GC.same_ranges(c, OPT_NO_DMA)
        assert GC.same_ranges(c, OPT_NO_DMA | OPT_LEAN) == same
        if (c.ak, c.bk) == (1, 1) or p['splitk'] == 1:
            assert same
        else:                                       # 16-deep default against the 32-deep register kernel
            T, s = sum(c.Ks) // 32, p['splitk']
            assert same == (not 0 < T % s <= s // 2) or p['empty']
        coincide.add(((c.ak, c.bk) == (1, 1), same))
        assert p['ws_floats'] * 4 <= c.ws
    assert (False, True) in coincide and (False, False) in coincide
    for c in GC.MEDIUM_RAGGED_CASES:
        p = plan(c)
        assert p['tile'] == 128 and p['splitk'] == 3 and c.M % 128 and c.N % 128
        assert p['kernel'] == ('dma_ragged' if (c.ak, c.bk) == (1, 1) else 'reg')
        assert GC.same_ranges(c, OPT_LEAN) and GC.same_ranges(c, OPT_NO_DMA)
    # the issue's example: K = 11456, s = 3: 3840 / 7680 in steps of 32, 3824 / 7648 in steps of 16
    assert [e for _, e in GC.k_ranges([11456], 32, 3)] == [3840, 7680, 11456]
    assert [e for _, e in GC.k_ranges([11456], 16, 3)] == [3824, 7648, 11456]
    assert GC.k_ranges([11456], 16, 3, unit=32) == GC.k_ranges([11456], 32, 3)


def test_colsum_workspace_and_lstm_cases():
    for bk in (0, 1):
        mine = [(c, plan(c)) for c in GC.COLSUM_CASES if c.bk == bk]
        assert all(c.ak == 0 and c.colsum and p['kernel'] in ('fast', 'reg') for c, p in mine)
        got = {(p['tile'], p['vec'], p['splitk'] > 1) for c, p in mine}
        assert got == {(t, v, s) for t in (64, 128) for v in (True, False) for s in (True, False)} - {(128, False, True)}
        assert any(c.acc for c, p in mine) and any(c.M % 64 for c, p in mine) and any(c.soff for c, p in mine)
        assert all(plan(but(c, tickets=0))['finish'] == 'ticket' for c, p in mine if p['splitk'] > 1)
    by = {c.name: (c, plan(c)) for c in GC.WS_CASES}
    for t in ('11', '00', '01'):
        c, p = by['ws %s cap=want' % t]
        assert p['splitk'] == p['cap'] == 7 and (c.ws >> 20) * (1 << 18) // (c.M * c.N * c.G) == 8
        c, p = by['ws %s cap<want' % t]
        assert p['splitk'] == p['cap'] == 7 and sum(c.Ks) // 32 // 4 == 8
        if c.colsum:                                # a split of 8 without the + M: the rider's slab lies past ws_bytes
            assert c.M * c.N * 8 * 4 == c.ws < (c.M * c.N + c.M) * 8 * 4
        assert by['ws %s 1 MiB less' % t][1]['splitk'] == 3
        assert by['ws %s too small' % t][1]['splitk'] == 1 and by['ws %s misaligned' % t][1]['splitk'] == 1
        assert all(p_['ws_floats'] * 4 <= c_.ws for c_, p_ in by.values())
    for c in GC.LSTM_CASES:
        p = plan(c, lstm=True)
        assert (c.M * (c.N // 4)) % 256 and c.N % 4 == 0
        assert (p['finish'] == 'lstm') == (c.name.split()[1] == 'split') == (p['splitk'] > 1)
    assert {c.drop for c in GC.LSTM_CASES} == {0.0, 0.3} and {c.G for c in GC.LSTM_CASES} == {1, 3}


def test_every_finish_and_kernel_is_reached():
    fin, ker = set(), set()
    for c in GC.FP64_CASES:
        for tk in (None, 0, -1):
            for f in GC.FLAG_SETS:
                p = plan(but(c, tickets=tk, flags=c.flags | f))
                fin.add(p['finish'])
                ker.add((p['tile'], p['kernel'], p['BK'], p['splitk'] > 1))
    assert fin == {'none', 'reduce_v4', 'reduce_scalar', 'ticket'}
    for t in (64, 128):
        for s in (False, True):
            assert {(t, 'dma', 32, s), (t, 'dma_ragged', 32, s), (t, 'reg', 32, s)} <= ker
    assert {(128, 'dma', 16, True), (128, 'dma', 16, False), (128, 'fast', 32, True), (128, 'fast', 32, False)} <= ker


MARGIN_CASES = [c for c in GC.FP64_CASES if c.M * c.N * max(1, sum(c.Ks)) <= 70 * 80 * 2100 and sum(c.Ks) > 0]


def test_the_tolerances_tell_a_dropped_term_from_rounding():
    """For the table's own inputs: a plain fp32 product passes the check, the same product with one k step of one
    segment dropped (what the K = 0 defect did), one term doubled or one element left at its previous value fails it."""
    assert len(MARGIN_CASES) > 100
    for c in MARGIN_CASES:
        inp = GC.make_inputs(c, groups=1)
        ref, mag = GC.ref_group(c, inp, 0)
        good = ref.float()
        GC.check_product(good, ref, mag, c, 1, GC.yard(c)[0])
        s = len(c.Ks) - 1
        A, B = inp['A'][0][s], inp['B'][0][s]
        k = c.Ks[s] - 1
        term = (A[:, k:k + 1].double() * B[:, k].double())
        for bad in ((ref - term).float(), (ref + term).float()):
            with pytest.raises(AssertionError):
                GC.check_product(bad, ref, mag, c, 1, GC.yard(c)[0])
        assert float(term.abs().max()) > 1e3 * GC.YARD_FACTOR * GC.yard(c)[0]


def test_margin_of_the_long_products():
    """the longest K of the table: a dropped K step of 16 is still far above 4 x the yardstick"""
    c = GC.MEDIUM_CASES[0]
    yc = GC.yard(c)[0]
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(64, 16, generator=g).double(), torch.randn(64, 16, generator=g).double()
    assert float((a @ b.t()).abs().max()) > 1e3 * GC.YARD_FACTOR * yc
