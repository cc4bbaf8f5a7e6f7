"""The tables of the decoder-cell sweep (tests/deccell_cases.py: a plain-Python restatement of the launchers of
csrc/rfn_deccell.hip) reach every kernel instantiation, branch and loop trip they are meant to reach, at 256 compute units
and at another count; no case needs more than 32 MiB of device memory; the explicit formulas agree with autograd through the
un-hoisted ones; the committed yardsticks are the measured ones, and 4 x a yardstick tells a dropped term from rounding.
No GPU."""
import pytest
import torch

import deccell_cases as DC

CUS = [256, 304, 64]


def fwd_plans(cus):
    return {c['name']: DC.fwd_geometry(c, cus) for c in DC.FWD_CASES}


# =================================================================================================================
# the model itself
# =================================================================================================================
def test_the_model_restates_the_launchers():
    # the example of the forward launcher: at R = 256 a batch of cus rows gives one thread per unit, half of it two, two rows four
    for cus in CUS:
        assert [DC.fwd_plan(B, 8, 512, 256, cus, 512, 4096)['tpu'] for B in (cus, cus - 1, cus // 2, cus // 2 - 1, 2)] == [1, 2, 2, 4, 4]
        assert [DC.fwd_plan(B, 8, 512, 256, cus, 512, 4096, hp_al=False)['ub'] for B in (cus, cus // 2, 2)] == [256, 128, 64]
        assert DC.fwd_plan(2 * cus, 8, 512, 512, cus, 512, 4096)['tpu'] == 1 and DC.fwd_plan(1, 8, 512, 1024, cus, 512, 4096)['tpu'] == 4
    fast = dict(B=2, L=8, A=512, R=256, cus=256, psb=512, psl=512)
    assert DC.fwd_plan(**fast)['kernel'] == 'fast'
    for k, v in (('A', 516), ('A', 510), ('L', 9), ('R', 384), ('psb', 513), ('psl', 514), ('proj_al', False), ('hp_al', False),
                 ('w_al', False)):
        assert DC.fwd_plan(**dict(fast, **{k: v}))['kernel'] == 'general', k
    assert DC.fwd_plan(**dict(fast, hp_al=False))['vecA'] and not DC.fwd_plan(**dict(fast, proj_al=False))['vecA']
    assert not DC.fwd_plan(**dict(fast, A=510))['vecA'] and not DC.fwd_plan(**dict(fast, psl=514))['vecA']
    for k, v in (('L', 0), ('L', 1025), ('B', 0), ('row_div', 0), ('drop_p', 1.0), ('drop_p', -0.1), ('A', 0), ('R', 0)):
        assert DC.fwd_plan(**dict(fast, **{k: v}))['kernel'] == 'refused', k
    assert DC.fwd_plan(**dict(fast, L=1024))['kernel'] == 'general'
    # the general kernel's LDS limit is exact: 2 * 8188 + 8 floats are 64 KiB
    assert DC.fwd_plan(1, 8, 8188, 4, 256, 8188, 8188) == dict(DC.fwd_plan(1, 8, 8188, 4, 256, 8188, 8188), kernel='general', lds=16384)
    assert DC.fwd_plan(1, 8, 8192, 4, 256, 8192, 8192)['kernel'] == 'refused'
    # ub / 2 >= R: a row of 7 units takes a 64-thread block whatever the batch; 130 units keep 256 threads when B fills the device
    assert DC.fwd_plan(10000, 5, 30, 7, 256, 30, 30)['ub'] == 64 and DC.fwd_plan(256, 5, 30, 130, 256, 30, 30)['ub'] == 256
    assert DC.fwd_plan(256, 5, 30, 128, 256, 30, 30)['ub'] == 128

    bw = dict(L=8, A=512, GD=1024, psb=4096, psl=512, usb=8192, usl=1024, ldg=1024, dpsb=4096, dpsl=512)
    assert DC.bwd_plan(**bw)['kernel'] == 'fast'
    for k in ('hp', 'w'):                          # what fast_ok checks and vec / vecu do not
        assert DC.bwd_plan(al={k: False}, **bw)['kernel'] == 'vec_vecu'
    for k in ('proj', 'dproj', 'dhp', 'dwp'):
        assert DC.bwd_plan(al={k: False}, **bw)['kernel'] == 'scal_vecu'
    for k in ('U', 'dg'):
        assert DC.bwd_plan(al={k: False}, **bw)['kernel'] == 'vec_scalu'
    for k in ('psb', 'psl', 'dpsb', 'dpsl'):
        assert DC.bwd_plan(**dict(bw, **{k: bw[k] + 1}))['kernel'] == 'scal_vecu'
    for k in ('usb', 'usl', 'ldg'):
        assert DC.bwd_plan(**dict(bw, **{k: bw[k] + 1}))['kernel'] == 'vec_scalu'
    assert DC.bwd_plan(**dict(bw, L=9))['kernel'] == 'vec_vecu' and DC.bwd_plan(**dict(bw, A=516))['kernel'] == 'vec_vecu'
    assert DC.bwd_plan(**dict(bw, A=510, GD=1022))['kernel'] == 'scal_scalu'
    assert DC.bwd_plan(**dict(bw, L=1025))['kernel'] == 'refused' and DC.bwd_plan(**dict(bw, L=1024))['kernel'] == 'vec_vecu'
    assert DC.bwd_plan(**dict(bw, L=1, A=8172))['lds'] == 16384 and DC.bwd_plan(**dict(bw, L=1, A=8176))['kernel'] == 'refused'

    assert DC.du_plan(3, 2, 8, 1024, 8192, 1024)['kernel'] == 'vector'
    for kw in (dict(GD=1023), dict(usb=8193), dict(usl=1025), dict(dg_al=False), dict(du_al=False)):
        assert DC.du_plan(**dict(dict(S=3, B=2, L=8, GD=1024, usb=8192, usl=1024), **kw))['kernel'] == 'scalar'
    S, B, L, GD = DC.DU_LIMIT
    assert S * L == 16385 and GD % 4 == 0
    assert DC.du_plan(S, B, L, GD, L * GD, GD)['kernel'] == 'refused'               # the vector path alone has the limit
    assert DC.du_plan(S, B, L, GD, L * GD, GD, du_al=False)['kernel'] == 'scalar'
    assert DC.du_plan(4096, 1, 4, 4, 16, 4)['kernel'] == 'vector'                       # exactly 64 KiB


# =================================================================================================================
# forward coverage
# =================================================================================================================
@pytest.mark.parametrize('cus', CUS)
def test_forward_cases_reach_every_instantiation_branch_and_trip(cus):
    P = fwd_plans(cus)
    plan = lambda n: P[n][1]  # noqa: E731
    assert all(p['kernel'] != 'refused' for _, p, _ in P.values())
    # six instantiations of the fast kernel
    fast = {(5 if c['maxout'] else 4, p['tpu']) for c, p, _ in P.values() if p['kernel'] == 'fast'}
    assert fast == {(ng, t) for ng in (4, 5) for t in (1, 2, 4)}
    for n, ng, t in (('fast_4_1', 4, 1), ('fast_4_2', 4, 2), ('fast_4_4', 4, 4), ('fast_5_1', 5, 1), ('fast_5_2', 5, 2), ('fast_5_4_L1', 5, 4)):
        assert plan(n)['kernel'] == 'fast' and plan(n)['tpu'] == t and (5 if P[n][0]['maxout'] else 4) == ng
    # the general kernel: NG x block size x vecA
    gen = {(5 if c['maxout'] else 4, p['ub'], p['vecA']) for c, p, _ in P.values() if p['kernel'] == 'general'}
    for ng in (4, 5):
        for ub in (64, 128, 256):
            assert (ng, ub, True) in gen, (ng, ub)
        assert (ng, 64, False) in gen
    # the bit-identity pairs: same problem on the fast kernel and, hproj / w_out one float off, on the general one with vecA
    for f, g, ub in (('fast_4_1', 'gen_256', 256), ('fast_4_2', 'gen_128', 128), ('fast_4_4', 'gen_64', 64), ('fast_5_1', 'gen_5_256', 256)):
        cf, cg = P[f][0], P[g][0]
        assert all(cf[k] == cg[k] for k in ('B', 'L', 'A', 'R', 'maxout')) and cg['hp_off'] + cg['w_off'] > 0
        assert plan(g)['kernel'] == 'general' and plan(g)['vecA'] and plan(g)['ub'] == ub
    # dropout at kernel level: fast and general, with maxout, with ldh = R + 4
    drop = [(c, p) for c, p, _ in P.values() if c['drop'] > 0]
    assert {p['kernel'] for _, p in drop} == {'fast', 'general'}
    assert any(p['kernel'] == 'general' and c['maxout'] and c['lh'] == 'padded4' for c, p in drop)
    assert any(p['kernel'] == 'general' and not p['vecA'] for c, p in drop)
    # layouts: every operand with a stride sees a padded one, proj and U every layout, b_out NULL, B % row_div != 0
    lays = {'packed', 'padded4', 'ld_plus_1', 'offset_1', 'time_major'}
    assert {c['lp'] for c, _, _ in P.values()} == lays and {c['lu'] for c, _, _ in P.values()} == lays
    for k in ('lg', 'lcp', 'lcn', 'lh'):
        assert {'packed', 'padded4', 'ld_plus_1', 'offset_1'} <= {c[k] for c, _, _ in P.values()}, k
    for kern in ('fast', 'general'):
        mine = [c for c, p, _ in P.values() if p['kernel'] == kern]
        assert any(not c['bo'] for c in mine) and any(c['B'] % c['row_div'] for c in mine), kern
        assert any(c['lh'] != 'packed' for c in mine) and any(c['lg'] != 'packed' for c in mine)
        assert any(c['lcp'] != 'packed' for c in mine) and any(c['lcn'] != 'packed' for c in mine)
    # an offset hproj / w_out, and each 16-B condition of proj, moves a call off the fast kernel
    assert plan('scal_off_A260')['kernel'] == 'general' and not plan('scal_off_A260')['vecA']
    # L: 1, 2, every count up to 8 on the fast kernel's two rows per wave, the tail loop's first and later trips
    Ls = {c['L'] for c, _, _ in P.values()}
    assert {1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 257, 1024} <= Ls
    assert {c['L'] for c, p, _ in P.values() if p['kernel'] == 'fast'} >= {1, 2, 3, 4, 5, 7, 8}
    assert {p['rows_per_wave'] for _, p, _ in P.values() if p['kernel'] == 'fast'} == {1, 2}
    tails = {p['tail'] for _, p, _ in P.values() if p['kernel'] == 'general'}
    assert {0, 1, 8, 9, 249, 1016} <= tails
    at = {p['alpha_trips'] for _, p, _ in P.values() if p['kernel'] == 'general'}                       # l = tid loop: L > ub
    assert 1 in at and max(at) >= 3 and 257 % plan('L257')['ub'] == 1                                  # ... whose last trip holds one l
    assert plan('L257')['alpha_trips'] >= 2 and plan('L1024')['alpha_trips'] >= 4
    # A: chunk trips of the score dot -- vector 1, 2, 3 (A = 516: the third trip holds one chunk), 5; scalar 1, 5, 9
    vt = {p['chunk_trips'] for _, p, _ in P.values() if p['kernel'] == 'general' and p['vecA']}
    st = {p['chunk_trips'] for _, p, _ in P.values() if p['kernel'] == 'general' and not p['vecA']}
    assert {1, 2, 3, 5} <= vt and {1, 5, 9} <= st
    assert plan('A516')['vecA'] and plan('A516')['chunk_trips'] == 3 and not plan('A516_scal')['vecA']
    assert {1, 2} <= {p['chunk_trips'] for _, p, _ in P.values() if p['kernel'] == 'fast'}
    assert {1, 2} <= {p['stage_trips'] for _, p, _ in P.values() if p['kernel'] == 'general'} and plan('A516')['stage_trips'] > 2
    # R: one block with dead threads, several blocks, blocks of the fast kernel 1 / 2 / 4 / 8 per row
    assert plan('r130_ub256')['ub'] == 256 and plan('r130_ub256')['dead'] == 126 and plan('r130_ub64')['blocks'] == 3
    assert plan('scal_small')['dead'] == 57 and plan('L9_r512')['blocks'] == 8 and plan('fast_r512_L2')['blocks'] == 8
    assert {c['R'] for c, _, _ in P.values()} == {4, 7, 130, 256, 512}
    assert plan('A8188_lds')['lds'] == DC.LDS_FLOATS
    # b_z, b_out and alpha one float off on both kernels
    assert {p['kernel'] for c, p, _ in P.values() if c['soff'] and c['bo']} == {'fast', 'general'}
    # ldh != R together with dropout
    assert any(c['drop'] > 0 and c['lh'] == 'padded4' for c, _, _ in P.values())
    # every value regime on both kernels
    for r in ('sat', 'small', 'shift+', 'shift-'):
        assert {p['kernel'] for c, p, _ in P.values() if c['regime'] == r} == {'fast', 'general'}
    for c, p, _ in P.values():                      # the regime a case claims is the one its shape is in
        assert (c['L'] > 17) == (c['regime'] == 'long') and (c['A'] > 512) == (c['regime'] == 'wide'), c['name']


# =================================================================================================================
# backward and dU coverage
# =================================================================================================================
def test_backward_cases_reach_all_five_kernels_and_every_trip():
    P = {c['name']: (c, DC.bwd_geometry(c)[0]) for c in DC.BWD_CASES}
    by = {}
    for c, p in P.values():
        assert p['kernel'] != 'refused'
        by.setdefault(p['kernel'], []).append((c, p))
    assert set(by) == {'fast', 'vec_vecu', 'scal_vecu', 'vec_scalu', 'scal_scalu'}
    prefix = dict(fast='fast', vec_vecu='vv', scal_vecu='sv', vec_scalu='vs', scal_scalu='ss')
    for c, p in P.values():
        assert c['name'].startswith(prefix[p['kernel']] + '_'), (c['name'], p['kernel'])
    for k, cases in by.items():
        assert {c['acc'] for c, _ in cases} == {0, 1}, k
    assert {c['L'] for c, _ in by['fast']} == {1, 2, 3, 4, 5, 6, 7, 8}
    assert {2} <= {p['gd_trips'] for _, p in by['fast']}                                  # GD > 1024 on the fast body
    # the l0 groups of 8 with their clamp, and the 4-row groups with theirs, on the vector kernel
    for k in ('vec_vecu', 'scal_vecu', 'vec_scalu', 'scal_scalu'):
        assert any(p['l_groups'] >= 2 and p['l_clamp'] for _, p in by[k]), k
    vv = by['vec_vecu']
    assert {c['L'] for c, _ in vv} >= {5, 8, 9, 16, 17, 257, 1024}
    assert any(p['l4_groups'] >= 3 and p['l4_clamp'] for _, p in vv) and any(p['l_groups'] == 2 and not p['l_clamp'] for _, p in vv)
    assert any(p['ltid_trips'] == 2 for _, p in vv) and any(p['ltid_trips'] == 4 for _, p in vv)
    assert any(p['ltid_trips'] == 2 for _, p in by['scal_scalu'])
    # GD > 1024 vector, > 256 scalar; A > 1024 vector, > 256 scalar: second trips off the fast kernel
    assert any(p['gd_trips'] == 2 for _, p in vv) and any(p['gd_trips'] >= 5 for _, p in vv)
    assert any(p['gd_trips'] == 2 for _, p in by['vec_scalu']) and any(p['gd_trips'] == 2 for _, p in by['scal_scalu'])
    assert any(p['a_trips'] == 2 for _, p in vv) and any(p['a_trips'] == 2 for _, p in by['scal_scalu'] + by['scal_vecu'])
    # what pushes a fast shape onto <true, true>
    for n in ('vv_L8_hpoff', 'vv_L5_woff'):
        c = P[n][0]
        assert c['L'] <= 8 and c['A'] <= 512 and c['hp_off'] + c['w_off'] == 1
    # dproj with strides of its own; every layout of proj, dproj, U, dgates
    assert any(c['lp'] != c['ldp'] for c, _ in P.values())
    lays = {'packed', 'padded4', 'ld_plus_1', 'offset_1', 'time_major'}
    assert {c['ldp'] for c, _ in P.values()} == lays and {c['lu'] for c, _ in P.values()} == lays
    assert {c['lp'] for c, _ in P.values()} == lays and P['sv_poff_L5'][1]['kernel'] == 'scal_vecu'     # rfn_aligned16(proj) alone
    assert {c['lg'] for c, _ in P.values()} == {'packed', 'padded4', 'ld_plus_1', 'offset_1'}
    assert any(c['dhp_off'] for c, _ in P.values()) and any(c['dwp_off'] for c, _ in P.values())
    # hproj / w_out one float off on the scalar kernels too, and alpha one float off
    for k in ('scal_vecu', 'vec_scalu', 'scal_scalu'):
        assert any(c['hp_off'] or c['w_off'] for c, _ in by[k]), k
    assert any(c['soff'] for c, _ in by['scal_vecu']) and any(c['soff'] for c, _ in by['scal_scalu'])
    for c, _ in P.values():
        reg = 'long' if c['L'] > 17 else 'wide' if c['A'] > 512 else 'deep' if c['GD'] > 2560 else 'std'
        assert c['regime'] == reg, c['name']


def test_du_cases_reach_both_kernels_and_every_trip():
    plans = [(c, DC.du_geometry(*c)[0]) for c in DC.DU_CASES]
    vec = [(c, p) for c, p in plans if p['kernel'] == 'vector']
    sca = [(c, p) for c, p in plans if p['kernel'] == 'scalar']
    assert len(vec) + len(sca) == len(plans) and vec and sca
    assert {c[0] for c, _ in plans} >= {1} and {c[2] for c, _ in vec} >= {1, 8, 9, 17} and {c[3] for c, _ in plans} >= {4, 35, 1024, 1028}
    assert {c[4] for c, _ in vec} == {'packed', 'time_major', 'padded4'}
    assert any(c[4] == 'offset_1' and c[3] % 4 == 0 for c, _ in sca) and any(c[4] == 'ld_plus_1' and c[3] % 4 == 0 for c, _ in sca)
    assert any(c[3] % 4 for c, _ in sca)
    assert any(p['col_blocks'] == 2 for _, p in vec) and any(p['col_blocks'] >= 2 for _, p in sca)
    assert any(p['l_groups'] == 2 and p['guard'] for _, p in vec) and any(p['l_groups'] == 3 for _, p in vec)
    assert any(p['guard'] and c[4] == 'time_major' for c, p in vec)              # the guarded stores under a time-major dU
    assert any(p['stage_trips'] >= 3 for _, p in vec)
    for S, B, L, GD, lay in DC.DU_SOFF_CASES:       # a misaligned dgates alone: the scalar kernel under an aligned, 4-strided dU
        assert DC.du_geometry(S, B, L, GD, lay)[0]['kernel'] == 'vector' and DC.du_geometry(S, B, L, GD, lay, 1)[0]['kernel'] == 'scalar'


@pytest.mark.parametrize('cus', CUS)
def test_no_case_needs_more_than_32_mib(cus):
    for c in DC.FWD_CASES:
        assert DC.fwd_geometry(c, cus)[2] <= DC.MEM_LIMIT, c['name']
    for c in DC.BWD_CASES:
        assert DC.bwd_geometry(c)[1] <= DC.MEM_LIMIT, c['name']
    for c in DC.DU_CASES + [DC.DU_LIMIT + ('packed',)] + [c + (1,) for c in DC.DU_SOFF_CASES]:
        assert DC.du_geometry(*c)[1] <= DC.MEM_LIMIT, c


# =================================================================================================================
# references, yardsticks, detection
# =================================================================================================================
def test_explicit_formulas_are_the_unhoisted_mathematics():
    """fp64: the hoisted formulas against ref_cell (z = sum alpha v, then z2h) and against autograd through it, up to the
    float32 rounding of the proj and U the kernels are given"""
    from test_deccell_gpu import ref_cell
    for name in ('scal_odd_L9', 'fast_5_4_L1', 'scal_small'):
        c = DC.resolve(DC.FWD_BY_NAME[name], 256)
        d = DC.fwd_inputs(c)
        dd = lambda t: t.double()  # noqa: E731
        vx = dd(d['v']).repeat_interleave(c['row_div'], 0)[:c['B']]
        bo = dd(d['bo']) if d['bo'] is not None else torch.zeros(1, dtype=torch.float64)
        alpha, sig, g, c1, h1, _ = ref_cell(vx, dd(d['Wa']), dd(d['ba']), dd(d['hp']), dd(d['w']), bo, dd(d['Wz']), dd(d['bz']),
                                            dd(d['gin']), dd(d['c0']), c['maxout'])
        got = DC.cell_formulas(d)
        for k, ref in zip(DC.FWD_KEYS, (alpha, sig, g, c1, h1)):
            assert float((got[k] - ref).abs().max()) < 3e-7, (name, k)
    for name in ('ss_small', 'vv_L9', 'fast_L5_acc'):
        c = DC.BWD_BY_NAME[name]
        d = DC.bwd_inputs(c)
        got, ref = DC.bwd_formulas(d), DC.bwd_autograd(d)
        for k in DC.BWD_KEYS:
            assert float((got[k] - ref[k]).abs().max()) < 1e-6 * max(1.0, float(ref[k].abs().max())), (name, k)


def test_the_committed_yardsticks_are_the_measured_ones():
    """the fp32 side is plain torch on the CPU; another libm may move the last digits: equal to 25 %, floor 1e-10"""
    fw, bw = DC.yard_tables()
    assert set(fw) == set(DC.YARD_FWD) and set(bw) == set(DC.YARD_BWD), 'run `python tests/deccell_cases.py` and commit the tables'
    for got, want in ((fw, DC.YARD_FWD), (bw, DC.YARD_BWD)):
        for k in got:
            for a, b in zip(got[k], want[k]):
                assert abs(a - b) <= 0.25 * b + 1e-10, (k, got[k], want[k])


def test_four_yardsticks_tell_a_dropped_term_from_rounding():
    """one l left out of every row's gate sum (the l of the row's largest alpha: in the saturated regime the others can be
    zero) moves gates, c and h out of 4 x the yardstick; one 4-column chunk left out of every d alpha dot moves dproj, dhproj
    and dw out of it.  The standard regime's tolerances are checked the same way on one case per kernel."""
    fwc, bwc = DC.yard_cases()
    for c in fwc + [DC.FWD_BY_NAME[n] for n in ('fast_4_4', 'scal_small', 'L17')]:
        c = DC.resolve(c, 256)
        d = DC.fwd_inputs(c)
        ref, bad = DC.cell_formulas(d), DC.cell_formulas(d, drop_l='max')
        bar = dict(zip(DC.FWD_KEYS, (DC.YARD_FACTOR * y for y in DC.YARD_FWD[c['name']]))) if c['regime'] != 'std' else DC.TOL
        if c['L'] == 1:
            continue
        for k in ('sig', 'c', 'h'):
            assert float((bad[k] - ref[k]).abs().max()) > bar[k], (c['name'], k)
    for c in bwc + [DC.BWD_BY_NAME[n] for n in ('fast_L8', 'vv_L17', 'ss_small')]:
        d = DC.bwd_inputs(c)
        ref, bad = DC.bwd_formulas(d, acc=c['acc']), DC.bwd_formulas(d, acc=c['acc'], drop_chunk=0)
        if c['regime'] != 'std':
            bar = dict(zip(DC.BWD_KEYS, (DC.YARD_FACTOR * y for y in DC.YARD_BWD[c['name']])))
        else:
            scale = max(1.0, float(ref['dproj'].abs().max()))
            bar = dict(dproj=DC.TOL['dproj'] * scale, dhp=DC.TOL['dhp'] * scale, dw=DC.TOL['dw'] * max(1.0, float(ref['dw'].abs().max())))
        for k in DC.BWD_KEYS:
            assert float((bad[k] - ref[k]).abs().max()) > bar[k], (c['name'], k)
