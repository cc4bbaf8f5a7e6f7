"""Case tables of the decoder-cell sweep (tests/test_deccell_edges_gpu.py), a plain-Python restatement of the choices the
three launchers of csrc/rfn_deccell.hip make (rfn_dec_cell_fwd, rfn_dec_attn_bwd, rfn_dec_du), the inputs of every case and
the fp32 yardsticks of the value regimes the existing tolerances do not cover.  Nothing is imported from the C side and
nothing here needs a GPU: tests/test_deccell_cases_cpu.py asserts that the tables reach every branch and loop trip they are
meant to reach, at 256 compute units and at another count, that no case needs more than 32 MiB of device memory, and that
the tolerances tell a dropped term from rounding.  `python tests/deccell_cases.py` re-measures the yardstick tables.

Constants and choices restated from csrc/rfn_deccell.hip, csrc/rfn_deccell_body.h and csrc/rfn_attn_small_body.h:
    DEC_LREG 8 (thought vectors a thread keeps in registers), ATT_THREADS 256, ATT_WAVES 4, ATS_MAX_L 1024, 64 KiB of LDS.
    forward, fast kernel: A % 4 == 0, A <= 512, L <= 8, R % 256 == 0, (psb | psl) % 4 == 0, proj, hproj, w_out 16-B aligned;
        tpu = 1; while tpu < 4 and B * (R // (256 // tpu)) < cus: tpu *= 2; grid (R / (256 / tpu), B), 256 threads;
    forward, general kernel: ub = 256; while ub > 64 and (B * cdiv(R, ub) < cus or ub // 2 >= R): ub //= 2; grid
        (cdiv(R, ub), B), ub threads; LDS 2 * up4(A) + L floats, refused above 64 KiB; vecA = A % 4 == 0 and
        (psb | psl) % 4 == 0 and proj aligned: a wave's lanes take 16-B chunks 256 floats apart, else floats 64 apart; a
        block's waves take the rows l = wave, wave + ub / 64, ...; the gate sum runs l < 8 from registers, then a tail loop.
    backward: refused at L > 1024 or 2 * up4(A) + 2 * up4(L) + 32 floats above 64 KiB; fast body under fast_ok (see
        bwd_plan); else dec_attn_bwd_k<VEC, VECU>: the d alpha sums walk L in groups of 8 rows (rows past the end re-read
        row L - 1), GD in trips of 1024 (vector) / 256 (scalar) columns; the `l = tid` loops trip again at L > 256; the tanh
        backward walks A in trips of 1024 / 256 columns and, on the vector form, L in groups of 4 rows (same clamp).
    rfn_dec_du: scalar kernel when GD % 4, dgates or dU misaligned, or (usb | usl) % 4; else S * L floats of LDS, refused
        above 64 KiB; 1024 columns per block (scalar 256); L in groups of 8 whose stores are guarded by l0 + j < L.

Layouts: those of tests/test_attention_edges_gpu.py per strided operand (lp proj, lu U, lg gates / dgates, lcp, lcn, lh, ldp
dproj); hp_off / w_off / dhp_off / dwp_off put hproj, w_out, dhproj, dw_part one float off (what the fast kernels check);
soff puts the operands that are only accessed as scalars -- b_z, b_out, alpha; rfn_dec_du's alpha and dgates -- one float off.
The exact-LDS forward case A8188_lds is the issue's B = 1, R = 4.

Tolerances: tests/test_deccell_gpu.py's, unchanged, in its regime (TOL below).  A new regime -- L > 17, A > 512, GD > 2560,
saturated (proj * 30), small (proj, hproj * 0.01), b_out = +-1e4 -- gets the YARDSTICK: the same operation in plain fp32
torch in the kernels' formula order (the header's 1 - 2 / (e^2x + 1) tanh, serial softmax, l-ordered sums), its max error
against the same formulas in fp64 on the same float32 inputs; the kernel is allowed 4 x that.  A yardstick is a maximum,
and the smallest shape that reaches a branch can have as few as two independent softmax rows, whose maximum says little: it
is measured over YARD_ROWS batch rows of the case's shape (same L, A, R / GD, layouts irrelevant).  rfn_dec_du is held to the
worst case of any summation order, (S + 1) * 2^-24 * sum_s |alpha * dgates| per element.
"""
import torch

from test_attention_edges_gpu import lay2, lay3, up4          # the layouts of the attention sweep (no GPU needed to import)

U24 = 2.0 ** -24
DEC_LREG, THREADS, WAVES, MAX_L, LDS_FLOATS = 8, 256, 4, 1024, 64 * 1024 // 4
GUARD = 8
MEM_LIMIT = 32 << 20
DV = 6                                             # width of the thought vectors behind proj and U (the un-hoisted reference)
DROP_P, DROP_SEED, DROP_OFF = 0.25, 1234, (1 << 32) + 3
TOL = dict(alpha=3e-6, sig=3e-6, g=1e-5, c=1e-5, h=1e-5, dproj=3e-5, dhp=1e-4, dw=1e-4)      # tests/test_deccell_gpu.py
YARD_FACTOR = 4.0
YARD_ROWS = 16                                     # batch rows a yardstick is measured over, at least
FWD_KEYS = ('alpha', 'sig', 'g', 'c', 'h')
BWD_KEYS = ('dproj', 'dhp', 'dw')


def cdiv(a, b):
    return (a + b - 1) // b


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


# =================================================================================================================
# the launchers' choices
# =================================================================================================================
def fwd_plan(B, L, A, R, cus, psb, psl, proj_al=True, hp_al=True, w_al=True, row_div=1, drop_p=0.0):
    """what rfn_dec_cell_fwd does with a call: kernel 'refused' / 'fast' / 'general' and the trip counts of its loops"""
    if B <= 0 or L <= 0 or L > MAX_L or A <= 0 or R <= 0 or row_div < 1 or drop_p < 0.0 or drop_p >= 1.0:
        return dict(kernel='refused')
    vec = A % 4 == 0 and (psb | psl) % 4 == 0 and proj_al
    if vec and A <= 512 and L <= DEC_LREG and R % 256 == 0 and hp_al and w_al:
        tpu = 1
        while tpu < 4 and B * (R // (256 // tpu)) < cus:
            tpu *= 2
        return dict(kernel='fast', tpu=tpu, blocks=R // (256 // tpu), chunk_trips=cdiv(A, 256), rows_per_wave=cdiv(L, WAVES))
    ub = 256
    while ub > 64 and (B * cdiv(R, ub) < cus or ub // 2 >= R):
        ub //= 2
    lds = 2 * up4(A) + L
    if lds > LDS_FLOATS:
        return dict(kernel='refused', lds=lds)
    return dict(kernel='general', ub=ub, vecA=vec, lds=lds, blocks=cdiv(R, ub), dead=cdiv(R, ub) * ub - R,
                stage_trips=cdiv(A, ub), chunk_trips=cdiv(A, 256) if vec else cdiv(A, 64), rows_per_wave=cdiv(L, ub // 64),
                alpha_trips=cdiv(L, ub), tail=max(0, L - DEC_LREG))


def bwd_plan(L, A, GD, psb, psl, usb, usl, ldg, dpsb, dpsl, al=None, B=1):
    """rfn_dec_attn_bwd.  al: alignment (True = 16-B aligned) of proj, dproj, dhp, dwp, U, dg, hp, w; missing = aligned"""
    al = dict(dict(proj=True, dproj=True, dhp=True, dwp=True, U=True, dg=True, hp=True, w=True), **(al or {}))
    if B <= 0 or L <= 0 or L > MAX_L or A <= 0 or GD <= 0:
        return dict(kernel='refused')
    lds = 2 * up4(A) + 2 * up4(L) + WAVES * DEC_LREG
    if lds > LDS_FLOATS:
        return dict(kernel='refused', lds=lds)
    vecu = GD % 4 == 0 and al['U'] and al['dg'] and (usb | usl | ldg) % 4 == 0
    vec = A % 4 == 0 and (psb | psl | dpsb | dpsl) % 4 == 0 and al['proj'] and al['dproj'] and al['dhp'] and al['dwp']
    fast = (A % 4 == 0 and A <= 512 and L <= DEC_LREG and GD % 4 == 0 and (psb | psl | dpsb | dpsl | usb | usl | ldg) % 4 == 0
            and all(al.values()))
    kernel = 'fast' if fast else ('vec' if vec else 'scal') + '_' + ('vecu' if vecu else 'scalu')
    return dict(kernel=kernel, lds=lds, l_groups=1 if fast else cdiv(L, DEC_LREG), l_clamp=L % DEC_LREG != 0,
                gd_trips=cdiv(GD, 1024 if (fast or vecu) else 256), ltid_trips=cdiv(L, THREADS),
                a_trips=1 if fast else cdiv(A, 1024 if vec else 256), l4_groups=cdiv(L, 4), l4_clamp=L % 4 != 0)


def du_plan(S, B, L, GD, usb, usl, dg_al=True, du_al=True):
    if S <= 0 or B <= 0 or L <= 0 or GD <= 0:
        return dict(kernel='refused')
    if GD % 4 or not dg_al or not du_al or (usb | usl) % 4:
        return dict(kernel='scalar', col_blocks=cdiv(GD, 256))
    if S * L > LDS_FLOATS:
        return dict(kernel='refused', lds=S * L)
    return dict(kernel='vector', lds=S * L, col_blocks=cdiv(GD, 1024), l_groups=cdiv(L, DEC_LREG), guard=L % DEC_LREG != 0,
                stage_trips=cdiv(S * L, 256))


def span(shape, strides, off=0):
    """floats of the guarded buffer an operand is carved out of (Op of tests/test_attention_edges_gpu.py)"""
    return GUARD + off + 1 + sum((s - 1) * st for s, st in zip(shape, strides)) + GUARD


def span3(B, L, R, variant):
    st, off = lay3(B, L, R, variant)
    return span((B, L, R), st, off)


def span2(B, R, variant):
    ld, off = lay2(R, variant)
    return span((B, R), (ld, 1), off)


# =================================================================================================================
# forward cases
# =================================================================================================================
def F(name, B, L, A, R, maxout=0, row_div='B', lp='packed', lu='packed', lg='packed', lcp='packed', lcn='packed', lh='packed',
      hp_off=0, w_off=0, bo=True, drop=0.0, regime='std', soff=0):
    return dict(name=name, B=B, L=L, A=A, R=R, maxout=maxout, row_div=row_div, lp=lp, lu=lu, lg=lg, lcp=lcp, lcn=lcn, lh=lh,
                hp_off=hp_off, w_off=w_off, bo=bo, drop=drop, regime=regime, soff=soff)


# B: a number, 'cus' or 'half' (cus // 2); row_div 'B': every row reads the one row of proj / U
FWD_CASES = [
    # ---- fast kernel: <NG, TPU> in all six forms --------------------------------------------------------------------
    F('fast_4_1', 'cus', 8, 512, 256),
    F('fast_4_2', 'half', 8, 512, 256),
    F('fast_4_4', 2, 8, 512, 256),
    F('fast_5_1', 'cus', 7, 260, 256, maxout=1, lp='padded4', lu='padded4', lg='padded4', lh='padded4', drop=DROP_P),
    F('fast_5_2', 'half', 5, 256, 256, maxout=1, lcp='padded4', lcn='ld_plus_1', drop=DROP_P),
    F('fast_5_4_L1', 3, 1, 4, 256, maxout=1, row_div=2, bo=False, lg='ld_plus_1', lu='ld_plus_1'),
    F('fast_r512_L2', 5, 2, 256, 512, row_div=1, lp='time_major', lu='time_major', lcp='padded4', lcn='padded4', bo=False),
    F('fast_L3', 7, 3, 4, 256, row_div=3, lu='offset_1', lg='offset_1', lcp='offset_1', lcn='offset_1', lh='offset_1', soff=1),
    F('fast_L4_drop', 2, 4, 256, 256, lh='padded4', drop=DROP_P),
    # ---- general kernel with 16-B score reads, forced by hproj / w_out one float off: ub 256 / 128 / 64 ------------------
    F('gen_256', 'cus', 8, 512, 256, hp_off=1),
    F('gen_128', 'half', 8, 512, 256, w_off=1),
    F('gen_64', 2, 8, 512, 256, hp_off=1),
    F('gen_5_drop', 3, 8, 256, 256, maxout=1, row_div=2, w_off=1, lh='padded4', lg='padded4', drop=DROP_P),
    F('gen_5_256', 'cus', 7, 260, 256, maxout=1, hp_off=1, w_off=1, lp='padded4', bo=False),
    # ---- general kernel on its own conditions -------------------------------------------------------------------------
    F('scal_small', 4, 5, 30, 7, row_div=1),
    F('scal_odd_L9', 3, 9, 30, 7, maxout=1, row_div=2, lp='ld_plus_1', lu='ld_plus_1', lg='ld_plus_1', lcp='ld_plus_1',
      lcn='ld_plus_1', lh='ld_plus_1', drop=DROP_P),
    F('scal_off_A260', 2, 2, 260, 4, row_div=1, lp='offset_1', lu='padded4'),
    F('scal_tm_A256', 3, 3, 256, 130, row_div=1, lp='ld_plus_1', lu='time_major', hp_off=1, w_off=1, soff=1),
    F('r130_ub256', 'cus', 3, 4, 130, bo=False),
    F('r130_ub64', 7, 4, 4, 130, maxout=1, row_div=4),
    F('L9', 2, 9, 256, 256, lp='padded4'),
    F('L16', 'half', 16, 256, 256, maxout=1, drop=DROP_P, lh='padded4'),
    F('L17', 'cus', 17, 4, 256),
    F('L9_r512', 2, 9, 256, 512, row_div=1, lp='time_major', lu='time_major'),
    F('L257', 1, 257, 4, 130, regime='long'),
    F('L1024', 1, 1024, 4, 130, maxout=1, regime='long'),
    F('A516', 2, 2, 516, 130, row_div=1, regime='wide'),
    F('A516_scal', 2, 3, 516, 7, row_div=2, lp='offset_1', regime='wide'),
    F('A1028', 1, 4, 1028, 130, regime='wide'),
    F('A8188_lds', 1, 8, 8188, 4, regime='wide'),
    # ---- value regimes: fast kernel and scalar general kernel -----------------------------------------------------------
    F('sat_fast', 2, 8, 256, 256, regime='sat'), F('sat_scal', 2, 5, 30, 7, maxout=1, row_div=1, regime='sat'),
    F('small_fast', 2, 8, 256, 256, maxout=1, regime='small'), F('small_scal', 2, 5, 30, 7, row_div=1, regime='small'),
    F('shift+_fast', 2, 8, 256, 256, regime='shift+'), F('shift+_scal', 2, 5, 30, 7, row_div=1, regime='shift+'),
    F('shift-_fast', 2, 8, 256, 256, regime='shift-'), F('shift-_scal', 2, 5, 30, 7, maxout=1, row_div=1, regime='shift-'),
]
FWD_BY_NAME = {c['name']: c for c in FWD_CASES}


def resolve(c, cus):
    """the case with B and row_div as numbers for a device of `cus` compute units"""
    B = {'cus': cus, 'half': cus // 2}.get(c['B'], c['B'])
    return dict(c, B=B, row_div=B if c['row_div'] == 'B' else c['row_div'])


def fwd_geometry(c, cus):
    """-> resolved case, plan, bytes of device memory"""
    c = resolve(c, cus)
    B, L, A, R = c['B'], c['L'], c['A'], c['R']
    GD, Bc = (5 if c['maxout'] else 4) * R, cdiv(B, c['row_div'])
    (psb, psl, _), poff = lay3(Bc, L, A, c['lp'])
    plan = fwd_plan(B, L, A, R, cus, psb, psl, poff % 4 == 0, c['hp_off'] % 4 == 0, c['w_off'] % 4 == 0, c['row_div'], c['drop'])
    floats = (span3(Bc, L, A, c['lp']) + span3(Bc, L, GD, c['lu']) + span2(B, GD, c['lg']) + span2(B, R, c['lcp'])
              + span2(B, R, c['lcn']) + span2(B, R, c['lh']) + span((B, A), (A, 1), c['hp_off']) + span((A,), (1,), c['w_off'])
              + span((1,), (1,), c['soff']) + span((GD,), (1,), c['soff']) + span((B, L), (L, 1), c['soff']))
    return c, plan, 2 * 4 * floats                 # every operand has a snapshot beside it


def fwd_inputs(c):
    """CPU inputs of a resolved case.  proj and U are the float32 products of DV-wide thought vectors with att_2_att_h / z2h
    weights, so that the un-hoisted reference (ref_cell of tests/test_deccell_gpu.py) can be run on the same problem."""
    B, L, A, R, mo = c['B'], c['L'], c['A'], c['R'], c['maxout']
    GD, Bc = (5 if mo else 4) * R, cdiv(B, c['row_div'])
    v = rnd(Bc, L, DV, seed=1)
    Wa, ba = rnd(A, DV, seed=2, scale=0.1), rnd(A, seed=3, scale=0.1)
    Wz, bz = rnd(GD, DV, seed=4, scale=0.1), rnd(GD, seed=5, scale=0.1)
    hp, w, bo = rnd(B, A, seed=6), rnd(A, seed=7, scale=0.3), rnd(1, seed=8)
    gin, c0 = rnd(B, GD, seed=9), rnd(B, R, seed=10)
    if mo:                                         # three units whose two candidate chunks tie exactly
        gin[:, 4 * R:4 * R + 3] = gin[:, 3 * R:3 * R + 3]
        Wz[4 * R:4 * R + 3] = Wz[3 * R:3 * R + 3]
        bz[4 * R:4 * R + 3] = bz[3 * R:3 * R + 3]
    proj = (v.double() @ Wa.double().t() + ba.double()).float()                         # (Bc, L, A)
    Uv = (v.double() @ Wz.double().t()).float()                                         # (Bc, L, GD), no bias
    reg = c['regime']
    if reg == 'sat':
        proj = proj * 30.0
    elif reg == 'small':
        proj, hp = proj * 0.01, hp * 0.01
    elif reg == 'shift+':
        bo = torch.tensor([1e4])
    elif reg == 'shift-':
        bo = torch.tensor([-1e4])
    return dict(v=v, Wa=Wa, ba=ba, Wz=Wz, bz=bz, hp=hp, w=w, bo=bo if c['bo'] else None, gin=gin, c0=c0, proj=proj, U=Uv,
                row_div=c['row_div'], maxout=mo)


def tanh_(p, fast):
    return 1.0 - 2.0 / (torch.exp(2.0 * p) + 1.0) if fast else torch.tanh(p)


def cell_formulas(d, dtype=torch.float64, drop_l=None):
    """The hoisted cell in the kernels' formula order on the float32 inputs the kernel is given, in `dtype` (float32: the
    header's tanh).  drop_l: leave that l out of every row's gate sum (the mutant the tolerances must notice); 'max': the l
    of the row's largest alpha.  -> dict(alpha, sig, g, c, h, pre)"""
    f32 = dtype == torch.float32
    t = lambda x: x.to(dtype)  # noqa: E731
    B, rd, mo = d['gin'].shape[0], d['row_div'], d['maxout']
    R = d['c0'].shape[1]
    pb = torch.arange(B) // rd
    proj, Uv = t(d['proj'])[pb], t(d['U'])[pb]
    e = tanh_(proj + t(d['hp'])[:, None, :], f32)
    s = (e * t(d['w'])).sum(2)
    if d['bo'] is not None:
        s = s + t(d['bo'])
    ex = torch.exp(s - s.max(1, keepdim=True)[0])
    al = ex * (1.0 / ex.sum(1, keepdim=True))
    if drop_l == 'max':
        drop_l = al.argmax(1)
    acc = torch.zeros(B, Uv.shape[2], dtype=dtype)
    for l in range(al.shape[1]):
        term = al[:, l, None] * Uv[:, l]
        if drop_l is not None:
            term = term * (torch.as_tensor(drop_l) != l).to(dtype).reshape(-1, 1)
        acc = acc + term
    pre = (acc + t(d['bz'])) + t(d['gin'])
    sig = torch.sigmoid(pre[:, :3 * R]) if not f32 else 1.0 / (1.0 + torch.exp(-pre[:, :3 * R]))
    g = torch.max(pre[:, 3 * R:4 * R], pre[:, 4 * R:]) if mo else torch.tanh(pre[:, 3 * R:])
    c1 = sig[:, R:2 * R] * t(d['c0']) + sig[:, :R] * g
    h1 = sig[:, 2 * R:] * torch.tanh(c1)
    return dict(alpha=al, sig=sig, g=g, c=c1, h=h1, pre=pre)


def errs(a, b, keys):
    return tuple(float((a[k].double() - b[k].double()).abs().max()) for k in keys)


def fwd_yard(c):
    if c['B'] < YARD_ROWS:                         # more rows of the same shape; rows that shared one proj / U row still do
        c = dict(c, B=YARD_ROWS, row_div=YARD_ROWS if c['row_div'] >= c['B'] else c['row_div'])
    d = fwd_inputs(c)
    return errs(cell_formulas(d, torch.float32), cell_formulas(d), FWD_KEYS)


# =================================================================================================================
# backward cases
# =================================================================================================================
def Bk(name, B, L, A, GD, lp='packed', ldp='packed', lu='packed', lg='packed', acc=0, hp_off=0, w_off=0, dhp_off=0, dwp_off=0,
       regime='std', soff=0):
    return dict(name=name, B=B, L=L, A=A, GD=GD, lp=lp, ldp=ldp, lu=lu, lg=lg, acc=acc, hp_off=hp_off, w_off=w_off, dhp_off=dhp_off,
                dwp_off=dwp_off, regime=regime, soff=soff)


BWD_CASES = [
    # ---- fast body ----------------------------------------------------------------------------------------------------
    Bk('fast_L8', 2, 8, 512, 1024), Bk('fast_L5_acc', 3, 5, 256, 1280, lp='padded4', ldp='padded4', lu='padded4', lg='padded4', acc=1),
    Bk('fast_L1', 2, 1, 4, 4), Bk('fast_L4_gd2048', 2, 4, 260, 2048, ldp='time_major', acc=1),
    Bk('fast_L7_tm', 3, 7, 256, 1024, lp='time_major', ldp='padded4', lu='time_major'),
    Bk('fast_L2', 2, 2, 256, 1280, acc=1), Bk('fast_L3', 2, 3, 512, 1024, ldp='padded4'), Bk('fast_L6', 2, 6, 4, 1028, acc=1),
    # ---- <VEC, VECU> = <true, true> -----------------------------------------------------------------------------------------
    Bk('vv_L9', 2, 9, 256, 1024, acc=1), Bk('vv_L16', 2, 16, 256, 1028, lp='padded4', ldp='time_major'),
    Bk('vv_L17', 3, 17, 260, 1280, lp='time_major', lu='time_major', lg='padded4', acc=1),
    Bk('vv_L8_hpoff', 2, 8, 512, 1024, hp_off=1), Bk('vv_L5_woff', 2, 5, 256, 1280, w_off=1, acc=1),
    Bk('vv_L257', 1, 257, 256, 1024, regime='long', acc=1), Bk('vv_L1024', 1, 1024, 64, 64, regime='long'),
    Bk('vv_A516', 2, 2, 516, 64, regime='wide'), Bk('vv_A1028', 1, 5, 1028, 64, regime='wide', acc=1, ldp='padded4'),
    Bk('vv_GD4100', 1, 9, 64, 4100, regime='deep', acc=1),
    # ---- <false, true>: A % 4, proj or dproj off the 16-B conditions, dhproj / dw_part one float off --------------------
    Bk('sv_A30', 2, 5, 30, 1024, hp_off=1, soff=1), Bk('sv_poff_L5', 2, 5, 256, 1024, lp='offset_1', acc=1),
    Bk('sv_ld1_L9', 2, 9, 256, 1028, lp='ld_plus_1', acc=1), Bk('sv_dpoff_L17', 2, 17, 256, 1024, ldp='offset_1'),
    Bk('sv_dhpoff', 2, 8, 256, 1024, dhp_off=1, acc=1), Bk('sv_dwpoff_A260', 2, 3, 260, 2048, dwp_off=1, ldp='ld_plus_1'),
    # ---- <true, false>: GD % 4, U or dgates off the 16-B conditions ------------------------------------------------------
    Bk('vs_GD35', 2, 5, 256, 35, acc=1, w_off=1), Bk('vs_uoff_L9', 2, 9, 256, 1024, lu='offset_1'), Bk('vs_ldg1', 2, 8, 512, 1024, lg='ld_plus_1', acc=1),
    Bk('vs_GD258_L17', 2, 17, 260, 258, lu='padded4', ldp='padded4'), Bk('vs_dgoff', 2, 4, 4, 260, lg='offset_1', lu='time_major'),
    # ---- <false, false> ---------------------------------------------------------------------------------------------------
    Bk('ss_small', 4, 5, 30, 35, hp_off=1, w_off=1, soff=1), Bk('ss_L9_A260', 2, 9, 260, 258, lp='ld_plus_1', ldp='ld_plus_1', lu='ld_plus_1', lg='ld_plus_1', acc=1),
    Bk('ss_L257', 1, 257, 30, 35, regime='long'), Bk('ss_L1', 2, 1, 30, 35, acc=1),
]
BWD_BY_NAME = {c['name']: c for c in BWD_CASES}


def bwd_geometry(c):
    B, L, A, GD = c['B'], c['L'], c['A'], c['GD']
    (psb, psl, _), poff = lay3(B, L, A, c['lp'])
    (dpsb, dpsl, _), dpoff = lay3(B, L, A, c['ldp'])
    (usb, usl, _), uoff = lay3(B, L, GD, c['lu'])
    ldg, goff = lay2(GD, c['lg'])
    al = dict(proj=poff % 4 == 0, dproj=dpoff % 4 == 0, U=uoff % 4 == 0, dg=goff % 4 == 0, hp=c['hp_off'] % 4 == 0,
              w=c['w_off'] % 4 == 0, dhp=c['dhp_off'] % 4 == 0, dwp=c['dwp_off'] % 4 == 0)
    plan = bwd_plan(L, A, GD, psb, psl, usb, usl, ldg, dpsb, dpsl, al, B)
    floats = (span3(B, L, A, c['lp']) + span3(B, L, A, c['ldp']) + span3(B, L, GD, c['lu']) + span2(B, GD, c['lg'])
              + 3 * span((B, A), (A, 1), 1) + span((A,), (1,), 1) + span((B, L), (L, 1)))
    return plan, 2 * 4 * floats


def bwd_inputs(c):
    B, L, A, GD = c['B'], c['L'], c['A'], c['GD']
    v = rnd(B, L, DV, seed=1)
    Wa, ba, Wz = rnd(A, DV, seed=2, scale=0.1), rnd(A, seed=3, scale=0.1), rnd(GD, DV, seed=4, scale=0.1)
    hp, w, bo = rnd(B, A, seed=6), rnd(A, seed=7, scale=0.3), rnd(1, seed=8)
    proj = (v.double() @ Wa.double().t() + ba.double()).float()
    Uv = (v.double() @ Wz.double().t()).float()
    e = (torch.tanh(proj.double() + hp.double()[:, None, :]) @ w.double()) + bo.double()
    alpha = torch.softmax(e, 1).float()            # the forward's float32 alpha, as the backward is given it
    return dict(v=v, Wz=Wz, hp=hp, w=w, bo=bo, proj=proj, U=Uv, alpha=alpha, dg=rnd(B, GD, seed=11), base=rnd(B, L, A, seed=12))


def bwd_formulas(d, dtype=torch.float64, acc=0, drop_chunk=None):
    """rfn_dec_attn_bwd in the kernels' formula order on the float32 inputs, in `dtype`.  drop_chunk: leave that 4-column
    chunk out of every d alpha dot.  -> dict(dproj, dhp, dwp, dw = dwp.sum(0))"""
    f32 = dtype == torch.float32
    t = lambda x: x.to(dtype)  # noqa: E731
    Uv, dg, al = t(d['U']), t(d['dg']), t(d['alpha'])
    if drop_chunk is not None:
        dg = dg.clone()
        dg[:, 4 * drop_chunk:4 * drop_chunk + 4] = 0
    da = (Uv * dg[:, None, :]).sum(2)
    L = al.shape[1]
    dot = torch.zeros(al.shape[0], dtype=dtype)
    for l in range(L):
        dot = dot + al[:, l] * da[:, l]
    ds = al * (da - dot[:, None])
    th = tanh_(t(d['proj']) + t(d['hp'])[:, None, :], f32)
    dpre = ds[:, :, None] * t(d['w']) * (1.0 - th * th)
    dhp, dwp = torch.zeros_like(dpre[:, 0]), torch.zeros_like(dpre[:, 0])
    for l in range(L):
        dhp, dwp = dhp + dpre[:, l], dwp + ds[:, l, None] * th[:, l]
    return dict(dproj=t(d['base']) + dpre if acc else dpre, dhp=dhp, dwp=dwp, dw=dwp.sum(0))


def bwd_autograd(d):
    """fp64 autograd through the un-hoisted formulas (z = sum_l alpha_l v_l, then z2h), as tests/test_deccell_gpu.py:
    d proj, d hproj, d w_out of sum(z2h(z) * dgates)"""
    dd = lambda x: x.double()  # noqa: E731
    pr, hr, wr = dd(d['proj']).requires_grad_(True), dd(d['hp']).requires_grad_(True), dd(d['w']).requires_grad_(True)
    e = (torch.tanh(pr + hr[:, None, :]) @ wr) + dd(d['bo'])
    al = torch.softmax(e, dim=1)
    z = (dd(d['v']) * al[:, :, None]).sum(1)
    ((z @ dd(d['Wz']).t()) * dd(d['dg'])).sum().backward()
    return dict(dproj=pr.grad, dhp=hr.grad, dw=wr.grad)


def bwd_yard(c):
    d = bwd_inputs(dict(c, B=max(c['B'], YARD_ROWS)))
    return errs(bwd_formulas(d, torch.float32, c['acc']), bwd_formulas(d, acc=c['acc']), BWD_KEYS)


# =================================================================================================================
# rfn_dec_du cases: S, B, L, GD, dU layout
# =================================================================================================================
DU_CASES = [
    (1, 2, 1, 4, 'packed'), (3, 2, 8, 1024, 'packed'), (5, 3, 9, 1028, 'time_major'), (4, 2, 17, 1028, 'padded4'),
    (17, 2, 8, 4, 'padded4'), (1, 3, 17, 1024, 'time_major'), (66, 1, 9, 4, 'packed'),                 # S * L > 256: the staging loop again
    (4, 3, 8, 35, 'packed'), (3, 2, 9, 35, 'time_major'), (1, 2, 1, 35, 'padded4'),                     # scalar: GD % 4
    (3, 2, 9, 1028, 'offset_1'), (4, 2, 17, 1024, 'ld_plus_1'), (2, 3, 8, 4, 'offset_1'), (5, 2, 1, 260, 'ld_plus_1'),
]
# the same with alpha and dgates one float off and dU aligned: the scalar kernel by `!rfn_aligned16(dgates)` alone
DU_SOFF_CASES = [(3, 2, 9, 1028, 'packed'), (4, 2, 8, 1024, 'padded4'), (1, 3, 17, 4, 'time_major')]
DU_LIMIT = (3277, 1, 5, 4)                         # S * L = 16385 floats with GD % 4 == 0: one float over 64 KiB


def du_geometry(S, B, L, GD, lay, soff=0):
    """soff: alpha and dgates one float off (a misaligned dgates alone puts the call on the scalar kernel)"""
    (usb, usl, _), off = lay3(B, L, GD, lay)
    plan = du_plan(S, B, L, GD, usb, usl, soff % 4 == 0, off % 4 == 0)
    return plan, 2 * 4 * (span3(B, L, GD, lay) + span((S, B, L), (B * L, L, 1), soff) + span((S, B, GD), (B * GD, GD, 1), soff))


# =================================================================================================================
# measured yardsticks (`python tests/deccell_cases.py` prints these tables)
# =================================================================================================================
YARD_FWD = {
    # case: (alpha, sigmoid gates, g, c, h)
    'L257': (8.35e-10, 8.5e-08, 5.08e-08, 2.32e-07, 1.02e-07),
    'L1024': (2.76e-10, 7.44e-08, 1.27e-07, 3.44e-07, 1.08e-07),
    'A516': (4.02e-07, 1.55e-07, 5.49e-07, 5.28e-07, 1.98e-07),
    'A516_scal': (4.35e-07, 1.13e-07, 2.33e-07, 1.69e-07, 7.55e-08),
    'A1028': (1.29e-07, 9.33e-08, 1.63e-07, 2.33e-07, 1.04e-07),
    'A8188_lds': (2.08e-06, 2.67e-07, 1.24e-06, 3.52e-07, 1.66e-07),
    'sat_fast': (2.05e-07, 8.46e-08, 1.17e-07, 2.68e-07, 1.28e-07),
    'sat_scal': (1.19e-07, 7.82e-08, 9.33e-08, 1.68e-07, 7.23e-08),
    'small_fast': (6.5e-08, 8.46e-08, 1.6e-07, 3.04e-07, 1.26e-07),
    'small_scal': (3.81e-08, 7.42e-08, 4.46e-08, 1.03e-07, 8.68e-08),
    'shift+_fast': (0.000131, 2.77e-05, 8.67e-05, 6.86e-05, 3.27e-05),
    'shift+_scal': (0.000173, 2.91e-05, 0.000116, 9.36e-05, 6.05e-05),
    'shift-_fast': (0.000131, 2.77e-05, 8.67e-05, 6.86e-05, 3.27e-05),
    'shift-_scal': (0.000173, 4.04e-05, 0.000139, 8.83e-05, 3.92e-05),
}
YARD_BWD = {
    # case: (dproj, dhproj, dw_part.sum(0))
    'vv_L257': (2.36e-07, 1.43e-06, 5.09e-06),
    'vv_L1024': (2.75e-09, 2.65e-07, 6.17e-07),
    'vv_A516': (1.15e-07, 1.47e-07, 6.36e-07),
    'vv_A1028': (2.41e-07, 2.58e-07, 7.41e-07),
    'vv_GD4100': (7.42e-07, 1.04e-06, 6.18e-06),
    'ss_L257': (4.77e-09, 8.3e-08, 3.07e-07),
}


def yard_cases():
    return ([c for c in FWD_CASES if c['regime'] != 'std'], [c for c in BWD_CASES if c['regime'] != 'std'])


def yard_tables():
    fw, bw = yard_cases()
    return {c['name']: fwd_yard(resolve(c, 256)) for c in fw}, {c['name']: bwd_yard(c) for c in bw}


if __name__ == '__main__':
    for title, tab in zip(('YARD_FWD', 'YARD_BWD'), yard_tables()):
        print('%s = {' % title)
        for k, v in tab.items():
            print("    '%s': (%s)," % (k, ', '.join('%.3g' % x for x in v)))
        print('}')
