"""The f32 GEMM on the bf16 matrix cores (csrc/rfn_gemm_x3.hip: rfn_x3_split, rfn_x3_split_ks, rfn_x3_gemm, rfn_x3_gemm_ks
and the host helpers) swept over the shapes, strides, pointer alignments, groups and K slices at which a launcher or a loop
changes behaviour, through the C ABI (the _native.x3_* wrappers allocate images and workspace themselves: no guards).  The
cases and a Python model of the host's choices live in tests/x3_cases.py, whose docstring restates the constants;
tests/test_x3_cases_cpu.py proves without a GPU that the tables reach every branch and that the bars below tell a dropped
plane product from rounding.

Conventions: every f32 source, bias, C and `part` buffer is carved out of a NaN-filled buffer (Op / Workspace of
tests/test_gemm_edges_gpu.py) with guards in front and behind; images sit between 256 sentinel bytes.  After a call the
guards and the padding between rows hold their bits, no input (images included) has changed, every output element was
written, an image is exactly rfn_x3_image_bytes long (its pad rows and columns are zero, the sentinel is not), and `part`
was written on exactly [0, splitk * M * N) floats.  A NaN next to a source also catches an over-read that reaches the image.

What is compared with what
--------------------------
* base products (no bias, no groups, packed C, unsplit) against fp64: the hard cap (K_pad + splitk + 5) * 2^-24 * (|A||B|^T +
  |bias| + |C_prev|) element-wise, and the bars of x3_cases (6 / 8 / 16 * 2^-24 of sum |a||b| for standard-normal operands,
  4 x the committed sequential-fp32 yardstick for all-positive and wide-range ones).
* everything else is pinned to a base product BIT FOR BIT, as the epilogue and the reduce are written: + bias and + C_prev are
  f32 adds in that order; the 16-byte and the one-float epilogue store the same values; groups only move pointers; a K split
  is the slice-ordered f32 sum of the unsplit products over the slices' k ranges (an empty slice adds zeros), then + bias,
  then + C_prev; fragment-order and k-slow images give the same bits; rows do not see each other (tail quarter tiles, a
  non-finite row).
* images: x0 + x1 + x2 == x exactly, pad rows and columns zero in every plane, and every storage of the same logical matrix
  (packed, padded, odd ld, base + 1 float, either orientation, groups, one launch or two) gives byte-identical images.

Covered by reading, not by a run: the gridDim.y cap of rfn_x3_split_ks (it needs more than 65535 * 1024 columns, an image
of 12.9 GB at the least: the check is one comparison of (Mp / 4 + 255) / 256 with 65535 in front of the launch, after the
argument checks and before anything is written); the 32-bit offset limit at any M but 1, where a missing check could not
write out of bounds.
"""
import ctypes as C
import pytest
import torch

import x3_cases as XC
from x3_cases import U, cdiv
from test_gemm_edges_gpu import Op, Workspace
from test_x3_gpu import _decode, _decode_ks

pytestmark = pytest.mark.gpu

SENT = 0xA5
IMG_GUARD = 256
ERR_SHAPE, ERR_ARG = -1, -5


def N():
    import recurrent_fusion_network_amd._native as n
    return n


def cus_of(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# =================================================================================================================
# guarded images, the two writers
# =================================================================================================================
class Img:
    """`nbytes` of image between two runs of IMG_GUARD sentinel bytes (the image itself sentinel-filled too)"""

    def __init__(self, dev, nbytes):
        self.n = nbytes
        self.buf = torch.full((IMG_GUARD + nbytes + IMG_GUARD,), SENT, dtype=torch.uint8, device=dev)
        self.img = self.buf[IMG_GUARD:IMG_GUARD + nbytes]
        self.ptr = self.buf.data_ptr() + IMG_GUARD
        assert self.ptr % 16 == 0
        self.snap = None

    def guards_ok(self):
        return bool((self.buf[:IMG_GUARD] == SENT).all()) and bool((self.buf[IMG_GUARD + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())

    def freeze(self):
        self.snap = self.buf.clone()
        return self

    def unchanged(self):
        return torch.equal(self.buf, self.snap)


def ptrs(ops):
    arr = (C.c_void_p * len(ops))()
    for i, o in enumerate(ops):
        arr[i] = o if isinstance(o, int) or o is None else o.ptr
    return arr


def src_lay(cols, variant):
    """storage of an f32 source with `cols` contiguous elements per row: (ld, base offset in floats)"""
    ld4 = XC.up4(cols + 3)
    return {'packed': (cols, 0), 'padded4': (ld4, 0), 'ld_plus_1': (ld4 + 1, 0), 'offset_1': (ld4, 1)}[variant]


def write_image(dev, mats, k_fast=True, lay='packed'):
    """rfn_x3_split of the logical (rows, K) matrices `mats` (CPU), one source group each -> Img, every guard checked"""
    n = N()
    rows, K = mats[0].shape
    srcs = []
    for m in mats:
        t = m if k_fast else m.t()
        ld, off = src_lay(t.shape[1], lay)
        srcs.append(Op(t, dev, (ld, 1), off))
    nbytes = n.lib.rfn_x3_image_bytes(len(mats) * rows, K)
    assert nbytes == XC.image_bytes(len(mats) * rows, K)
    img = Img(dev, nbytes)
    rc = n.lib.rfn_x3_split(ptrs(srcs), len(srcs), ld, rows, K, int(k_fast), img.ptr, n.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert all(s.unchanged() for s in srcs), 'rfn_x3_split wrote into a source'
    assert img.guards_ok(), 'rfn_x3_split wrote outside the image'
    return img.freeze()


def write_image_ks(dev, mats, pad=0):
    """rfn_x3_split_ks of the logical (K, cols) matrices `mats` (CPU), one column group each, ld = cols + pad -> Img"""
    n = N()
    K, cols = mats[0].shape
    srcs = [Op(m, dev, (cols + pad, 1)) for m in mats]
    nbytes = n.lib.rfn_x3_image_bytes(len(mats) * cols, K)
    assert nbytes == XC.image_bytes(len(mats) * cols, K)
    img = Img(dev, nbytes)
    rc = n.lib.rfn_x3_split_ks(ptrs(srcs), len(srcs), cols + pad, K, cols, img.ptr, n.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert all(s.unchanged() for s in srcs), 'rfn_x3_split_ks wrote into a source'
    assert img.guards_ok(), 'rfn_x3_split_ks wrote outside the image'
    return img.freeze()


def check_planes(pl, x, what):
    """pl: [3][rows_pad][K_pad] decoded planes (device); x: the logical (rows, K) matrix (CPU)"""
    rows, K = x.shape
    s = pl.double().sum(0)
    assert torch.equal(s[:rows, :K].cpu(), x.double()), '%s: x0 + x1 + x2 != x' % what
    assert float(pl[:, rows:].abs().sum()) == 0.0, '%s: a pad row is not zero' % what
    assert float(pl[:, :, K:].abs().sum()) == 0.0, '%s: a pad column is not zero' % what


def values(rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, K, generator=g) * torch.exp(2 * torch.randn(rows, K, generator=g))


# =================================================================================================================
# 1. rfn_x3_split: shapes, storages, orientations
# =================================================================================================================
@pytest.mark.parametrize('rows', [1, 16, 17, 255, 256, 257])
def test_split_storages_and_orientations_give_one_image(dev, rows):
    """k_fast = 1: packed (scalar lanes unless K % 4 == 0), ld = K + 3 rounded up to 4 (float4 lanes; at K = 45 the last
    eight reduction indices of a row go through scalar lanes), that + 1 and base + 1 float (scalar); k_fast = 0 of the
    transposed data: packed, odd ld, base + 1 float.  Seven storages, one image."""
    for K in (1, 7, 8, 9, 31, 32, 33, 45):
        x = values(rows, K, 100 * rows + K)
        ref = write_image(dev, [x], True, 'packed')
        check_planes(_decode(ref.img, rows, K), x, 'rows %d K %d' % (rows, K))
        for lay in ('padded4', 'ld_plus_1', 'offset_1'):
            assert torch.equal(write_image(dev, [x], True, lay).img, ref.img), ('k_fast', rows, K, lay)
        for lay in ('packed', 'ld_plus_1', 'offset_1'):
            assert torch.equal(write_image(dev, [x], False, lay).img, ref.img), ('row-fast', rows, K, lay)
    assert XC.split_lanes(45, src_lay(45, 'padded4')[0], 0) == {'vec', 'scalar'}


@pytest.mark.parametrize('groups,rows', [(2, 32), (8, 32), (3, 64), (64, 32)])
def test_split_of_source_groups_equals_the_image_of_their_concatenation(dev, groups, rows):
    """8 x 32 and 64 x 32 fill whole multiples of 256 rows: one launch; 2 x 32 and 3 x 64 need the pad-row launch"""
    assert XC.pad_launch(groups, rows) == (groups * rows % 256 != 0)
    for K in (45, 32):
        mats = [values(rows, K, 7 * g + K + rows) for g in range(groups)]
        whole = torch.cat(mats, 0)
        ref = write_image(dev, [whole], True, 'packed')
        check_planes(_decode(ref.img, groups * rows, K), whole, '%d x %d' % (groups, rows))
        for k_fast in (True, False):
            for lay in ('packed', 'padded4', 'offset_1'):
                got = write_image(dev, mats, k_fast, lay)
                assert torch.equal(got.img, ref.img), (groups, rows, K, k_fast, lay)


# =================================================================================================================
# 2. rfn_x3_split_ks
# =================================================================================================================
@pytest.mark.parametrize('groups', [1, 3, 64])
def test_k_slow_images(dev, groups):
    for cols in (4, 36, 256, 260):
        for K in (1, 31, 32, 33, 70):
            mats = [values(K, cols, 11 * g + K + cols) for g in range(groups)]
            whole = torch.cat(mats, 1)
            imgs = [write_image_ks(dev, mats, pad) for pad in (0, 4)]
            pl = _decode_ks(imgs[0].img, K, groups * cols)              # [3][k_pad][mp]
            check_planes(pl, whole, 'k-slow %d x %d x %d' % (groups, cols, K))
            assert torch.equal(imgs[0].img, imgs[1].img), 'ld = cols + 4 gives another image'


# =================================================================================================================
# the GEMM runner
# =================================================================================================================
_IMGS, _BASE, _REF = {}, {}, {}


def gemm_images(dev, kind, a, b, key=None):
    """images of A (M, K) and B (N, K) (CPU) of the kind: fragment order through rfn_x3_split, k-slow through rfn_x3_split_ks
    of the transposed operands ((K, M) and (K, N), columns zero-padded to a multiple of 4: pad columns of an image are zero)"""
    if key is not None and (kind,) + key in _IMGS:
        return _IMGS[(kind,) + key]
    out = []
    for x in (a, b):
        if kind == 'frag':
            out.append(write_image(dev, [x], True, 'packed'))
        else:
            t = torch.zeros(x.shape[1], XC.up4(x.shape[0]))
            t[:, :x.shape[0]] = x.t()
            im = write_image_ks(dev, [t])
            assert im.n == XC.image_bytes(x.shape[0], x.shape[1])
            out.append(im)
    if key is not None:
        if len(_IMGS) > 64:
            _IMGS.clear()
        _IMGS[(kind,) + key] = out
    return out


def gemm(dev, kind, imgs, M, N_, K, gm=None, gn=None, lay='packed', bias=None, prev=None, splitk=1, boff=0, finite=True):
    """One rfn_x3_gemm / rfn_x3_gemm_ks call with every operand guarded -> the M x N result assembled on the device.
    bias: (N,) CPU or None; prev: (M, N) CPU or None (then accumulate = 0 onto NaN-filled C)."""
    n = N()
    gm_, gn_ = gm or M, gn or N_
    ngm, ngn = cdiv(M, gm_), cdiv(N_, gn_)
    ldc, off = XC.lay2(min(gn_, N_), lay)
    Cs, Bs, where = [], [], []
    for i in range(ngm):
        for j in range(ngn):
            r0, r1, c0, c1 = i * gm_, min(M, (i + 1) * gm_), j * gn_, min(N_, (j + 1) * gn_)
            Cs.append(Op(prev[r0:r1, c0:c1] if prev is not None else (r1 - r0, c1 - c0), dev, (ldc, 1), off))
            where.append((r0, r1, c0, c1))
            if bias is not None:
                Bs.append(Op(bias[c0:c1], dev, off=boff))
    ws = Workspace(dev, 4 * splitk * M * N_) if splitk > 1 else None
    if ws:
        assert n.lib.rfn_x3_part_floats(M, N_, splitk) == ws.n
    fn = n.lib.rfn_x3_gemm_ks if kind == 'ks' else n.lib.rfn_x3_gemm
    rc = fn(M, N_, K, imgs[0].ptr, imgs[1].ptr, gm_, gn_, ptrs(Cs), ptrs(Bs) if Bs else None, ldc, int(prev is not None),
            splitk, ws.ptr if ws else None, n.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert imgs[0].unchanged() and imgs[1].unchanged(), 'the GEMM wrote into an image'
    assert all(b.unchanged() for b in Bs), 'the GEMM wrote into a bias'
    for c in Cs:
        assert c.outside_ok(), 'the GEMM wrote outside its output (guards or the padding between rows)'
        assert c.written() or not finite, 'an output element was never written'
    if ws:
        ws.check(splitk * M * N_)
    out = torch.empty(M, N_, device=dev)
    for c, (r0, r1, c0, c1) in zip(Cs, where):
        out[r0:r1, c0:c1] = c.v
    return out


def base(dev, kind, M, N_, K, regime='normal', krange=None):
    """the unsplit, bias-free, packed, single-group product of the case's operands (over the k range, if given), cached"""
    key = (kind, M, N_, K, regime, krange)
    if key not in _BASE:
        a, b, _, _ = XC.operands(M, N_, K, regime, prev=False) if regime == 'normal' else XC.operands(M, N_, K, regime)
        if krange is not None:
            a, b = a[:, krange[0]:krange[1]].contiguous(), b[:, krange[0]:krange[1]].contiguous()
        imgs = gemm_images(dev, kind, a, b, (M, N_, K, regime, krange))
        if len(_BASE) > 64:
            _BASE.clear()
        _BASE[key] = gemm(dev, kind, imgs, M, N_, a.shape[1])
    return _BASE[key]


def images_of(dev, kind, M, N_, K, regime='normal'):
    a, b, _, _ = XC.operands(M, N_, K, regime, prev=False) if regime == 'normal' else XC.operands(M, N_, K, regime)
    return gemm_images(dev, kind, a, b, (M, N_, K, regime, None))


def fp64(dev, M, N_, K, regime='normal'):
    key = (M, N_, K, regime)
    if key not in _REF:
        a, b, _, _ = XC.operands(M, N_, K, regime, prev=False) if regime == 'normal' else XC.operands(M, N_, K, regime)
        if len(_REF) > 8:
            _REF.clear()
        _REF[key] = ((a.double() @ b.double().t()).to(dev), (a.double().abs() @ b.double().abs().t()).to(dev))
    return _REF[key]


def check_fp64(dev, got, M, N_, K, bar, regime='normal', bias=None, prev=None, splitk=1, what=''):
    ref, mag = fp64(dev, M, N_, K, regime)
    if bias is not None:
        ref, mag = ref + bias.double().to(dev), mag + bias.double().abs().to(dev)
    if prev is not None:
        ref, mag = ref + prev.double().to(dev), mag + prev.double().abs().to(dev)
    err = XC.rel_err(got, ref, mag)
    print('%s %dx%dx%d %s splitk %d: %.3f x 2^-24 of sum |a||b| (bar %.1f)' % (what, M, N_, K, regime, splitk, err / U, bar / U))
    assert XC.hard_cap_ok(got, ref, mag, K, splitk), '%s: outside the worst-case bound' % what
    assert err <= bar, '%s: %.3f x 2^-24 > %.1f' % (what, err / U, bar / U)


def ids(shapes):
    return ['x'.join(map(str, s)) for s in shapes]


# =================================================================================================================
# 3. base products: smallest tiles, K edges, tile edges, wave-tile edges, the tile walk
# =================================================================================================================
@pytest.mark.parametrize('shape', XC.BASE_SHAPES + XC.WALK, ids=ids(XC.BASE_SHAPES + XC.WALK))
def test_base_products_against_fp64_on_both_image_kinds(dev, shape):
    """onto a NaN-filled C: every element is written, by exactly the tiles the walk hands out"""
    M, N_, K = shape
    outs = {}
    for kind in XC.KINDS:
        outs[kind] = base(dev, kind, M, N_, K)
        check_fp64(dev, outs[kind], M, N_, K, XC.BAR_PLAIN, what=kind)
    assert torch.equal(outs['frag'], outs['ks']), 'fragment-order and k-slow images give other bits'
    if shape in XC.WALK:
        _BASE.clear()
        _IMGS.clear()


# =================================================================================================================
# 4. bias, accumulate, the two epilogues
# =================================================================================================================
@pytest.mark.parametrize('shape', XC.SMALL + XC.K_EDGES + XC.WAVE_EDGES, ids=ids(XC.SMALL + XC.K_EDGES + XC.WAVE_EDGES))
def test_bias_and_accumulate_are_f32_adds_onto_the_base_product(dev, shape):
    M, N_, K = shape
    _, _, bias, prev = XC.operands(M, N_, K)
    for kind in XC.KINDS:
        b0 = base(dev, kind, M, N_, K)
        imgs = images_of(dev, kind, M, N_, K)
        wb = gemm(dev, kind, imgs, M, N_, K, bias=bias)
        assert torch.equal(wb, b0 + bias.to(dev)), '%s: bias is not base + bias' % kind
        acc = gemm(dev, kind, imgs, M, N_, K, bias=bias, prev=prev, boff=1)
        assert torch.equal(acc, (b0 + bias.to(dev)) + prev.to(dev)), '%s: accumulate is not (base + bias) + C_prev' % kind
        assert torch.equal(gemm(dev, kind, imgs, M, N_, K, prev=prev), b0 + prev.to(dev))
        check_fp64(dev, acc, M, N_, K, XC.BAR_BIAS, bias=bias, prev=prev, what=kind)


@pytest.mark.parametrize('shape', XC.EPILOGUE_SHAPES, ids=ids(XC.EPILOGUE_SHAPES))
def test_the_two_epilogues_store_the_same_bits(dev, shape):
    """packed and ldc = N + 4: 16-byte stores for whole wave tiles; ldc + 1 and base + 1 float: one float at a time for all.
    (256, 256): every wave tile is whole, so the scalar epilogue runs for alignment alone."""
    M, N_, K = shape
    _, _, bias, prev = XC.operands(M, N_, K)
    for kind in XC.KINDS:
        b0 = base(dev, kind, M, N_, K)
        imgs = images_of(dev, kind, M, N_, K)
        want = {None: b0, 'bias': b0 + bias.to(dev)}
        for lay in XC.LAYOUTS:
            kinds_ = XC.epilogues(kind, M, N_, *XC.lay2(N_, lay))
            assert (kinds_['vector'] > 0) == (lay in ('packed', 'padded4'))
            assert torch.equal(gemm(dev, kind, imgs, M, N_, K, lay=lay), want[None]), (kind, lay)
            assert torch.equal(gemm(dev, kind, imgs, M, N_, K, lay=lay, bias=bias, boff=1), want['bias']), (kind, lay, 'bias')
        assert torch.equal(gemm(dev, kind, imgs, M, N_, K, lay='padded4', bias=bias, prev=prev),
                           (b0 + bias.to(dev)) + prev.to(dev))


# =================================================================================================================
# 5. output groups
# =================================================================================================================
@pytest.mark.parametrize('case', XC.GROUP_CASES, ids=[c[0].replace(' ', '_') for c in XC.GROUP_CASES])
def test_output_groups_only_move_pointers(dev, case):
    _, M, N_, K, gm, gn, with_bias = case
    _, _, bias, _ = XC.operands(M, N_, K, prev=False)
    bias = bias if with_bias else None
    for kind in XC.KINDS:
        b0 = base(dev, kind, M, N_, K)
        imgs = images_of(dev, kind, M, N_, K)
        one = gemm(dev, kind, imgs, M, N_, K, bias=bias)
        assert torch.equal(one, b0 + bias.to(dev) if with_bias else b0)
        for lay in ('packed', 'offset_1'):
            got = gemm(dev, kind, imgs, M, N_, K, gm=gm, gn=gn, bias=bias, lay=lay)
            assert torch.equal(got, one), '%s %s: groups change the bits' % (kind, lay)
        check_fp64(dev, one, M, N_, K, XC.BAR_BIAS if with_bias else XC.BAR_PLAIN, bias=bias, what=kind)
    _BASE.clear()
    _IMGS.clear()


# =================================================================================================================
# 6. split-K
# =================================================================================================================
def slice_sum(dev, kind, M, N_, K, splitk):
    """((p0 + p1) + ...) of the unsplit products over the slices' k ranges; an empty slice contributes zeros"""
    total = None
    for b, e in XC.slices(K, splitk):
        p = base(dev, kind, M, N_, K, krange=(b, e)) if e > b else torch.zeros(M, N_, device=dev)
        total = p if total is None else total + p
    return total


@pytest.mark.parametrize('splitk', XC.SPLITKS)
@pytest.mark.parametrize('kind', XC.KINDS)
def test_split_k_is_the_slice_ordered_sum(dev, kind, splitk):
    """nkc = 11: 7 slices leave a one-piece slice and an empty one, 11 slices one piece each; with row groups, bias,
    accumulate and a padded ldc, each alone and all together"""
    M, N_, K = XC.SPLIT_SHAPE
    _, _, bias, prev = XC.operands(M, N_, K)
    imgs = images_of(dev, kind, M, N_, K)
    want = slice_sum(dev, kind, M, N_, K, splitk)
    assert sum(1 for b, e in XC.slices(K, splitk) if e <= b) == (1 if splitk == 7 else 0)
    for name, gm, wb, acc, lay in XC.SPLIT_OPTS:
        got = gemm(dev, kind, imgs, M, N_, K, gm=gm, lay=lay, bias=bias if wb else None, prev=prev if acc else None, splitk=splitk)
        w = want
        if wb:
            w = w + bias.to(dev)
        if acc:
            w = w + prev.to(dev)
        assert torch.equal(got, w), '%s splitk %d %s: not the slice-ordered sum' % (kind, splitk, name)
        check_fp64(dev, got, M, N_, K, XC.BAR_BIAS if wb or acc else XC.BAR_PLAIN, bias=bias if wb else None,
                   prev=prev if acc else None, splitk=splitk, what='%s %s' % (kind, name))


@pytest.mark.parametrize('kind', XC.KINDS)
def test_split_k_over_column_groups_and_with_trailing_empty_slices(dev, kind):
    M, N_, K, gn, splitk = XC.SPLIT_GN
    _, _, bias, prev = XC.operands(M, N_, K)
    imgs = images_of(dev, kind, M, N_, K)
    want = slice_sum(dev, kind, M, N_, K, splitk) + bias.to(dev)
    for gm in (None, 256):
        assert torch.equal(gemm(dev, kind, imgs, M, N_, K, gm=gm, gn=gn, bias=bias, splitk=splitk), want)
        assert torch.equal(gemm(dev, kind, imgs, M, N_, K, gm=gm, gn=gn, bias=bias, prev=prev, splitk=splitk, lay='padded4'),
                           want + prev.to(dev))
    check_fp64(dev, want, M, N_, K, XC.BAR_BIAS, bias=bias, splitk=splitk, what=kind)
    # nkc = 10 in 7 slices: per = 2, two empty slices behind the last piece
    M, N_, K, splitk = 70, 72, 320, 7
    assert [e > b for b, e in XC.slices(K, splitk)] == [True] * 5 + [False] * 2
    got = gemm(dev, kind, images_of(dev, kind, M, N_, K), M, N_, K, splitk=splitk)
    assert torch.equal(got, slice_sum(dev, kind, M, N_, K, splitk))
    check_fp64(dev, got, M, N_, K, XC.BAR_PLAIN, splitk=splitk, what=kind)


# =================================================================================================================
# 7. the tail round
# =================================================================================================================
@pytest.mark.parametrize('kind', XC.KINDS)
def test_tail_round_under_three_tile_columns_with_groups_and_bias(dev, kind):
    """tiles_n = 3 < 4: every index of the walk lies in the ragged column group; the tiles behind two rounds of the chip are
    done as quarter tiles.  Column groups of 256 with their bias vectors; the last 300 rows keep the bits of a 300-row
    launch, which has no tail."""
    cus = cus_of(dev)
    M, N_, K = XC.tail_shape(cus)
    assert XC.has_tail(M, N_, cus) and not XC.has_tail(300, N_, cus)
    a, b, bias, _ = XC.operands(M, N_, K, prev=False)
    imgs = gemm_images(dev, kind, a, b)
    out = gemm(dev, kind, imgs, M, N_, K, gn=256, bias=bias)
    ad, bd = a.to(dev).double(), b.to(dev).double()
    ref, mag = ad @ bd.t() + bias.to(dev).double(), ad.abs() @ bd.abs().t() + bias.to(dev).double().abs()
    err = XC.rel_err(out, ref, mag)
    print('%s tail %dx%dx%d: %.3f x 2^-24' % (kind, M, N_, K, err / U))
    assert XC.hard_cap_ok(out, ref, mag, K) and err <= XC.BAR_TAIL
    del ref, mag, ad, bd
    last = gemm_images(dev, kind, a[M - 300:].contiguous(), b)
    out2 = gemm(dev, kind, last, 300, N_, K, gn=256, bias=bias)
    assert torch.equal(out2, out[M - 300:]), 'the quarter tiles of the tail give other bits than whole tiles'
    del out, out2, imgs, last
    torch.cuda.empty_cache()


# =================================================================================================================
# 8. values
# =================================================================================================================
@pytest.mark.parametrize('kind', XC.KINDS)
def test_a_non_finite_row_stays_in_its_row(dev, kind):
    M, N_, K = 70, 72, 33
    a, b, _, _ = XC.operands(M, N_, K, prev=False)
    a = a.clone()
    a[5, 3], a[40, 20] = float('inf'), float('nan')
    got = gemm(dev, kind, gemm_images(dev, kind, a, b), M, N_, K, finite=False)
    clean = base(dev, kind, M, N_, K)
    rows = [r for r in range(M) if r not in (5, 40)]
    assert torch.equal(got[rows], clean[rows]), 'a non-finite value of one row of A reached another output row'
    assert not bool(torch.isfinite(got[[5, 40]]).any())


@pytest.mark.parametrize('case', XC.VALUE_CASES, ids=['%s_%dx%dx%d_s%d' % c for c in XC.VALUE_CASES])
def test_all_positive_and_wide_range_operands_against_the_yardstick(dev, case):
    regime, M, N_, K, splitk = case
    outs = []
    for kind in XC.KINDS:
        imgs = images_of(dev, kind, M, N_, K, regime)
        got = gemm(dev, kind, imgs, M, N_, K, splitk=splitk)
        check_fp64(dev, got, M, N_, K, XC.bar(regime, M, N_, K), regime=regime, splitk=splitk, what=kind)
        outs.append(got)
    assert torch.equal(outs[0], outs[1])


# =================================================================================================================
# 9. refusals: the documented code, nothing launched, nothing written
# =================================================================================================================
GEMM_REFUSALS = [
    # name, M, N, K, gm, gn, ldc, splitk, with part, NULL argument, code
    ('null image A', 64, 64, 64, 64, 64, 64, 1, True, 'A', ERR_ARG),
    ('null image B', 64, 64, 64, 64, 64, 64, 1, True, 'B', ERR_ARG),
    ('null C table', 64, 64, 64, 64, 64, 64, 1, True, 'C', ERR_ARG),
    ('M 0', 0, 64, 64, 64, 64, 64, 1, True, None, ERR_ARG),
    ('N -1', 64, -1, 64, 64, 64, 64, 1, True, None, ERR_ARG),
    ('K 0', 64, 64, 0, 64, 64, 64, 1, True, None, ERR_ARG),
    ('gm 0', 64, 64, 64, 0, 64, 64, 1, True, None, ERR_ARG),
    ('68 groups', 17 * 256, 4 * 256, 8, 256, 256, 256, 1, True, None, ERR_SHAPE),
    ('gn 100 three column groups', 256, 256, 32, 256, 100, 100, 1, True, None, ERR_SHAPE),
    ('gm 100 two row groups', 200, 64, 32, 100, 64, 64, 1, True, None, ERR_SHAPE),
    ('splitk nkc + 1', 64, 64, 64, 64, 64, 64, 3, True, None, ERR_SHAPE),
    ('split without part', 64, 64, 64, 64, 64, 64, 2, False, None, ERR_ARG),
    ('split N % 4', 64, 66, 64, 64, 66, 66, 2, True, None, ERR_ARG),
    ('ldc 2^22', 1, 4, 8, 1, 4, 2 ** 22, 1, True, None, ERR_SHAPE),
]


@pytest.mark.parametrize('kind', XC.KINDS)
@pytest.mark.parametrize('r', GEMM_REFUSALS, ids=[r[0].replace(' ', '_') for r in GEMM_REFUSALS])
def test_gemm_refusals_write_nothing(dev, kind, r):
    """every buffer is as large as the refused call would need, so a missing check could not write out of bounds either"""
    n = N()
    name, M, N_, K, gm, gn, ldc, splitk, with_part, null, code = r
    assert XC.gemm_refusal(M, N_, K, gm, gn, ldc, splitk, with_part, null is not None) == code
    m1, n1, k1 = max(M, 1), max(N_, 1), max(K, 1)
    imgs = [Img(dev, XC.image_bytes(m1, k1)), Img(dev, XC.image_bytes(n1, k1))]
    ngroups = cdiv(m1, max(gm, 1)) * cdiv(n1, max(gn, 1))
    rows, cols = min(m1, max(gm, 1)), min(n1, max(gn, 1))
    ldo = cols if ldc >= 2 ** 22 else ldc
    Cs = [Op((rows, cols), dev, (ldo, 1)) for _ in range(ngroups)]
    Bs = [Op((cols,), dev) for _ in range(ngroups)]
    ws = Workspace(dev, 4 * max(splitk * m1 * n1, 1024))
    fn = n.lib.rfn_x3_gemm_ks if kind == 'ks' else n.lib.rfn_x3_gemm
    rc = fn(M, N_, K, None if null == 'A' else imgs[0].ptr, None if null == 'B' else imgs[1].ptr, gm, gn,
            None if null == 'C' else ptrs(Cs), ptrs(Bs), ldc, 0, splitk, ws.ptr if with_part else None, n.stream_ptr())
    torch.cuda.synchronize()
    assert rc == code, (name, rc)
    assert all(o.unchanged() for o in Cs + Bs), '%s: a refused call wrote into C or a bias' % name
    assert all(i.untouched() for i in imgs)
    ws.check(0)


SPLIT_REFUSALS = [
    # name, groups, rows, K, NULL argument, code
    ('65 groups', 65, 32, 8, None, ERR_ARG), ('rows % 32 with two groups', 2, 48, 8, None, ERR_SHAPE),
    ('null table', 1, 32, 8, 'table', ERR_ARG), ('null image', 1, 32, 8, 'image', ERR_ARG), ('null entry', 2, 32, 8, 'entry', ERR_ARG),
    ('rows 0', 1, 0, 8, None, ERR_ARG), ('K 0', 1, 32, 0, None, ERR_ARG), ('groups 0', 0, 32, 8, None, ERR_ARG),
]


@pytest.mark.parametrize('k_fast', [1, 0])
@pytest.mark.parametrize('r', SPLIT_REFUSALS, ids=[r[0].replace(' ', '_') for r in SPLIT_REFUSALS])
def test_split_refusals_write_nothing(dev, k_fast, r):
    n = N()
    name, groups, rows, K, null, code = r
    assert XC.split_refusal(groups, rows, K, null is not None) == code
    g1, r1, k1 = max(groups, 1), max(rows, 1), max(K, 1)
    srcs = [Op(torch.ones(r1, k1) if k_fast else torch.ones(k1, r1), dev) for _ in range(g1)]
    img = Img(dev, XC.image_bytes(g1 * r1, k1))
    arr = ptrs(srcs)
    if null == 'entry':
        arr[1] = None
    rc = n.lib.rfn_x3_split(None if null == 'table' else arr, groups, k1 if k_fast else r1, rows, K, k_fast,
                            None if null == 'image' else img.ptr, n.stream_ptr())
    torch.cuda.synchronize()
    assert rc == code, (name, rc)
    assert img.untouched() and all(s.unchanged() for s in srcs), '%s: a refused call wrote' % name


SPLIT_KS_REFUSALS = [
    # name, groups, cols, ld, K, source offset in floats, NULL argument, code
    ('65 groups', 65, 4, 4, 8, 0, None, ERR_ARG), ('cols % 4', 1, 6, 8, 8, 0, None, ERR_SHAPE), ('ld % 4', 1, 4, 9, 8, 0, None, ERR_SHAPE),
    ('misaligned source', 1, 4, 8, 8, 1, None, ERR_ARG), ('null table', 1, 4, 4, 8, 0, 'table', ERR_ARG),
    ('null image', 1, 4, 4, 8, 0, 'image', ERR_ARG), ('null entry', 2, 4, 4, 8, 0, 'entry', ERR_ARG),
    ('K 0', 1, 4, 4, 0, 0, None, ERR_ARG), ('cols 0', 1, 0, 4, 8, 0, None, ERR_ARG), ('groups 0', 0, 4, 4, 8, 0, None, ERR_ARG),
]


@pytest.mark.parametrize('r', SPLIT_KS_REFUSALS, ids=[r[0].replace(' ', '_') for r in SPLIT_KS_REFUSALS])
def test_k_slow_split_refusals_write_nothing(dev, r):
    n = N()
    name, groups, cols, ld, K, off, null, code = r
    assert XC.split_ks_refusal(groups, ld, K, cols, off, null is not None) == code
    g1, c1, k1 = max(groups, 1), max(cols, 1), max(K, 1)
    srcs = [Op(torch.ones(k1, XC.up4(c1)), dev, (ld + 4, 1), off) for _ in range(g1)]
    img = Img(dev, XC.image_bytes(g1 * XC.up4(c1), k1))
    arr = ptrs(srcs)
    if null == 'entry':
        arr[1] = None
    rc = n.lib.rfn_x3_split_ks(None if null == 'table' else arr, groups, ld, K, cols, None if null == 'image' else img.ptr,
                               n.stream_ptr())
    torch.cuda.synchronize()
    assert rc == code, (name, rc)
    assert img.untouched() and all(s.unchanged() for s in srcs), '%s: a refused call wrote' % name


# =================================================================================================================
# 10. host helpers
# =================================================================================================================
def test_image_and_workspace_sizes_follow_the_documented_formulas(dev):
    n = N()
    for rows in (-1, 0, 1, 255, 256, 257, 5000, 100000):
        for K in (-1, 0, 1, 31, 32, 33, 50176):
            assert n.lib.rfn_x3_image_bytes(rows, K) == XC.image_bytes(rows, K) == (
                0 if rows < 1 or K < 1 else cdiv(rows, 256) * 256 * cdiv(K, 32) * 32 * 6)
    for M, N_, s in ((0, 5, 3), (5, 0, 3), (5, 7, 0), (5, 7, 1), (5, 7, 2), (512, 260, 7), (50000, 50000, 3)):
        assert n.lib.rfn_x3_part_floats(M, N_, s) == XC.part_floats(M, N_, s) == (s * M * N_ if s > 1 else 0)


def test_the_suggested_split_keeps_its_promises(dev):
    """at least 1; 1 when one round of tiles fills the chip; otherwise nkc / s >= 64 unless s == 1 (the slice rule's per =
    ceil(nkc / s) is then >= 64: slices average 64 pieces or more; the last one holds what is left and may be shorter or
    empty, which the kernel supports); never above nkc, the bound rfn_x3_gemm_ks refuses beyond"""
    n = N()
    cus = cus_of(dev)
    for M in (1, 256, 257, 1000, 2048, 4096, 10000):
        for N_ in (4, 256, 260, 1000, 2048, 8192):
            for K in (1, 32, 2047, 2048, 2049, 4096, 10000, 50176, 200000):
                s, nkc = n.lib.rfn_x3_splitk_for(M, N_, K), cdiv(K, 32)
                tiles = cdiv(M, 256) * cdiv(N_, 256)
                assert s == XC.splitk_for(M, N_, K, cus), (M, N_, K)
                assert 1 <= s <= nkc
                if tiles >= cus:
                    assert s == 1
                elif s > 1:
                    assert nkc // s >= 64 and cdiv(nkc, s) >= 64
                    assert XC.gemm_refusal(M, XC.up4(N_), K, M, XC.up4(N_), XC.up4(N_), s) == XC.OK
