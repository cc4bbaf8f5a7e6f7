"""Case tables of the bf16-plane GEMM sweep (tests/test_x3_edges_gpu.py) and a plain-Python restatement of the host-side
choices of csrc/rfn_gemm_x3.hip: the padded image sizes, the K slices of a split and which of them are empty, the tail
round, the tile walk (XCD remap, bands, column groups, quarter tiles), which epilogue a wave tile takes, and the refusals.
Nothing is imported from the C side and nothing here needs a GPU: tests/test_x3_cases_cpu.py asserts that the tables reach
every branch, that the walk is a bijection, and that the tolerances tell a dropped plane product from rounding.

Constants restated from csrc/rfn_gemm_x3.hip and include/rfn.h:
    block tile 256 x 256 (X3_BM x X3_BN); pieces of 16 rows x 32 k (1 KiB per plane); image rows padded to 256, K to 32,
    6 bytes per padded element; at most 64 source groups and 64 output groups; gm (gn) a multiple of 256 unless it covers M (N);
    wave tiles: fragment-order images 4 x 2 waves = 64 rows x 128 columns each, k-slow images 2 x 4 waves = 128 x 64 (the
    quarter tiles of the tail round: 32 x 64 and 64 x 32); a wave tile wholly outside M x N returns early;
    epilogue of a wave tile: 16-byte stores through LDS when the wave tile lies wholly inside M x N, accumulate is off and
    both its first element's address and the leading dimension in bytes are multiples of 16; else one float at a time;
    tile walk: bands of 8 tile rows x groups of 4 tile columns, row-major inside a group, ragged last band / last group;
    block id -> walk index over 8 XCDs: q, r = divmod(main_tiles, 8), xcd = id % 8, index = (xcd < r ? xcd (q + 1) :
    r (q + 1) + (xcd - r) q) + id / 8;
    tail rule: tiles // CUs >= 2, 0 < rem = tiles % CUs, 4 * rem <= CUs and splitk == 1: the last rem tiles are done as
    four quarter tiles each (quarter qd at rows (qd >> 1) * 128, columns (qd & 1) * 128);
    slice rule: per = ceil(nkc / splitk); slice s takes the pieces [s * per, min((s + 1) * per, nkc)), possibly none (it
    then writes zeros); splitk <= nkc; the reduce adds the slices in order, then the bias, then the previous C;
    rfn_x3_splitk_for: 1 when tiles >= CUs, else the largest s <= (CUs + tiles / 2) / tiles with nkc / s >= 64, at least 1;
    32-bit tile offsets: 256 * ldc * 4 (split: 256 * N * 4) < 2^32, i.e. ldc < 2^22.

Tolerances (in units of sum_k |a||b|, as tests/test_x3_gpu.py):
    hard cap (derived, loose): (K_pad + splitk + 5) * 2^-24 * (|A||B|^T + |bias| + |C_prev|) element-wise;
    standard-normal operands: 6 * 2^-24 plain or split, 8 * 2^-24 with bias or accumulate (the bars test_x3_gpu.py uses);
    the tail shape (max over ~3e7 outputs): 16 * 2^-24;
    all-positive and wide-range operands: the YARDSTICK -- the same product accumulated sequentially in k order in plain
    fp32 on the CPU, max error against fp64 over sum_k |a||b| -- measured per case and committed in YARD below; the kernel
    gets 4 x that for its other association, never less than 6 * 2^-24.  `python tests/x3_cases.py` re-measures YARD.
"""
import numpy as np
import torch

U = 2.0 ** -24
TILE, RB, KC, ROW_PAD = 256, 16, 32, 256
BAND_ROWS, BAND_COLS, XCDS = 8, 4, 8
MAX_GROUPS = 64
WAVES = {'frag': (4, 2), 'ks': (2, 4)}             # image kind -> (waves along M, waves along N) of a block
KINDS = ('frag', 'ks')
OK, ERR_SHAPE, ERR_ARG = 0, -1, -5
LAYOUTS = ('packed', 'padded4', 'ld_plus_1', 'offset_1')
YARD_FACTOR, YARD_FLOOR = 4.0, 6 * U
BAR_PLAIN, BAR_BIAS, BAR_TAIL = 6 * U, 8 * U, 16 * U


def cdiv(a, b):
    return (a + b - 1) // b


def up4(v):
    return (v + 3) // 4 * 4


def lay2(cols, variant):
    """leading dimension and base offset (floats) of a row-major matrix with `cols` columns"""
    return {'packed': (cols, 0), 'padded4': (cols + 4, 0), 'ld_plus_1': (cols + 5, 0), 'offset_1': (cols + 4, 1)}[variant]


# =================================================================================================================
# the model
# =================================================================================================================
def rows_pad(rows):
    return cdiv(rows, ROW_PAD) * ROW_PAD


def k_pad(K):
    return cdiv(K, KC) * KC


def image_bytes(rows, K):
    return 0 if rows < 1 or K < 1 else rows_pad(rows) * k_pad(K) * 6


def part_floats(M, N, splitk):
    return splitk * M * N if splitk > 1 else 0


def slices(K, splitk):
    """[(first k, last k + 1)] of every K slice; an empty slice is (K, K)"""
    nkc = k_pad(K) // KC
    per = cdiv(nkc, max(1, splitk))
    out = []
    for s in range(max(1, splitk)):
        b, e = s * per, min(nkc, (s + 1) * per)
        out.append((b * KC, min(K, e * KC)) if e > b else (K, K))
    return out


def main_tiles(tiles, cus, splitk=1):
    """tiles done whole; the rest go to the tail round"""
    rem = tiles % cus
    tail = splitk == 1 and tiles // cus >= 2 and rem > 0 and 4 * rem <= cus
    return tiles - rem if tail else tiles


def has_tail(M, N, cus, splitk=1):
    tiles = cdiv(M, TILE) * cdiv(N, TILE)
    return main_tiles(tiles, cus, splitk) < tiles


def tile_of(wg, tiles_m, tiles_n):
    """walk index -> (tile row, tile column); wg an int or an integer array (x3_tile_of)"""
    wg = np.asarray(wg)
    per_band = BAND_ROWS * tiles_n
    band = wg // per_band
    idx = wg - band * per_band
    br = np.minimum(BAND_ROWS, tiles_m - band * BAND_ROWS)
    per_group = br * BAND_COLS
    grp = idx // per_group
    full = tiles_n // BAND_COLS
    ragged = grp >= full
    grp = np.where(ragged, full, grp)
    gc = np.where(ragged, tiles_n - full * BAND_COLS, BAND_COLS)
    gc = np.maximum(gc, 1)                          # (never divides when tiles_n % 4 == 0: no index reaches the ragged group)
    idx = idx - grp * per_group
    r = idx // gc
    return band * BAND_ROWS + r, grp * BAND_COLS + (idx - r * gc)


def xcd_remap(main):
    """block id -> walk index for the `main` whole-tile blocks"""
    wg = np.arange(main)
    q, r = divmod(main, XCDS)
    xcd = wg % XCDS
    return np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + wg // XCDS


def walk(tiles_m, tiles_n, main):
    """every block of a launch -> (tile row, tile column, quarter); quarter -1: the whole tile"""
    tiles = tiles_m * tiles_n
    tm, tn = tile_of(xcd_remap(main), tiles_m, tiles_n)
    t = np.arange(4 * (tiles - main))
    tm2, tn2 = tile_of(main + t // 4, tiles_m, tiles_n)
    return (np.concatenate([tm, tm2]), np.concatenate([tn, tn2]), np.concatenate([np.full(main, -1), t % 4]))


def coverage(tiles_m, tiles_n, main):
    """how often every quarter of every tile is computed: [tiles_m][tiles_n][4]"""
    tm, tn, qd = walk(tiles_m, tiles_n, main)
    assert tm.min() >= 0 and tm.max() < tiles_m and tn.min() >= 0 and tn.max() < tiles_n
    cover = np.zeros((tiles_m, tiles_n, 4), dtype=np.int64)
    whole = qd < 0
    np.add.at(cover, (tm[whole], tn[whole]), 1)
    np.add.at(cover, (tm[~whole], tn[~whole], qd[~whole]), 1)
    return cover


def epilogue(row_w, col_w, h, w, M, N, ldc, c_off, accumulate, raw, ks=0, gm=None, gn=None):
    """what the wave tile of h x w at (row_w, col_w) does with its accumulators: 'skip' | 'vector' | 'scalar'.
    c_off: offset of every group's C from a 16-byte boundary in floats; raw: a K slice `ks` writing into part."""
    if row_w >= M or col_w >= N:
        return 'skip'
    full = row_w + h <= M and col_w + w <= N
    if raw:
        first, ld = (ks * M + row_w) * N + col_w, N
    else:
        gm, gn = gm or M, gn or N
        first, ld = c_off + (row_w % gm) * ldc + col_w % gn, ldc
    return 'vector' if full and not (accumulate and not raw) and first % 4 == 0 and ld % 4 == 0 else 'scalar'


def epilogues(kind, M, N, ldc, c_off=0, accumulate=False, splitk=1, cus=256, gm=None, gn=None):
    """the multiset {epilogue: number of wave tiles} of one launch (every K slice counted)"""
    tiles_m, tiles_n = cdiv(M, TILE), cdiv(N, TILE)
    main = main_tiles(tiles_m * tiles_n, cus, splitk)
    wgm, wgn = WAVES[kind]
    out = {'skip': 0, 'vector': 0, 'scalar': 0}
    for tm, tn, qd in zip(*walk(tiles_m, tiles_n, main)):
        bm = TILE if qd < 0 else TILE // 2
        r0 = tm * TILE + (0 if qd < 0 else (qd >> 1) * bm)
        c0 = tn * TILE + (0 if qd < 0 else (qd & 1) * bm)
        for ks in range(splitk):
            for wm in range(wgm):
                for wn in range(wgn):
                    h, w = bm // wgm, bm // wgn
                    out[epilogue(r0 + wm * h, c0 + wn * w, h, w, M, N, ldc, c_off, accumulate, splitk > 1, ks, gm, gn)] += 1
    return out


def split_lanes(K, ld, off):
    """how the lanes of rfn_x3_split (k_fast = 1) read their 8 reduction indices: {'vec', 'scalar'}"""
    return {'vec' if k0 + 8 <= K and ld % 4 == 0 and off % 4 == 0 else 'scalar' for k0 in range(0, k_pad(K), 8)}


def pad_launch(ngroups, rows):
    """does rfn_x3_split need its second launch, the one that zero-fills the row blocks behind the last group?"""
    total = ngroups * rows
    return rows_pad(total) // RB - cdiv(total, RB) > 0


def split_refusal(ngroups, rows, K, nulls=False):
    if nulls or rows < 1 or K < 1 or ngroups < 1 or ngroups > MAX_GROUPS:
        return ERR_ARG
    return ERR_SHAPE if ngroups > 1 and rows % 32 else OK


def split_ks_refusal(ngroups, ld, K, cols, off=0, nulls=False):
    if nulls or K < 1 or cols < 1 or ngroups < 1 or ngroups > MAX_GROUPS:
        return ERR_ARG
    if cols % 4 or ld % 4:
        return ERR_SHAPE
    return ERR_ARG if off % 4 else OK


def gemm_refusal(M, N, K, gm, gn, ldc, splitk, part=True, nulls=False):
    """return code of rfn_x3_gemm / rfn_x3_gemm_ks for a call with valid pointers (nulls: a NULL image or C table)"""
    if M < 1 or N < 1 or K < 1 or nulls or gm < 1 or gn < 1:
        return ERR_ARG
    splitk = max(1, splitk)
    ngm, ngn = cdiv(M, gm), cdiv(N, gn)
    if ngm * ngn > MAX_GROUPS:
        return ERR_SHAPE
    if (ngm > 1 and gm % TILE) or (ngn > 1 and gn % TILE):
        return ERR_SHAPE
    if splitk > k_pad(K) // KC:
        return ERR_SHAPE
    if splitk > 1 and (not part or N % 4 or gn % 4):
        return ERR_ARG
    if TILE * (N if splitk > 1 else ldc) * 4 >= 2 ** 32:
        return ERR_SHAPE
    return OK


def splitk_for(M, N, K, cus):
    tiles = cdiv(M, TILE) * cdiv(N, TILE)
    if tiles >= cus:
        return 1
    iters = k_pad(K) // KC
    sk = (cus + tiles // 2) // tiles
    while sk > 1 and iters // sk < 64:
        sk -= 1
    return max(1, sk)


# =================================================================================================================
# values
# =================================================================================================================
def operands(M, N, K, regime='normal', seed=0, prev=True):
    """A (M, K), B (N, K), bias (N,), C_prev (M, N) (None unless asked for) on the CPU, seeded by the shape: every storage
    of a shape gets the same values"""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + 7919 * seed)
    a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    if not prev:
        assert regime == 'normal'
        return a, b, torch.randn(N, generator=g), None
    if regime == 'positive':
        a, b = a.abs(), b.abs()
    elif regime == 'wide':                          # the `wide` case of tests/test_x3_gpu.py
        a = a * torch.exp(3 * torch.randn(M, K, generator=g))
        b = b * torch.exp(3 * torch.randn(N, K, generator=g))
    else:
        assert regime == 'normal'
    return a, b, torch.randn(N, generator=g), torch.randn(M, N, generator=g)


def _bf16_rne(v):
    """bits of the bf16 nearest to the f32 values v (ties to even), as int64"""
    u = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def _bf16_as_f32(p):
    w = p << 16
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).view(torch.float32)


def planes(x):
    """the exact three-way bf16 split of finite f32 values (x3_split of csrc/rfn_common.h): three f32 tensors with 8
    significant bits each, x0 + x1 + x2 == x"""
    x = x.float().contiguous()
    u = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    p0 = _bf16_rne(x)
    p0 = torch.where((p0 & 0x7F80) == 0x7F80, u >> 16, p0)      # rounding up would overflow: truncate
    x0 = _bf16_as_f32(p0)
    r = x - x0
    x1 = _bf16_as_f32(_bf16_rne(r))
    r = r - x1
    return x0, x1, _bf16_as_f32(_bf16_rne(r))


PRODUCTS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))         # (plane of A, plane of B), in the kernel's order


def six_products(a, b, drop=None, drop_piece=None):
    """sum of the six plane products in fp64; drop: one of PRODUCTS left out; drop_piece: one 32-wide piece of K left out"""
    pa, pb = [p.double() for p in planes(a)], [p.double() for p in planes(b)]
    if drop_piece is not None:
        keep = torch.ones(a.shape[1], dtype=torch.bool)
        keep[drop_piece * KC:(drop_piece + 1) * KC] = False
        pa, pb = [p[:, keep] for p in pa], [p[:, keep] for p in pb]
    out = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float64)
    for i, j in PRODUCTS:
        if (i, j) != drop:
            out += pa[i] @ pb[j].t()
    return out


def seq_fp32(a, b):
    """the yardstick's product: one fp32 accumulator per element, k in order"""
    A, B = a.numpy(), b.numpy()
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for k in range(A.shape[1]):
        acc += A[:, k:k + 1] * B[:, k]
    return torch.from_numpy(acc)


def rel_err(got, ref, mag):
    """max error in units of sum |a||b| (+ |bias| + |C_prev|)"""
    return float(((got.double() - ref).abs() / (mag + 1e-30)).max())


def hard_cap_ok(got, ref, mag, K, splitk=1):
    return bool(((got.double() - ref).abs() <= (k_pad(K) + splitk + 5) * U * mag).all())


# =================================================================================================================
# the tables
# =================================================================================================================
SMALL = [(1, 4, 1), (16, 16, 32), (17, 20, 33)]
K_EDGES = [(70, 72, K) for K in (31, 32, 33, 64, 65)]
TILE_EDGES = [(M, N, 40) for M in (255, 256, 257) for N in (252, 256, 260)]
WAVE_EDGES = [(M, N, 40) for M in (65, 129) for N in (68, 132)]
WALK = [(2200, 1100, 33), (4200, 700, 33)]
BASE_SHAPES = SMALL + K_EDGES + TILE_EDGES + WAVE_EDGES
EPILOGUE_SHAPES = [(256, 256, 40), (255, 252, 40), (257, 260, 40), (129, 132, 40)]

# (name, M, N, K, gm, gn, bias)
GROUP_CASES = [
    ('row groups 188 short', 700, 260, 40, 256, None, False),
    ('column groups 88 short bias', 260, 600, 40, None, 256, True),
    ('both', 700, 600, 40, 256, 256, True),
    ('64 groups', 16 * 256, 4 * 256, 8, 256, 256, True),
]

SPLIT_SHAPE = (512, 260, 330)                       # nkc = 11
SPLITKS = (2, 3, 4, 7, 11)                          # 7: per = 2, a one-piece slice and an empty one; 11 = nkc
# (name, gm, bias, accumulate, layout of C)
SPLIT_OPTS = [('plain', None, False, False, 'packed'), ('gm', 256, False, False, 'packed'), ('bias', None, True, False, 'packed'),
              ('accumulate', None, False, True, 'packed'), ('ldc', None, False, False, 'padded4'),
              ('all', 256, True, True, 'padded4')]
SPLIT_GN = (512, 512, 70, 256, 3)                   # (M, N, K, gn, splitk): a split over column groups, with bias

# (regime, M, N, K, splitk): all-positive and wide-range operands, held to 4 x their yardstick.  The all-positive yardstick
# grows with K (a sequential fp32 sum of like-signed terms) while the trace of a dropped low plane product falls as
# 1 / sqrt(K): from K ~ 65 on 4 x the yardstick would no longer tell the two apart (32 against 34 units of 2^-24 at K = 65,
# measured on the CPU), so the positive cases stay at K <= 40 (tests/test_x3_cases_cpu.py holds the margin).
VALUE_CASES = [('positive', 130, 132, 20, 1), ('positive', 130, 132, 40, 2), ('wide', 130, 132, 65, 1), ('wide', 70, 72, 330, 3)]


def tail_shape(cus):
    """three tile columns and just over two rounds of the chip: M ends 100 rows short of a tile, N 4 columns short"""
    tiles_m = cdiv(2 * cus + 1, 3)
    return tiles_m * TILE - 100, 3 * TILE - 4, 40


def value_key(regime, M, N, K):
    return '%s %dx%dx%d' % (regime, M, N, K)


def measure_yardstick(regime, M, N, K):
    a, b, _, _ = operands(M, N, K, regime)
    ref, mag = a.double() @ b.double().t(), a.double().abs() @ b.double().abs().t()
    return rel_err(seq_fp32(a, b), ref, mag)


def bar(regime, M, N, K, bias=False):
    """the bar a base product of this case is held to, in units of sum |a||b|"""
    if regime == 'normal':
        return BAR_BIAS if bias else BAR_PLAIN
    return max(YARD_FACTOR * YARD[value_key(regime, M, N, K)], YARD_FLOOR)


# ---- measured yardsticks, in units of sum |a||b|; re-measure with `python tests/x3_cases.py` ---------------------------
YARD = {
    'positive 130x132x20': 2.91e-07,
    'positive 130x132x40': 3.96e-07,
    'wide 130x132x65': 6.26e-07,
    'wide 70x72x330': 1.04e-06,
}


def yard_table():
    return {value_key(r, M, N, K): float('%.3g' % measure_yardstick(r, M, N, K)) for r, M, N, K, _ in VALUE_CASES}


if __name__ == '__main__':
    for k, v in yard_table().items():
        print('    %r: %.3g,' % (k, v))
