"""Shared by tests/test_input_grads_cpu.py and tests/test_dseq_steps_gpu.py: the fp64 restatement of
rfn_attn_context_bwd_dseq_steps' contract (rfn.h), its derived error bar, and the case table of the kernel sweep with the
launcher constants it is built around (csrc/rfn_attn.hip, DSS_*)."""
import numpy as np

DT = 1024            # DSS_DT: columns of a full D tile
LC_BIG, LC_SMALL, MIN_BLOCKS = 32, 8, 1024     # rows per block: 32 when B * tiles * ceil(L / 32) >= 1024 blocks, else 8
LDS_FLOATS = 16384   # T * min(Dp, 1024) + 32 * Tp floats of LDS at most (Xp: X rounded up to 4)


def rows_per_block(B, L, D):
    return LC_BIG if B * -(-D // DT) * -(-L // LC_BIG) >= MIN_BLOCKS else LC_SMALL


def max_steps(D):
    tw = min((D + 3) // 4 * 4, DT)
    return max(T for T in range(1, LDS_FLOATS // tw + 1) if T * tw + LC_BIG * ((T + 3) // 4 * 4) <= LDS_FLOATS)


def dseq_steps_ref(alpha, dz, prev, accumulate, lens=None):
    """fp64: alpha (T, B, L), dz (T, B, D), prev (B, L, D) -> (out, mag) with out[b, l, :] = (prev if accumulate else 0) +
    sum_t alpha[t, b, l] * dz[t, b, :] for l < n_b = clamp(lens[b], 1, L); rows l >= n_b are 0 (overwrite) or prev
    (accumulate) whatever alpha holds there.  mag = |start| + sum_t |alpha * dz| on the live rows (0 on the others): what the
    error bar scales with."""
    T, B, L = alpha.shape
    a = np.array(alpha, dtype=np.float64)
    n = np.full(B, L) if lens is None else np.clip(np.asarray(lens), 1, L)
    live = np.arange(L)[None, :] < n[:, None]                     # (B, L)
    a = np.where(live[None], a, 0.0)                              # padded alpha (NaN in the tests) is never used
    g = np.asarray(dz, dtype=np.float64)
    start = np.array(prev, dtype=np.float64) if accumulate else np.zeros(prev.shape)
    with np.errstate(invalid='ignore'):      # a padded row may start from NaN (accumulate): it is passed through, not used
        out = np.where(live[:, :, None], start + np.einsum('tbl,tbd->bld', a, g), start)
        mag = np.where(live[:, :, None], np.abs(start), 0.0) + np.einsum('tbl,tbd->bld', np.abs(a), np.abs(g))
    return out, mag


def bar(T, mag):
    """Per element: T products and T additions in f32, each within 2^-24 relative of a partial sum that |start| + sum |a dz|
    bounds, plus the rounding of the f32 inputs' exact products into the chain -- 2 * (T + 1) * 2^-24 * mag."""
    return 2.0 * (T + 1) * 2.0 ** -24 * mag


# (T, B, L, D)
CASES = [
    (1, 1, 1, 1),
    (3, 2, 5, 7),              # scalar: D % 4 != 0
    (8, 3, 49, 64),
    (8, 2, 196, 2048),         # the benchmark map at B = 2: two full D tiles, 8-row chunks
    (9, 2, 6, 12),             # 3 threads per row: 256 is not a multiple, one thread of the block idles
    # the D tile +- 4 (16-byte form) and +- 1 (scalar form)
    (2, 1, 3, DT - 4), (2, 1, 3, DT), (2, 1, 3, DT + 4), (2, 1, 3, DT - 1), (2, 1, 3, DT + 1),
    # the 8-row chunk +- 1, one row per thread pass (D = 1024) and many (D = 8)
    (2, 1, LC_SMALL - 1, DT), (2, 1, LC_SMALL, DT), (2, 1, LC_SMALL + 1, DT), (2, 2, LC_SMALL + 1, 8),
    # the 32-row chunk +- 1 (1024 blocks and more), and the last grid that still takes 8-row chunks
    (2, MIN_BLOCKS, LC_BIG - 1, 4), (2, MIN_BLOCKS, LC_BIG, 4), (2, MIN_BLOCKS, LC_BIG + 1, 4), (2, MIN_BLOCKS - 1, LC_SMALL + 1, 4),
    # a thread's row groups: 4 rows in flight, 5 = one full group and a tail (D = 1024: one row per pass)
    (3, 1, 5, DT),
    # the LDS limit: the last sizes that fit (the first refused ones are checked apart)
    (max_steps(DT), 1, 2, DT), (max_steps(4), 1, 1, 4), (max_steps(3), 1, 2, 3), (max_steps(64), 2, 3, 64),
]
REFUSED = [(max_steps(DT) + 1, 1, 2, DT), (max_steps(DT - 3) + 1, 1, 2, DT - 3), (max_steps(4) + 1, 1, 1, 4),
           (max_steps(1) + 1, 1, 1, 1), (max_steps(64) + 1, 2, 3, 64)]
