"""numpy restatement of the dropout masks include/rfn.h documents (rfn_dropout_mask): Philox4x32-10 as Salmon et al.
define it ("Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library), keyed by the 64-bit seed,
counting (element index, call-site offset).  Written from that description and the standard, not from the device code,
so that a wrong counter word, a swapped key half or a lost high half of the offset in the library shows as a mismatch.

    counter words = (idx lo, idx hi, offset lo, offset hi)      key words = (seed lo, seed hi)
    one round     : (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2  ->  (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
    between rounds: k0 += W0, k1 += W1 (mod 2^32);  ten rounds
    u = float32(word 0 >> 8) * 2^-24 in [0, 1);  unit kept iff u >= float32(p)
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # key bumps (golden ratio, sqrt(3) - 1)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: (..., 4) and key: (..., 2) arrays of 32-bit words (broadcast against each other) -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK32
    k = np.asarray(key, dtype=np.uint64) & _MASK32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = np.uint64(M0) * c0              # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & _MASK32
        k1 = (k1 + np.uint64(W1)) & _MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def uniforms(seed, offset, n):
    """u[idx], idx = 0 .. n-1, of call site `offset` under key `seed` (both 64-bit): float32, shape (n,), in [0, 1)."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    idx = np.arange(int(n), dtype=np.uint64)
    ctr = np.stack([idx & _MASK32, idx >> np.uint64(32), np.full_like(idx, offset & 0xFFFFFFFF),
                    np.full_like(idx, offset >> 32)], -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    w0 = philox4x32_10(ctr, key)[..., 0]
    return (w0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(seed, offset, n, p):
    """The keep mask rfn_dropout_mask publishes: float32 (n,), 1.0 = kept, 0.0 = dropped; p = 0 keeps everything."""
    p = np.float32(p)
    if not (0.0 <= p < 1.0):
        raise ValueError('p must be in [0, 1)')
    if p == 0.0:
        return np.ones(int(n), dtype=np.float32)
    return (uniforms(seed, offset, n) >= p).astype(np.float32)
