"""tests/philox_cpu.py, the numpy restatement of the documented dropout stream (include/rfn.h: rfn_dropout_mask), checked
on its own: the GPU tests compare the library's masks with it bit for bit, so it has to be right by itself."""
import numpy as np
import pytest

import philox_cpu as P


def _philox_ints(ctr, key):
    """The same ten rounds on Python integers, one block at a time: a second, independent evaluation."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


# Random123's known-answer vectors for philox4x32-10 (kat_vectors: zero, all-ones and the digits-of-pi block).  The
# integer evaluation above reproduces all three, word for word, so they were confirmed here and not only remembered.
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_known_answer_vectors(ctr, key, want):
    assert _philox_ints(ctr, key) == want
    got = P.philox4x32_10(ctr, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert got.tolist() == want


def test_vectorised_blocks_equal_the_integer_evaluation():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(50, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(2,), dtype=np.uint64)
    got = P.philox4x32_10(ctr, key)
    assert got.shape == (50, 4)
    for i in range(50):
        assert got[i].tolist() == _philox_ints([int(x) for x in ctr[i]], [int(x) for x in key])


def test_uniforms_contract():
    seed, offset = 0x123456789ABCDEF0, 2 ** 33 + 7
    u = P.uniforms(seed, offset, 1000)
    assert u.dtype == np.float32 and u.shape == (1000,)
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert np.array_equal(u, P.uniforms(seed, offset, 1000))                  # a function of its arguments
    assert np.array_equal(u[:10], P.uniforms(seed, offset, 10))               # element idx does not depend on n
    # the counter is (idx lo, idx hi, offset lo, offset hi), the key (seed lo, seed hi): element 5 by hand
    w = _philox_ints([5, 0, offset & 0xFFFFFFFF, offset >> 32], [seed & 0xFFFFFFFF, seed >> 32])
    assert u[5] == np.float32(w[0] >> 8) * np.float32(2.0 ** -24)
    # every half of seed and offset matters
    for s2, o2 in ((seed ^ 1, offset), (seed ^ (1 << 32), offset), (seed, offset ^ 1), (seed, offset ^ (1 << 32))):
        assert not np.array_equal(u, P.uniforms(s2, o2, 1000))
    # the two halves of the seed are not interchangeable
    assert not np.array_equal(u, P.uniforms(((seed & 0xFFFFFFFF) << 32) | (seed >> 32), offset, 1000))


def test_keep_mask_contract():
    m = P.keep_mask(11, 3, 4096, 0.3)
    assert m.dtype == np.float32 and m.shape == (4096,)
    assert set(np.unique(m).tolist()) <= {0.0, 1.0}
    assert np.array_equal(m, (P.uniforms(11, 3, 4096) >= np.float32(0.3)).astype(np.float32))
    assert abs(float(m.mean()) - 0.7) < 0.03                                   # 4 sigma of 4096 draws is 0.029
    assert np.array_equal(P.keep_mask(11, 3, 100, 0.0), np.ones(100, dtype=np.float32))
    # a higher p drops a superset
    assert bool(np.all(P.keep_mask(11, 3, 4096, 0.5) <= m))
    with pytest.raises(ValueError):
        P.keep_mask(11, 3, 4, 1.0)
