"""CPU: the restatement of truncated sampling (tests/decode_truncation_cpu.py) against a brute-force loop, the share of `near`
rows in every case the GPU test uses, the option parsing, and the new C symbols' argument checks (no kernel is launched)."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import decode_truncation_cpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')


def brute(x, top_k, top_p, inv_temp):
    """The definition, entry by entry, in Python floats: selection sort by (x descending, id ascending), then the two cuts."""
    V1 = len(x)
    if any(math.isnan(v) for v in x) or all(v == -INF for v in x):
        return None
    left, order = list(range(V1)), []
    while left:
        best = left[0]
        for v in left[1:]:
            if x[v] > x[best] or (x[v] == x[best] and v < best):
                best = v
        order.append(best)
        left.remove(best)
    order = [v for v in order if x[v] > -INF]
    if 0 < top_k < V1:
        order = order[:top_k]
    if top_p < 1.0:
        w = [math.exp((x[v] - x[order[0]]) * inv_temp) for v in order]
        total, c, J = math.fsum(w), 0.0, len(order)
        for j, wj in enumerate(w):
            c = math.fsum(w[:j + 1])
            if c >= top_p * total:
                J = j + 1
                break
        order = order[:J]
    return sorted(order)


def test_restatement_equals_the_brute_force_loop_on_short_rows():
    """Rows of at most 8 entries over a few values, so that ties are everywhere (all 3^4 rows of length 4 are enumerated), with
    -inf entries, a NaN and every knob setting.  top_p avoids the cumulative sums these few values can produce."""
    vals = (-0.5, -1.0, -INF)
    rows = [list(r) for r in itertools.product(vals, repeat=4)]
    rng = np.random.default_rng(0)
    for V1 in (1, 2, 3, 5, 8):
        for _ in range(40):
            rows.append(rng.choice([-0.25, -0.5, -1.0, -2.0, -INF, -0.0, 0.0], size=V1).tolist())
    rows.append([-1.0, float('nan'), -2.0])
    checked = 0
    for x in rows:
        for k, p, it in itertools.product((0, 1, 2, 3, len(x), len(x) + 1), (1e-6, 0.37, 0.713, 1.0), (1.0, 2.5)):
            want = brute(x, k, float(np.float32(p)), it)
            mask, J, near = T.keep_mask(np.array(x, dtype=np.float32), k, p, it)
            if want is None:
                assert mask is None and J == 0
                continue
            if near:
                continue
            checked += 1
            assert sorted(np.flatnonzero(mask).tolist()) == want and J == len(want), (x, k, p, it, want)
            assert J >= 1
    assert checked > 5000


def test_ties_at_the_cut_go_to_the_lower_ids():
    x = np.array([-2.0, -1.0, -2.0, -1.0, -2.0, -INF, -2.0], dtype=np.float32)
    assert np.flatnonzero(T.keep_mask(x, 3, 1.0, 1.0)[0]).tolist() == [0, 1, 3]
    assert np.flatnonzero(T.keep_mask(x, 4, 1.0, 1.0)[0]).tolist() == [0, 1, 2, 3]
    assert np.flatnonzero(T.keep_mask(x, 7, 1.0, 1.0)[0]).tolist() == [0, 1, 2, 3, 4, 6]      # top_k beyond the finite count
    # weights 1, 1, e^-1 x 4: total 3.4715; p = 0.7 -> target 2.43: both -1 entries and the two lowest -2 entries (2.7358)
    assert np.flatnonzero(T.keep_mask(x, 0, 0.7, 1.0)[0]).tolist() == [0, 1, 2, 3]
    # top-k first: of the survivors {1, 3, 0} (total 2.3679) p = 0.7 needs 1.6575 -> the first two
    assert np.flatnonzero(T.keep_mask(x, 3, 0.7, 1.0)[0]).tolist() == [1, 3]
    assert T.keep_mask(x, 0, 1e-6, 1.0)[1] == 1 and np.flatnonzero(T.keep_mask(x, 0, 1e-6, 1.0)[0]).tolist() == [1]


def test_near_rows_stay_under_the_cap_in_every_gpu_case():
    """The restatement alone: no generated case calls more than 1 row in 100 near, so the GPU comparison is exact nearly
    everywhere (with 1 or 3 rows: everywhere)."""
    worst = 0.0
    for V1 in T.V1S:
        for rows in T.ROWS:
            P = T.Prepared(T.case(V1, rows))
            for k, p, it in T.params(V1):
                near = P.keep(k, p, it)[2]
                worst = max(worst, near.sum() / rows)
                assert near.sum() <= T.NEAR_CAP * rows, (V1, rows, k, p, it, np.flatnonzero(near))
    x, p = T.flat_case()
    for it in T.INV_TEMPS:
        mask, J, near, _ = T.Prepared(x).keep(0, p, it)
        assert not near.any() and (J == 334).all() and (np.flatnonzero(mask[0]) == np.arange(334)).all()
    print('largest near share: %.4f' % worst)


def test_sampling_options_accept_and_refuse():
    from recurrent_fusion_network_amd.decode import _Sampling
    for off in ({}, {'top_k': 0}, {'top_p': 1.0}, {'sample_n': 1}, {'top_k': 0, 'top_p': 1.0, 'sample_n': 1},
                {'top_k': None, 'top_p': None, 'sample_n': None}):
        assert _Sampling.parse(off) is None, off
    s = _Sampling.parse({'top_k': 50})
    assert (s.k, s.p, s.n) == (50, 1.0, 1)
    s = _Sampling.parse({'top_p': 0.9, 'sample_n': 5})
    assert (s.k, s.p, s.n) == (0, 0.9, 5)
    s = _Sampling.parse({'top_k': 3, 'top_p': 1e-6, 'sample_n': 2, 'beam_size': 1, 'temperature': 0.5})
    assert (s.k, s.p, s.n) == (3, 1e-6, 2)
    st = s.struct()
    assert (st.top_k, st.rows_per_image) == (3, 2) and st.top_p == np.float32(1e-6)
    for bad in ({'top_k': -1}, {'top_p': 0.0}, {'top_p': -0.1}, {'top_p': 1.5}, {'top_p': float('nan')}, {'top_p': INF},
                {'sample_n': 0}, {'sample_n': -3}):
        with pytest.raises(ValueError):
            _Sampling.parse(bad)


def test_new_symbols_are_declared_exported_and_check_their_arguments():
    """Fails on a tree without the feature: the library has no rfn_logp_truncate_rows."""
    import recurrent_fusion_network_amd._native as N
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(rfn_[a-z0-9_]+)\s*\(', src))
    for s in ('rfn_logp_truncate_rows', 'rfn_decoder_loop_ex2'):
        assert s in declared and s in N.EXPORTS and hasattr(N.lib, s), s
    assert 'rfn_decode_sampling' in src and N.lib.rfn_abi_version() == 9                 # additive: the ABI version stays
    assert C.sizeof(N.DecodeSampling) == 16
    FAKE = 1 << 40                                         # never dereferenced: no call below reaches a launch
    tr = N.lib.rfn_logp_truncate_rows
    SHAPE, UNSUPPORTED, ARG = -1, -2, -5
    assert tr(FAKE, 50, 0, 50, 5, 0.9, 1.0, None, None) == SHAPE                         # rows
    assert tr(FAKE, 50, 4, 0, 5, 0.9, 1.0, None, None) == SHAPE                          # V1
    assert tr(FAKE, 49, 4, 50, 5, 0.9, 1.0, None, None) == SHAPE                         # row stride below V1
    for it in (0.0, -1.0, float('nan')):
        assert tr(FAKE, 50, 4, 50, 5, 0.9, it, None, None) == SHAPE
    for p in (0.0, -0.5, float('nan'), INF):
        assert tr(FAKE, 50, 4, 50, 5, p, 1.0, None, None) == SHAPE
    assert tr(None, 50, 4, 50, 5, 0.9, 1.0, None, None) == ARG
    for k, p in ((0, 1.0), (-3, 1.0), (50, 1.0), (51, 2.0), (0, 1.5)):                   # both knobs off: nothing to do
        assert tr(FAKE, 50, 4, 50, k, p, 1.0, None, None) == 0
    assert tr(FAKE, 70000, 4, 70000, 5, 0.9, 1.0, None, None) == UNSUPPORTED             # past the 64-bit mass sums
    assert tr(FAKE, 70000, 4, 70000, 0, 1.0, 1.0, None, None) == 0
