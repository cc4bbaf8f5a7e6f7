"""CPU: consensus reranking (include/rfn.h "consensus reranking").  The restatement (tests/consensus_cpu.py) against the goldens
the reference's own CiderD produced (tools/make_consensus_golden.py), the identity that ties the pairwise utility to the shipped
scorer's definition, the option parsing with its refusals, and the new entry points' host-side checks -- no kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import ciderd_cpu as CPU
import consensus_cpu as CC
from conftest import GOLDEN_DIR

TIERS = ('table', 'edge', 'corpus')
RTOL, ATOL = 1e-12, 1e-13        # the bar tools/make_ciderd_golden.py holds the CIDEr-D restatement to


def golden(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, 'consensus_%s.npz' % name)))


def df_of(g):
    """(df dict, ref_docs) of a golden tier: (None, None) for the corpus tier."""
    if 'df_ids' not in g:
        return None, None
    return CPU.df_from_arrays(g['df_ids'], g['df_counts']), float(g['ref_docs'])


def random_case(seed, n_img, n, T, vocab=60, ragged=True, zero_weights=True):
    """Candidates from a small vocabulary (so they overlap), ragged n_cand and weights with exact zeros."""
    rng = np.random.default_rng(seed)
    cands = rng.integers(1, vocab + 1, (n_img, n, T)).astype(np.int64)
    cands[..., : max(1, T // 2)] = rng.integers(1, 8, (n_img, n, max(1, T // 2)))        # shared words up front
    for k in range(n_img):
        for j in range(n):
            if rng.random() < 0.75:
                cands[k, j, int(rng.integers(0 if T == 1 else 1, T))] = 0               # most captions end early
    n_cand = rng.integers(1, n + 1, n_img).astype(np.int32) if ragged else np.full(n_img, n, dtype=np.int32)
    weights = rng.random((n_img, n))
    if zero_weights:
        weights[rng.random((n_img, n)) < 0.25] = 0.0
    return cands, n_cand, weights


def table_df(cands, n_cand):
    """A df counted from the candidates themselves (per candidate), for table mode on random cases."""
    df = {}
    for k in range(cands.shape[0]):
        for j in range(int(n_cand[k])):
            for g in CPU.ngram_counts(CPU.caption(cands[k, j])):
                df[g] = df.get(g, 0.0) + 1.0
    return df


@pytest.mark.parametrize('name', TIERS)
def test_restatement_matches_the_reference_goldens(name):
    g = golden(name)
    df, docs = df_of(g)
    best, c, U = CC.consensus(g['cands'], g['n_cand'], None, df, docs)
    if name == 'corpus':      # the reference pins the include-self row means (and with them the corpus df); the pairs are ours
        np.testing.assert_allclose(U.mean(2), g['row_means'], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(U, g['U'], rtol=RTOL, atol=ATOL, equal_nan=True)
    np.testing.assert_allclose(c, g['c'], rtol=RTOL, atol=ATOL, equal_nan=True)
    assert np.array_equal(best, g['best'])
    nc = g['n_cand']
    for k in range(len(nc)):
        assert np.isnan(U[k, nc[k]:]).all() and np.isnan(U[k, :, nc[k]:]).all() and np.isnan(c[k, nc[k]:]).all()
        assert not np.isnan(U[k, :nc[k], :nc[k]]).any()


def test_edge_tier_holds_the_cases_it_names():
    g = golden('edge')
    cands, nc, U, c, best = g['cands'], g['n_cand'], g['U'], g['c'], g['best']
    assert nc.tolist() == [1, 2, 3, 7] and cands.shape == (4, 7, 8)
    assert c[0, 0] == 0.0 and best[0] == 0                                    # one candidate: the empty sum
    assert CPU.caption(cands[1, 0]) == CPU.caption(cands[1, 1]) and not np.array_equal(cands[1, 0], cands[1, 1])
    assert U[1, 0, 1] == U[1, 0, 0] and c[1, 0] == c[1, 1] and best[1] == 0     # identical captions: an exact tie picks the first
    assert CPU.caption(cands[2, 0]) == [0] and 0 not in cands[2, 1]
    assert U[2, 0, 2] > 0 and U[2, 1, 2] == 0                                  # the pair that shares only END; no 0 at all
    assert not np.allclose(U[3, :7, :7], U[3, :7, :7].T)                       # U is not symmetric


@pytest.mark.parametrize('name', ('table', 'corpus'))
def test_committed_fixtures_have_no_near_tie(name):
    """tests/test_consensus_gpu.py demands the restatement's pick on every image of the n >= 3 fixtures; that is sound only while
    the runner-up lies far outside its 1e-9 rounding allowance (n = 2 and some n = 3 images tie mathematically: the generator's
    seeds were chosen so that the committed fixtures hold none)."""
    g = golden(name)
    assert g['cands'].shape[1] >= 3
    assert CC.min_relative_gap(g['c'], g['cands'], g['n_cand']).min() > 1e-3


@pytest.mark.parametrize('n', (2, 3, 5, 8))
@pytest.mark.parametrize('mode', ('table', 'corpus'))
def test_row_mean_of_U_is_the_shipped_scorer(mode, n):
    """mean over the valid j of U[k][i][j] == ciderd_cpu.score_rows with the compacted candidates as res and the candidates as
    gts: what defines the corpus df, and ties U to the already-pinned scorer in both modes."""
    cands, n_cand, _ = random_case(100 + n, 6, n, 12)
    df, docs = (table_df(cands, n_cand), 5000) if mode == 'table' else (None, None)
    U = CC.utilities(cands, n_cand, df, docs)
    res, row_img = CC.compact(cands, n_cand)
    want = CPU.score_rows(res, row_img, cands, n_cand, df, docs)
    got = np.array([U[k, i, :n_cand[k]].mean() for k in range(len(n_cand)) for i in range(int(n_cand[k]))])
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def test_bad_input_rules():
    cands, n_cand, w = random_case(7, 6, 4, 8, ragged=False, zero_weights=False)
    good = CC.consensus(cands, n_cand, w, table_df(cands, n_cand), 5000)
    bad_c, bad_n, bad_w = cands.copy(), n_cand.copy(), w.copy()
    bad_c[0, 1, 0] = 61                       # id above vocab = 60, inside the caption
    bad_n[1] = 0
    bad_n[2] = 5
    bad_w[3, 2] = -1.0
    bad_w[4, 0] = np.nan
    best, c, U = CC.consensus(bad_c, bad_n, bad_w, table_df(cands, n_cand), 5000, vocab=60)
    assert best[:5].tolist() == [-1] * 5 and np.isnan(c[:5]).all() and np.isnan(U[:5]).all()
    assert best[5] == good[0][5] and np.array_equal(c[5], good[1][5]) and np.array_equal(U[5], good[2][5])
    # an id after the END is not read; an empty candidate is bad only when the END is excluded
    cands[5, 0] = [3, 0, 99, 99, 99, 99, 99, 99]
    assert CC.consensus(cands, n_cand, w, {}, 5000, vocab=60)[0][5] >= 0
    cands[5, 1] = 0
    assert CC.consensus(cands, n_cand, w, {}, 5000)[0][5] >= 0
    assert CC.consensus(cands, n_cand, w, {}, 5000, end_token=False)[0][5] == -1
    # all weights but the candidate's own are zero: the empty weight sum scores 0
    w0 = np.zeros((6, 4))
    w0[:, 0] = 1.0
    assert (CC.consensus(cands, n_cand, w0, {}, 5000)[1][:, 0] == 0.0).all()


# ---- option parsing --------------------------------------------------------------------------------------------------------
def _keys():
    from recurrent_fusion_network_amd import rewards as RW
    from recurrent_fusion_network_amd.decode import _Consensus, _Sampling
    return RW, _Consensus, _Sampling


def test_keys_are_off_by_default():
    RW, K, S = _keys()
    assert K.parse({}, 9488, 16, 5) is None and K.parse({'consensus': None}, 9488, 16, 5) is None
    assert K.parse_sample({'sample_n': 3, 'sample_max': 0}, 9488, 16, S.parse({'sample_n': 3}), 0) is None
    c = K.parse({'consensus': RW.CiderD()}, 9488, 16, 5)
    assert (c.n, c.how) == (5, 'uniform')
    c = K.parse({'consensus': RW.CiderD(), 'consensus_n': 32, 'consensus_weights': 'prob'}, 32768, 64, 5)
    assert (c.n, c.how) == (32, 'prob')
    assert K.parse_sample({'consensus': RW.CiderD(), 'sample_n': 3}, 9488, 16, S.parse({'sample_n': 3}), 0).n == 3


def test_refusals():
    RW, K, S = _keys()
    sc, N = RW.CiderD(), __import__('recurrent_fusion_network_amd._native', fromlist=['x'])
    with pytest.raises(ValueError):                                   # consensus without sample_n > 1
        K.parse_sample({'consensus': sc}, 9488, 16, None, 0)
    with pytest.raises(ValueError):
        K.parse_sample({'consensus': sc, 'sample_n': 1, 'top_k': 5}, 9488, 16, S.parse({'top_k': 5}), 0)
    with pytest.raises(ValueError):                                   # consensus with sample_max = 1
        K.parse_sample({'consensus': sc, 'sample_n': 3}, 9488, 16, S.parse({'sample_n': 3}), 1)
    with pytest.raises(ValueError):                                   # sample_beam's keys on sample
        K.parse_sample({'consensus': sc, 'sample_n': 3, 'consensus_weights': 'prob'}, 9488, 16, S.parse({'sample_n': 3}), 0)
    for opt in ({'consensus': sc, 'consensus_n': 0}, {'consensus': sc, 'consensus_n': 33}, {'consensus': sc, 'consensus_weights': 'x'},
                {'consensus_n': 3}, {'consensus_weights': 'prob'}):
        with pytest.raises(ValueError):
            K.parse(opt, 9488, 16, 5)
    with pytest.raises(N.RfnError):                                   # V1 > 32768: refused up front
        K.parse({'consensus': sc}, 32769, 16, 5)
    with pytest.raises(N.RfnError):
        K.parse({'consensus': sc}, 9488, 65, 5)
    for other in (RW.BleuD(), RW.RougeL(), object()):
        with pytest.raises(NotImplementedError):
            K.parse({'consensus': other}, 9488, 16, 5)
        with pytest.raises(NotImplementedError):
            RW.consensus(other, None)


# ---- the C entry points: declared, exported, bound, and checked without a launch ---------------------------------------------
NEW = ('rfn_consensus_ws_bytes', 'rfn_consensus_ciderd', 'rfn_consensus_gather')


def test_new_symbols_are_declared_exported_and_bound():
    from test_native_abi import header_symbols
    import recurrent_fusion_network_amd._native as N
    for s in NEW:
        assert s in header_symbols() and s in N.EXPORTS and getattr(N.lib, s).argtypes is not None
    assert N.lib.rfn_abi_version() == 9 and N.ABI_VERSION == 9      # additive: the ABI version stays


def call(N, n_img=4, n=5, T=16, n_cand=None, weights=None, table=None, slots=0, docs=0.0, vocab=9487, flags=0, U=None, c=256,
         best=256, ws=256, ws_bytes=None, cands=256):
    if ws_bytes is None:
        ws_bytes = N.lib.rfn_consensus_ws_bytes(n_img, n, T, int(table is None))
    return N.lib.rfn_consensus_ciderd(cands, n_img, n, T, n_cand, weights, table, slots, C.c_double(docs), vocab, C.c_double(6.0),
                                      flags, U, c, best, ws, ws_bytes, None)


def test_ws_bytes_and_argument_checks():
    import recurrent_fusion_network_amd._native as N
    f = N.lib.rfn_consensus_ws_bytes
    base = f(4, 5, 16, 0)
    assert base > 0 and f(4, 5, 16, 1) > base and f(8, 5, 16, 0) > base and f(4, 6, 16, 0) > base and f(4, 5, 17, 0) > base
    assert f(4, 5, 16, 0) >= N.lib.rfn_ciderd_ws_bytes(20, 16, 4, 5, 16, 0)          # the cooked candidates, plus the counts
    assert f(0, 5, 16, 0) == 0 and f(4, 0, 16, 0) == 0 and f(4, 33, 16, 0) == 0 and f(4, 5, 0, 0) == 0 and f(4, 5, 65, 0) == 0
    assert f(1, 32, 64, 1) > 0
    SHAPE, WS, ARG = -1, -4, -5
    big = 1 << 30
    assert call(N, n=33, ws_bytes=big) == SHAPE and call(N, T=65, ws_bytes=big) == SHAPE and call(N, n_img=0, ws_bytes=big) == SHAPE
    assert call(N, vocab=32768) == SHAPE and call(N, vocab=-1) == SHAPE
    assert call(N, table=256, slots=1000, docs=5000.0) == SHAPE and call(N, table=256, slots=1024, docs=0.0) == SHAPE
    assert call(N, flags=2) == ARG and call(N, cands=None) == ARG and call(N, c=None) == ARG and call(N, best=None) == ARG
    assert call(N, ws=None) == ARG and call(N, ws=264) == ARG
    need = f(4, 5, 16, 1)
    assert call(N, ws_bytes=need - 1) == WS and call(N, table=256, slots=1024, docs=5000.0, ws_bytes=f(4, 5, 16, 0) - 1) == WS
    # precedence: shape, then arg, then workspace
    assert call(N, n=33, flags=2, ws_bytes=0) == SHAPE and call(N, flags=2, ws_bytes=0) == ARG and call(N, c=None, ws_bytes=0) == ARG
    g = N.lib.rfn_consensus_gather
    assert g(256, 0, 5, 16, 256, 256, None, None, None, None, None) == SHAPE
    assert g(256, 4, 0, 16, 256, 256, None, None, None, None, None) == SHAPE
    assert g(256, 4, 5, 0, 256, 256, None, None, None, None, None) == SHAPE
    assert g(None, 4, 5, 16, 256, 256, None, None, None, None, None) == ARG
    assert g(256, 4, 5, 16, None, None, None, None, None, None, None) == ARG          # nothing to gather
    assert g(256, 4, 5, 16, 256, None, None, None, None, None, None) == ARG           # a pair with one side
    assert g(256, 4, 5, 16, None, None, 256, None, None, None, None) == ARG
    assert g(256, 4, 5, 16, None, None, None, None, None, 256, None) == ARG
