"""CPU: the caption-set diversity metrics (include/rfn.h "caption-set diversity").  The restatement (tests/diversity_cpu.py) against
the goldens (tools/make_diversity_golden.py: mBLEU from the reference's own Bleu scorer, U from the consensus goldens), the
properties the definitions promise, the option plumbing, and the new entry points' host-side checks -- no kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import ciderd_cpu as CPU
import diversity_cpu as DC
from conftest import GOLDEN_DIR
from test_consensus_cpu import golden as consensus_golden, random_case, table_df

BLEU_TOL = dict(rtol=1e-12, atol=0)          # tests/test_evalcap_cpu.py's bars
CIDER_TOL = dict(rtol=1e-12, atol=1e-13)


def golden(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, 'diversity_%s.npz' % name)))


def df_of(g):
    return CPU.df_from_arrays(g['df_ids'], g['df_counts']), float(g['ref_docs'])


# the GPU tests' added inputs (tests/test_diversity_gpu.py imports them): name -> (cands, n_cand, vocab)
def extra_cases():
    out = {}
    c, nc, _ = random_case(5, 2, 32, 64, ragged=False)
    c[0, 0] = np.arange(1, 65) % 59 + 1                       # a caption without a 0: all 4 T n-gram slots
    out['lds_limit'] = (c, nc, 60)
    out['n2'] = random_case(6, 5, 2, 12, ragged=False)[:2] + (60,)
    out['n1'] = random_case(7, 4, 1, 9)[:2] + (60,)
    c, nc, _ = random_case(8, 6, 3, 1, ragged=False)
    c[c == 0] = 3                                             # T = 1: one word each (a 0 would be an empty caption)
    out['T1'] = (c, nc, 60)
    c, nc, _ = random_case(9, 9, 6, 10)
    nc[:4] = [1, 6, 2, 1]
    out['ragged'] = (c, nc, 60)
    c, nc, _ = random_case(10, 5, 4, 8, ragged=False)
    c[2, 1, 0] = 61                                           # an id above vocab among good images
    out['bad_id'] = (c, nc, 60)
    for c, _, _ in out.values():                              # no empty caption under either convention but by intent
        c[:, :, 0] = np.where(c[:, :, 0] == 0, 5, c[:, :, 0])
    return out


@pytest.mark.parametrize('name', ('table', 'edge'))
def test_restatement_matches_the_goldens(name):
    g, cg = golden(name), consensus_golden(name)
    df, docs = df_of(g)
    assert np.array_equal(g['cands'], cg['cands']) and np.array_equal(g['n_cand'], cg['n_cand'])
    for end_token, sfx in ((True, ''), (False, '_words')):
        d = DC.diversity(g['cands'], g['n_cand'], df, docs, end_token=end_token)
        if end_token:
            np.testing.assert_allclose(d['U'], cg['U'], equal_nan=True, **CIDER_TOL)          # what the reference's CiderD pins
        np.testing.assert_allclose(d['mbleu'], g['mbleu' + sfx], equal_nan=True, **BLEU_TOL)   # the reference's Bleu, per row ...
        np.testing.assert_allclose(d['mbleu_corpus'], g['mbleu_corpus' + sfx], equal_nan=True, **BLEU_TOL)   # ... and per slot
        assert np.array_equal(d['mbleu_comps'], g['mbleu_comps' + sfx])
        assert np.array_equal(d['distinct'], g['distinct' + sfx]) and np.array_equal(d['words'], g['words' + sfx])
        assert np.array_equal(d['div'], g['div' + sfx], equal_nan=True)
        np.testing.assert_allclose(d['eig'], g['eig' + sfx], equal_nan=True, **CIDER_TOL)
        np.testing.assert_allclose(d['self_cider'], g['self_cider' + sfx], equal_nan=True, **CIDER_TOL)
        nc = g['n_cand']
        for k in range(len(nc)):
            assert np.isnan(d['mbleu'][k, nc[k]:]).all() and np.isnan(d['eig'][k, nc[k]:]).all()


def test_edge_tier_holds_the_cases_it_names():
    g = golden('edge')
    assert g['n_cand'].tolist() == [1, 2, 3, 7]
    # n_cand = 1: Div is defined, mBLEU and Self-CIDEr are NaN
    assert g['words'][0] == 4 and g['distinct'][0].tolist() == [4, 3, 2, 1] and not np.isnan(g['div'][0]).any()
    assert np.isnan(g['mbleu'][0]).all() and np.isnan(g['self_cider'][0]) and g['mbleu_comps'][0].sum() == 0
    # two identical captions: Self-CIDEr exactly 0, mBLEU-4 exactly what a perfect match gives
    assert g['self_cider'][1] == 0.0 and g['distinct'][1].tolist() == [4, 3, 2, 1] and g['words'][1] == 8
    assert g['mbleu_comps'][1, 0].tolist() == [4, 4, 4, 3, 2, 1, 4, 3, 2, 1]
    # the END-only candidate is an empty caption when the END is excluded: the image is bad there only
    assert not np.isnan(g['self_cider'][2]) and np.isnan(g['self_cider_words'][2]) and np.isnan(g['div_words'][2]).all()
    assert g['distinct_words'][2].sum() == 0 and g['words_words'][2] == 0 and np.isnan(g['mbleu_words'][2]).all()
    # slots 3..6 exist in one image only, slot 0 in three (image 0 has nothing to compare with)
    assert not np.isnan(g['mbleu_corpus']).any()


@pytest.mark.parametrize('name', ('table', 'edge', 'corpus'))
def test_symmetrisation_is_needed_and_threshold_is_unambiguous(name):
    g = consensus_golden(name)
    df, docs = (CPU.df_from_arrays(g['df_ids'], g['df_counts']), float(g['ref_docs'])) if 'df_ids' in g else (None, None)
    d = DC.diversity(g['cands'], g['n_cand'], df, docs, end_token=True)
    for k, nc in enumerate(g['n_cand']):
        assert not DC.ambiguous_threshold(d['eig'][k], int(nc)), (name, k)
        K = d['K'][k]
        assert np.array_equal(K, K.T)
    if name == 'edge':
        u = g['U'][3]
        assert np.nanmax(np.abs(u - u.T)) > 0.5               # CIDEr-D clips: one triangle is not the matrix


def test_the_gpu_tests_added_inputs_are_clear_of_the_threshold():
    for name, (cands, n_cand, vocab) in extra_cases().items():
        for end_token in (True, False):
            for df in (None, table_df(cands, np.where((n_cand >= 1) & (n_cand <= cands.shape[1]), n_cand, 0))):
                d = DC.diversity(cands, n_cand, df, 5000, end_token=end_token, vocab=vocab)
                for k, nc in enumerate(n_cand):
                    if not np.isnan(d['eig'][k, 0]):
                        assert not DC.ambiguous_threshold(d['eig'][k], int(nc)), (name, end_token, k)
    ex = extra_cases()
    d = DC.diversity(*ex['bad_id'][:2], None, None, vocab=60)
    assert np.isnan(d['div'][2]).all() and d['distinct'][2].sum() == 0 and not np.isnan(np.delete(d['self_cider'], 2)).any()
    assert np.isnan(DC.diversity(*ex['n1'][:2], None, None, vocab=60)['self_cider']).all()


def test_identical_captions_have_no_diversity():
    w, n = 6, 5
    cap = [7, 3, 9, 3, 11, 12, 0, 0]
    cands = np.array([[cap] * n])
    for end_token in (True, False):
        d = DC.diversity(cands, None, {}, 5000, end_token=end_token)
        assert d['self_cider'][0] == 0.0                                       # exactly: one eigenvalue survives the cut
        words = n * (w + (1 if end_token else 0))
        uni = 5 + (1 if end_token else 0)
        assert d['distinct'][0, 0] == uni and d['words'][0] == words and d['div'][0, 0] == uni / (words + 1e-6)
        np.testing.assert_allclose(d['mbleu'][0, :, 3], 1.0, rtol=1e-9)


def test_disjoint_equal_length_captions_are_maximally_diverse():
    n, w = 4, 5
    cands = np.zeros((1, n, 8), dtype=np.int64)
    for j in range(n):
        cands[0, j, :w] = np.arange(1, w + 1) + 10 * j
    d = DC.diversity(cands, None, {}, 5000, end_token=False)
    assert abs(d['self_cider'][0] - 1.0) <= 1e-12
    assert d['distinct'][0].tolist() == [n * w, n * (w - 1), n * (w - 2), n * (w - 3)] and d['mbleu_comps'][0, :, 6:].sum() == 0


@pytest.mark.parametrize('mode', ('table', 'corpus'))
def test_permuting_the_candidates_changes_nothing(mode):
    cands, n_cand, _ = random_case(21, 6, 5, 12, ragged=False)
    df = table_df(cands, n_cand) if mode == 'table' else None
    a = DC.diversity(cands, n_cand, df, 5000)
    perm = np.array([3, 0, 4, 2, 1])
    b = DC.diversity(cands[:, perm], n_cand, df, 5000)
    assert np.array_equal(a['distinct'], b['distinct']) and np.array_equal(a['words'], b['words'])
    assert np.array_equal(a['div'], b['div'])
    np.testing.assert_allclose(b['self_cider'], a['self_cider'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(b['eig'], a['eig'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(b['mbleu'], a['mbleu'][:, perm], rtol=0, atol=1e-12)
    np.testing.assert_allclose(b['mbleu_corpus'], a['mbleu_corpus'][perm], rtol=0, atol=1e-12)
    ra, rb = DC.report(a), DC.report(b)
    assert all(abs(ra[k] - rb[k]) <= 1e-12 for k in ra)
    # upstream's one-triangle reading is NOT invariant: the reason K is symmetrised
    tri = lambda U: np.linalg.eigvalsh(np.tril(U) + np.tril(U, -1).T)   # noqa: E731
    assert max(np.abs(tri(a['U'][k]) - tri(b['U'][k])).max() for k in range(6)) > 1e-6


def test_one_candidate():
    cands, _, _ = random_case(3, 4, 3, 8, ragged=False)
    cands[:, :, 0] = 5
    d = DC.diversity(cands, np.array([1, 3, 1, 2]), None, None)
    for k in (0, 2):
        assert not np.isnan(d['div'][k]).any() and d['words'][k] > 0
        assert np.isnan(d['mbleu'][k]).all() and np.isnan(d['self_cider'][k]) and not np.isnan(d['eig'][k, 0])
    assert not np.isnan(d['mbleu'][1]).any() and not np.isnan(d['mbleu_corpus'][:2]).any()
    assert np.isnan(d['mbleu'][3, 2]).all() and not np.isnan(d['mbleu_corpus'][2]).any()   # slot 2: image 1 only


def test_group_stats_restatement():
    s = np.array([1.0, 3.0, 3.0, 2.0, np.nan, 1.0, 5.0, 4.0, np.nan])
    best, arg, mean = DC.group_stats(s, 3)
    assert arg.tolist() == [1, -1, -1] and best[0] == 3.0 and mean[0] == (1.0 + 3.0 + 3.0) / 3 and np.isnan(best[1:]).all()
    best, arg, mean = DC.group_stats(s, 3, [3, 1, 2])
    assert arg.tolist() == [1, 0, 0] and best.tolist() == [3.0, 2.0, 5.0] and mean.tolist() == [7.0 / 3, 2.0, 4.5]


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
def test_keep_candidates_key_is_off_by_default():
    from recurrent_fusion_network_amd.decode import keep_candidates_n
    assert keep_candidates_n({}, 5) is None and keep_candidates_n({'keep_candidates': False}, 5) is None
    assert keep_candidates_n({'keep_candidates': True}, 5) == 5
    assert keep_candidates_n({'keep_candidates': True, 'consensus_n': 3}, 5) == 3


def test_python_layer_refusals():
    import torch
    from recurrent_fusion_network_amd import _native as N, eval_shim, evalcap, rewards as RW
    with pytest.raises(NotImplementedError):
        RW.diversity(RW.BleuD(), None)
    with pytest.raises(N.RfnError):                                            # no CPU fallback
        RW.diversity(RW.CiderD(), torch.zeros(2, 3, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        RW.group_stats(torch.zeros(6, dtype=torch.float64), 3)                 # a CPU tensor
    with pytest.raises(NotImplementedError):
        evalcap.DiversityEval(100, metrics=('SPICE',))
    with pytest.raises(ValueError):
        evalcap.DiversityEval(100, metrics=('Div', 'nope'))
    with pytest.raises(NotImplementedError):
        evalcap.DiversityEval(100, scorer=RW.BleuD())
    ev = evalcap.DiversityEval(100)
    assert len(ev) == 0 and ev.skipped is None
    with pytest.raises(N.RfnError):
        ev.add(torch.zeros(2, 3, 4, dtype=torch.int64), [np.zeros((1, 4))] * 2)
    with pytest.raises(ValueError):
        ev.compute()
    for opt, kw in (({}, {}), ({'sample_n': 3}, {}), ({'sample_n': 1}, dict(sample_max=0))):     # one candidate per image
        with pytest.raises(ValueError):
            eval_shim.eval_split(torch.nn.Linear(1, 1), None, [], 5, 100, decode_opt=opt, diversity=ev, **kw)


# ---- the C entry points: declared, exported, bound, and checked without a launch ---------------------------------------------
NEW = ('rfn_capset_ws_bytes', 'rfn_capset_diversity', 'rfn_score_group_stats')


def test_new_symbols_are_declared_exported_and_bound():
    from test_native_abi import header_symbols
    import recurrent_fusion_network_amd._native as N
    for s in NEW:
        assert s in header_symbols() and s in N.EXPORTS and getattr(N.lib, s).argtypes is not None
    assert N.lib.rfn_abi_version() == 9 and N.ABI_VERSION == 9      # additive: the ABI version stays


def call(N, n_img=4, n=5, T=16, n_cand=None, table=None, slots=0, docs=0.0, vocab=9487, flags=0, outs=(256,) * 9, ws=256,
         ws_bytes=None, cands=256):
    if ws_bytes is None:
        ws_bytes = N.lib.rfn_capset_ws_bytes(n_img, n, T, int(table is None))
    return N.lib.rfn_capset_diversity(cands, n_img, n, T, n_cand, table, slots, C.c_double(docs), vocab, C.c_double(6.0), flags,
                                      *outs, ws, ws_bytes, None)


def test_ws_bytes_and_argument_checks():
    import recurrent_fusion_network_amd._native as N
    f = N.lib.rfn_capset_ws_bytes
    base = f(4, 5, 16, 0)
    assert base > N.lib.rfn_consensus_ws_bytes(4, 5, 16, 0) and f(4, 5, 16, 1) > base and f(8, 5, 16, 0) > base
    assert f(0, 5, 16, 0) == 0 and f(4, 0, 16, 0) == 0 and f(4, 33, 16, 0) == 0 and f(4, 5, 0, 0) == 0 and f(4, 5, 65, 0) == 0
    assert f(2, 32, 64, 1) > 0
    SHAPE, WS, ARG = -1, -4, -5
    big = 1 << 30
    assert call(N, n=33, ws_bytes=big) == SHAPE and call(N, T=65, ws_bytes=big) == SHAPE and call(N, n_img=0, ws_bytes=big) == SHAPE
    assert call(N, vocab=32768) == SHAPE and call(N, vocab=-1) == SHAPE
    assert call(N, table=256, slots=1000, docs=5000.0) == SHAPE and call(N, table=256, slots=1024, docs=0.0) == SHAPE
    assert call(N, flags=2) == ARG and call(N, cands=None) == ARG and call(N, ws=None) == ARG and call(N, ws=264) == ARG
    assert call(N, ws_bytes=f(4, 5, 16, 1) - 1) == WS
    assert call(N, table=256, slots=1024, docs=5000.0, ws_bytes=base - 1) == WS
    # precedence: shape, then arg, then workspace
    assert call(N, n=33, flags=2, ws_bytes=0) == SHAPE and call(N, flags=2, ws_bytes=0) == ARG and call(N, cands=None, ws_bytes=0) == ARG
    assert call(N, outs=(None,) * 9) == 0                             # every output NULL: nothing to launch
    g = N.lib.rfn_score_group_stats
    assert g(256, 1, 0, 3, None, 256, 256, 256, None) == SHAPE and g(256, 1, 4, 0, None, 256, 256, 256, None) == SHAPE
    assert g(256, 0, 4, 3, None, 256, 256, 256, None) == SHAPE
    assert g(None, 1, 4, 3, None, 256, 256, 256, None) == ARG and g(256, 1, 4, 3, None, None, None, None, None) == ARG
