"""CPU: the CIDEr-D restatement (tests/ciderd_cpu.py) reproduces the reference's scores on every golden tier, and the
host side of the rfn_ciderd_* / rfn_scst_reward ABI validates its arguments -- no kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import ciderd_cpu as CPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIERS = ('edge', 'c5', 'spi5', 'table')


def golden(name):
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'ciderd_%s.npz' % name))


@pytest.mark.parametrize('name', TIERS)
def test_restatement_matches_reference_goldens(name):
    g = golden(name)
    B, spi = int(g['B']), int(g['seq_per_img'])
    df, docs = None, None
    if name == 'table':
        df, docs = CPU.df_from_arrays(g['df_ids'], g['df_counts']), float(g['ref_docs'])
    s = CPU.score_rows(g['res'], CPU.scst_rows(B, spi), g['gts'], g['n_refs'], df, docs)
    np.testing.assert_allclose(s, g['scores'], rtol=1e-12, atol=1e-14)
    T = g['res'].shape[1]
    np.testing.assert_array_equal(CPU.reward(g['scores'], B, T), g['reward64'])
    np.testing.assert_array_equal(CPU.reward(g['scores'], B, T, 0.5, False), g['reward64_nobase'])
    assert g['reward32'].dtype == np.float32 and np.array_equal(g['reward32'], g['reward64'].astype(np.float32))


def test_edge_tier_holds_the_traps():
    g = golden('edge')
    res, n_refs = g['res'], g['n_refs']
    assert (res[:, 0] == 0).any()                                   # a hypothesis that is only the end token
    assert ((res != 0).all(axis=1)).any()                           # a full-length row without 0
    assert n_refs.min() == 1 and n_refs.max() == 7                  # variable ref counts
    assert np.isfinite(g['scores']).all() and (g['scores'] == 0).any() and (g['scores'] > 5).any()


def test_golden_tiers_are_small_and_shaped_like_compute_reward():
    for name in TIERS:
        path = os.path.join(ROOT, 'tests', 'golden', 'ciderd_%s.npz' % name)
        assert os.path.getsize(path) < 1 << 20
        g = golden(name)
        B = int(g['B'])
        assert g['res'].shape[0] == 2 * B and g['scores'].shape == (2 * B,)
        assert g['reward32'].shape == (B, g['res'].shape[1])
    c5, spi5 = golden('c5'), golden('spi5')
    assert c5['res'].shape == (256, 16) and c5['gts'].shape == (128, 5, 16)
    assert spi5['res'].shape == (1280, 16) and int(spi5['seq_per_img']) == 5
    assert spi5['n_refs'].min() == 5 and spi5['n_refs'].max() == 7


def test_restatement_semantics_by_hand():
    assert CPU.caption([3, 4, 0, 5]) == [3, 4, 0] and CPU.caption([3, 4]) == [3, 4] and CPU.caption([0, 0]) == [0]
    # a hypothesis equal to its only reference, with every n-gram's idf above zero, scores 10
    s = CPU.score_rows(np.array([[3, 4, 0], [5, 6, 0]]), [0, 1], np.array([[[3, 4, 0]], [[7, 8, 0]]]), [1, 1])
    assert s[0] > 0 and s[1] == 0.0
    # the unigram 0 of every document has idf exactly 0: its norm is 0 and the division is skipped
    s = CPU.score_rows(np.array([[0, 0]]), [0], np.array([[[0, 0]]]), [1])
    assert s[0] == 0.0


# ---- host logic of the ABI: shape / argument / workspace errors before any launch ---------------------------------------
def native():
    import recurrent_fusion_network_amd._native as N
    return N


def score_call(N, n_rows=4, T=16, n_img=2, R=5, Tg=16, vocab=9487, table=None, slots=0, docs=0.0, ws=256, ws_bytes=None,
               res=256, scores=256):
    if ws_bytes is None:
        ws_bytes = N.lib.rfn_ciderd_ws_bytes(n_rows, T, n_img, R, Tg, int(table is None))
    return N.lib.rfn_ciderd_score(res, n_rows, T, 256, 256, 256, n_img, R, Tg, table, slots, C.c_double(docs), vocab,
                                  C.c_double(6.0), scores, ws, ws_bytes, None)


def test_ciderd_ws_bytes_grows_with_its_sizes():
    N = native()
    f = N.lib.rfn_ciderd_ws_bytes
    base = f(256, 16, 128, 5, 16, 1)
    assert base > 0
    assert f(256, 16, 256, 5, 16, 1) > base and f(256, 16, 128, 7, 16, 1) > base and f(256, 16, 128, 5, 32, 1) > base
    assert 0 < f(256, 16, 128, 5, 16, 0) < base          # table mode keeps no df table in the workspace
    for bad in ((256, 65, 128, 5, 16), (256, 16, 128, 33, 16), (256, 16, 128, 5, 65), (0, 16, 128, 5, 16),
                (256, 16, 0, 5, 16), (256, 0, 128, 5, 16)):
        assert f(*bad, 1) == 0
    assert N.lib.rfn_ciderd_table_bytes(1024) == 16 * 1024 and N.lib.rfn_ciderd_table_bytes(1000) == 0


def test_ciderd_score_rejects_bad_calls_without_launching():
    N = native()
    SHAPE, WS, ARG = -1, -4, -5
    assert score_call(N, T=65, ws_bytes=1 << 30) == SHAPE
    assert score_call(N, Tg=65, ws_bytes=1 << 30) == SHAPE
    assert score_call(N, R=33, ws_bytes=1 << 30) == SHAPE
    assert score_call(N, vocab=32768) == SHAPE and score_call(N, vocab=-1) == SHAPE
    assert score_call(N, table=256, slots=1000, docs=113287.0) == SHAPE          # slots not a power of two
    assert score_call(N, table=256, slots=1024, docs=0.0) == SHAPE               # a table needs its document count
    assert score_call(N, ws=None) == ARG and score_call(N, res=None) == ARG and score_call(N, scores=None) == ARG
    assert score_call(N, ws=8) == ARG                                             # misaligned workspace
    need = N.lib.rfn_ciderd_ws_bytes(4, 16, 2, 5, 16, 1)
    assert score_call(N, ws_bytes=need - 1) == WS
    assert N.lib.rfn_ciderd_table_build(256, 256, 600, 100, 256, 1024, None) == SHAPE   # more than slots / 2 entries
    assert N.lib.rfn_ciderd_table_build(256, 256, 10, 32768, 256, 1024, None) == SHAPE
    assert N.lib.rfn_ciderd_table_build(256, 256, 10, 100, None, 1024, None) == ARG
    assert N.lib.rfn_scst_reward(256, 0, 16, C.c_double(1.0), 1, 256, None, None) == SHAPE
    assert N.lib.rfn_scst_reward(None, 4, 16, C.c_double(1.0), 1, 256, None, None) == ARG
    assert N.lib.rfn_scst_reward(256, 4, 16, C.c_double(1.0), 1, None, None, None) == ARG


def test_python_layer_checks_without_a_gpu():
    from recurrent_fusion_network_amd import rewards as RW
    with pytest.raises(ValueError):
        RW._words('3 4 x')
    with pytest.raises(ValueError):
        RW._words('3 04 0')
    with pytest.raises(ValueError):
        RW._row([3, 0, 4, 0], 4)
    assert RW._row([3, 4, 0], 5) == [3, 4, 0, 0, 0] and RW._row([3, 4], 2) == [3, 4]
    with pytest.raises(NotImplementedError):
        RW.CiderD(n=3)
    t = RW.CiderD(df={('3',): 2.0, ('3', '4'): 1.0, ('a',): 5.0}, df_mode='coco-val')
    assert t.ref_docs == 5000 and t._table_src[0].shape == (2, 4)
    with pytest.raises(ValueError):
        RW.CiderD(df={('3',): 2.0})

    class Opt:
        bleu4_weight, spice_weight, cider_weight, use_baseline = 0.5, 0, 1, 1
    with pytest.raises(NotImplementedError, match='BLEU-D and SPICE-D'):
        RW.get_self_critical_reward_feat_array(None, None, [], [], {'gts': []}, None, Opt())
