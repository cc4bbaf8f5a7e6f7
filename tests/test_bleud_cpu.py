"""CPU: the BLEU-D restatement (tests/bleud_cpu.py) reproduces the reference's scores on every golden tier
(tests/golden/bleud_*.npz, tools/make_bleud_golden.py), the goldens cover what they are meant to cover, and the host side of
the rfn_bleud_* / rfn_scst_reward_mix ABI validates its arguments -- no kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import bleud_cpu as BCPU
import ciderd_cpu as CPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIERS = ('edge', 'c5', 'spi5', 'near', 'near_spi5')
NEAR = ('near', 'near_spi5')


def golden(name):
    """The tier's BLEU-D golden joined with its inputs (stored in it, or in the CIDEr-D golden of the same name) -> dict with
    res, gts, n_refs, B, seq_per_img, vocab, cider, bleu, comps, corpus, mix_weights, mix_<k>_64, mix_<k>_32."""
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'bleud_%s.npz' % name)))
    if 'res' not in g:
        c = np.load(os.path.join(ROOT, 'tests', 'golden', 'ciderd_%s.npz' % name))
        g.update({k: c[k] for k in ('res', 'gts', 'n_refs', 'B', 'seq_per_img', 'vocab')}, cider=c['scores'])
    return g


@pytest.mark.parametrize('name', TIERS)
def test_restatement_matches_reference_goldens(name):
    g = golden(name)
    B, spi, T = int(g['B']), int(g['seq_per_img']), g['res'].shape[1]
    bleu, comps, corpus = BCPU.score_rows(g['res'], CPU.scst_rows(B, spi), g['gts'], g['n_refs'])
    np.testing.assert_allclose(bleu, g['bleu'], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(comps, g['comps'])
    np.testing.assert_allclose(corpus, g['corpus'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(BCPU.corpus_of(g['comps']), g['corpus'], rtol=1e-12, atol=0)
    assert g['bleu'].shape == (2 * B, 4) and g['comps'].shape == (2 * B, 10) and g['comps'].dtype == np.int32
    assert (g['bleu'] > 0).all()             # strictly positive: what lets the GPU test drop the absolute tolerance
    assert [tuple(w) for w in g['mix_weights']] == [(1.0, 0.0, 1.0), (0.5, 1.0, 1.0), (0.3, 0.7, 0.0)]
    for k, (w_b, w_c, base) in enumerate(g['mix_weights']):
        m = BCPU.mix(g['bleu'], g['cider'], B, T, w_b, w_c, bool(base))
        np.testing.assert_array_equal(m, g['mix_%d_64' % k])
        assert g['mix_%d_32' % k].dtype == np.float32 and np.array_equal(g['mix_%d_32' % k], m.astype(np.float32))
        assert m.shape == (B, T)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'bleud_%s.npz' % name)) < 1 << 20


def test_near_tiers_store_the_reference_ciderd_of_their_own_inputs():
    for name in NEAR:
        g = golden(name)
        B, spi = int(g['B']), int(g['seq_per_img'])
        s = CPU.score_rows(g['res'], CPU.scst_rows(B, spi), g['gts'], g['n_refs'])
        np.testing.assert_allclose(s, g['cider'], rtol=1e-12, atol=1e-14)
    assert golden('near')['res'].shape == (256, 16) and int(golden('near')['seq_per_img']) == 1
    assert golden('near_spi5')['res'].shape == (640, 16) and int(golden('near_spi5')['seq_per_img']) == 5
    for name in NEAR:
        n = golden(name)['n_refs']
        assert n.min() == 3 and n.max() == 7


def row_facts(g):
    """Per row: clipping active (0 < max over refs < count in the row for some n-gram), closest-length tie (two different
    reference lengths at the smallest distance)."""
    B, spi = int(g['B']), int(g['seq_per_img'])
    clip, tie = [], []
    for r in range(2 * B):
        i = (r % B) // spi
        refs = [CPU.caption(g['gts'][i, j]) for j in range(int(g['n_refs'][i]))]
        hyp = CPU.caption(g['res'][r])
        most = {}
        for ref in refs:
            for gram, c in CPU.ngram_counts(ref).items():
                most[gram] = max(most.get(gram, 0), c)
        clip.append(any(0 < most.get(gram, 0) < c for gram, c in CPU.ngram_counts(hyp).items()))
        d = sorted({(abs(len(ref) - len(hyp)), len(ref)) for ref in refs})
        tie.append(len(d) > 1 and d[0][0] == d[1][0])
    return np.array(clip), np.array(tie)


@pytest.mark.parametrize('name', NEAR)
def test_near_tiers_reach_the_long_ngrams_and_every_branch(name):
    g = golden(name)
    comps = g['comps']
    clip, tie = row_facts(g)
    assert (comps[:, 9] > 0).mean() >= 0.50                  # correct[3] > 0: a matching 4-gram
    assert clip.mean() >= 0.25
    assert (comps[:, 0] < comps[:, 1]).mean() >= 0.10        # testlen < reflen: the brevity penalty
    assert tie.mean() >= 0.03
    assert (g['res'] != 0).all(axis=1).mean() >= 0.10        # rows without an end token


def test_edge_tier_holds_the_traps():
    g = golden('edge')
    res, comps, bleu = g['res'], g['comps'], g['bleu']
    only_end = res[:, 0] == 0
    assert only_end.any() and (comps[only_end, 0] == 1).all()                        # a row that is only the end token
    equal = [r for r in range(len(res)) if any(CPU.caption(res[r]) == CPU.caption(ref)
                                               for ref in g['gts'][(r % 6)][:int(g['n_refs'][r % 6])])]
    full = [r for r in equal if comps[r, 0] >= 4]                                    # ... long enough to hold a 4-gram
    assert full and all((bleu[r] >= 1 - 1e-8).all() for r in full)                   # a row equal to a reference scores 1
    assert all(bleu[r, 0] >= 1 - 1e-8 for r in equal)
    assert (comps[:, 5] == 0).any()                                                  # guess[3] == 0
    assert int(g['B']) == 6 and int(g['seq_per_img']) == 1


def one(hyp, refs):
    T = max(len(hyp), max(len(r) for r in refs))

    def pad(w):
        return list(w) + [0] * (T - len(w))
    bleu, comps, _ = BCPU.score_rows(np.array([pad(hyp)]), [0], np.array([[pad(r) for r in refs]]), [len(refs)])
    return bleu[0], comps[0]


def test_restatement_semantics_by_hand():
    # closest length: testlen 4 between references of 3 and 5 words -> the shorter one
    _, c = one([7, 8, 9, 0], [[1, 2, 0], [1, 2, 3, 4, 0]])
    assert c[0] == 4 and c[1] == 3
    _, c = one([7, 8, 9, 0], [[1, 2, 3, 4, 0], [1, 2, 0]])          # whatever the order of the references
    assert c[1] == 3
    _, c = one([7, 8, 9, 0], [[1, 2, 3, 4, 0], [1, 2, 0], [5, 5, 5, 0]])
    assert c[1] == 4                                                  # an exact length beats both
    # clipping takes the maximum over the references, not the sum: 5 twice in each of two references, four times in the row
    _, c = one([5, 5, 5, 5, 0], [[5, 5, 1, 0], [5, 2, 5, 0]])
    assert list(c[6:]) == [3, 2, 0, 0]           # unigrams: min(4, 2) + the end token (a sum over references would give 5);
    #                                              bigrams: (5, 5) min(3, 1) + (5, 0) once
    # ids behind the first 0 are not read
    b1, c1 = one([3, 4, 0, 9, 9, 9], [[3, 4, 0, 0, 0, 0]])
    b2, c2 = one([3, 4, 0, 0, 0, 0], [[3, 4, 0, 7, 7, 7]])
    assert np.array_equal(b1, b2) and np.array_equal(c1, c2) and c1[0] == 3 and list(c1[2:6]) == [3, 2, 1, 0]
    # the scores themselves, by the formula: correct = guess = (3, 2, 1), guess[3] = 0; equal lengths still give a ratio
    # just below 1 (3 / (3 + 1e-9)), so the reference applies a penalty of 1 - 3.3e-10
    p1, p2, p3 = 3 / (3 + 1e-9), 2 / (2 + 1e-9), 1 / (1 + 1e-9)
    bp = np.exp(1 - 1 / (3 / (3 + 1e-9)))
    want = [p1 * bp, (p1 * p2) ** 0.5 * bp, (p1 * p2 * p3) ** (1 / 3) * bp, (p1 * p2 * p3 * (1e-15 / 1e-9)) ** 0.25 * bp]
    np.testing.assert_allclose(b1, want, rtol=1e-12)
    # brevity penalty: one matching word out of a 5-word reference
    b, c = one([0], [[1, 2, 3, 4, 0]])
    assert c[0] == 1 and c[1] == 5 and abs(b[0] - (1 / (1 + 1e-9)) * np.exp(1 - 1 / ((1 + 1e-15) / (5 + 1e-9)))) < 1e-15
    # the mix: a missing term is a zero, the baseline is subtracted per term
    bleu = np.array([[0, 0, 0, 0.5], [0, 0, 0, 0.25]])
    assert BCPU.mix(bleu, np.array([2.0, 1.0]), 1, 3, 0.5, 1.0, True).tolist() == [[1.125] * 3]
    assert BCPU.mix(bleu, None, 1, 2, 0.5, 1.0, False).tolist() == [[0.25] * 2]


# ---- host logic of the ABI: shape / argument / workspace errors before any launch ---------------------------------------
def native():
    import recurrent_fusion_network_amd._native as N
    return N


def score_call(N, n_rows=4, T=16, n_img=2, R=5, Tg=16, vocab=9487, ws=256, ws_bytes=None, res=256, scores=256, row_img=256,
               gts=256, n_refs=256, comps=None, corpus=None):
    if ws_bytes is None:
        ws_bytes = N.lib.rfn_bleud_ws_bytes(n_rows, T, n_img, R, Tg)
    return N.lib.rfn_bleud_score(res, n_rows, T, row_img, gts, n_refs, n_img, R, Tg, vocab, scores, comps, corpus, ws, ws_bytes,
                                 None)


def test_bleud_ws_bytes_grows_with_its_sizes():
    N = native()
    f = N.lib.rfn_bleud_ws_bytes
    base = f(256, 16, 128, 5, 16)
    assert base > 0
    # rows (their components), images, references per image and reference width each add to it; the row width T_res is
    # held in LDS only, so it takes part in the limits alone
    assert f(512, 16, 128, 5, 16) > base and f(256, 16, 256, 5, 16) > base and f(256, 16, 128, 7, 16) > base
    assert f(256, 16, 128, 5, 32) > base and f(256, 64, 128, 5, 16) >= base
    assert f(1, 1, 1, 1, 1) > 0 and f(4096, 64, 2048, 32, 64) > 0
    for bad in ((256, 65, 128, 5, 16), (256, 16, 128, 33, 16), (256, 16, 128, 5, 65), (0, 16, 128, 5, 16), (256, 16, 0, 5, 16),
                (256, 0, 128, 5, 16), (256, 16, 128, 0, 16), (256, 16, 128, 5, 0), (-1, 16, 128, 5, 16)):
        assert f(*bad) == 0, bad


def test_bleud_score_rejects_bad_calls_without_launching():
    N = native()
    SHAPE, WS, ARG = -1, -4, -5
    assert score_call(N, T=65, ws_bytes=1 << 30) == SHAPE
    assert score_call(N, Tg=65, ws_bytes=1 << 30) == SHAPE
    assert score_call(N, R=33, ws_bytes=1 << 30) == SHAPE
    assert score_call(N, n_rows=0, ws_bytes=1 << 30) == SHAPE and score_call(N, n_img=0, ws_bytes=1 << 30) == SHAPE
    assert score_call(N, vocab=32768) == SHAPE and score_call(N, vocab=-1) == SHAPE
    for name in ('ws', 'res', 'scores', 'row_img', 'gts', 'n_refs'):
        assert score_call(N, **{name: None}) == ARG, name
    assert score_call(N, ws=8) == ARG                                             # misaligned workspace
    need = N.lib.rfn_bleud_ws_bytes(4, 16, 2, 5, 16)
    assert score_call(N, ws_bytes=need - 1) == WS and score_call(N, ws_bytes=0) == WS
    assert score_call(N, ws_bytes=need - 1, comps=256, corpus=256) == WS


def test_scst_reward_mix_rejects_bad_calls_without_launching():
    N = native()
    SHAPE, ARG = -1, -5
    f = N.lib.rfn_scst_reward_mix
    w = C.c_double(1.0)
    assert f(256, w, 256, w, 0, 16, 1, 256, None, None) == SHAPE
    assert f(256, w, 256, w, 4, 0, 1, 256, None, None) == SHAPE
    assert f(None, w, None, w, 4, 16, 1, 256, None, None) == ARG                   # neither term
    assert f(256, w, 256, w, 4, 16, 1, None, None, None) == ARG                    # no output
    assert N.lib.rfn_abi_version() == 9                                            # additive: the ABI version stays
    for name in ('rfn_bleud_ws_bytes', 'rfn_bleud_score', 'rfn_scst_reward_mix'):
        assert name in N.EXPORTS


def test_python_layer_checks_without_a_gpu():
    import torch
    from recurrent_fusion_network_amd import rewards as RW
    with pytest.raises(NotImplementedError):
        RW.BleuD(n=3)
    b = RW.BleuD()
    assert b.method() == 'Bleu'
    with pytest.raises(RW.N.RfnError):                                             # no CPU fallback
        b.score_ids(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                    torch.zeros(1, 1, 4, dtype=torch.int64), torch.ones(1, dtype=torch.int32))
    with pytest.raises(ValueError):
        RW.scst_reward(None, torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64), None, None, 1)

    class Opt:
        bleu4_weight, spice_weight, cider_weight, use_baseline = 0.5, 0.1, 1, 1
    for kw in ({}, {'bleu_scorer': b}, {'bleu_scorer': b, 'scorer': RW.CiderD()}):
        with pytest.raises(NotImplementedError, match='SPICE-D'):                  # before model or data are touched
            RW.get_self_critical_reward_feat_array(None, None, [], [], {'gts': []}, None, Opt(), **kw)
        with pytest.raises(NotImplementedError, match='SPICE-D'):
            RW.get_self_critical_reward(None, None, None, None, {'gts': []}, None, Opt(), **kw)
    Opt.spice_weight = 0
    with pytest.raises(NotImplementedError, match='bleu_scorer='):                 # BLEU-D is ported, but needs its scorer
        RW.get_self_critical_reward(None, None, None, None, {'gts': []}, None, Opt())
