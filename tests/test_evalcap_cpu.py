"""CPU: the validation-metric restatement (tests/evalcap_cpu.py) reproduces the reference's Bleu(4), Rouge() and Cider() on every
golden tier (tests/golden/evalcap_*.npz, tools/make_evalcap_golden.py), the goldens hold what they are meant to hold, and the host
side of the rfn_rougel_* / rfn_*_score_ex / rfn_score_mean ABI validates its arguments -- no kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ciderd_cpu as CPU
import evalcap_cases as CASES
import evalcap_cpu as ECPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIERS = ('edge', 'edge1', 'near', 'near_spi', 'val')
REUSED = {'near': 'near', 'near_spi': 'near_spi5'}      # tiers whose inputs are those of tests/golden/bleud_<value>.npz
NEW_SYMBOLS = ('rfn_ciderd_score_ex', 'rfn_bleud_score_ex', 'rfn_rougel_ws_bytes', 'rfn_rougel_score', 'rfn_score_mean')


def golden(name):
    """The tier's golden joined with its inputs -> dict with res, row_img, gts, n_refs, vocab and the reference's results."""
    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'evalcap_%s.npz' % name)))
    if name in REUSED:
        b = np.load(os.path.join(ROOT, 'tests', 'golden', 'bleud_%s.npz' % REUSED[name]))
        g.update(res=b['res'], gts=b['gts'], n_refs=b['n_refs'], vocab=b['vocab'],
                 row_img=CPU.scst_rows(int(b['B']), int(b['seq_per_img'])))
    return g


@pytest.mark.parametrize('name', TIERS)
def test_restatement_matches_reference_goldens(name):
    g = golden(name)
    res, row_img, gts, n_refs = g['res'], g['row_img'], g['gts'], g['n_refs']
    bleu, comps, corpus = ECPU.bleu_rows(res, row_img, gts, n_refs)
    np.testing.assert_array_equal(comps, g['comps'])
    np.testing.assert_allclose(bleu, g['bleu'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(corpus, g['bleu_corpus'], rtol=1e-12, atol=0)
    for end, suffix in ((False, ''), (True, '_end')):
        rouge, lcs = ECPU.rouge_rows(res, row_img, gts, n_refs, end_token=end)
        np.testing.assert_array_equal(lcs, g['lcs' + suffix])
        np.testing.assert_allclose(rouge, g['rouge' + suffix], rtol=1e-14, atol=0)
        np.testing.assert_allclose(np.mean(rouge), g['rouge%s_mean' % suffix], rtol=1e-13, atol=0)
    cider = ECPU.cider_rows(res, row_img, gts, n_refs)
    np.testing.assert_allclose(cider, g['cider'], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(np.mean(cider), g['cider_mean'], rtol=1e-12, atol=1e-13)
    N = len(res)
    assert g['bleu'].shape == (N, 4) and g['comps'].shape == (N, 10) and g['comps'].dtype == np.int32
    assert g['lcs'].shape == (N, gts.shape[1]) and g['lcs'].dtype == np.int32 and g['rouge'].shape == (N,) == g['cider'].shape
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'evalcap_%s.npz' % name)) < 1 << 18


def test_language_eval_restatement_is_the_three_scorers_with_one_row_per_image():
    g = golden('val')
    assert np.array_equal(g['row_img'], np.arange(300)) and g['res'].shape == (300, 16)
    assert g['n_refs'].min() == 3 and g['n_refs'].max() == 7
    out, per = ECPU.language_eval(g['res'], g['gts'], g['n_refs'])
    assert sorted(out) == ['Bleu_1', 'Bleu_2', 'Bleu_3', 'Bleu_4', 'CIDEr', 'ROUGE_L']
    np.testing.assert_allclose([out['Bleu_%d' % k] for k in (1, 2, 3, 4)], g['bleu_corpus'], rtol=1e-12)
    np.testing.assert_allclose(out['ROUGE_L'], g['rouge_mean'], rtol=1e-13)
    np.testing.assert_allclose(out['CIDEr'], g['cider_mean'], rtol=1e-12)
    np.testing.assert_array_equal(per['lcs'], g['lcs'])


def test_the_tiers_reach_what_they_are_for():
    for name in ('near', 'near_spi', 'val'):
        g = golden(name)
        assert (g['comps'][:, 9] > 0).mean() >= 0.5, name            # correct[3] > 0: a matching 4-gram
        assert (g['comps'][:, 8] > 0).mean() >= 0.5, name            # ... and 3-gram
        assert (g['cider'] > 0).mean() >= 0.9 and 0.3 < g['rouge_mean'] < 0.95
        # the LCS is longer than the longest common substring on a good share of the pairs: the subsequence is exercised
        assert (g['lcs'].max(1) > g['comps'][:, 6:].astype(bool).sum(1)).mean() >= 0.2, name
    g = golden('edge')
    res, comps = g['res'], g['comps']
    assert res[0, 0] == 0 and comps[0, 0] == 0 and g['rouge'][0] == 0 and g['cider'][0] == 0 and (g['bleu'][0] == 0).all()
    assert (res[1] != 0).all() and comps[1, 0] == 8 and g['rouge'][1] == 1.0        # full width, no 0, equal to a reference
    assert (g['bleu'][1] >= 1 - 1e-8).all()
    assert len(set(res[2, :6])) == 1 and comps[2, 0] == 6                            # one word repeated
    assert comps[3, 0] == 1 and g['rouge'][3] == 1.0                                 # a single token
    assert g['rouge'][4] == 1.0 and (g['bleu'][4] >= 1 - 1e-8).all()                 # equal to a reference
    assert g['rouge'][6] == 0 and (g['lcs'][6] == 0).all()                           # nothing in common
    assert len(set(g['n_refs'].tolist())) >= 5                                       # unequal reference counts
    # the end token is a word of the other convention: it alone is a common subsequence of length 1
    assert (g['lcs_end'][6, :2] == 1).all() and g['rouge_end'][0] > 0
    g1 = golden('edge1')
    assert g1['res'].shape[0] == 1 and g1['cider'][0] == 0 and g1['rouge'][0] > 0


def test_restatement_semantics_by_hand():
    assert ECPU.caption([3, 4, 0, 9]) == [3, 4] and ECPU.caption([3, 4, 0, 9], True) == [3, 4, 0] and ECPU.caption([0, 1]) == []
    assert ECPU.caption([3, 4, 5]) == [3, 4, 5] == ECPU.caption([3, 4, 5], True)
    assert ECPU.lcs_length([1, 2, 3, 4, 5], [2, 9, 4, 5, 1]) == 3 and ECPU.lcs_length([], [1]) == 0
    assert ECPU.lcs_length([7, 8, 9, 7, 8, 9], [9, 8, 7, 9, 8, 7]) == 3       # e.g. 8 9 8
    s, lcs = ECPU.rouge_l([1, 2, 3, 4], [[1, 3, 9], [2, 3, 4, 5, 6, 7]])
    p, q = 3 / 4.0, max(2 / 3.0, 3 / 6.0)
    assert lcs == [2, 3] and s == (1 + 1.2 ** 2) * p * q / (q + 1.2 ** 2 * p)      # the maxima come from different references
    assert ECPU.rouge_l([], [[1]])[0] == 0.0 and ECPU.rouge_l([2], [[1]])[0] == 0.0
    # an empty validation caption: BLEU 0 through the brevity penalty, guess all 0
    bleu, comps, _ = ECPU.bleu_rows(np.array([[0, 5, 5]]), [0], np.array([[[5, 5, 0]]]), [1])
    assert list(comps[0]) == [0, 2, 0, 0, 0, 0, 0, 0, 0, 0] and (bleu[0] == 0).all()
    # CIDEr: an image scored against itself among others gets 10 (every n), the one-image corpus 0
    seq = np.array([[1, 2, 3, 4, 0], [5, 6, 7, 8, 0]])
    gts = seq[:, None, :].copy()
    np.testing.assert_allclose(ECPU.cider_rows(seq, [0, 1], gts, [1, 1]), [10.0, 10.0], rtol=1e-12)
    assert ECPU.cider_rows(seq[:1], [0], gts[:1], [1])[0] == 0


def test_cases_are_deterministic_and_in_range():
    a, b = CASES.val_split(3, 20), CASES.val_split(3, 20)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    seq, gts, n_refs, vocab = CASES.val_split(4, 50, 3, 7)
    assert seq.min() >= 0 and seq.max() <= vocab and gts.max() <= vocab and (gts[:, 0, 0] > 0).all() and (n_refs >= 3).all()
    for seed in range(24):
        f = CASES.fuzz_case(seed)
        for i in range(f.n_img):
            assert (f.gts[i, :f.n_refs[i], 0] != 0).all()


# ---- host logic of the ABI: shape / argument / workspace errors before any launch ---------------------------------------
def native():
    import recurrent_fusion_network_amd._native as N
    return N


def test_new_symbols_are_exported_and_header_and_library_agree():
    N = native()
    for name in NEW_SYMBOLS:
        assert hasattr(N.lib, name) and name in N.EXPORTS, name
    assert N.lib.rfn_abi_version() == 9 and N.CAPTION_END_EXCLUDED == 1               # additive: the ABI version stays
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    assert re.search(r'#define RFN_CAPTION_END_EXCLUDED 1u', src)
    declared = set(re.findall(r'\b(rfn_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    assert set(NEW_SYMBOLS) <= declared
    # every rfn_* function the library's dynamic symbol table defines is declared in the header, and the other way round
    data = open(N.LIB_PATH, 'rb').read()
    exported = dynamic_functions(data)
    assert set(NEW_SYMBOLS) <= exported
    assert exported - declared == set(), sorted(exported - declared)
    assert declared - exported == set(), sorted(declared - exported)


def dynamic_functions(data):
    """Names of the defined rfn_* functions in an ELF64 little-endian file's .dynsym."""
    import struct
    shoff, = struct.unpack_from('<Q', data, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', data, 0x3A)
    sections = [struct.unpack_from('<IIQQQQIIQQ', data, shoff + k * shentsize) for k in range(shnum)]
    out = set()
    for sec in sections:
        if sec[1] != 11:                                  # SHT_DYNSYM
            continue
        str_off = sections[sec[6]][4]
        for k in range(sec[5] // sec[9]):
            name, info, _, shndx, _, _ = struct.unpack_from('<IBBHQQ', data, sec[4] + k * sec[9])
            if shndx != 0 and (info & 15) == 2:           # defined, STT_FUNC
                end = data.index(b'\0', str_off + name)
                s = data[str_off + name:end].decode()
                if s.startswith('rfn_'):
                    out.add(s)
    return out


def test_rougel_ws_bytes_inside_and_outside_the_limits():
    f = native().lib.rfn_rougel_ws_bytes
    base = f(256, 16, 128, 5, 16)
    assert base > 0 and f(512, 16, 128, 5, 16) >= base and f(256, 16, 128, 7, 16) >= base   # one launch: nothing is kept in it
    assert f(1, 1, 1, 1, 1) > 0 and f(40000, 64, 40000, 32, 64) > 0
    for bad in ((256, 65, 128, 5, 16), (256, 16, 128, 33, 16), (256, 16, 128, 5, 65), (0, 16, 128, 5, 16), (256, 16, 0, 5, 16),
                (256, 0, 128, 5, 16), (256, 16, 128, 0, 16), (256, 16, 128, 5, 0), (-1, 16, 128, 5, 16)):
        assert f(*bad) == 0, bad


def rouge_call(N, n_rows=4, T=16, n_img=2, R=5, Tg=16, vocab=9487, flags=1, beta=1.2, ws=256, ws_bytes=None, res=256, scores=256,
               row_img=256, gts=256, n_refs=256, lcs=None):
    if ws_bytes is None:
        ws_bytes = N.lib.rfn_rougel_ws_bytes(n_rows, T, n_img, R, Tg)
    return N.lib.rfn_rougel_score(res, n_rows, T, row_img, gts, n_refs, n_img, R, Tg, vocab, flags, C.c_double(beta), scores, lcs,
                                  ws, ws_bytes, None)


def test_new_score_calls_reject_bad_calls_without_launching():
    N = native()
    SHAPE, WS, ARG = -1, -4, -5
    big = 1 << 30
    assert rouge_call(N, T=65, ws_bytes=big) == SHAPE and rouge_call(N, Tg=65, ws_bytes=big) == SHAPE
    assert rouge_call(N, R=33, ws_bytes=big) == SHAPE and rouge_call(N, n_rows=0, ws_bytes=big) == SHAPE
    assert rouge_call(N, n_img=0, ws_bytes=big) == SHAPE
    assert rouge_call(N, vocab=32768) == SHAPE and rouge_call(N, vocab=-1) == SHAPE
    assert rouge_call(N, beta=0.0) == SHAPE and rouge_call(N, beta=-1.2) == SHAPE
    for flags in (2, 3, 1 << 31):
        assert rouge_call(N, flags=flags) == ARG, flags
    for name in ('ws', 'res', 'scores', 'row_img', 'gts', 'n_refs'):
        assert rouge_call(N, **{name: None}) == ARG, name
    assert rouge_call(N, ws=8) == ARG                                                 # misaligned workspace
    need = N.lib.rfn_rougel_ws_bytes(4, 16, 2, 5, 16)
    assert rouge_call(N, ws_bytes=need - 1) == WS and rouge_call(N, ws_bytes=0, lcs=256) == WS
    # the _ex forms: the checks of the calls they extend, and the flag bits
    one = C.c_double(1.0)
    cw = N.lib.rfn_ciderd_ws_bytes(4, 16, 2, 5, 16, 1)
    bw = N.lib.rfn_bleud_ws_bytes(4, 16, 2, 5, 16)

    def cider(flags=1, T=16, res=256, ws_bytes=cw):
        return N.lib.rfn_ciderd_score_ex(res, 4, T, 256, 256, 256, 2, 5, 16, None, 0, one, 9487, C.c_double(6.0), flags, 256, 256,
                                         ws_bytes, None)

    def bleu(flags=1, T=16, res=256, ws_bytes=bw):
        return N.lib.rfn_bleud_score_ex(res, 4, T, 256, 256, 256, 2, 5, 16, 9487, flags, 256, None, None, 256, ws_bytes, None)
    for f in (cider, bleu):
        assert f(T=65) == SHAPE and f(flags=2) == ARG and f(flags=5) == ARG and f(res=None) == ARG and f(ws_bytes=16) == WS
    mean = N.lib.rfn_score_mean
    assert mean(256, 0, 1, 256, None, None) == SHAPE and mean(256, 4, 0, 256, None, None) == SHAPE
    assert mean(None, 4, 1, 256, None, None) == ARG and mean(256, 4, 1, None, None, None) == ARG


def test_python_layer_checks_without_a_gpu():
    import torch
    from recurrent_fusion_network_amd import eval_shim, evalcap
    from recurrent_fusion_network_amd import rewards as RW
    r = RW.RougeL()
    assert r.method() == 'Rouge' and r.beta == 1.2
    with pytest.raises(ValueError):
        RW.RougeL(beta=0)
    ids = (torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 1, 4, dtype=torch.int64),
           torch.ones(1, dtype=torch.int32))
    for sc in (r, RW.CiderD(), RW.BleuD()):
        with pytest.raises(RW.N.RfnError):                                            # no CPU fallback
            sc.score_ids(*ids, end_token=False)
    with pytest.raises(ValueError):
        RW.mean_score(torch.zeros(4, dtype=torch.float64))
    for m in ('METEOR', 'SPICE'):
        with pytest.raises(NotImplementedError, match='Java'):
            evalcap.LanguageEval(100, metrics=('Bleu', m))
    with pytest.raises(ValueError):
        evalcap.LanguageEval(100, metrics=('Rouge',))
    with pytest.raises(ValueError):
        evalcap.LanguageEval(40000)
    le = evalcap.LanguageEval(100)
    assert le.metrics == ('Bleu', 'ROUGE_L', 'CIDEr') and len(le) == 0
    with pytest.raises(RW.N.RfnError):
        le.add(torch.zeros(2, 4, dtype=torch.int64), [np.zeros((1, 4), dtype=np.int64)] * 2)
    with pytest.raises(ValueError):
        le.compute()
    assert callable(eval_shim.eval_split)
    # validation strings (no 0) and array_to_str strings become id rows of their own convention
    res_a, row_img, gts_a, n_refs, vocab = RW._id_arrays({7: ['3 4', '5']}, [{'image_id': 7, 'caption': ['']}], end_token=False)
    assert res_a.tolist() == [[0]] and gts_a.tolist() == [[[3, 4], [5, 0]]] and n_refs.tolist() == [2] and vocab == 5
    with pytest.raises(ValueError):
        RW._id_arrays({7: ['3 4', '5']}, [{'image_id': 7, 'caption': ['3']}])         # the reward's form needs its end token
