"""GPU: the caption-set diversity metrics (include/rfn.h "caption-set diversity"; csrc/rfn_reward.hip cs_div_k / cs_loo_bleu_k /
cs_bleu_corpus_k / cs_eig_k / rw_group_stats_k; rewards.diversity, rewards.group_stats, evalcap.DiversityEval, the
'keep_candidates' key and eval_split(diversity=)) against the NumPy restatement (tests/diversity_cpu.py), whose mBLEU the
reference's own Bleu scorer pins and whose U its CiderD pins (tests/test_diversity_cpu.py).

Eigenvalue bar: both solvers are backward stable to a small multiple of n * eps * ||K||, so |eig - eigvalsh(K)| <= 64 * n * 2^-52 *
||K||_F.  Every comparison prints its ratio |diff| / (n * 2^-52 * ||K||_F); the worst one measured on an MI355X over this file's
inputs is recorded in profiles/diversity_metrics.json."""
import ctypes as C

import numpy as np
import pytest
import torch

import diversity_cpu as DC
from test_consensus_cpu import df_of, golden as consensus_golden, random_case, table_df
from test_consensus_gpu import bits, eq, scorer_of
from test_diversity_cpu import extra_cases

pytestmark = pytest.mark.gpu

INT_KEYS, CLOSE_KEYS = ('distinct', 'words', 'mbleu_comps'), ('mbleu', 'mbleu_corpus', 'U')
_worst = {'eig_ratio': 0.0}


def RW():
    from recurrent_fusion_network_amd import rewards
    return rewards


def run(sc, cands, n_cand, dev, end_token=False, vocab=32767, want=None):
    t = lambda a, dt: None if a is None else torch.as_tensor(np.asarray(a), dtype=dt).to(dev)   # noqa: E731
    kw = {} if want is None else dict(want=want)
    out = sc.diversity(t(cands, torch.int64), t(n_cand, torch.int32), end_token, vocab, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12, equal_nan=True)       # tests/test_consensus_gpu.py::close


def check(got, want, n_cand):
    for k in INT_KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got['div'], want['div'], equal_nan=True)          # equal doubles: the same bits wherever it is a number
    for k in CLOSE_KEYS:
        close(got[k], want[k])
    n = got['eig'].shape[1]
    left_out = 0
    for k in range(len(n_cand)):
        K = want['K'][k]
        if K is None:
            assert np.isnan(got['eig'][k]).all() and np.isnan(got['self_cider'][k]), k
            continue
        nc = int(n_cand[k])
        unit = n * 2.0 ** -52 * np.linalg.norm(K)
        diff = np.abs(got['eig'][k, :nc] - want['eig'][k, :nc]).max()
        print('image %d: eig diff %.3e = %.3f n eps ||K||_F' % (k, diff, diff / unit if unit else 0.0))
        if unit:
            _worst['eig_ratio'] = max(_worst['eig_ratio'], diff / unit)
        assert diff <= 64 * unit, (k, diff, unit)
        assert np.isnan(got['eig'][k, nc:]).all() and (np.diff(got['eig'][k, :nc]) >= 0).all()
        # the formula apart from the solver: the GPU's own eigenvalues through the restatement's formula
        mine = DC.self_cider_of(got['eig'][k], nc)
        assert (np.isnan(mine) and np.isnan(got['self_cider'][k])) or abs(mine - got['self_cider'][k]) <= 1e-12, (k, mine)
        if DC.ambiguous_threshold(want['eig'][k], nc):
            left_out += 1
            continue
        close(got['self_cider'][k], want['self_cider'][k])
    assert left_out == 0                      # the cap: no image of this file's inputs sits on the eigenvalue cut
    print('worst eig ratio so far %.3f' % _worst['eig_ratio'])


# ---- 1. every output against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize('end_token', (True, False))
@pytest.mark.parametrize('name', ('table', 'edge', 'corpus'))
def test_consensus_golden_shapes(name, end_token, dev):
    g = consensus_golden(name)
    df, docs = df_of(g)
    got = run(scorer_of(df, 'coco-train-synth'), g['cands'], g['n_cand'], dev, end_token)
    want = DC.diversity(g['cands'], g['n_cand'], df, docs, end_token=end_token)
    check(got, want, g['n_cand'])
    if end_token:
        close(got['U'], g['U'])                                    # the reference's own CiderD


@pytest.mark.parametrize('mode', ('table', 'corpus'))
@pytest.mark.parametrize('name', sorted(extra_cases()))
def test_edge_shapes(name, mode, dev):
    cands, n_cand, vocab = extra_cases()[name]
    df = table_df(cands, n_cand) if mode == 'table' else None
    sc = scorer_of(df)
    for end_token in (True, False):
        want = DC.diversity(cands, n_cand, df, 5000, end_token=end_token, vocab=vocab)
        check(run(sc, cands, n_cand, dev, end_token, vocab), want, n_cand)
    if name == 'ragged':                                           # n_cand = NULL: all valid
        want = DC.diversity(cands, None, df, 5000, vocab=vocab)
        check(run(sc, cands, None, dev, vocab=vocab), want, np.full(len(n_cand), cands.shape[1]))
    if name == 'bad_id':
        got = run(sc, cands, n_cand, dev, vocab=vocab)
        assert np.isnan(got['div'][2]).all() and np.isnan(got['mbleu'][2]).all() and np.isnan(got['U'][2]).all()
        assert got['distinct'][2].sum() == 0 and got['words'][2] == 0 and got['mbleu_comps'][2].sum() == 0
        assert not np.isnan(got['self_cider'][[0, 1, 3, 4]]).any()
    if name == 'n1':
        got = run(sc, cands, n_cand, dev, vocab=vocab)
        assert not np.isnan(got['div']).any() and np.isnan(got['mbleu']).all() and np.isnan(got['self_cider']).all()
        assert np.isnan(got['mbleu_corpus']).all()


# ---- 2. reproducibility ----------------------------------------------------------------------------------------------------------
def test_bitwise_repeatable_and_independent_of_the_batch(dev):
    cands, n_cand, _ = random_case(31, 7, 5, 12)
    n_cand[3] = 5
    df = table_df(cands, n_cand)
    sc = scorer_of(df)
    a, b = run(sc, cands, n_cand, dev), run(sc, cands, n_cand, dev)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    alone = run(sc, cands[3:4], n_cand[3:4], dev)                  # table mode: an image is its own
    for k in a:
        if k != 'mbleu_corpus':
            assert alone[k][0].tobytes() == a[k][3].tobytes(), k
    other = cands.copy()
    other[:3], other[4:] = other[:3][::-1] + 1, 7
    moved = run(sc, np.roll(other, 2, axis=0), np.roll(n_cand, 2), dev)
    for k in ('div', 'mbleu', 'U', 'eig', 'self_cider', 'distinct'):
        assert moved[k][5].tobytes() == a[k][3].tobytes(), k
    for mode_df in (df, None):                                     # with every output but U NULL: rfn_consensus_ciderd's U
        sc2 = scorer_of(mode_df)
        t = lambda x, dt: torch.as_tensor(x, dtype=dt).to(dev)     # noqa: E731
        only = run(sc2, cands, n_cand, dev, end_token=True, want=('U',))
        assert sorted(only) == ['U']
        _, _, U = sc2.consensus(t(cands, torch.int64), t(n_cand, torch.int32), None, True, True)
        assert only['U'].tobytes() == U.cpu().numpy().tobytes()
        full = run(sc2, cands, n_cand, dev, end_token=True)
        assert full['U'].tobytes() == only['U'].tobytes()
        some = run(sc2, cands, n_cand, dev, end_token=True, want=('div', 'self_cider', 'mbleu_corpus'))
        assert all(some[k].tobytes() == full[k].tobytes() for k in some) and len(some) == 3


# ---- 3. group stats --------------------------------------------------------------------------------------------------------------
def test_group_stats(dev):
    nan = float('nan')
    col = np.array([1.0, 3.0, 3.0, 2.0, 0.5, nan, 1.0, -2.0, -2.0, -3.0, nan, 1.0, 7.0, 7.0, 7.0, 7.0], dtype=np.float64)
    n_cand = np.array([4, 1, 2, 4], dtype=np.int32)                # images 1 and 2: their NaN lies behind n_cand
    wide = np.full((16, 4), 99.0)
    wide[:, 0] = col                                               # a stride of 4
    for scores, stride in ((col, 1), (wide, 4)):
        for nc in (n_cand, None):
            want = DC.group_stats(scores, 4, nc, stride)
            got = RW().group_stats(torch.from_numpy(scores).to(dev), 4, None if nc is None else torch.from_numpy(nc).to(dev))
            assert got[0].dtype == torch.float64 and got[1].dtype == torch.int64
            for g, w in zip(got, want):
                assert np.array_equal(g.cpu().numpy(), w, equal_nan=True)
    best, arg, mean = (x.cpu().numpy() for x in RW().group_stats(torch.from_numpy(col).to(dev), 4, torch.from_numpy(n_cand).to(dev)))
    assert arg.tolist() == [1, 0, 0, 0] and best.tolist() == [3.0, 0.5, -2.0, 7.0]      # ties: the lowest index
    assert mean[0] == (((0.0 + 1.0) + 3.0) + 3.0 + 2.0) / 4.0
    assert RW().group_stats(torch.from_numpy(col).to(dev), 4)[1].tolist() == [1, -1, -1, 0]
    bad = RW().group_stats(torch.from_numpy(col).to(dev), 4, torch.tensor([0, 5, 2, 2], dtype=torch.int32))
    assert bad[1].tolist() == [-1, -1, 0, 0] and np.isnan(bad[0][:2].cpu().numpy()).all()


# ---- 4. the oracle numbers -------------------------------------------------------------------------------------------------------
def oracle_inputs(seed, B, n, T, dev):
    cands, _, _ = random_case(seed, B, n, T, ragged=False)
    gts, n_refs, _ = random_case(seed + 1, B, 4, T)
    cands[:, :, 0], gts[:, :, 0] = 5, 5                            # no empty caption
    return torch.from_numpy(cands).to(dev), torch.from_numpy(gts).to(dev), torch.from_numpy(n_refs).to(dev)


def test_one_candidate_is_language_eval(dev):
    from recurrent_fusion_network_amd.evalcap import DiversityEval, LanguageEval
    cands, gts, n_refs = oracle_inputs(40, 9, 1, 10, dev)
    ev, lang = DiversityEval(60), LanguageEval(60)
    ev.add(cands[:5], gts[:5], n_refs[:5])
    ev.add(cands[5:].reshape(4, 10), gts[5:], n_refs[5:], n=1)     # the (B * n, T) form
    lang.add(cands[:, 0], gts, n_refs)
    got, want = ev.compute(), lang.compute()
    for m, key in (('CIDEr', 'CIDEr'), ('Bleu_4', 'Bleu_4'), ('ROUGE_L', 'ROUGE_L')):
        assert got['Oracle_' + m] == got['Mean_' + m] == want[key], m
        assert type(got['Oracle_' + m]) is float
    p, lp = ev.per_image(), lang.per_image()
    assert bits(p['Oracle_CIDEr']) == bits(lp['CIDEr']) == bits(p['Mean_CIDEr']) and bits(p['CIDEr']) == bits(lp['CIDEr'])
    assert bits(p['Oracle_ROUGE_L']) == bits(lp['ROUGE_L']) == bits(p['Mean_ROUGE_L'])
    assert bits(p['Oracle_Bleu_4']) == bits(lp['Bleu'][:, 3].contiguous()) and bits(p['Bleu'].view(9, 4)) == bits(lp['Bleu'])
    assert len(ev) == 9 and ev.skipped['Oracle_CIDEr'] == 0 and ev.skipped['Self_CIDEr'] == 9      # n = 1: nothing to compare
    assert np.isnan(got['Self_CIDEr']) and np.isnan(got['mBleu_4']) and got['Div_1'] > 0
    ev.reset()
    assert len(ev) == 0 and ev.skipped is None


def test_oracle_is_the_best_slot_of_language_eval(dev):
    from recurrent_fusion_network_amd.evalcap import DiversityEval, LanguageEval
    B, n = 8, 3
    cands, gts, n_refs = oracle_inputs(50, B, n, 10, dev)
    ev = DiversityEval(60)
    ev.add(cands, gts, n_refs)
    got, p = ev.compute(), ev.per_image()
    per = {'CIDEr': [], 'ROUGE_L': [], 'Bleu': []}
    corpus4 = []
    for j in range(n):
        lang = LanguageEval(60)
        lang.add(cands[:, j], gts, n_refs)
        corpus4.append(lang.compute()['Bleu_4'])
        for k in per:
            per[k].append(lang.per_image()[k])
    cider = torch.stack(per['CIDEr'], 1)
    assert bits(p['CIDEr']) == bits(cider)                          # a corpus df: one call per slot, LanguageEval's df
    assert bits(p['Oracle_CIDEr']) == bits(cider.max(1).values)
    assert bits(p['Oracle_ROUGE_L']) == bits(torch.stack(per['ROUGE_L'], 1).max(1).values)
    assert bits(p['Oracle_Bleu_4']) == bits(torch.stack(per['Bleu'], 1)[:, :, 3].max(1).values)
    assert abs(got['Mean_Bleu_4'] - float(np.mean(corpus4))) <= 1e-15            # the slots' corpus BLEU-4, averaged
    assert got['Oracle_CIDEr'] >= got['Mean_CIDEr'] and got['Oracle_ROUGE_L'] >= got['Mean_ROUGE_L']
    want = DC.report(DC.diversity(cands.cpu().numpy(), None, None, None, vocab=60))
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-10 * max(1.0, abs(v)), k
    assert sorted(got) == sorted(['Div_%d' % m for m in range(1, 5)] + ['mBleu_%d' % m for m in range(1, 5)] +
                                 ['Self_CIDEr'] + [a + b for a in ('Oracle_', 'Mean_') for b in ('CIDEr', 'Bleu_4', 'ROUGE_L')])
    # ragged: the stats ignore the slots behind n_cand, whatever they hold
    n_cand = torch.tensor([3, 1, 2, 3, 3, 2, 1, 3], dtype=torch.int32)
    junk = cands.clone()
    for k in range(B):
        junk[k, int(n_cand[k]):] = 61
    ev2 = DiversityEval(60, metrics=('CIDEr', 'ROUGE_L', 'Bleu_4'))
    ev2.add(junk, gts, n_refs, n_cand=n_cand)
    p2 = ev2.per_image()
    valid = (torch.arange(n)[None, :] < n_cand[:, None]).to(dev)
    for m, full in (('CIDEr', cider), ('ROUGE_L', torch.stack(per['ROUGE_L'], 1))):
        assert bits(p2['Oracle_' + m]) == bits(torch.where(valid, full, torch.full_like(full, -1.0)).max(1).values), m
    assert ev2.skipped['Oracle_CIDEr'] == 0 and sorted(ev2.compute()) == sorted(a + b for a in ('Oracle_', 'Mean_')
                                                                                for b in ('CIDEr', 'Bleu_4', 'ROUGE_L'))


# ---- 5. decode -------------------------------------------------------------------------------------------------------------------
def test_keep_candidates(dev):
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    from test_decode_constraints_gpu import setup
    model, fc, att = setup('tiny0', dev)
    B, S = fc[0].size(0), model.seq_length
    with torch.no_grad():
        for opt in ({'beam_size': 4}, {'beam_size': 4, 'group_size': 2}, {'beam_size': 4, 'consensus': scorer_of(None)}):
            for owner in (model, EnsembleDecoder([model])):
                plain = owner.sample_beam(fc, att, opt)
                assert owner.candidates is None                    # without the key
                kept = owner.sample_beam(fc, att, dict(opt, keep_candidates=True))
                assert bits(plain[0]) == bits(kept[0]) and bits(plain[1]) == bits(kept[1]) and eq(list(plain[2]), list(kept[2]))
                seq, n_cand = owner.candidates['seq'].cpu(), owner.candidates['n_cand'].cpu()
                assert seq.dtype == torch.int64 and n_cand.dtype == torch.int32 and owner.candidates['seq'].device.type == 'cuda'
                lists = owner.diverse_beams if 'group_size' in opt else [img[:4] for img in owner.done_beams]
                assert tuple(seq.shape) == (B, 2 if 'group_size' in opt else 4, S)
                for k, img in enumerate(lists):
                    assert n_cand[k] == len(img) and all(torch.equal(seq[k, j], d['seq']) for j, d in enumerate(img))
        out = model.sample(fc, att, {'beam_size': 4, 'keep_candidates': True})       # sample(beam_size > 1) forwards the key
        assert tuple(model.candidates['seq'].shape) == (B, 4, S) and bits(out[0]) == bits(model.sample_beam(fc, att, {'beam_size': 4})[0])
        model.sample(fc, att, {'sample_max': 1})
        assert model.candidates is None


def test_eval_split_feeds_the_diversity_eval(dev):
    from oracle import rfn_oracle as O
    from recurrent_fusion_network_amd import eval_shim
    from recurrent_fusion_network_amd.evalcap import DiversityEval, LanguageEval
    from reward_cases import drop_in_data, small_model
    R, cfg, model, fc, att, top = small_model(dev)
    _, _, labels, masks, _ = O.synthetic_batch(cfg, 8, seed=7)
    data, B, spi = drop_in_data(cfg)
    batch = dict(fc_feats=fc, att_feats=att, labels=labels.to(dev), masks=masks.to(dev), top_words=top, gts=data['gts'])
    crit = R.ReviewNetEnsembleCriterion(cfg)
    model.eval()
    n, imgs, S = 3, B // spi, cfg.seq_length
    r = torch.rand(2, S + 1, imgs * n, generator=torch.Generator().manual_seed(9)).to(dev)
    opt = {'sample_n': n, 'top_k': 30}
    ev, lang = DiversityEval(cfg.vocab_size), LanguageEval(cfg.vocab_size)
    model._ss_uniforms = r
    try:
        loss, scores = eval_shim.eval_split(model, crit, [batch], spi, cfg.vocab_size, sample_max=0, decode_opt=opt, diversity=ev,
                                            language_eval=lang)
        rows = eval_shim.unique_image_rows(8, spi, dev)
        with torch.no_grad():
            seq = model.sample([f.index_select(0, rows) for f in fc], [a.index_select(0, rows) for a in att],
                               dict(opt, sample_max=0))[0]
    finally:
        model._ss_uniforms = None
    assert seq.size(0) == imgs * n and len(ev) == imgs and len(lang) == imgs and np.isfinite(loss)
    by_hand, lang2 = DiversityEval(cfg.vocab_size), LanguageEval(cfg.vocab_size)
    by_hand.add(seq, data['gts'], n=n)
    lang2.add(seq.view(imgs, n, -1)[:, 0], data['gts'])                 # draw 0: the call's one caption per image
    assert ev.compute() == by_hand.compute() and scores == lang2.compute() and len(ev.compute()) == 15
    ev_b = DiversityEval(cfg.vocab_size, metrics=('Div', 'mBleu', 'Self_CIDEr', 'ROUGE_L'))
    eval_shim.eval_split(model, crit, [batch], spi, cfg.vocab_size, beam_size=3, diversity=ev_b)
    by_hand = DiversityEval(cfg.vocab_size, metrics=('Div', 'mBleu', 'Self_CIDEr', 'ROUGE_L'))
    by_hand.add(model.candidates['seq'], data['gts'], n_cand=model.candidates['n_cand'])
    assert ev_b.compute() == by_hand.compute() and model.candidates['seq'].size(1) == 3
    assert all(np.isfinite(v) for v in ev_b.compute().values())


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------
def test_errors(dev):
    import recurrent_fusion_network_amd._native as N
    cands = torch.ones(2, 3, 8, dtype=torch.int64, device=dev)
    ws = torch.empty(N.lib.rfn_capset_ws_bytes(2, 3, 8, 1), dtype=torch.uint8, device=dev)
    div = torch.full((2, 4), -7.0, dtype=torch.float64, device=dev)

    def call(n=3, T=8, flags=0, ws_bytes=ws.numel(), vocab=60):
        outs = [None, None, div.data_ptr()] + [None] * 6
        return N.lib.rfn_capset_diversity(cands.data_ptr(), 2, n, T, None, None, 0, C.c_double(0.0), vocab, C.c_double(6.0), flags,
                                          *outs, ws.data_ptr(), ws_bytes, N.stream_ptr())
    assert call(n=33) == -1 and call(T=65) == -1 and call(vocab=32768) == -1          # RFN_ERR_SHAPE
    assert call(ws_bytes=ws.numel() - 1) == -4                                      # RFN_ERR_WORKSPACE
    assert call(flags=2) == -5                                                      # RFN_ERR_ARG
    torch.cuda.synchronize()
    assert (div == -7.0).all()                                                      # a refused call launches nothing
    assert call() == 0                                                              # 3 captions of 8 ones, no END: 24 words
    torch.cuda.synchronize()
    assert torch.equal(div[:, 0], torch.full((2,), 1 / (1e-6 + 24), dtype=torch.float64, device=dev))
    sc = RW().CiderD()
    with pytest.raises(N.RfnError):
        sc.diversity(cands.cpu())
    with pytest.raises(ValueError):
        sc.diversity(torch.ones(1, 33, 8, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        sc.diversity(cands, want=('div', 'nope'))
