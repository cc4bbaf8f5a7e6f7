"""GPU: BLEU-D and the mixed CIDEr-D / BLEU-4 self-critical reward (csrc/rfn_reward.hip, rewards.BleuD, scst_reward with
bleu_scorer=) against the reference's own scores (tests/golden/bleud_*.npz, tools/make_bleud_golden.py) and against the CPU
restatement (tests/bleud_cpu.py) on fuzzed shapes; determinism, graph capture, out-of-range ids and the get_rewards drop-in."""
import types

import numpy as np
import pytest
import torch

import bleud_cpu as BCPU
import ciderd_cpu as CPU
from reward_cases import device_inputs, drop_in_data, fuzz_case, small_model, string_dicts
from test_bleud_cpu import TIERS, golden

pytestmark = pytest.mark.gpu

RTOL = 1e-10   # test_ciderd_gpu.close's relative tolerance; no absolute term: every BLEU-D score is strictly positive


def close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    rel = np.abs(got - want) / np.abs(want)
    print('%s: max relative error %.3g over %d values (smallest |want| %.3g)' % (what, rel.max(), rel.size, np.abs(want).min()))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


@pytest.mark.parametrize('name', TIERS)
def test_golden_tiers_scores_components_and_corpus(name, dev):
    from recurrent_fusion_network_amd import rewards as RW
    g = golden(name)
    B, spi, res, row_img, gts, n_refs = device_inputs(g, dev)
    comps = torch.full((2 * B, 10), -7, dtype=torch.int32, device=dev)
    corpus = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    s = RW.BleuD().score_ids(res, row_img, gts, n_refs, vocab=int(g['vocab']), comps=comps, corpus=corpus)
    assert s.shape == (2 * B, 4) and s.dtype == torch.float64
    np.testing.assert_array_equal(comps.cpu().numpy(), g['comps'])
    close(s.cpu().numpy(), g['bleu'], name + ' bleu')
    close(corpus.cpu().numpy(), g['corpus'], name + ' corpus')
    out = torch.empty(2 * B, 4, dtype=torch.float64, device=dev)
    assert RW.BleuD().score_ids(res, row_img, gts, n_refs, out=out) is out and torch.equal(out, s)   # default vocab, no extras


@pytest.mark.parametrize('name', TIERS)
def test_golden_tiers_mixed_reward(name, dev):
    from recurrent_fusion_network_amd import rewards as RW
    g = golden(name)
    B, spi, res, row_img, gts, n_refs = device_inputs(g, dev)
    T = res.shape[1]
    cider, bleu = RW.CiderD(), RW.BleuD()
    b4, c = np.abs(g['bleu'][:, 3]), np.abs(g['cider'])
    for k, (w_b, w_c, base) in enumerate(g['mix_weights']):
        out64 = torch.empty(B, T, dtype=torch.float64, device=dev)
        r32 = RW.scst_reward(cider, res[:B], res[B:], gts, n_refs, spi, cider_weight=float(w_c), use_baseline=bool(base),
                             out64=out64, bleu_scorer=bleu, bleu4_weight=float(w_b))
        assert r32.dtype == torch.float32 and r32.shape == (B, T)
        # the score tolerance carried through the subtraction and the weights
        bound = RTOL * (w_b * (b4[:B] + b4[B:]) + w_c * (c[:B] + c[B:]))[:, None]
        want64, want32 = g['mix_%d_64' % k], g['mix_%d_32' % k]
        err64 = np.abs(out64.cpu().numpy() - want64)
        ulp32 = np.spacing(np.abs(want32)).astype(np.float64)
        err32 = np.abs(r32.cpu().numpy().astype(np.float64) - want32.astype(np.float64))
        print('%s mix %s: f64 max err %.3g (bound there %.3g), f32 max err %.3g' % (
            name, (w_b, w_c, base), err64.max(), np.broadcast_to(bound, err64.shape).flat[int(err64.argmax())], err32.max()))
        assert (err64 <= bound).all()
        assert (err32 <= bound + ulp32).all()
    # without a BLEU scorer: today's path, bit for bit
    a64, b64 = (torch.empty(B, T, dtype=torch.float64, device=dev) for _ in range(2))
    a = RW.scst_reward(cider, res[:B], res[B:], gts, n_refs, spi, 0.7, True, out64=a64)
    scores = cider.score_ids(res, row_img, gts, n_refs)
    b = torch.empty(B, T, dtype=torch.float32, device=dev)
    RW.N.check(RW.N.lib.rfn_scst_reward(scores.data_ptr(), B, T, RW.C.c_double(0.7), 1, b.data_ptr(), b64.data_ptr(),
                                        RW.N.stream_ptr()))
    assert torch.equal(a, b) and torch.equal(a64, b64)
    assert torch.equal(a, RW.scst_reward(cider, res[:B], res[B:], gts, n_refs, spi, 0.7, True, bleu_scorer=None, bleu4_weight=0.5))
    # BLEU alone needs no CIDEr-D scorer: the reference's bleu4 * w + 0 * w_c
    only = RW.scst_reward(None, res[:B], res[B:], gts, n_refs, spi, cider_weight=0.0, bleu_scorer=bleu, bleu4_weight=1.0)
    np.testing.assert_array_equal(only.cpu().numpy(), RW.scst_reward(cider, res[:B], res[B:], gts, n_refs, spi, cider_weight=0.0,
                                                                     bleu_scorer=bleu, bleu4_weight=1.0).cpu().numpy())


def test_reference_interface_compute_score(dev):
    """BleuD.compute_score on compute_reward's string dicts equals the reference's per-row lists and corpus four."""
    from recurrent_fusion_network_amd import rewards as RW
    for name in ('spi5', 'near_spi5'):
        g = golden(name)
        B = int(g['B'])
        gts, res = string_dicts(g)
        corpus, rows = RW.BleuD(4).compute_score(gts, res)
        assert isinstance(corpus, list) and len(corpus) == 4 and isinstance(rows, list) and len(rows) == 4
        assert all(isinstance(r, list) and len(r) == 2 * B for r in rows)
        close(np.array(rows).T, g['bleu'], name + ' compute_score rows')
        close(corpus, g['corpus'], name + ' compute_score corpus')
    assert RW.BleuD().method() == 'Bleu'
    with pytest.raises(ValueError):
        RW.BleuD().compute_score({0: ['3 4 0']}, [{'image_id': 0, 'caption': ['3 dog 0']}])


@pytest.mark.parametrize('seed', range(24))
def test_fuzz_against_cpu_restatement(seed, dev):
    from recurrent_fusion_network_amd import rewards as RW
    f = fuzz_case(2000, seed)
    T, Tg, vocab, max_refs, B, res, row_img, gts, n_refs = f.T, f.Tg, f.vocab, f.max_refs, f.B, f.res, f.row_img, f.gts, f.n_refs
    want, want_comps, want_corpus = BCPU.score_rows(res, row_img, gts, n_refs)
    comps = torch.empty(2 * B, 10, dtype=torch.int32, device=dev)
    corpus = torch.empty(4, dtype=torch.float64, device=dev)
    got = RW.BleuD().score_ids(torch.from_numpy(res).to(dev), torch.from_numpy(row_img), torch.from_numpy(gts),
                               torch.from_numpy(n_refs), vocab=vocab, comps=comps, corpus=corpus)
    np.testing.assert_array_equal(comps.cpu().numpy(), want_comps)
    close(got.cpu().numpy(), want, 'fuzz %d (T %d, Tg %d, refs %d, vocab %d)' % (seed, T, Tg, max_refs, vocab))
    close(corpus.cpu().numpy(), want_corpus, 'fuzz %d corpus' % seed)


def test_bitwise_repeatable_and_graph_capturable(dev):
    from recurrent_fusion_network_amd import rewards as RW
    g = golden('near_spi5')
    B, spi, res, row_img, gts, n_refs = device_inputs(g, dev)
    cider, bleu = RW.CiderD(), RW.BleuD()
    kw = dict(cider_weight=1.0, bleu_scorer=bleu, bleu4_weight=0.5)
    a = RW.scst_reward(cider, res[:B], res[B:], gts, n_refs, spi, **kw).clone()
    corpus1, corpus2 = (torch.empty(4, dtype=torch.float64, device=dev) for _ in range(2))
    s1 = bleu.score_ids(res, row_img, gts, n_refs, corpus=corpus1).clone()
    s2 = bleu.score_ids(res, row_img, gts, n_refs, corpus=corpus2).clone()
    assert torch.equal(s1, s2) and torch.equal(corpus1, corpus2)
    assert torch.equal(a, RW.scst_reward(cider, res[:B], res[B:], gts, n_refs, spi, **kw))
    gen, greedy = res[:B].clone(), res[B:].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        RW.scst_reward(cider, gen, greedy, gts, n_refs, spi, **kw)    # warm the workspaces and the row map outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = RW.scst_reward(cider, gen, greedy, gts, n_refs, spi, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    greedy.copy_(gen)                                    # new inputs through the same graph: sample == greedy -> reward 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))


def test_out_of_range_id_scores_nan_only_on_its_row(dev):
    from recurrent_fusion_network_amd import rewards as RW
    g = golden('near')
    B, spi, res, row_img, gts, n_refs = device_inputs(g, dev)
    T = res.shape[1]
    sc = RW.BleuD()
    base = sc.score_ids(res, row_img, gts, n_refs, vocab=9487).cpu().numpy()
    bad = res.clone()
    bad[3, 0] = 9488
    bad[7, 0] = -4
    tail = next(r for r in range(12, res.shape[0]) if bool((res[r, :T - 1] == 0).any()))
    first_zero = int((res[tail] == 0).nonzero()[0])
    bad[tail, first_zero + 1:] = 99999      # after the end token: not part of the caption, the score stays
    bad_gts = gts.clone()
    bad_gts[20, 0, 0] = 9488                # a bad reference: every row of image 20 (rows 20 and B + 20 at one row per image)
    comps = torch.empty(2 * B, 10, dtype=torch.int32, device=dev)
    corpus = torch.empty(4, dtype=torch.float64, device=dev)
    s = sc.score_ids(bad, row_img, bad_gts, n_refs, vocab=9487, comps=comps, corpus=corpus).cpu().numpy()
    nan = {3, 7, 20, B + 20}
    for r in range(len(s)):
        if r in nan:
            assert np.isnan(s[r]).all(), r          # all four columns
        else:
            assert np.array_equal(s[r], base[r]), r
    keep = np.array([r not in nan for r in range(2 * B)])
    np.testing.assert_array_equal(comps.cpu().numpy()[keep], g['comps'][keep])
    assert (comps.cpu().numpy()[~keep] == 0).all()
    close(corpus.cpu().numpy(), BCPU.corpus_of(g['comps'][keep]), 'corpus without the NaN rows')
    assert not np.allclose(corpus.cpu().numpy(), g['corpus'], rtol=1e-6, atol=0)   # ... which moved it


def test_get_rewards_drop_in_and_full_self_critical_step(dev):
    from recurrent_fusion_network_amd import rewards as RW
    R, cfg, model, fc, att, top = small_model(dev)
    data, B, spi = drop_in_data(cfg)
    opt = types.SimpleNamespace(bleu4_weight=0.5, spice_weight=0, cider_weight=1.0, use_baseline=1)
    model.eval()
    with torch.no_grad():
        gen = model.sample(fc, att, {'sample_max': 0})[0]
        greedy = model.sample(fc, att)[0]
    rw = RW.get_self_critical_reward_feat_array(None, model, fc, att, data, gen, opt, scorer=RW.CiderD(), bleu_scorer=RW.BleuD())
    assert isinstance(rw, np.ndarray) and rw.dtype == np.float64 and rw.shape == gen.shape
    assert not model.training                                     # the mode is left as it was
    gts, n_refs = CPU.pad_gts(data['gts'])
    res = np.concatenate([gen.cpu().numpy(), greedy.cpu().numpy()])
    row_img = CPU.scst_rows(B, spi)
    cider = CPU.score_rows(res, row_img, gts, n_refs)
    bleu = BCPU.score_rows(res, row_img, gts, n_refs)[0]
    want = BCPU.mix(bleu, cider, B, gen.shape[1], 0.5, 1.0, True)
    bound = RTOL * (0.5 * (bleu[:B, 3] + bleu[B:, 3]) + 1.0 * (np.abs(cider[:B]) + np.abs(cider[B:])))[:, None] + 1e-12
    print('drop-in mix: max err %.3g' % np.abs(rw - want).max())
    assert (np.abs(rw - want) <= bound).all()      # + 1e-12: test_ciderd_gpu.close's absolute term for the CIDEr-D part
    # cider_weight == 0 beside BLEU-D: no CIDEr-D scorer is needed (the default one would read the df pickle)
    opt0 = types.SimpleNamespace(bleu4_weight=0.5, spice_weight=0, cider_weight=0, use_baseline=1)
    rw0 = RW.get_self_critical_reward_feat_array(None, model, fc, att, data, gen, opt0, scorer=None, bleu_scorer=RW.BleuD())
    want0 = BCPU.mix(bleu, None, B, gen.shape[1], 0.5, 0.0, True)
    assert (np.abs(rw0 - want0) <= RTOL * (0.5 * (bleu[:B, 3] + bleu[B:, 3]))[:, None]).all()
    assert 'scorer' not in RW._DEFAULT
    # the full step of train_rl.py:160-203 with the mixed reward
    model.train()
    rl_crit = R.ReviewNetRewardCriterion(cfg)
    adam = R.FusedClampAdam(model, lr=5e-5, weight_decay=0.0, grad_clip=1.0)
    adam.zero_grad()
    seq, lp, lp_all, reason = model.sample(fc, att, {'sample_max': 0})
    reward = RW.get_self_critical_reward_feat_array(None, model, fc, att, data, seq, opt, device=True, scorer=RW.CiderD(),
                                                    bleu_scorer=RW.BleuD())
    assert model.training and reward.is_cuda and reward.dtype == torch.float32 and reward.shape == seq.shape
    assert torch.isfinite(reward).all()
    rl_crit(lp, seq, reward, lp_all, 0.01, reason, top, 1.0, None, cfg).backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)
    adam.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())
