"""GPU: CIDEr-D and the self-critical reward (csrc/rfn_reward.hip, recurrent_fusion_network_amd/rewards.py) against the
reference's own scores (tests/golden/ciderd_*.npz, tools/make_ciderd_golden.py) and against the CPU restatement
(tests/ciderd_cpu.py) on fuzzed shapes; determinism, graph capture, out-of-range ids and the get_rewards drop-in."""
import types

import numpy as np
import pytest
import torch

import ciderd_cpu as CPU
from reward_cases import device_inputs, drop_in_data, fuzz_case, small_model, string_dicts
from test_ciderd_cpu import TIERS, golden

pytestmark = pytest.mark.gpu


def scorer_for(g, name):
    from recurrent_fusion_network_amd import rewards as RW
    if name == 'table':
        return RW.CiderD(df={tuple(str(int(x)) for x in row if x >= 0): float(c) for row, c in zip(g['df_ids'], g['df_counts'])},
                         df_mode='coco-train-synth')
    return RW.CiderD()


def close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('name', TIERS)
def test_golden_tiers_scores_and_rewards(name, dev):
    from recurrent_fusion_network_amd import rewards as RW
    g = golden(name)
    B, spi, res, row_img, gts, n_refs = device_inputs(g, dev)
    sc = scorer_for(g, name)
    s = sc.score_ids(res, row_img, gts, n_refs, vocab=int(g['vocab']))
    close(s.cpu().numpy(), g['scores'])
    out64 = torch.empty(B, res.shape[1], dtype=torch.float64, device=dev)
    r32 = RW.scst_reward(sc, res[:B], res[B:], gts, n_refs, spi, out64=out64)
    assert r32.dtype == torch.float32 and r32.shape == (B, res.shape[1])
    np.testing.assert_array_max_ulp(r32.cpu().numpy(), g['reward32'], maxulp=1)
    close(out64.cpu().numpy(), g['reward64'])
    r32n = RW.scst_reward(sc, res[:B], res[B:], gts, n_refs, spi, cider_weight=0.5, use_baseline=False)
    np.testing.assert_array_max_ulp(r32n.cpu().numpy(), g['reward32_nobase'], maxulp=1)


def test_reference_interface_compute_score(dev):
    """CiderD.compute_score on compute_reward's string dicts equals the reference's scores."""
    from recurrent_fusion_network_amd import rewards as RW
    g = golden('spi5')
    gts, res = string_dicts(g)
    mean, scores = RW.CiderD().compute_score(gts, res)
    close(scores, g['scores'])
    assert abs(mean - np.mean(g['scores'])) <= 1e-10 * abs(np.mean(g['scores']))
    with pytest.raises(ValueError):
        RW.CiderD().compute_score({0: ['3 4 0']}, [{'image_id': 0, 'caption': ['3 dog 0']}])


@pytest.mark.parametrize('seed', range(24))
def test_fuzz_against_cpu_restatement(seed, dev):
    from recurrent_fusion_network_amd import rewards as RW
    f = fuzz_case(1000, seed)
    vocab, n_img, res, row_img, gts, n_refs = f.vocab, f.n_img, f.res, f.row_img, f.gts, f.n_refs
    want = CPU.score_rows(res, row_img, gts, n_refs)
    got = RW.CiderD().score_ids(torch.from_numpy(res).to(dev), torch.from_numpy(row_img), torch.from_numpy(gts),
                                torch.from_numpy(n_refs), vocab=vocab)
    close(got.cpu().numpy(), want)
    if seed % 4 == 0:   # table mode on the same rows: a df counted from the references themselves
        df = {}
        for i in range(n_img):
            for j in range(int(n_refs[i])):
                for gram in CPU.ngram_counts(CPU.caption(gts[i, j])):
                    df[gram] = df.get(gram, 0.0) + 1.0
        want = CPU.score_rows(res, row_img, gts, n_refs, df, 5000)
        sc = RW.CiderD(df={tuple(str(x) for x in k): v for k, v in df.items()}, df_mode='coco-val')
        got = sc.score_ids(torch.from_numpy(res).to(dev), torch.from_numpy(row_img), torch.from_numpy(gts),
                           torch.from_numpy(n_refs), vocab=vocab)
        close(got.cpu().numpy(), want)


def test_bitwise_repeatable_and_graph_capturable(dev):
    from recurrent_fusion_network_amd import rewards as RW
    g = golden('spi5')
    B, spi, res, row_img, gts, n_refs = device_inputs(g, dev)
    sc = RW.CiderD()
    a = RW.scst_reward(sc, res[:B], res[B:], gts, n_refs, spi).clone()
    s1 = sc.score_ids(res, row_img, gts, n_refs).clone()
    s2 = sc.score_ids(res, row_img, gts, n_refs).clone()
    assert torch.equal(s1, s2)
    gen, greedy = res[:B].clone(), res[B:].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        RW.scst_reward(sc, gen, greedy, gts, n_refs, spi)    # warm the workspace and the row map outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = RW.scst_reward(sc, gen, greedy, gts, n_refs, spi)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    greedy.copy_(gen)                                    # new inputs through the same graph: sample == greedy -> reward 0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out))


def test_out_of_range_id_scores_nan_only_on_its_row(dev):
    from recurrent_fusion_network_amd import rewards as RW
    g = golden('c5')
    res = torch.from_numpy(g['res']).to(dev)
    row_img = torch.from_numpy(CPU.scst_rows(int(g['B']), 1))
    gts, n_refs = torch.from_numpy(g['gts']), torch.from_numpy(g['n_refs'])
    base = RW.CiderD().score_ids(res, row_img, gts, n_refs, vocab=9487).cpu().numpy()
    bad = res.clone()
    bad[3, 0] = 9488
    bad[7, 0] = -4
    bad[9, 15] = 40000
    T = res.shape[1]
    tail = next(r for r in range(12, res.shape[0]) if bool((res[r, :T - 1] == 0).any()))
    first_zero = int((res[tail] == 0).nonzero()[0])
    bad[tail, first_zero + 1:] = 99999      # after the end token: not part of the caption, the score stays
    s = RW.CiderD().score_ids(bad, row_img, gts, n_refs, vocab=9487).cpu().numpy()
    row9_reads_it = not bool((res[9, :15] == 0).any())
    nan = {3, 7} | ({9} if row9_reads_it else set())
    for r in range(len(s)):
        if r in nan:
            assert np.isnan(s[r]), r
        else:
            assert s[r] == base[r], r


def test_get_rewards_drop_in_and_full_self_critical_step(dev):
    from recurrent_fusion_network_amd import rewards as RW
    R, cfg, model, fc, att, top = small_model(dev)
    data, B, spi = drop_in_data(cfg)
    opt = types.SimpleNamespace(bleu4_weight=0, spice_weight=0, cider_weight=1.0, use_baseline=1)
    model.eval()
    with torch.no_grad():
        gen = model.sample(fc, att, {'sample_max': 0})[0]
        greedy = model.sample(fc, att)[0]
    rw = RW.get_self_critical_reward_feat_array(None, model, fc, att, data, gen, opt, scorer=RW.CiderD())
    assert isinstance(rw, np.ndarray) and rw.dtype == np.float64 and rw.shape == gen.shape
    assert not model.training                                     # the mode is left as it was
    gts, n_refs = CPU.pad_gts(data['gts'])
    res = np.concatenate([gen.cpu().numpy(), greedy.cpu().numpy()])
    want = CPU.reward(CPU.score_rows(res, CPU.scst_rows(B, spi), gts, n_refs), B, gen.shape[1])
    close(rw, want)
    # the full step of train_rl.py:160-203 with the real reward
    model.train()
    rl_crit = R.ReviewNetRewardCriterion(cfg)
    adam = R.FusedClampAdam(model, lr=5e-5, weight_decay=0.0, grad_clip=1.0)
    adam.zero_grad()
    seq, lp, lp_all, reason = model.sample(fc, att, {'sample_max': 0})
    reward = RW.get_self_critical_reward_feat_array(None, model, fc, att, data, seq, opt, device=True, scorer=RW.CiderD())
    assert model.training and reward.is_cuda and reward.dtype == torch.float32 and reward.shape == seq.shape
    assert torch.isfinite(reward).all()
    rl_crit(lp, seq, reward, lp_all, 0.01, reason, top, 1.0, None, cfg).backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)
    adam.step()
    assert all(torch.isfinite(p).all() for p in model.parameters())
