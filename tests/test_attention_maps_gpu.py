"""GPU: RecurrentFusionModel.attention (INTEGRATION.md "Attention maps") against the fp64 restatement built from the oracle's cells
(tests/attention_maps_cpu.py, pinned by test_attention_maps_cpu.py).

Bounds: every family of weights and every rollout map within 1e-4 max abs -- what tests/test_model_gpu.py uses for thought vectors
and states against the oracle on these tiers; the weights are softmax outputs of those states; `length` exact; dead steps bit-zero;
live rows sum to 1 within 1e-5."""
import copy
import functools

import numpy as np
import pytest
import torch

import mos_cpu as MC
from attention_maps_cpu import attention_maps, stats_np
from conftest import load_case

pytestmark = pytest.mark.gpu

MAP_TOL = 1e-4


def build(cfg, P, dev):
    import recurrent_fusion_network_amd as R
    model = R.RecurrentFusionModel(cfg)
    model.load_state_dict(P)
    return model.to(dev).eval()


@functools.lru_cache(maxsize=None)
def case(name):
    """One tier, its model inputs on the host and the restatement of attention(labels[:, 1:]): computed once, never modified."""
    cfg, spec, P, (fc, att, labels, masks, top), gold = load_case(name)
    return cfg, P, fc, att, labels, attention_maps(cfg, P, fc, att, labels[:, 1:])


def on(dev, ts):
    return [t.to(dev) for t in ts]


def err(t, ref):
    return float(np.abs(t.double().cpu().numpy() - ref).max())


def live_of(length, steps):
    return np.arange(steps)[None, :] < np.asarray(length)[:, None]


def check_against(got, ref, M, tol=MAP_TOL):
    steps = ref['decoder'].shape[1]
    assert got['length'].dtype == torch.int32 and np.array_equal(got['length'].cpu().numpy(), ref['length'])
    live = live_of(ref['length'], steps)
    figures = {'fusion': err(got['fusion'], ref['fusion']), 'decoder': err(got['decoder'], ref['decoder'])}
    for i in range(M):
        figures['encoder%d' % i] = err(got['encoder'][i], ref['encoder'][i])
        figures['rollout%d' % i] = err(got['rollout'][i], ref['rollout'][i])
    print('max abs error against the restatement:', figures)
    assert max(figures.values()) <= tol, figures
    dead = torch.from_numpy(~live)
    assert not bool(got['decoder'].cpu().view(torch.int32)[dead].any())
    assert abs(got['decoder'].double().sum(2).cpu().numpy()[live] - 1).max() <= 1e-5
    assert abs(got['fusion'].double().sum(3).cpu().numpy() - 1).max() <= 1e-5
    for i in range(M):
        assert abs(got['encoder'][i].double().sum(2).cpu().numpy() - 1).max() <= 1e-5
        G = got['rollout'][i]
        assert G.shape == ref['rollout'][i].shape and G.is_contiguous()
        assert not bool(G.cpu().view(torch.int32)[dead].any()), 'dead steps are not bit-zero'
        assert abs(G.double().sum(2).cpu().numpy()[live] - 1).max() <= 1e-5


@pytest.mark.parametrize('name', ['tiny0', 'odd', 'mid'])
def test_attention_against_the_restatement(dev, name):
    cfg, P, fc, att, labels, ref = case(name)
    model = build(cfg, P, dev)
    model.train()                                                   # dropout stays off whatever the mode (probabilities are 0 here)
    got = model.attention(on(dev, fc), on(dev, att), labels[:, 1:].to(dev))
    M, B = len(att), fc[0].size(0)
    T1, T2 = cfg.num_review_steps_0, cfg.num_review_steps
    steps = min(labels.size(1) - 1, cfg.seq_length) + 1
    assert sorted(got) == ['decoder', 'encoder', 'fusion', 'length', 'rollout']
    assert tuple(got['fusion'].shape) == (B, T2, M, T1) and tuple(got['decoder'].shape) == (B, steps, T2)
    assert [tuple(a.shape) for a in got['encoder']] == [(B, T1, a.size(1)) for a in att]
    check_against(got, ref, M)


def test_two_captions_per_image_equal_two_calls(dev):
    cfg, P, fc, att, labels, _ = case('odd')
    model = build(cfg, P, dev)
    fcd, attd = on(dev, fc), on(dev, att)
    s0, s1 = labels[:, 1:].to(dev), labels[:, 1:].flip(0).to(dev)
    both = model.attention(fcd, attd, torch.stack([s0, s1], 1))
    flat = model.attention(fcd, attd, torch.stack([s0, s1], 1).reshape(-1, s0.size(1)), {'n': 2})
    chunked = model.attention(fcd, attd, torch.stack([s0, s1], 1), {'max_rows': 3})      # several decoder calls: no bit changes
    assert torch.equal(chunked['decoder'], both['decoder']) and all(torch.equal(x, y) for x, y in zip(chunked['rollout'], both['rollout']))
    a, b = model.attention(fcd, attd, s0), model.attention(fcd, attd, s1)
    assert torch.equal(both['fusion'], a['fusion']) and torch.equal(both['fusion'], b['fusion'])
    assert torch.equal(both['length'].view(-1, 2), torch.stack([a['length'], b['length']], 1))
    for i in range(len(att)):
        assert torch.equal(both['encoder'][i], a['encoder'][i])
        assert torch.equal(both['rollout'][i], flat['rollout'][i])
        for j, one in enumerate((a, b)):
            assert float((both['rollout'][i][j::2] - one['rollout'][i]).abs().max()) <= 1e-6
    for j, one in enumerate((a, b)):
        assert float((both['decoder'][j::2] - one['decoder']).abs().max()) <= 1e-6


def test_ragged_maps(dev):
    cfg, P, fc, att, labels, ref_full = case('odd')
    model = build(cfg, P, dev)
    fcd, attd, seq = on(dev, fc), on(dev, att), labels[:, 1:].to(dev)
    B, Ls = fc[0].size(0), [a.size(1) for a in att]
    lens = [[1 if b == 0 else (L if b == 1 else max(1, L - 1 - b % 2)) for b in range(B)] for L in Ls]
    got = model.attention(fcd, attd, seq, att_lens=[torch.tensor(v) for v in lens])
    ref = attention_maps(cfg, P, fc, att, labels[:, 1:], att_lens=lens)
    check_against(got, ref, len(att))
    for i, L in enumerate(Ls):
        for b in range(B):
            assert not bool(got['encoder'][i][b, :, lens[i][b]:].cpu().view(torch.int32).any())
            assert not bool(got['rollout'][i][b, :, lens[i][b]:].cpu().view(torch.int32).any())
    full = model.attention(fcd, attd, seq, att_lens=[torch.full((B,), L) for L in Ls])
    plain = model.attention(fcd, attd, seq)
    for i in range(len(att)):
        assert float((full['rollout'][i] - plain['rollout'][i]).abs().max()) <= 1e-6
        assert float((full['encoder'][i] - plain['encoder'][i]).abs().max()) <= 1e-6
    assert float((full['decoder'] - plain['decoder']).abs().max()) <= 1e-6


def test_captions_from_a_decoding_call(dev):
    cfg, P, fc, att, labels, _ = case('mid')
    model = build(cfg, P, dev)
    fcd, attd = on(dev, fc), on(dev, att)
    with torch.no_grad():
        seq = model.sample(fcd, attd, {'sample_max': 1})[0]
    got = model.attention(fcd, attd, seq)
    words = (seq != 0).long().cumprod(1).sum(1)
    assert torch.equal(got['length'].long().cpu(), (words + 1).cpu()) and int(got['length'].max()) <= seq.size(1) + 1
    live = live_of(got['length'].cpu().numpy(), seq.size(1) + 1)
    assert abs(got['rollout'][0].double().sum(2).cpu().numpy()[live] - 1).max() <= 1e-5


def test_a_mixture_of_softmaxes_model_works_unchanged(dev):
    import recurrent_fusion_network_amd as R
    cfg, P, fc, att, labels, ref = case('tiny0')
    mcfg = copy.copy(cfg)                                           # tests/test_mos_model_gpu.build_mos, restated
    mcfg.use_mos, mcfg.num_expert = 1, 3
    mos = R.RecurrentFusionModel(mcfg)
    sd = dict(P)
    sd.update({'mos.' + k: v for k, v in MC.random_params(cfg.rnn_size, cfg.rnn_size, 3, cfg.vocab_size + 1, 31).items()})
    mos.load_state_dict(sd)
    mos = mos.to(dev).eval()
    plain = build(cfg, P, dev)
    fcd, attd, seq = on(dev, fc), on(dev, att), labels[:, 1:].to(dev)
    a, b = mos.attention(fcd, attd, seq), plain.attention(fcd, attd, seq)
    assert torch.equal(a['fusion'], b['fusion']) and all(torch.equal(x, y) for x, y in zip(a['encoder'], b['encoder']))
    live = live_of(ref['length'], a['decoder'].size(1))
    assert abs(a['decoder'].double().sum(2).cpu().numpy()[live] - 1).max() <= 1e-5
    check_against(a, ref, len(att))                                 # no output layer is involved: the same maps


def test_refusals_by_name(dev):
    import recurrent_fusion_network_amd._native as N
    cfg, P, fc, att, labels, ref = case('tiny0')
    model = build(cfg, P, dev)
    fcd, attd, seq = on(dev, fc), on(dev, att), labels[:, 1:].to(dev)
    rows, steps, Ls = seq.size(0), ref['decoder'].shape[1], [a.size(1) for a in att]
    for flag in (N.PATH_OPT_DEC_UNHOISTED, N.PATH_OPT_PERSIST_DEC_FWD):
        model.path_flags = flag
        with pytest.raises(N.RfnError, match='hoisted decoder cell'):
            model.attention(fcd, attd, seq)
    model.path_flags = 0
    model.fixed_decoder_steps = 3                                   # what a GraphedTrainStep sets while it owns the model
    with pytest.raises(N.RfnError, match='GraphedTrainStep'):
        model.attention(fcd, attd, seq)
    model.fixed_decoder_steps = None
    with pytest.raises(ValueError, match="'length_penalty'"):
        model.attention(fcd, attd, seq, {'length_penalty': 1.0})
    with pytest.raises(ValueError, match='outputs'):
        model.attention(fcd, attd, seq, {'outputs': ['rank']})
    with pytest.raises(ValueError, match='region_mask'):
        model.attention(fcd, attd, seq, {'outputs': ['mass']})
    ok = [torch.ones(rows, steps, L, dtype=torch.bool, device=dev) for L in Ls]
    for bad, what in ((ok[:1], 'list of 2'), ([ok[0][:, :-1], ok[1]], 'shape'), ([ok[0].float(), ok[1]], 'bool or uint8'),
                      ([ok[0].cpu(), ok[1]], 'lives on')):
        with pytest.raises(ValueError, match=what):
            model.attention(fcd, attd, seq, {'outputs': ['mass'], 'region_mask': bad})
    with pytest.raises(ValueError, match='caption rows'):
        model.attention(fcd, attd, seq[:2])
    assert sorted(model.attention(fcd, attd, seq, {'outputs': 'peak'})) == ['decoder', 'encoder', 'fusion', 'length', 'peak', 'rollout']


@pytest.mark.parametrize('name', ['tiny0', 'odd', 'mid'])
def test_peak_entropy_mass_against_the_restatement(dev, name):
    """The kernel test's rules.  entropy and mass within 1e-5 absolute of the restatement's.  peak equals the fp64 first argmax
    except where the two largest fp64 values are too close to call: with e the max abs error of THIS run's map against the
    restatement (asserted <= 1e-4 first), a different argmax needs ref[j] + e >= ref[i] - e, so only pairs whose fp64 top-two gap is
    <= 2 e are excepted -- and at most 1 % of the live pairs may be, asserted on the fp64 side.
    Independently of the model's error, the three outputs are also checked at EVERY live pair against the fp64 statistics of the
    map the call itself returned (peak exactly: the same f32 values, the first maximum on both sides): that pins which rows, strides and masks the statistics launches got."""
    cfg, P, fc, att, labels, ref = case(name)
    model = build(cfg, P, dev)
    M, rows, steps = len(att), labels.size(0), ref['decoder'].shape[1]
    rng = np.random.default_rng(5)
    masks = [rng.random((rows, steps, a.size(1))) < 0.5 for a in att]
    dmasks = [torch.from_numpy(m).to(dev) if i % 2 == 0 else torch.from_numpy(m.astype(np.uint8)).to(dev) for i, m in enumerate(masks)]
    dmasks[-1] = None
    got = model.attention(on(dev, fc), on(dev, att), labels[:, 1:].to(dev), {'outputs': ['mass', 'peak', 'entropy'], 'region_mask': dmasks})
    live = live_of(ref['length'], steps)
    assert live.any()
    for i in range(M):
        g_peak, g_ent = got['peak'][i].cpu().numpy(), got['entropy'][i].double().cpu().numpy()
        g_mass = None if dmasks[i] is None else got['mass'][i].double().cpu().numpy()
        assert got['peak'][i].dtype == torch.int32 and (dmasks[i] is not None or got['mass'][i] is None)
        # against the restatement
        e = err(got['rollout'][i], ref['rollout'][i])
        assert e <= MAP_TOL
        peak, gap, ent, mass = stats_np(ref['rollout'][i], ref['length'], masks[i])
        sure = live & (gap > 2 * e)
        share = float((live & ~sure).sum()) / float(live.sum())
        figures = (e, float(np.abs(g_ent - ent).max()), None if g_mass is None else float(np.abs(g_mass - mass).max()), share)
        print('encoder %d: map err %g, entropy err %g, mass err %s, share of pairs too close to call %g' % ((i,) + figures))
        assert share <= 0.01, figures
        assert np.array_equal(g_peak[sure], peak[sure])
        assert figures[1] <= 1e-5 and (g_mass is None or figures[2] <= 1e-5)
        assert not g_ent[~live].any() and (g_peak[~live] == -1).all() and (g_mass is None or not g_mass[~live].any())
        # against the map this call returned, every live pair
        own = got['rollout'][i].double().cpu().numpy()
        o_peak, o_gap, o_ent, o_mass = stats_np(own, ref['length'], masks[i])
        assert np.array_equal(g_peak[live], o_peak[live])    # both take the FIRST maximum, so exact ties agree too
        assert np.abs(g_ent - o_ent).max() <= 1e-5 and (g_mass is None or np.abs(g_mass - o_mass).max() <= 1e-5)


def test_persistent_stage_two_chain_keeps_its_weights(dev):
    """path_flags that select the persistent stage-II chains are accepted: the chain writes the same weights to
    the same slots, so every output is the bits of the call without the flags.  At the c2 tier, BASELINE config 2's shape, where
    tests/test_chain_gpu.py runs the chain."""
    import recurrent_fusion_network_amd._native as N
    cfg, spec, P, (fc, att, labels, masks, top), gold = load_case('c2')
    model = build(cfg, P, dev)
    fcd, attd, seq = on(dev, fc), on(dev, att), labels[:, 1:].to(dev)
    want = model.attention(fcd, attd, seq)
    model.path_flags = N.PATH_OPT_PERSIST_S2_FWD | N.PATH_OPT_PERSIST_S2_BWD
    got = model.attention(fcd, attd, seq)
    assert torch.equal(got['fusion'], want['fusion']) and torch.equal(got['decoder'], want['decoder'])
    assert all(torch.equal(a, b) for k in ('encoder', 'rollout') for a, b in zip(got[k], want[k]))
    live = live_of(want['length'].cpu().numpy(), want['decoder'].size(1))
    assert abs(got['fusion'].double().sum(3).cpu().numpy() - 1).max() <= 1e-5
    assert abs(got['rollout'][0].double().sum(2).cpu().numpy()[live] - 1).max() <= 1e-5
