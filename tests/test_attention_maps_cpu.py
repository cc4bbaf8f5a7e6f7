"""CPU: the fp64 restatement of model.attention (tests/attention_maps_cpu.py) is the oracle's computation -- same thought vectors,
same log-probs, to the bit -- so the attention weights it collects are the oracle's; every live row of every family and of every
rollout map is a distribution; ragged columns are exact zeros.  The GPU tests compare against this restatement."""
import numpy as np
import pytest
import torch

from attention_maps_cpu import attention_maps, rollout_np, stats_np
from conftest import load_case

TIERS = ['tiny0', 'odd']


def _double(P, fc, att):
    return {k: v.double() for k, v in P.items()}, [t.double() for t in fc], [t.double() for t in att]


@pytest.mark.parametrize('name', TIERS)
def test_restatement_is_the_oracles_computation(name):
    from oracle import rfn_oracle as O
    cfg, spec, P, (fc, att, labels, masks, top), gold = load_case(name)
    Pd, fcd, attd = _double(P, fc, att)
    got = attention_maps(cfg, P, fc, att, labels[:, 1:])
    hs, cs = O.init_state(cfg, Pd, fcd)
    comb, _, _ = O.thought_vectors(cfg, Pd, attd, hs, cs)
    assert np.array_equal(got['comb'], comb.numpy())
    lp, _ = O.forward(cfg, Pd, fcd, attd, labels)
    S = lp.size(1)
    assert 1 <= S <= got['log_prob'].shape[1]
    assert np.array_equal(got['log_prob'][:, :S], lp.numpy())
    # length = words + 1, capped at the steps
    words = (labels[:, 1:] != 0).long().cumprod(1).sum(1).numpy()
    steps = min(labels.size(1) - 1, cfg.seq_length) + 1
    assert np.array_equal(got['length'], np.minimum(words + 1, steps))
    assert got['decoder'].shape == (labels.size(0), steps, cfg.num_review_steps)


@pytest.mark.parametrize('name', TIERS)
def test_every_live_row_is_a_distribution(name):
    cfg, spec, P, (fc, att, labels, masks, top), gold = load_case(name)
    got = attention_maps(cfg, P, fc, att, labels[:, 1:])
    live = np.arange(got['decoder'].shape[1])[None, :] < got['length'][:, None]
    assert live.any()
    for a in got['encoder']:
        assert np.abs(a.sum(2) - 1).max() < 1e-12 and a.min() >= 0
    assert np.abs(got['fusion'].sum(3) - 1).max() < 1e-12
    assert np.abs(got['decoder'].sum(2)[live] - 1).max() < 1e-12
    assert not got['decoder'][~live].any()
    for G in got['rollout']:
        assert np.abs(G.sum(2)[live] - 1).max() < 1e-12 and G.min() >= 0
        assert not G[~live].any()


def test_n_rows_per_image_share_the_image():
    cfg, spec, P, (fc, att, labels, masks, top), gold = load_case('tiny0')
    seq = labels[:, 1:]
    two = torch.stack([seq, seq.flip(0)], 1).reshape(-1, seq.size(1))          # rows image-major: (b, 0), (b, 1)
    got = attention_maps(cfg, P, fc, att, two, n=2)
    a, b = attention_maps(cfg, P, fc, att, seq), attention_maps(cfg, P, fc, att, seq.flip(0))
    for i in range(len(att)):
        assert np.array_equal(got['encoder'][i], a['encoder'][i])
        assert np.abs(got['rollout'][i][0::2] - a['rollout'][i]).max() < 1e-14
        assert np.abs(got['rollout'][i][1::2] - b['rollout'][i]).max() < 1e-14


@pytest.mark.parametrize('name', TIERS)
def test_ragged_columns_are_exact_zeros(name):
    cfg, spec, P, (fc, att, labels, masks, top), gold = load_case(name)
    B = fc[0].size(0)
    Ls = [a.size(1) for a in att]
    lens = [[1 if b == 0 else (L if b == 1 else max(1, L - 1)) for b in range(B)] for L in Ls]
    lens[-1] = None                                                            # an encoder whose maps are full
    got = attention_maps(cfg, P, fc, att, labels[:, 1:], att_lens=lens)
    live = np.arange(got['decoder'].shape[1])[None, :] < got['length'][:, None]
    for i, L in enumerate(Ls):
        a, G = got['encoder'][i], got['rollout'][i]
        for b in range(B):
            n = L if lens[i] is None else lens[i][b]
            assert not a[b, :, n:].any() and not G[b, :, n:].any()
        assert np.abs(a.sum(2) - 1).max() < 1e-12
        assert np.abs(G.sum(2)[live] - 1).max() < 1e-12
    # all-full lengths: each image alone gives the batch's numbers up to the rounding of the batched products
    full = attention_maps(cfg, P, fc, att, labels[:, 1:], att_lens=[[L] * B for L in Ls])
    ref = attention_maps(cfg, P, fc, att, labels[:, 1:])
    for i in range(len(Ls)):
        assert np.abs(full['rollout'][i] - ref['rollout'][i]).max() < 1e-12


def test_rollout_and_stats_helpers():
    rng = np.random.default_rng(0)
    aD, a2, a1 = rng.random((4, 3, 2)), rng.random((2, 2, 5)), rng.random((2, 5, 7))
    G = rollout_np(aD, a2, a1, n=2, length=[0, 1, 3, 2], att_len=[7, 3])
    want = np.einsum('rst,rtu,rul->rsl', aD, np.repeat(a2, 2, 0), np.repeat(a1, 2, 0))
    assert np.abs(G[2, :, :3] - want[2, :, :3]).max() < 1e-14 and not G[2:, :, 3:].any() and not G[0].any() and not G[1, 1:].any()
    mask = rng.random(G.shape) < 0.5
    peak, gap, ent, mass = stats_np(G, [0, 1, 3, 2], mask)
    assert peak[0, 0] == -1 and ent[0, 0] == 0 and mass[0, 0] == 0 and peak[2, 1] == G[2, 1].argmax()
    assert abs(mass[2, 1] - G[2, 1][mask[2, 1]].sum()) < 1e-14
    p = np.array([[[0.5, 0.5, 0.0]]])
    assert stats_np(p)[0][0, 0] == 0 and abs(stats_np(p)[2][0, 0] - np.log(2)) < 1e-15 and stats_np(p)[1][0, 0] == 0


def test_native_entries_refuse_before_launching():
    """Shape defects win over NULL pointers, the LDS limit comes last; a refused call returns before it reads through a pointer or
    launches anything, so dummy addresses and no GPU do."""
    import ctypes as C
    import recurrent_fusion_network_amd._native as N
    P = 0x10000

    def rollout(rows=6, n=3, S=4, T1=3, T2=2, L=8, aD=P, a2=P, a1=P, out=P, o_ss=None):
        o_ss = L if o_ss is None else o_ss
        return N.lib.rfn_attn_rollout(aD, rows * max(T2, 1), max(T2, 1), a2, 2 * max(T1, 1), max(T1, 1), a1, 2 * max(L, 1), max(L, 1), None,
                                      None, rows, n, S, T1, T2, L, out, S * max(o_ss, 1), o_ss, None)

    for bad in (dict(rows=0), dict(n=0), dict(S=0), dict(T1=0), dict(T2=0), dict(L=0), dict(rows=5), dict(o_ss=7), dict(rows=0, aD=None)):
        assert rollout(**bad) == -1, bad
    for bad in (dict(aD=None), dict(a2=None), dict(a1=None), dict(out=None)):
        assert rollout(**bad) == -5, bad
    assert rollout(T2=1024, S=17) == -2 and rollout(T2=1024, S=17, out=None) == -5
    assert N.lib.rfn_attn_map_stats(P, 32, 8, None, None, 0, 0, 0, 4, 8, P, P, None, None) == -1
    assert N.lib.rfn_attn_map_stats(P, 32, 8, None, P, 32, 8, 6, 4, 8, P, P, None, None) == -5
    assert N.lib.rfn_attn_decoder_copy(P, 12, 2, None, 6, 4, 2, P, 8, 1, None) == -1
    d = N.make_dims(2, 16, 16, 16, 3, 3, 20, 51, [5, 7], [24, 40], [24, 32])
    ws = 1 << 20
    a1 = [N.lib.rfn_prefix_alpha1(C.byref(d), 3, t, i, ws) for t in (0, 1) for i in (0, 1)]
    assert all(a1) and a1[:2] == a1[2:], 'both workspace sizes keep the stage-I weights at the same offsets'
    assert N.lib.rfn_prefix_alpha2(C.byref(d), 3, 0, ws) == N.lib.rfn_prefix_alpha2(C.byref(d), 3, 1, ws) > ws
    assert N.lib.rfn_decoder_alpha(C.byref(d), 6, 4, 0, 1, ws) == N.lib.rfn_decoder_alpha(C.byref(d), 6, 4, 1, 1, ws) > ws
    assert N.lib.rfn_prefix_alpha1(C.byref(d), 3, 0, 2, ws) is None and N.lib.rfn_prefix_alpha1(C.byref(d), 0, 0, 0, ws) is None
    assert N.lib.rfn_decoder_alpha(C.byref(d), 6, 4, 0, 4, ws) is None and N.lib.rfn_decoder_alpha(C.byref(d), 6, 4, 0, 1, None) is None
