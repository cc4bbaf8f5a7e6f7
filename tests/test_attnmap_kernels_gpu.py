"""GPU: rfn_attn_rollout / rfn_attn_map_stats / rfn_attn_decoder_copy (rfn.h "attention maps") through the ctypes binding, on
random row-stochastic inputs against the fp64 nested sums of tests/attention_maps_cpu.py.

Shapes are the smallest at which the kernels change path: L around the 64-column (scalar) and 256-column (16-B) tiles and off the
4-float vector path, a mis-aligned base on an L % 4 == 0 map, one and several steps / review steps, 1 and 3 rows per image, dead
rows and steps, ragged maps, a non-compact output.

Tolerance of the rollout: absolute 4 * (T1 + T2) * 2^-24.  Every term is non-negative, every value <= 1 and the sums run in a
fixed order, so the f32 error of the nested dot products is bounded by about (T1 + T2 + 3) units of 2^-24; the factor 4 is margin."""
import numpy as np
import pytest
import torch

from attention_maps_cpu import rollout_np, stats_np

pytestmark = pytest.mark.gpu

LS = [1, 3, 4, 63, 64, 65, 196, 260]
TS = [(1, 1), (3, 4), (8, 8)]
SS = [1, 6, 17]
NS = [1, 3]
B = 2
SHAPE, UNSUPPORTED, ARG = -1, -2, -5


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def stochastic(rng, *shape, spike=False):
    """Rows (last axis) that sum to 1 in fp64, rounded to f32; `spike`: one entry per row stands out, so the argmax is not a tie."""
    x = rng.random(shape)
    if spike and shape[-1] > 1:
        j = rng.integers(0, shape[-1], size=shape[:-1])
        np.put_along_axis(x, j[..., None], np.take_along_axis(x, j[..., None], -1) + 1.0, -1)
    return (x / x.sum(-1, keepdims=True)).astype(np.float32)


def misaligned(t):
    """A copy of `t` whose base address is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


def rollout(N, aD, a2, a1, length, att_len, n, out, o_sr, o_ss):
    """aD (S, rows, T2), a2 (T2, B, T1), a1 (T1, B, L) device tensors in the workspaces' layouts."""
    S, rows, T2 = aD.shape
    T1, Bn, L = a1.shape
    return N.lib.rfn_attn_rollout(aD.data_ptr(), rows * T2, T2, a2.data_ptr(), Bn * T1, T1, a1.data_ptr(), Bn * L, L, N.ptr(length),
                                  N.ptr(att_len), rows, n, S, T1, T2, L, out.data_ptr(), o_sr, o_ss, N.stream_ptr())


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('L', LS)
def test_rollout_against_fp64_nested_sums(dev, L):
    N = native()
    rng = np.random.default_rng(100 + L)
    seen_len, seen_att, case = set(), set(), 0
    for (T1, T2) in TS:
        for S in SS:
            for n in NS:
                rows = B * n
                aD, a2, a1 = stochastic(rng, rows, S, T2), stochastic(rng, B, T2, T1), stochastic(rng, B, T1, L)
                lens = [[0, 1, S][(r + case) % 3] for r in range(rows)]
                alen = [(1, L), (max(1, L - 1), L), (L, 1)][case % 3]
                variant = case % 4          # 0: compact, lengths given; 1: non-compact; 2: mis-aligned a1; 3: no lengths at all
                if variant == 3:
                    lens, alen = None, None
                seen_len.update(lens or [])
                seen_att.update(alen or [])
                want = rollout_np(aD, a2, a1, n, lens, alen)
                tol = 4 * (T1 + T2) * 2.0 ** -24
                d_aD = torch.from_numpy(aD).to(dev).permute(1, 0, 2).contiguous()
                d_a2 = torch.from_numpy(a2).to(dev).permute(1, 0, 2).contiguous()
                d_a1 = torch.from_numpy(a1).to(dev).permute(1, 0, 2).contiguous()
                if variant == 2:
                    d_a1 = misaligned(d_a1)
                d_len = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
                d_alen = None if alen is None else torch.tensor(alen, dtype=torch.int32, device=dev)
                o_ss = L + 4 if variant == 1 else L
                o_sr = S * o_ss + (8 if variant == 1 else 0)
                runs = []
                for _ in range(2):
                    buf = torch.full((rows * o_sr,), float('nan'), device=dev)
                    assert rollout(N, d_aD, d_a2, d_a1, d_len, d_alen, n, buf, o_sr, o_ss) == 0
                    runs.append(buf)
                assert torch.equal(bits(runs[0]), bits(runs[1])), 'two runs differ'
                got = torch.as_strided(runs[0], (rows, S, L), (o_sr, o_ss, 1))
                written = torch.zeros(rows * o_sr, dtype=torch.bool, device=dev)
                torch.as_strided(written, (rows, S, L), (o_sr, o_ss, 1)).fill_(True)
                assert bool(torch.isnan(runs[0][~written]).all()), 'the kernel wrote between the rows of a non-compact output'
                assert not bool(torch.isnan(got).any())
                err = float(np.abs(got.double().cpu().numpy() - want).max())
                assert err <= tol, (L, T1, T2, S, n, variant, err, tol)
                zero = torch.from_numpy(want == 0).to(dev) if lens is not None else None
                if zero is not None:        # dead steps and ragged columns: fp64 zeros there are structural (the inputs are > 0)
                    dead = np.zeros(want.shape, dtype=bool)
                    dead[np.arange(S)[None, :] >= np.asarray(lens)[:, None]] = True
                    dead |= (np.arange(L)[None, :] >= np.repeat(alen, n)[:, None])[:, None, :]
                    assert np.array_equal(dead, want == 0)
                    assert bool((bits(got)[zero] == 0).all()), 'dead steps / ragged columns are not bit-zero'
                case += 1
    assert seen_len >= {0, 1} and seen_att >= {1, L, max(1, L - 1)}


def test_rollout_wide_t2_takes_the_64_column_tile(dev):
    """T2 = 64 (the model's limit): the 256-column tile of the 16-byte form needs more than 64 KiB of LDS, the map runs on the
    element-wise form instead of being refused."""
    N = native()
    rng = np.random.default_rng(11)
    rows, S, T1, T2, L = 2, 2, 2, 64, 8
    aD, a2, a1 = stochastic(rng, rows, S, T2), stochastic(rng, rows, T2, T1), stochastic(rng, rows, T1, L)
    want = rollout_np(aD, a2, a1)
    dD, d2, d1 = (torch.from_numpy(x).to(dev).permute(1, 0, 2).contiguous() for x in (aD, a2, a1))
    out = torch.full((rows, S, L), float('nan'), device=dev)
    assert out.data_ptr() % 16 == 0 and d1.data_ptr() % 16 == 0
    assert rollout(N, dD, d2, d1, None, None, 1, out, S * L, L) == 0
    assert float(np.abs(out.double().cpu().numpy() - want).max()) <= 4 * (T1 + T2) * 2.0 ** -24


def test_map_stats_against_fp64(dev):
    N = native()
    rng = np.random.default_rng(7)
    ents, near, pairs = [], 0, 0
    for L in LS:
        for S in SS:
            rows = 6
            G = stochastic(rng, rows, S, L, spike=True)
            lens = [[0, 1, S][(r + L + S) % 3] for r in range(rows)]
            mask = (rng.random((rows, S, L)) < 0.4).astype(np.uint8)
            peak_w, gap, ent_w, mass_w = stats_np(G, lens, mask)
            g_ss, g_sr = L + 3, S * (L + 3) + 5                    # a non-compact map
            buf = torch.zeros(rows * g_sr, device=dev)
            torch.as_strided(buf, (rows, S, L), (g_sr, g_ss, 1)).copy_(torch.from_numpy(G).to(dev))
            d_mask, d_len = torch.from_numpy(mask).to(dev), torch.tensor(lens, dtype=torch.int32, device=dev)
            peak = torch.full((rows, S), -7, dtype=torch.int32, device=dev)
            ent, mass = torch.full((rows, S), float('nan'), device=dev), torch.full((rows, S), float('nan'), device=dev)
            assert N.lib.rfn_attn_map_stats(buf.data_ptr(), g_sr, g_ss, d_len.data_ptr(), d_mask.data_ptr(), S * L, L, rows, S, L,
                                            peak.data_ptr(), ent.data_ptr(), mass.data_ptr(), N.stream_ptr()) == 0
            live = np.arange(S)[None, :] < np.asarray(lens)[:, None]
            tol = 4 * (8 + 8) * 2.0 ** -24                          # the widest rollout tolerance: what "a tie" means for a map
            tie = live & (gap < tol)
            near, pairs = near + int(tie.sum()), pairs + int(live.sum())
            got_peak = peak.cpu().numpy()
            assert np.array_equal(got_peak[~tie], peak_w[~tie]), (L, S)
            assert (got_peak[~live] == -1).all()
            assert np.abs(ent.cpu().numpy().astype(np.float64) - ent_w).max() <= 1e-5, (L, S)
            assert np.abs(mass.cpu().numpy().astype(np.float64) - mass_w).max() <= 1e-5, (L, S)
            assert not ent.cpu().numpy()[~live].any() and not mass.cpu().numpy()[~live].any()
            ents.append(ent_w[live])
            # no mask: mass is left alone
            mass2 = torch.full((rows, S), 3.0, device=dev)
            assert N.lib.rfn_attn_map_stats(buf.data_ptr(), g_sr, g_ss, None, None, 0, 0, rows, S, L, peak.data_ptr(), ent.data_ptr(),
                                            mass2.data_ptr(), N.stream_ptr()) == 0
            assert bool((mass2 == 3.0).all()) and bool((peak >= 0).all())
    assert near <= 0.01 * pairs, (near, pairs)                       # the inputs are built so that the exception is rare
    assert float(np.concatenate(ents).mean()) > 0.5                  # the entropy check is not vacuous


def test_first_argmax_on_exact_ties(dev):
    N = native()
    G = torch.zeros(1, 2, 130, device=dev)
    G[0, 0, [5, 70, 129]] = 1.0 / 3
    G[0, 1, [64, 65]] = 0.5
    peak = torch.empty(1, 2, dtype=torch.int32, device=dev)
    ent = torch.empty(1, 2, device=dev)
    assert N.lib.rfn_attn_map_stats(G.data_ptr(), 260, 130, None, None, 0, 0, 1, 2, 130, peak.data_ptr(), ent.data_ptr(), None,
                                    N.stream_ptr()) == 0
    assert peak.cpu().tolist() == [[5, 64]]
    assert np.allclose(ent.cpu().numpy(), [[np.log(3), np.log(2)]], atol=1e-6)


def test_decoder_copy(dev):
    N = native()
    rng = np.random.default_rng(3)
    rows, S, T2 = 5, 6, 4
    aD = torch.from_numpy(stochastic(rng, S, rows, T2)).to(dev)
    lens = [0, 1, 6, 3, 9]                                          # 9: clamped to S
    d_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.full((rows, S, T2 + 2), float('nan'), device=dev)
    assert N.lib.rfn_attn_decoder_copy(aD.data_ptr(), rows * T2, T2, d_len.data_ptr(), rows, S, T2, out.data_ptr(), S * (T2 + 2), T2 + 2,
                                       N.stream_ptr()) == 0
    want = aD.permute(1, 0, 2).clone()
    for r, n in enumerate(lens):
        want[r, n:] = 0
    assert torch.equal(bits(out[:, :, :T2]), bits(want)) and bool(torch.isnan(out[:, :, T2:]).all())
    assert N.lib.rfn_attn_decoder_copy(aD.data_ptr(), rows * T2, T2, None, rows, S, T2, out.data_ptr(), S * (T2 + 2), T2 + 2,
                                       N.stream_ptr()) == 0
    assert torch.equal(out[:, :, :T2], aD.permute(1, 0, 2))
    assert N.lib.rfn_attn_decoder_copy(aD.data_ptr(), rows * T2, T2, None, 0, S, T2, out.data_ptr(), S * T2, T2, N.stream_ptr()) == SHAPE
    assert N.lib.rfn_attn_decoder_copy(aD.data_ptr(), rows * T2, T2, None, rows, S, T2, out.data_ptr(), S * T2, T2 - 1, N.stream_ptr()) == SHAPE
    assert N.lib.rfn_attn_decoder_copy(None, rows * T2, T2, None, rows, S, T2, out.data_ptr(), S * T2, T2, N.stream_ptr()) == ARG


def test_refusals_return_their_code_without_launching(dev):
    N = native()
    rows, n, S, T1, T2, L = 6, 3, 4, 3, 2, 8
    aD, a2, a1 = torch.rand(S, rows, T2, device=dev), torch.rand(T2, 2, T1, device=dev), torch.rand(T1, 2, L, device=dev)
    out = torch.full((rows, S, L), 7.0, device=dev)
    st = N.stream_ptr()

    def call(**kw):
        a = dict(aD=aD.data_ptr(), a2=a2.data_ptr(), a1=a1.data_ptr(), out=out.data_ptr(), rows=rows, n=n, S=S, T1=T1, T2=T2, L=L,
                 o_sr=S * L, o_ss=L)
        a.update(kw)
        return N.lib.rfn_attn_rollout(a['aD'], rows * max(a['T2'], 1), max(a['T2'], 1), a['a2'], 2 * max(a['T1'], 1), max(a['T1'], 1),
                                      a['a1'], 2 * max(a['L'], 1), max(a['L'], 1), None, None, a['rows'], a['n'],
                                      a['S'], a['T1'], a['T2'], a['L'], a['out'], a['o_sr'], a['o_ss'], st)

    for bad in (dict(rows=0), dict(n=0), dict(S=0), dict(T1=0), dict(T2=0), dict(L=0), dict(rows=5), dict(o_ss=L - 1), dict(o_sr=L - 1),
                dict(rows=0, aD=None), dict(L=0, out=None)):       # the last two: a shape defect wins over a NULL pointer
        assert call(**bad) == SHAPE, bad
    for bad in (dict(aD=None), dict(a2=None), dict(a1=None), dict(out=None)):
        assert call(**bad) == ARG, bad
    # the LDS limit (rfn.h): (S * T2 + T2 * T1 + T2 * 64) floats <= 64 KiB even on the 64-column tile, else RFN_ERR_UNSUPPORTED
    assert call(T2=1024, S=17) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), 'a refused call wrote its output'
    G, peak, ent = torch.rand(rows, S, L, device=dev), torch.empty(rows, S, dtype=torch.int32, device=dev), torch.empty(rows, S, device=dev)
    m = torch.ones(rows, S, L, dtype=torch.uint8, device=dev)

    def stats(G_=G, rows_=rows, S_=S, L_=L, g_ss=L, m_=None, peak_=peak, ent_=ent, mass_=None):
        return N.lib.rfn_attn_map_stats(N.ptr(G_), S * L, g_ss, None, N.ptr(m_), S * L, L, rows_, S_, L_, N.ptr(peak_), N.ptr(ent_),
                                        N.ptr(mass_), st)

    assert stats(rows_=0) == SHAPE and stats(S_=0) == SHAPE and stats(L_=0) == SHAPE and stats(g_ss=L - 1) == SHAPE
    assert stats(rows_=0, G_=None) == SHAPE
    assert stats(G_=None) == ARG and stats(peak_=None) == ARG and stats(ent_=None) == ARG and stats(m_=m) == ARG
