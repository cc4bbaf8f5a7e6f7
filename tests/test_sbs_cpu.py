"""CPU: stochastic beam search (include/rfn.h "stochastic beam search"): the NumPy restatement (tests/sbs_cpu.py) against the
exact statistics of sampling without replacement on a model small enough to enumerate, its structural properties, the option
parse of sample_distinct, and the new entry points' bindings and refusals -- no kernel is launched."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import philox_cpu as P
import sbs_cpu as Sb
from test_native_abi import _OK_DIMS, header_symbols, native

TRIALS, W, S, SEED, OFFSET0 = 20000, 3, 3, 0x5B5C0FFEE, 11


@functools.lru_cache(maxsize=None)
def trials():
    """TRIALS images of the 4-token Markov model searched with W = 3, S = 3; the noise comes from philox_cpu through the
    restatement's counter layout, one call per step for all images.  -> list of Beams (with their weights attached)."""
    first, trans = Sb.markov_rows()
    V1 = Sb.MARKOV_V1
    e = [Sb.gumbels(SEED, OFFSET0 + t, np.arange(TRIALS * W), V1).reshape(TRIALS, W, V1) for t in range(1, S + 1)]
    g0 = Sb.gumbels(SEED, OFFSET0, np.arange(TRIALS) * W, V1)[:, 0]
    out = []
    for k in range(TRIALS):
        assert g0[k] == Sb.root_gumbel(SEED, OFFSET0, k, W, V1) or k >= 50
        b = Sb.Beams(W, S, g0[k])
        b.trace = []
        for t in range(1, S + 1):
            Sb.step(b, Sb.markov_x(first, trans, t, b), e[t - 1][k], t)
            b.trace.append((b.G.copy(), list(b.parents)))
        b.weight, b.n_live = Sb.weights(b)
        out.append(b)
    return out


def inclusion_probabilities(p, n):
    """P(caption i is among n draws without replacement), by enumerating the ordered n-tuples of distinct captions: the first is
    drawn with p_a, the next with p_b / (1 - p_a), and so on."""
    inc = np.zeros(p.size)
    for tup in itertools.permutations(range(p.size), n):
        pr, rest = 1.0, 1.0
        for i in tup:
            pr *= p[i] / rest
            rest -= p[i]
        inc[list(tup)] += pr
    return inc


def worst_z(counts, prob, n):
    """Largest |z| of binomial counts over the cells with expected count >= 25."""
    use = prob * n >= 25
    assert use.sum() >= 10
    z = (counts[use] - n * prob[use]) / np.sqrt(n * prob[use] * (1.0 - prob[use]))
    return float(np.abs(z).max())


def test_uniforms_are_the_documented_philox_stream():
    """The restatement's noise is word 0 of the stream philox_cpu documents: (n + 0.5) / 2^24 with n = 2^24 * uniforms()."""
    e = Sb.gumbels(SEED, 5, [0], 64)[0]
    u = P.uniforms(SEED, 5, 64).astype(np.float64) + 2.0 ** -25
    assert np.array_equal(e, -np.log(-np.log(u)))
    e2 = Sb.gumbels(SEED, 5, [3], 7)[0]                      # row 3 of a 7-token vocabulary: idx = 21 .. 27
    assert np.array_equal(e2, -np.log(-np.log(P.uniforms(SEED, 5, 28).astype(np.float64)[21:] + 2.0 ** -25)))
    assert np.isfinite(e).all()


def test_inclusion_probabilities_are_those_of_sampling_without_replacement():
    first, trans = Sb.markov_rows()
    caps, p = Sb.markov_captions(first, trans, S)
    assert len(caps) == 40
    inc = inclusion_probabilities(p, W)
    assert abs(inc.sum() - W) < 1e-9
    index = {c: i for i, c in enumerate(caps)}
    counts, row0 = np.zeros(len(caps)), np.zeros(len(caps))
    for b in trials():
        assert b.live.all()
        for j in range(W):
            counts[index[tuple(b.seq[j])]] += 1
        row0[index[tuple(b.seq[0])]] += 1
    z, z0 = worst_z(counts, inc, TRIALS), worst_z(row0, p, TRIALS)
    print('largest |z|: inclusion %.2f, row 0 %.2f' % (z, z0))
    assert z <= 5.0, z                                       # every caption with expected count >= 25 within 5 sigma
    assert z0 <= 5.0, z0                                     # row 0 is an ordinary sample of the model


def test_rows_are_distinct_and_ordered():
    for b in trials():
        assert len({tuple(r) for r in b.seq}) == W
        assert b.G[0] >= b.G[1] >= b.G[2]
        for G, _ in b.trace:
            assert (np.diff(G) <= 0).all()


def test_children_never_exceed_their_parent():
    seen_arg = seen_other = 0
    for b in trials()[:2000]:
        for G, parents in b.trace:
            for g, (gp, is_arg) in zip(G, parents):
                assert g <= gp
                if is_arg:
                    assert g == gp
                    seen_arg += 1
                else:
                    seen_other += 1
    assert seen_arg > 1000 and seen_other > 1000


def test_width_one_is_the_gumbel_max_trick_step_by_step():
    """W = 1: the search keeps, at every step, the token of largest x_v + e -- an ordinary ancestral sample drawn with the
    Gumbel-max trick from the same noise."""
    first, trans = Sb.markov_rows()
    V1 = Sb.MARKOV_V1
    for k in range(300):
        b = Sb.search(lambda t, bb: Sb.markov_x(first, trans, t, bb), 1, S, SEED, OFFSET0, k, V1)
        want, prev = [], None
        for t in range(1, S + 1):
            if prev == 0:
                want.append(0)
                continue
            row = first if prev is None else trans[prev]
            prev = int(np.argmax(row.astype(np.float64) + Sb.gumbels(SEED, OFFSET0 + t, [k], V1)[0]))
            want.append(prev)
        assert b.seq[0].tolist() == want, k
        assert b.G[0] == Sb.root_gumbel(SEED, OFFSET0, k, 1, V1) and Sb.weights(b)[0].tolist() == [0.0]


def test_fewer_candidates_than_rows_leaves_dead_rows():
    """Two tokens may be chosen and token 0 ends the caption: after step 1 an image has 2 live rows of its 4, after step 2 three
    (the finished one is carried, the other forks into two)."""
    x = np.full((4, 5), -Sb.INF, dtype=np.float32)
    x[:, 0], x[:, 3] = np.log(0.4), np.log(0.6)
    b = Sb.Beams(4, 2)
    Sb.step(b, x, Sb.gumbels(1, 1, np.arange(4), 5), 1)
    assert b.live.tolist() == [True, True, False, False] and sorted(b.seq[:2, 0].tolist()) == [0, 3]
    assert np.isneginf(b.phi[2:]).all() and np.isneginf(b.G[2:]).all() and not b.seq[2:].any() and not b.lp[2:].any()
    assert b.order[2:].tolist() == [2, 3] and not b.next_ids[2:].any()
    Sb.step(b, x, Sb.gumbels(1, 2, np.arange(4), 5), 2)
    assert b.live.tolist() == [True, True, True, False]
    assert sorted(tuple(r) for r in b.seq[:3].tolist()) == [(0, 0), (3, 0), (3, 3)]
    w, n = Sb.weights(b)
    assert n == 3 and w[2] == 0.0 and w[3] == 0.0 and (w[:2] > 0).all()
    assert 'dead' in b.events and 'fin_survives' in b.events
    # a NaN entry is never a candidate either
    x[0, 1] = np.nan
    tk, tv, ti, _ = Sb.row_list(x[0], Sb.gumbels(1, 3, [0], 5)[0], 4)
    assert sorted(ti[:2].tolist()) == [0, 3] and np.isneginf(tk[2:]).all() and np.isneginf(tv[2:]).all() and ti[2:].tolist() == [0, 0]


def test_weights_estimate_expectations():
    """The last live row weighs 0, and sum_i weight_i * 1 estimates 1: its mean over the images is within 5 standard errors.
    This holds because the root's G is a Gumbel(0) draw; with the constant 0 in its place the same 20 000 images give a mean of
    0.829 +- 0.002: the scores are then conditioned on their maximum, which the weights' q does not account for."""
    sums = []
    for b in trials():
        assert b.n_live == W and b.weight[W - 1] == 0.0 and (b.weight[:W - 1] > 0).all()
        sums.append(b.weight.sum())
    sums = np.array(sums)
    se = sums.std(ddof=1) / np.sqrt(sums.size)
    print('mean of sum of weights %.5f, standard error %.5f' % (sums.mean(), se))
    assert abs(sums.mean() - 1.0) <= 5.0 * se


def test_option_parse_refuses_every_other_key_by_name():
    from recurrent_fusion_network_amd.decode import _Stochastic
    ok = _Stochastic.parse({'seed': 2 ** 64 + 5, 'block_ngram': 2, 'banned_ids': [3], 'bad_endings': [4], 'temperature': 1.0}, 5, 16)
    assert ok.n == 5 and ok.seed == 5
    assert _Stochastic.parse({}, 32, 64).seed is None
    for key, val in (('temperature', 0.5), ('top_k', 3), ('top_p', 0.9), ('sample_n', 2), ('group_size', 2), ('diversity_lambda', 0.5),
                     ('require', [[[1]]]), ('consensus', object()), ('consensus_n', 3), ('length_penalty', 0.7), ('force_ids', None),
                     ('beam_size', 3), ('sample_max', 0), ('keep_candidates', True), ('no_such_key', 1)):
        with pytest.raises(ValueError, match=repr(key)):
            _Stochastic.parse({key: val}, 5, 16)
    for n in (0, 33, -1, 2.5, True):
        with pytest.raises(ValueError, match='captions per image'):
            _Stochastic.parse({}, n, 16)
    with pytest.raises(ValueError, match='seed'):
        _Stochastic.parse({'seed': 1.5}, 5, 16)
    with pytest.raises(native().RfnError):
        _Stochastic.parse({}, 5, 65)


def test_symbols_are_declared_exported_and_bound():
    N = native()
    names = ('rfn_log_softmax_topk_gumbel', 'rfn_beam_step_sbs', 'rfn_beam_loop_ex4', 'rfn_beam_sbs_begin')
    syms = header_symbols()
    for s in names:
        assert s in syms and s in N.EXPORTS and getattr(N.lib, s).argtypes is not None
    assert N.lib.rfn_abi_version() == 9 == N.ABI_VERSION
    assert C.sizeof(N.BeamStochastic) == 8 * 8 and N.BeamStochastic.phi.offset == 16 and N.BeamStochastic.topk64.offset == 56


def test_bad_calls_are_refused_before_any_launch():
    """Dummy addresses throughout: a refused call returns before it reads through any of them.  -1 RFN_ERR_SHAPE, -2
    RFN_ERR_UNSUPPORTED, -5 RFN_ERR_ARG."""
    N = native()
    A = 0x10000

    def topk(rows=6, V1=37, W=5, blk=None, blk_n=None, live=A, topk64=A, logits=A):
        return N.lib.rfn_log_softmax_topk_gumbel(logits, V1, rows, V1, W, blk, 70, blk_n, live, 1, 2, topk64, A, A, None)
    assert topk(rows=0) == -1 and topk(V1=0) == -1 and topk(W=0) == -1 and topk(W=33) == -1
    assert topk(live=None) == -5 and topk(topk64=None) == -5 and topk(logits=None) == -5 and topk(blk=A) == -5
    assert topk(W=33, live=None) == -1                       # the shape first, as rfn_log_softmax_topk_masked
    assert topk(V1=48 * 1024 * 8 + 1, blk=A, blk_n=A) == -1  # one bit per token in LDS

    def step(W=5, S=4, t=1, NB=2, V1=37, phi=A, weight=A):
        return N.lib.rfn_beam_step_sbs(A, A, A, V1, W, S, t, NB, A, A, phi, A, A, A, A, weight, A, None)
    assert step(W=0) == -1 and step(W=33) == -1 and step(S=65) == -1 and step(t=0) == -1 and step(t=5) == -1 and step(NB=0) == -1
    assert step(phi=None) == -5 and step(weight=None) == -5 and step(W=33, phi=None) == -1

    begin = lambda NB=2, W=5, V1=37, phi=A: N.lib.rfn_beam_sbs_begin(NB, W, V1, 1, 2, phi, A, A, None)  # noqa: E731
    assert begin(NB=0) == -1 and begin(W=0) == -1 and begin(W=33) == -1 and begin(V1=0) == -1 and begin(phi=None) == -5

    d = N.make_dims(**_OK_DIMS)
    B, Wb, Sq = 3, 2, 4
    size = N.lib.rfn_decoder_step_ws_bytes(C.byref(d), B * Wb)

    def loop(sbs, div=None, lex=None, S=Sq, beam_seq=A):
        return N.lib.rfn_beam_loop_ex4(C.byref(d), B, Wb, S, A, A, A, A, A, A, A, A, beam_seq, A, None, A, A, None, None, None, None,
                                       None, Wb * S, A, size, 0, None, div, lex, sbs, None)
    full = dict(seed=1, offset0=0, phi=A, gumbel=A, live=A, weight=A, n_live=A, topk64=A)
    for member in ('phi', 'gumbel', 'live', 'weight', 'n_live', 'topk64'):
        assert loop(C.byref(N.BeamStochastic(**dict(full, **{member: None})))) == -5, member
    sbs = C.byref(N.BeamStochastic(**full))
    assert loop(sbs, beam_seq=None) == -5
    assert loop(sbs, S=0) == -1 and loop(sbs, S=65) == -1
    assert loop(sbs, div=C.byref(N.BeamDiversity(2, 0.5, A))) == -2
    assert loop(sbs, lex=C.byref(N.BeamLexical(1, 1, A, A, A, A, A, A))) == -2
    assert loop(sbs, div=C.byref(N.BeamDiversity(3, 0.5, A))) == -1        # the diversity's own shape check still comes first
