"""CPU: lexically constrained beam search (include/rfn.h "lexically constrained beam search").  The NumPy restatement
(tests/lexical_beam_cpu.py) against an exhaustive enumeration at tiny sizes and against the plain search it degenerates to; the
host's parse of opt['require']; the ABI; and, on the restatement alone, the conditions that keep the GPU step test
(tests/test_lexical_beam_gpu.py) from passing vacuously -- over exactly the inputs that test uses."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import diverse_beam_cpu as Dv
import lexical_beam_cpu as Lx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# =================================================================================================================
# the definition against an enumeration
# =================================================================================================================
def _prefix_table(seed, V1, S):
    """A log-prob row for every prefix of fewer than S tokens: continuous draws, so no two sequences tie."""
    rng = np.random.default_rng(seed)
    table = {}
    for n in range(S):
        for pre in itertools.product(range(V1), repeat=n):
            x = 2.0 * rng.standard_normal(V1)
            table[pre] = (x - np.log(np.exp(x).sum())).astype(np.float32)
    return table


def _enumerate_best(table, V1, S, sets):
    """The argmax over all END-terminated or full-length sequences of (sets satisfied, p), p summed in fp32 in token order."""
    best = None
    for n in range(1, S + 1):
        for seq in itertools.product(range(V1), repeat=n):
            if 0 in seq[:-1] or (n < S and seq[-1] != 0):
                continue
            p = F(0.0)
            for i, v in enumerate(seq):
                p = F(p + table[seq[:i]][v])
            met = sum(1 for ids in sets if not ids or set(ids) & set(seq))
            key = (met, float(p))
            if best is None or key > best[0]:
                best = (key, seq)
    return best


@pytest.mark.parametrize('C_', [1, 2])
def test_wide_beam_returns_the_enumerations_argmax(C_):
    """V1 = 4, S = 3: with a beam that holds every prefix (Wb = 64 >= 4^3) nothing is ever pruned, so the restatement's best done
    beam is the enumeration's argmax -- this pins the definition independently of any kernel."""
    V1, S, Wb = 4, 3, 64
    configs = {1: [[[2]], [[1, 3]], [[]]], 2: [[[1], [2]], [[3], [3, 1]], [[2], []], [[1, 2], [2, 3]]]}[C_]
    for n, sets in enumerate(configs):
        for seed in range(6):
            table = _prefix_table(100 * n + seed, V1, S)
            want, bits, init = Lx.parse_sets(sets, C_)

            def rows(t, b):
                out = np.zeros((b.W, V1), dtype=np.float32)
                for q in b.occupied() if t else range(b.W):
                    out[q] = table[tuple(int(x) for x in b.seq[:t, q])]
                return out

            b = Lx.search(rows, Wb, C_, S, want, bits, init)
            top = b.done[Lx.rank_done(b.done, S)[0]]
            (met, p), seq = _enumerate_best(table, V1, S, sets)
            got = [int(x) for x in top['seq']]
            assert got[:len(seq)] == list(seq) and not any(got[len(seq):]), (sets, seed, got, seq)
            assert Lx.popcount(top['state']) == met and float(top['p']) == p, (sets, seed)


# =================================================================================================================
# agreement with the existing searches
# =================================================================================================================
def _same_beams(a, b, rows_a, rows_b):
    assert a.seq[:, rows_a].tolist() == b.seq[:, rows_b].tolist()
    assert a.lp[:, rows_a].view(np.int32).tolist() == b.lp[:, rows_b].view(np.int32).tolist()
    assert a.sum[rows_a].view(np.int32).tolist() == b.sum[rows_b].view(np.int32).tolist()
    assert (a.order[rows_a] - rows_a[0]).tolist() == (b.order[rows_b] - rows_b[0]).tolist()
    assert a.next_ids[rows_a].tolist() == b.next_ids[rows_b].tolist() and a.active == b.active


def _same_done(a, b):
    key = lambda d: (d['seq'].tolist(), d['logps'].view(np.int32).tolist(), np.float32(d['p']).tobytes())  # noqa: E731
    assert [key(d) for d in a.done] == [key(d) for d in b.done]


@pytest.mark.parametrize('Wb', [1, 3, 8])
def test_no_sets_is_the_plain_search(Wb):
    """C = 0: one state.  On rows without -inf and with V1 >= W the plain search never has fewer candidates than beams while a
    row is live, so neither departure (no stale rows, -inf dropped) can show: every array agrees after every step."""
    for S, V1 in ((1, 37), (4, 8), (17, 37)):
        rows = Dv.synthetic_rows(31 * Wb + S + V1, 2, Wb, S, V1)
        for k in range(2):
            a, b = Lx.LexBeams(Wb, 0, S), Dv.Beams(Wb, S)
            for t in range(1, S + 1):
                Lx.step(a, rows[t - 1][k], t, [], [])
                Dv.step(b, rows[t - 1][k], t)
                _same_beams(a, b, np.arange(Wb), np.arange(Wb))
            _same_done(a, b)


@pytest.mark.parametrize('C_', [1, 2, 3])
def test_all_sets_empty_is_the_plain_search_in_the_accepting_state(C_):
    for Wb, S, V1 in ((1, 4, 37), (3, 17, 37), (4, 4, 8)):
        G = 1 << C_
        rows = Dv.synthetic_rows(17 * Wb + S + C_, 1, G * Wb, S, V1)
        mine = np.arange((G - 1) * Wb, G * Wb)
        a, b = Lx.LexBeams(Wb, C_, S, G - 1), Dv.Beams(Wb, S)
        for t in range(1, S + 1):
            Lx.step(a, rows[t - 1][0], t, [], [])
            Dv.step(b, rows[t - 1][0][mine], t)
            _same_beams(a, b, mine, np.arange(Wb))
            assert a.state_n[:G - 1].sum() == 0
            assert a.order[:mine[0]].tolist() == list(range(mine[0])) and not a.next_ids[:mine[0]].any()
        _same_done(a, b)
        assert all(d['state'] == G - 1 for d in a.done)


# =================================================================================================================
# the host's parse
# =================================================================================================================
def _lexical():
    from recurrent_fusion_network_amd.decode import _Lexical
    return _Lexical


def test_parser_builds_want_bits_and_init_state():
    L = _lexical()
    req = [[[5, 6, 5], [7]], [[9]], [[4, 8], [8, 3]], [[], [2]]]       # dedup; ragged; id 8 in two sets; an empty first set
    lx = L.parse({'require': req}, 4, 50, 4)
    assert (lx.C, lx.G, lx.Wb, lx.W, lx.NW) == (2, 4, 4, 16, 3)
    assert lx.want == [[5, 6, 7], [9, -1, -1], [4, 8, 3], [2, -1, -1]]
    assert lx.want_bits == [[1, 1, 2], [1, 0, 0], [1, 3, 2], [2, 0, 0]]
    assert lx.init_state == [0, 2, 0, 1]
    for img, w, m, i0 in zip(req, lx.want, lx.want_bits, lx.init_state):   # the restatement's parse agrees
        want, bits, init = Lx.parse_sets(img, 2)
        assert (want, bits, init) == ([v for v in w if v >= 0], m[:len(want)], i0)
    t = torch.full((4, 2, 3), -1, dtype=torch.long)                     # the same sets as a padded tensor
    for k, img in enumerate(req):
        for i, ids in enumerate(img):
            t[k, i, :len(ids)] = torch.tensor(ids, dtype=torch.long)
    lt = L.parse({'require': t}, 4, 50, 4)
    assert (lt.want, lt.want_bits, lt.init_state) == (lx.want, lx.want_bits, lx.init_state)


def test_parser_returns_none_without_a_non_empty_set():
    L = _lexical()
    assert L.parse({}, 2, 50, 3) is None and L.parse({'require': None}, 2, 50, 3) is None
    assert L.parse({'require': [[], []]}, 2, 50, 3) is None and L.parse({'require': [[[]], [[], []]]}, 2, 50, 3) is None
    assert L.parse({'require': torch.full((2, 3, 4), -1, dtype=torch.int32)}, 2, 50, 3) is None


def test_parser_refusals():
    L = _lexical()
    V1 = 50
    bad = [([[[1], [2], [3], [4]]], 1),                                # C > 3
           ([[list(range(1, 18))]], 16),                               # more than 16 unique ids
           ([[[0]]], 2), ([[[V1]]], 2), ([[[-3]]], 2),                 # ids outside [1, V1)
           ([[[1, 2, 3]]], 2),                                         # NW = 3 > W - Wb = 2
           ([[[1], [2]]], 9),                                          # W = 36 > 32
           ([[[1]], [[2]]], 2)]                                        # two images' sets for a batch of one
    for req, Wb in bad:
        with pytest.raises(ValueError):
            L.parse({'require': req}, 1, V1, Wb)
    with pytest.raises(ValueError):
        L.parse({'require': torch.zeros(1, 2)}, 1, V1, 2)
    assert L.parse({'require': [[list(range(1, 17))]]}, 1, V1, 16).NW == 16      # the limits themselves pass
    assert L.parse({'require': [[[1, 2]]]}, 1, V1, 2).NW == 2


# =================================================================================================================
# ABI
# =================================================================================================================
def test_abi_declares_and_exports_the_new_symbols():
    import recurrent_fusion_network_amd._native as N
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rfn.h')).read(), flags=re.S)
    for name in ('rfn_log_softmax_topk_want', 'rfn_beam_step_lex', 'rfn_beam_loop_ex3'):
        assert re.search(r'\b%s\s*\(' % name, src), name
        assert hasattr(N.lib, name) and name in N.EXPORTS, name
    assert 'rfn_beam_lexical' in src and C.sizeof(N.BeamLexical) == 2 * 4 + 6 * 8
    assert re.search(r'#define\s+RFN_LEX_MAX_SETS\s+3\b', src) and re.search(r'#define\s+RFN_LEX_MAX_IDS\s+16\b', src)
    assert (N.LEX_MAX_SETS, N.LEX_MAX_IDS) == (3, 16)
    assert N.lib.rfn_abi_version() == 9 == N.ABI_VERSION


def test_step_refuses_bad_shapes_before_launching():
    """Every refused shape returns RFN_ERR_SHAPE before any pointer is read (no GPU needed)."""
    import recurrent_fusion_network_amd._native as N
    P = C.c_void_p(0x10000)

    def call(NW, C_, W, S, t=1):
        return N.lib.rfn_beam_step_lex(P, P, P, P, P, NW, C_, 37, W, S, t, 1, W * S, *([P] * 13), None)

    assert call(1, 4, 16, 4) == -1 and call(1, -1, 16, 4) == -1         # C
    assert call(1, 2, 6, 4) == -1 and call(1, 3, 12, 4) == -1           # W % 2^C
    assert call(-1, 1, 8, 4) == -1 and call(17, 1, 32, 4) == -1         # NW
    assert call(5, 1, 8, 4) == -1 and call(13, 2, 16, 4) == -1          # NW > W - Wb
    assert call(1, 1, 34, 4) == -1 and call(1, 1, 8, 65) == -1          # W, S
    assert N.lib.rfn_log_softmax_topk_want(P, 37, 1, 37, 4, 1, P, 17, 17, None, 0, None, P, P, P, None) == -1
    assert N.lib.rfn_log_softmax_topk_want(P, 37, 1, 37, 4, 1, P, 1, 2, None, 0, None, P, P, P, None) == -1


# =================================================================================================================
# non-vacuity of the GPU step test, on the restatement alone
# =================================================================================================================
@pytest.mark.parametrize('Wb,C_', Lx.SHAPES)
def test_step_cases_exercise_the_new_ground(Wb, C_):
    """Over exactly the cases the GPU step test runs for this shape: (a) some selected move candidate's token lies outside its
    row's W-wide top list -- only the want values can have brought it in; (b) some image has an empty state beside an occupied one
    after step 2; (c) some image ends with a done beam in the accepting state and some image with none, so the fallback ordering is
    exercised; (d) some image's returned caption differs from the unconstrained search's (the plain search of width Wb on the same
    rows)."""
    G, W = 1 << C_, Wb << C_
    outside = beside = accepting = none_accepting = differs = 0
    for NB, S, V1, NW, sets, rows in Lx.step_cases(Wb, C_):
        ref = Lx.run_case(Wb, C_, NB, S, sets, rows)
        for k, b in enumerate(ref):
            outside += b.moves_outside
            if S >= 2:
                n2 = b.occupancy[1]
                beside += bool((n2 == 0).any() and (n2 > 0).any())
            has = any(d['state'] == G - 1 for d in b.done)
            accepting += has
            none_accepting += not has
            plain = Dv.Beams(Wb, S)
            for t in range(1, S + 1):
                Dv.step(plain, rows[t - 1][k][:Wb], t)
            mine = b.done[Lx.rank_done(b.done, S)[0]]['seq'].tolist()
            theirs = plain.done[sorted(range(len(plain.done)), key=lambda i: -float(plain.done[i]['p']))[0]]['seq'].tolist()
            differs += mine != theirs
    assert outside > 0, 'no selected move candidate from outside the top lists'
    assert beside > 0, 'no image with an empty state beside an occupied one after step 2'
    assert accepting > 0 and none_accepting > 0, (accepting, none_accepting)
    assert differs > 0
