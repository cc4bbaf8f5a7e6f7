"""CPU: the caption-scoring restatement (tests/score_cpu.py) on hand-worked rows, the option parse of score(), and the host side
of the new entry points (rfn_score_logits, rfn_score_captions, rfn_decoder_score_ws_bytes, rfn_decoder_score): declared, exported,
bound, and refusing bad calls before anything is launched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import score_cpu as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('rfn_score_logits', 'rfn_score_captions', 'rfn_decoder_score_ws_bytes', 'rfn_decoder_score')
OK_DIMS = dict(M=2, R=16, A=16, E=16, T1=3, T2=3, K=20, V1=51, L=[5, 7], D=[24, 40], Fc=[24, 32])
SHAPE, UNSUPPORTED, WORKSPACE, ARG = -1, -2, -4, -5
LN2 = math.log(2.0)


# ---- the restatement, by hand ---------------------------------------------------------------------------------------------
# one row: logits (ln 1, ln 2, ln 1, -inf) = probabilities (1/4, 1/2, 1/4, 0), log-sum-exp ln 4, entropy 1.5 ln 2
ROW = np.array([0.0, LN2, 0.0, -np.inf])


def _one_row(tg, include_end=True):
    lp, rank, ent = SC.score_logits(ROW.reshape(1, 1, 4), np.array([[tg]]), include_end)
    return lp[0, 0], rank[0, 0], ent[0, 0]


def test_a_tie_ranks_the_lower_id_first():
    lp0, r0, e0 = _one_row(0)            # token 0 is the END: live with include_end
    lp2, r2, e2 = _one_row(2)
    assert abs(lp0 + 2 * LN2) < 1e-15 and abs(lp2 + 2 * LN2) < 1e-15
    assert r0 == 1                        # behind token 1 only: the equal token 2 has the higher id
    assert r2 == 2                        # behind token 1 and the equal token 0
    assert _one_row(1)[1] == 0            # the argmax
    assert abs(e0 - 1.5 * LN2) < 1e-15 and e0 == e2


def test_a_minus_inf_entry_counts_zero_in_the_entropy_and_scores_minus_inf_as_a_target():
    lp, rank, ent = _one_row(3)
    assert lp == -np.inf and rank == 3 and abs(ent - 1.5 * LN2) < 1e-15 and np.isfinite(ent)
    # two -inf entries: the tie rule holds among them too
    row = np.array([-np.inf, 0.0, -np.inf]).reshape(1, 1, 3)
    _, rank, ent = SC.score_logits(row, np.array([[2]]), True)
    assert rank[0, 0] == 2 and ent[0, 0] == 0.0


def test_a_nan_row_is_nan_and_counts_only_true_comparisons():
    x = np.zeros((1, 2, 4))
    x[0, 0] = [1.0, np.nan, 3.0, 2.0]
    x[0, 1] = ROW
    lp, rank, ent = SC.score_logits(x, np.array([[3], [1]]), True)
    assert np.isnan(lp[0, 0]) and np.isnan(ent[0, 0]) and rank[0, 0] == 1          # only 3.0 > 2.0 is true
    assert abs(lp[1, 0] + LN2) < 1e-15 and rank[1, 0] == 0


# captions: empty; never ending; garbage after the first 0; ids out of range (read as 0)
TARGET = np.array([[0, 0, 0], [1, 2, 1], [2, 0, 3], [1, -7, 2], [1, 4, 2]])


def test_the_live_rule_on_hand_worked_captions():
    with_end = SC.live_mask(TARGET, 4, True)
    assert with_end.tolist() == [[True, False, False], [True, True, True], [True, True, False], [True, True, False],
                                 [True, True, False]]
    words = SC.live_mask(TARGET, 4, False)
    assert words.tolist() == [[False, False, False], [True, True, True], [True, False, False], [True, False, False],
                              [True, False, False]]
    assert SC.live_mask(TARGET, 5, False)[4].tolist() == [True, True, True]       # 4 is a word once the vocabulary holds it


def test_dead_positions_and_caption_sums():
    x = np.broadcast_to(ROW, (3, 5, 4))
    lp, rank, ent = SC.score_logits(x, TARGET, True)
    assert lp[0].tolist() == [lp[0, 0], 0.0, 0.0] and rank[0].tolist() == [1, -1, -1] and ent[0, 1] == 0.0 == ent[0, 2]
    assert rank[1].tolist() == [0, 2, 0] and rank[2].tolist() == [2, 1, -1]
    assert rank[3].tolist() == [0, 1, -1]                                          # -7 is scored as token 0
    lp32 = lp.astype(np.float32)
    cap, n = SC.score_captions(lp32, TARGET, 4, True)
    assert n.tolist() == [1, 3, 2, 2, 2]
    assert cap[1] == (np.float64(lp32[1, 0]) + np.float64(lp32[1, 1])) + np.float64(lp32[1, 2])
    cap0, n0 = SC.score_captions(lp32, TARGET, 4, False)
    assert n0.tolist() == [0, 3, 1, 1, 1] and cap0[0] == 0.0 and cap0[2] == np.float64(lp32[2, 0])
    # the order is ascending from 0.0: (0 + 1e8) + -1e8 + 1 = 1, not 0
    t = np.array([[1, 1, 1]])
    assert SC.score_captions(np.array([[1e8, -1e8, 1.0]], dtype=np.float32), t, 4, True)[0][0] == 1.0
    assert SC.score_captions(np.array([[1.0, 1e8, -1e8]], dtype=np.float32), t, 4, True)[0][0] == 1.0   # exact in fp64


# ---- the option parse ----------------------------------------------------------------------------------------------------
def test_score_options_parse_and_refuse():
    from recurrent_fusion_network_amd.decode import _Scoring
    s = _Scoring.parse({})
    assert (s.n, s.alpha, s.rank, s.entropy, s.include_end, s.max_rows) == (None, 0.0, False, False, True, None)
    s = _Scoring.parse({'n': 5, 'length_penalty': 0.7, 'outputs': ('rank', 'entropy'), 'include_end': False, 'max_rows': 12})
    assert (s.n, s.alpha, s.rank, s.entropy, s.include_end, s.max_rows) == (5, 0.7, True, True, False, 12)
    assert _Scoring.parse({'outputs': 'entropy'}).entropy and not _Scoring.parse({'outputs': 'entropy'}).rank
    assert _Scoring.parse({'outputs': []}).rank is False
    for bad in ({'beam_size': 3}, {'n': 0}, {'n': -1}, {'n': 2.5}, {'n': True}, {'n': 'x'}, {'length_penalty': -0.1},
                {'length_penalty': float('nan')}, {'outputs': ('rank', 'perplexity')}, {'outputs': 'logits'}, {'include_end': 2},
                {'include_end': 'yes'}, {'max_rows': 0}, {'max_rows': 1.5}, {'max_rows': [4]}):
        with pytest.raises(ValueError):
            _Scoring.parse(bad)


def test_score_shapes_and_chunks():
    from recurrent_fusion_network_amd.decode import _Scoring
    s = _Scoring.parse({})
    assert s.layout((4, 9), 4, 16) == (4, 1, 9)
    assert s.layout((4, 5, 17), 4, 16) == (20, 5, 17)
    assert _Scoring.parse({'n': 5}).layout((20, 3), 4, 16) == (20, 5, 3)
    assert _Scoring.parse({'n': 5}).layout((4, 5, 3), 4, 16) == (20, 5, 3)
    for so, shape in ((s, (4, 18)), (s, (4, 0)), (s, (5, 9)), (s, (4,)), (s, (4, 2, 2, 2)), (s, (3, 5, 9)), (s, (4, 0, 9)),
                      (_Scoring.parse({'n': 3}), (4, 5, 9)), (_Scoring.parse({'n': 3}), (4, 9))):
        with pytest.raises(ValueError):
            so.layout(shape, 4, 16)
    # max_rows: down to a multiple of n, at least n; the default keeps steps * rows * V1 floats under 1 GiB
    assert _Scoring.parse({'max_rows': 12}).rows_per_call(5, 17, 9488) == 10
    assert _Scoring.parse({'max_rows': 3}).rows_per_call(5, 17, 9488) == 5
    per = s.rows_per_call(5, 17, 9488)
    assert per % 5 == 0 and 4 * 17 * 9488 * per <= 1 << 30 < 4 * 17 * 9488 * (per + 5)


def test_rescore_refuses_a_flat_candidate_matrix():
    import torch
    from recurrent_fusion_network_amd import decode
    with pytest.raises(ValueError):
        decode.rescore(None, None, None, torch.zeros(6, 4, dtype=torch.long))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def native():
    import recurrent_fusion_network_amd._native as N
    return N


def test_new_symbols_are_declared_exported_and_the_abi_version_stays():
    N = native()
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    assert 'caption scoring' in src
    declared = set(re.findall(r'\b(rfn_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', src, flags=re.S)))
    for s in NEW_SYMBOLS:
        assert s in declared and s in N.EXPORTS and hasattr(N.lib, s), s
        assert getattr(N.lib, s).argtypes is not None
    assert N.lib.rfn_abi_version() == 9 == N.ABI_VERSION


def test_score_workspace_is_the_inference_workspace():
    N = native()
    dp = C.byref(N.make_dims(**OK_DIMS))
    for B, S, n in ((3, 4, 1), (6, 2, 3), (12, 5, 4), (12, 5, 12)):
        assert N.lib.rfn_decoder_score_ws_bytes(dp, B, S, n) == N.lib.rfn_decoder_ws_bytes_ex(dp, B, S, 0, n) > 0
    drop = C.byref(N.make_dims(drop_lm=0.5, **OK_DIMS))                     # dropout is off whatever the dims say
    assert N.lib.rfn_decoder_score_ws_bytes(drop, 6, 2, 3) == N.lib.rfn_decoder_score_ws_bytes(dp, 6, 2, 3)
    for B, S, n in ((6, 4, 4), (6, 4, 0), (6, 4, -1), (0, 4, 1), (6, 0, 1)):
        assert N.lib.rfn_decoder_score_ws_bytes(dp, B, S, n) == 0
    assert N.lib.rfn_decoder_score_ws_bytes(C.byref(N.make_dims(**dict(OK_DIMS, R=0))), 6, 4, 1) == 0


def test_score_kernels_refuse_bad_calls_before_launching():
    N = native()
    p = 0x10000

    def sl(logits=p, ldl=52, B=2, T=3, t0=0, V1=52, target=p, include_end=1, lp=p, ld_out=3):
        return N.lib.rfn_score_logits(logits, ldl, B, T, t0, V1, target, 4, include_end, lp, p, p, ld_out, None)

    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(V1=0, ldl=0), dict(t0=-1), dict(ldl=51), dict(ld_out=2), dict(t0=1),
               dict(t0=2, T=1, ld_out=2), dict(B=1 << 20, T=1 << 12, ld_out=1 << 12)):
        assert sl(**kw) == SHAPE, kw
    for kw in (dict(logits=None), dict(target=None), dict(lp=None)):
        assert sl(**kw) == ARG, kw
    assert sl(B=0, logits=None) == SHAPE                                    # the shape is checked first

    def sc(lp=p, ld_lp=3, target=p, B=2, T=3, V1=52, cap=p, n=p):
        return N.lib.rfn_score_captions(lp, ld_lp, target, 4, B, T, V1, 1, cap, n, None)

    for kw in (dict(B=0), dict(T=0), dict(V1=0), dict(ld_lp=2)):
        assert sc(**kw) == SHAPE, kw
    for kw in (dict(lp=None), dict(target=None), dict(cap=None), dict(cap=None, n=None)):
        assert sc(**kw) == ARG, kw
    assert sc(T=0, cap=None) == SHAPE


def test_decoder_score_refuses_bad_calls_before_launching():
    N = native()
    d = N.make_dims(**OK_DIMS)
    un = N.make_dims(path_flags=N.PATH_OPT_DEC_UNHOISTED, **OK_DIMS)
    bad = N.make_dims(**dict(OK_DIMS, R=0))
    P = 0x10000
    size = N.lib.rfn_decoder_score_ws_bytes(C.byref(d), 6, 4, 1)
    assert N.lib.rfn_decoder_score_ws_bytes(C.byref(d), 6, 4, 2) <= size

    def call(dd=d, B=6, S=4, prm=P, comb=P, h0=P, c0=P, ids=P, target=P, lp=P, ld_out=4, cap=P, cap_len=P, ws=P, wsb=size, n=1):
        return N.lib.rfn_decoder_score(None if dd is None else C.byref(dd), B, S, prm, comb, h0, c0, ids, 5, target, 5, 1, lp, P, P,
                                       ld_out, cap, cap_len, ws, wsb, n, None)

    assert call(dd=None) == ARG and call(dd=bad) == SHAPE
    for kw in (dict(B=0), dict(S=0), dict(ld_out=3), dict(n=0), dict(n=-2), dict(n=4), dict(dd=un, n=4), dict(B=0, prm=None)):
        assert call(**kw) == SHAPE, kw
    assert call(dd=un, n=2) == UNSUPPORTED and call(dd=un, n=2, ws=None) == UNSUPPORTED
    for name in ('prm', 'comb', 'h0', 'c0', 'ids', 'target', 'lp', 'ws'):
        assert call(**{name: None}) == ARG, name
        assert call(n=2, **{name: None}) == ARG, name
    assert call(cap=None, cap_len=P) == ARG                                 # a length without the sum it belongs to
    assert call(wsb=size - 1) == WORKSPACE and call(wsb=0, n=3) == WORKSPACE
    assert call(ws=None, wsb=0) == ARG                                      # the pointers are checked before the size
    # rfn_decoder_fwd_ex still has no logits-only form with n > 1 for its callers
    assert N.lib.rfn_decoder_fwd_ex(C.byref(d), 6, 4, P, P, P, P, P, 4, None, P, size, 0, 0, 2, None) == ARG
