"""CPU: the restatement of the decoding constraints (tests/decode_constraints_cpu.py) against hand-written cases, the
length-penalty ordering against a hand-sorted list, the option parsing of the hosts, and the new C symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import decode_constraints_cpu as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ('rfn_decode_blocklist', 'rfn_logp_mask_rows', 'rfn_log_softmax_topk_masked', 'rfn_decoder_loop_ex',
               'rfn_beam_loop_ex')


def test_repeated_bigram_blocks_its_continuation():
    # "a man on a bike on": the bigram (on, ?) already went on -> a; history = [a=4 man=7 on=9 a=4 bike=5 on=9]
    assert D.blocked_ids([4, 7, 9, 4, 5, 9], t=7, n=2) == [4]
    # the last token occurs twice before: both continuations, in history order
    assert D.blocked_ids([4, 7, 4, 5, 4], t=6, n=2) == [7, 5]
    # the trailing occurrence itself has no continuation yet, and END is never blocked
    assert D.blocked_ids([4, 4], t=3, n=2) == [4]
    assert D.blocked_ids([3, 8], t=3, n=2) == []


def test_trigram_prefix_twice_with_different_continuations():
    h = [1, 2, 3, 9, 1, 2, 4, 8, 1, 2]
    assert D.blocked_ids(h, t=11, n=3) == [3, 4]
    assert D.blocked_ids(h, t=11, n=2) == [3, 4]          # (2, ?) went on 3 and 4 as well
    assert D.blocked_ids(h, t=11, n=4) == []              # (8, 1, 2) has not occurred before
    assert D.blocked_ids([5, 1, 2, 7, 5, 1, 2], t=8, n=4) == [7]


def test_steps_before_n_block_nothing():
    assert D.blocked_ids([], t=1, n=2) == []
    assert D.blocked_ids([6], t=2, n=3) == []
    assert D.blocked_ids([6, 6], t=3, n=4) == []
    assert D.blocked_ids([6, 6], t=3, n=3) == []          # t == n: the only trigram position is the suffix itself
    assert D.blocked_ids([6, 6, 6], t=4, n=3) == [6]


def test_finished_row_is_left_alone():
    assert D.blocked_ids([4, 7, 4, 0], t=5, n=2, banned=[3], bad_endings=[0, 4]) == []
    assert D.blocked_ids([0], t=2, n=2, banned=[3]) == []


def test_bad_ending_blocks_the_end_token():
    assert D.blocked_ids([4, 7], t=3, bad_endings=[7, 9]) == [0]
    assert D.blocked_ids([4, 7], t=3, bad_endings=[4]) == []          # only the LAST token counts
    assert D.blocked_ids([], t=1, bad_endings=[4]) == []
    # at the last step t = S the rule is the same; the search's forced close of every beam at t = S is not a token choice
    assert D.blocked_ids([4, 7, 4, 7], t=5, n=2, bad_endings=[7]) == [4, 0]


def test_banned_ids_and_duplicates():
    assert D.blocked_ids([], t=1, banned=[9, 2]) == [2, 9]
    # 4 is banned AND a repeated-bigram continuation: listed twice, consumers tolerate it
    assert D.blocked_ids([4, 7, 9, 4, 5, 9], t=7, n=2, banned=[4], bad_endings=[9]) == [4, 4, 0]
    lp = np.log(np.full((2, 10), 0.1, dtype=np.float32))
    m = D.mask_rows(lp, [[4, 7, 9, 4, 5, 9], [1, 0, 0, 0, 0, 0]], 7, 2, [4], [9])
    assert np.isinf(m[0, [0, 4]]).all() and np.array_equal(m[0, [1, 2, 3, 5, 6, 7, 8, 9]], lp[0, [1, 2, 3, 5, 6, 7, 8, 9]])
    assert np.array_equal(m[1], lp[1])                     # the finished row keeps every bit


def test_length_penalty_order_against_a_hand_sorted_list():
    S = 8
    seqs = [[5, 0, 0, 0, 0, 0, 0, 0], [5, 6, 7, 0, 0, 0, 0, 0], [5, 6, 7, 8, 9, 1, 2, 3], [4, 0, 0, 0, 0, 0, 0, 0],
            [4, 6, 7, 0, 0, 0, 0, 0]]
    lens = [D.caption_len(s, S) for s in seqs]
    assert lens == [2, 4, 8, 2, 4]
    ps = [-2.0, -3.0, -4.0, -2.0, -3.0]
    assert D.rank_done(ps, lens, 0.0) == [0, 3, 1, 4, 2]             # raw sums: the shortest first, ties stable
    # alpha = 1: -1, -0.75, -0.5, -1, -0.75
    assert D.rank_done(ps, lens, 1.0) == [2, 1, 4, 0, 3]
    # alpha = 0.5: -1.414, -1.5, -1.414, -1.414, -1.5
    assert D.rank_done(ps, lens, 0.5) == [0, 2, 3, 1, 4]
    assert D.has_repeated_ngram([4, 7, 4, 7, 0, 4, 7], 2) and not D.has_repeated_ngram([4, 7, 4, 0, 4, 7], 2)


def test_option_parsing_refuses_what_the_kernels_cannot_take():
    from recurrent_fusion_network_amd.decode import _Constraints, _length_penalty
    V1, S = 51, 5
    assert _Constraints.parse({}, V1, S) is None
    assert _Constraints.parse({'block_ngram': 0, 'banned_ids': [], 'bad_endings': None}, V1, S) is None
    c = _Constraints.parse({'block_ngram': 3, 'banned_ids': [7, 3, 7], 'bad_endings': (2,)}, V1, S)
    assert (c.n, c.banned, c.bad) == (3, [3, 7], [2])
    for bad in ({'block_ngram': 1}, {'block_ngram': 5}, {'banned_ids': [0]}, {'banned_ids': list(range(1, 66))},
                {'bad_endings': list(range(1, 66))}, {'banned_ids': [V1]}, {'bad_endings': [-1]}):
        with pytest.raises(ValueError):
            _Constraints.parse(bad, V1, 70)
    assert len(_Constraints.parse({'banned_ids': list(range(1, 65))}, 200, S).banned) == 64
    assert _length_penalty({}) == 0.0 and _length_penalty({'length_penalty': 0.5}) == 0.5
    with pytest.raises(ValueError):
        _length_penalty({'length_penalty': -1.0})


def test_new_symbols_are_declared_exported_and_refuse_bad_shapes():
    import recurrent_fusion_network_amd._native as N
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(rfn_[a-z0-9_]+)\s*\(', src))
    for s in NEW_SYMBOLS:
        assert s in declared and s in N.EXPORTS and hasattr(N.lib, s), s
    assert 'rfn_decode_constraints' in src and N.lib.rfn_abi_version() == 9
    assert C.sizeof(N.DecodeConstraints) == 16 + 4 * 8
    FAKE = 1 << 40                                         # never dereferenced: every call below fails before a launch
    bl = lambda S, t, n, nb, nbad: N.lib.rfn_decode_blocklist(FAKE, 1, 1, None, 4, S, t, n, FAKE, nb, FAKE, nbad, 50, FAKE, FAKE, None)  # noqa: E731
    assert bl(65, 1, 2, 0, 0) == -1 and bl(8, 9, 2, 0, 0) == -1 and bl(8, 0, 2, 0, 0) == -1
    assert bl(8, 1, 1, 0, 0) == -1 and bl(8, 1, 5, 0, 0) == -1
    assert bl(8, 1, 2, 65, 0) == -1 and bl(8, 1, 2, 0, 65) == -1
    assert N.lib.rfn_decode_blocklist(None, 1, 1, None, 4, 8, 1, 2, FAKE, 0, FAKE, 0, 50, FAKE, FAKE, None) == -5
    assert N.lib.rfn_logp_mask_rows(FAKE, 40, 4, 50, FAKE, 72, FAKE, None) == -1          # row stride below V1
    assert N.lib.rfn_logp_mask_rows(FAKE, 50, 4, 50, None, 72, FAKE, None) == -5
    assert N.lib.rfn_log_softmax_topk_masked(FAKE, 50, 4, 50, 33, FAKE, 72, FAKE, FAKE, FAKE, None) == -1
    assert N.lib.rfn_log_softmax_topk_masked(FAKE, 50, 4, 50, 3, FAKE, 72, None, FAKE, FAKE, None) == -5
