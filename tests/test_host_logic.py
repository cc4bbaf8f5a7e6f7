"""Host-side pieces that need no GPU."""
import pickle

from recurrent_fusion_network_amd.decode import _LazyList, early_exit


def test_lazy_list_never_shows_a_placeholder():
    """sample_beam's per-image lists fill themselves on first use: every read path of `list` must see the
    filled entries, and it must pickle as a plain list."""
    calls = []

    def mk():
        return _LazyList(2, lambda: calls.append(1) or [5, 6])

    assert len(mk()) == 2 and not calls                     # the length is known without filling
    assert mk() + [7] == [5, 6, 7] and [4] + mk() == [4, 5, 6] and mk() * 2 == [5, 6, 5, 6]
    assert mk().copy() == [5, 6] and list(reversed(mk())) == [6, 5] and mk()[::-1] == [6, 5]
    assert mk().index(6) == 1 and mk().count(5) == 1 and 6 in mk() and sorted(mk()) == [5, 6]
    assert pickle.loads(pickle.dumps(mk())) == [5, 6] and type(pickle.loads(pickle.dumps(mk()))) is list
    lst = mk()
    lst.append(9)
    lst += [1]
    assert lst == [5, 6, 9, 1] and repr(mk()) == '[5, 6]' and mk() != [None, None]
    one = mk()
    n = len(calls)
    assert one[0] == 5 and one[1] == 6 and list(one) == [5, 6] and len(calls) == n + 1      # filled exactly once


def test_lazy_list_has_no_c_level_back_door():
    """a `list` SUBCLASS is read by C fast paths (json's C encoder, str.join, PySequence_Fast) through its item
    array, behind every Python-level hook: an unfilled lazy list showed them its placeholders.  The type is a plain
    MutableSequence now: consumers either go through __iter__ / __getitem__ (and see the filled entries) or refuse it."""
    import json

    import pytest
    assert not isinstance(_LazyList(1, lambda: [0]), list)
    lazy = _LazyList(2, lambda: [0.5, 0.25])
    with pytest.raises(TypeError):
        json.dumps(lazy)                                      # loud, never '[null, null]'
    assert json.dumps(list(_LazyList(2, lambda: [0.5, 0.25]))) == '[0.5, 0.25]'
    assert json.dumps(_LazyList(2, lambda: [0.5, 0.25]).materialize()) == '[0.5, 0.25]'
    assert json.dumps(_LazyList(2, lambda: [0.5, 0.25]), default=list) == '[0.5, 0.25]'
    assert ','.join(_LazyList(2, lambda: ['a', 'b'])) == 'a,b'        # PySequence_Fast on a non-list iterates
    assert tuple(_LazyList(2, lambda: [1, 2])) == (1, 2) and [*_LazyList(2, lambda: [1, 2])] == [1, 2]
    import numpy as np
    assert np.asarray(_LazyList(2, lambda: [1.0, 2.0])).tolist() == [1.0, 2.0]
    with pytest.raises(Exception):
        _LazyList(3, lambda: [1]).materialize()               # a producer that breaks its promise is an error, not a short list


def test_early_exit_is_the_first_step_with_no_unfinished_row():
    """alive[t - 1] = rows still unfinished after the t-th token; the loop stops at the first t >= 1 where it is 0."""
    assert early_exit([3, 1, 0, 0], 4) == 3                 # the first zero in the middle; later zeros do not matter
    assert early_exit([0, 0, 0, 0], 4) == 1                 # every row ended with its first token
    assert early_exit([3, 0, 2, 0], 4) == 2                 # the FIRST zero, whatever follows
    assert early_exit([4, 4, 2, 1], 4) == 5                 # no zero: S + 1, all S tokens are kept
    assert early_exit([2, 1, 1, 0], 4) == 4                 # a zero only at the last step
    assert early_exit([0], 1) == 1 and early_exit([7], 1) == 2      # S = 1
