"""CPU: the NumPy restatement of diverse beam search (tests/diverse_beam_cpu.py) against the oracle's beam search, the claim
that each row's W best entries are all the search needs, lambda = 0 as G independent searches, and the host-side refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import diverse_beam_cpu as Dv
from conftest import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def beam_tuple(d):
    return ([int(x) for x in d['seq']], np.asarray(d['logps'], dtype=np.float32).tobytes(), np.float32(d['p']).tobytes())


@pytest.mark.parametrize('name', ['tiny0', 'tiny1'])
def test_one_group_is_the_oracles_beam_search(name):
    """(a) G == 1: the driver around oracle.one_time_step, one image at a time on beam_size copies of its features (the
    layout of O.sample_beam), returns O.sample_beam's done beams: ids equal, p (and the token log-probs) bit-equal."""
    from oracle import rfn_oracle as O
    cfg, spec, P, batch, _ = load_case(name)
    fc, att = batch[0], batch[1]
    S = cfg.seq_length
    for W in (2, 3):
        with torch.no_grad():
            want = O.sample_beam(cfg, P, fc, att, W)[5]
            for k in range(fc[0].size(0)):
                fc_k = [f[k:k + 1].expand(W, f.size(1)).contiguous() for f in fc]
                att_k = [a[k:k + 1].expand(W, a.size(1), a.size(2)).contiguous() for a in att]
                hs, cs = O.init_state(cfg, P, fc_k)
                comb, _, (h, c) = O.thought_vectors(cfg, P, att_k, hs, cs)
                st = [h, c]

                def step_fn(t, order, ids):
                    idx = torch.from_numpy(order)
                    logits, st[0], st[1] = O.one_time_step(cfg, P, P['embed.weight'][torch.from_numpy(ids)], comb, st[0][idx], st[1][idx])
                    return torch.log_softmax(logits, dim=1).numpy()

                b = Dv.search(step_fn, W, S)
                got = sorted(b.done, key=lambda d: -float(d['p']))
                assert all(d['group'] == 0 for d in got)
                assert [beam_tuple(d) for d in got] == [beam_tuple(d) for d in want[k]], (name, W, k)


def run_synthetic(rng_seed, W, G, S, V1, lam, ncols=None, rows_of=None):
    """A whole synthetic search of one image on Dv.synthetic_rows; rows_of: the slice of beam rows to search (a group)."""
    rows = Dv.synthetic_rows(rng_seed, 1, W, S, V1)
    lo, hi = rows_of if rows_of is not None else (0, W)
    b = Dv.Beams(hi - lo, S)
    trace = []
    for t in range(1, S + 1):
        Dv.step(b, rows[t - 1][0, lo:hi], t, G, lam, ncols)
        trace.append((b.order.tolist(), b.next_ids.tolist(), b.active, b.seq.tolist(), b.lp.tobytes(), b.sum.tobytes(),
                      [beam_tuple(d) + (d['group'],) for d in b.done]))
    return b, trace


SHAPES = [(2, 2), (4, 2), (6, 3), (6, 6), (12, 4)]


@pytest.mark.parametrize('W,G', SHAPES)
def test_the_w_best_entries_of_a_row_suffice(W, G):
    """(b) The restatement fed only each row's W best entries equals the full-row restatement, step by step, on rows with a
    small vocabulary and many exact ties (every third row quantised), for V1 in {W, W + 1, 50}."""
    differs = 0
    for V1 in (W, W + 1, 50):
        for S in (1, 4, 9):
            for lam in (0.0, 0.5, 1e30):
                seed = 1000 * W + 100 * G + V1 + S
                full = run_synthetic(seed, W, G, S, V1, lam)[1]
                cut = run_synthetic(seed, W, G, S, V1, lam, ncols=min(W, V1))[1]
                assert full == cut, (V1, S, lam)
                if lam:
                    differs += full != run_synthetic(seed, W, G, S, V1, 0.0)[1]
    assert differs > 0                               # the penalty did something on these rows


@pytest.mark.parametrize('W,G', SHAPES)
def test_lambda_zero_is_g_independent_searches(W, G):
    """(c) With lambda = 0 every group's outcome equals a G == 1 search of width Wg on the group's rows."""
    Wg = W // G
    for V1 in (W, 37):
        for S in (1, 4, 9):
            seed = 7000 + 100 * W + G + V1 + S
            b, _ = run_synthetic(seed, W, G, S, V1, 0.0)
            for g in range(G):
                lo, hi = g * Wg, (g + 1) * Wg
                one, _ = run_synthetic(seed, W, 1, S, V1, 0.0, rows_of=(lo, hi))
                assert np.array_equal(b.seq[:, lo:hi], one.seq) and b.lp[:, lo:hi].tobytes() == one.lp.tobytes()
                assert b.sum[lo:hi].tobytes() == one.sum.tobytes()
                assert [beam_tuple(d) for d in b.done if d['group'] == g] == [beam_tuple(d) for d in one.done], (V1, S, g)


def test_synthetic_rows_leave_a_group_inert_beside_a_live_one():
    """The END bias of the synthetic rows ends beams early: some case has a group without candidates next to a live one."""
    seen = 0
    for W, G in SHAPES:
        b, _ = run_synthetic(5, W, G, 9, 37, 0.5)
        seen += len(b.inert_groups) > 0
    assert seen > 0


def test_options_are_parsed_and_refused():
    from recurrent_fusion_network_amd.decode import _Diversity
    assert _Diversity.parse({}, 6) is None and _Diversity.parse({'group_size': 1, 'diversity_lambda': 7.0}, 5) is None
    d = _Diversity.parse({'group_size': 3}, 6)
    assert d.groups == 3 and d.lam == 0.5
    assert _Diversity.parse({'group_size': 2, 'diversity_lambda': 0}, 6).lam == 0.0
    for bad in ({'group_size': 0}, {'group_size': -2}, {'group_size': 4}, {'group_size': 2, 'diversity_lambda': -0.5},
                {'group_size': 2, 'diversity_lambda': float('nan')}, {'group_size': 1, 'diversity_lambda': -1.0}):
        with pytest.raises(ValueError):
            _Diversity.parse(bad, 6)


def test_c_entry_refuses_before_launching():
    """RFN_ERR_SHAPE (-1) for G < 1, G not dividing W and lambda < 0 or NaN: returned before any pointer is read."""
    import recurrent_fusion_network_amd._native as N
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    assert 'rfn_beam_diversity' in src and 'diverse beam search' in src and N.lib.rfn_abi_version() == 9   # additive
    assert C.sizeof(N.BeamDiversity) == 16 and N.BeamDiversity.done_group.offset == 8
    P = C.c_void_p(0x10000)
    call = lambda W, G, lam: N.lib.rfn_beam_step_div(P, P, 37, W, G, lam, 4, 1, 1, 4 * W, P, P, P, P, P, P, P, P, P, P, P, None)  # noqa: E731
    assert call(6, 0, 0.5) == -1 and call(6, -1, 0.5) == -1 and call(6, 4, 0.5) == -1
    assert call(6, 3, -0.5) == -1 and call(6, 3, float('nan')) == -1
    assert call(33, 3, 0.5) == -1 and call(64, 2, 0.5) == -1                 # beam_size > 32
    assert N.lib.rfn_beam_step_div(P, P, 37, 6, 3, 0.5, 4, 1, 1, 24, P, P, P, P, P, P, P, P, P, None, P, None) == -5   # no done_group
