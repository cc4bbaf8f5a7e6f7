"""CPU: the oracle's self-critical RL gradients (oracle/rfn_oracle.py rl_step_loss_and_grads) pinned to what the reference
produced (the goldens' rl_gradnorm/* and rl_gradslice/*, oracle/make_golden.py rl_section), fp64 against fp32, and the
element-wise comparator the GPU checks (tests/test_rl_grads_gpu.py) rely on.

The bars of the pin are the ones make_golden.py applied to reference against oracle when the goldens were made: norms within
1e-5 + 1e-4 * norm, slices within 2e-5 + 1e-4 * max|g|.  The c5 decode tier is left to the GPU suite (4 x 196 x 2048 encoders:
its oracle pass is the slow one this file has no exclusion for)."""
import numpy as np
import pytest
import torch

from rl_grad_check import RL_TIERS, compare_grads, fed_from_raw, grad_bar, load_rl_case


def maxerr(a, b):
    return float((torch.as_tensor(a).double() - torch.as_tensor(b).double()).abs().max())


def _helper(name, dtype=None):
    from oracle import rfn_oracle as O
    cfg, P, fc, att, top, gold = load_rl_case(name)
    out = O.rl_step_loss_and_grads(cfg, P, fc, att, fed_from_raw(gold['rl_raw_ids']), torch.from_numpy(gold['rl_reward']), top,
                                   0.01, 1.0, dtype=dtype)
    return (cfg, P, fc, att, top, gold) + tuple(out)


@pytest.mark.parametrize('name', RL_TIERS)
def test_rl_gradients_reproduce_the_references(name):
    cfg, P, fc, att, top, gold, loss, grads, seq, seq_lp, lp_all = _helper(name)
    assert torch.equal(seq, torch.from_numpy(gold['rl_seq']))
    assert maxerr(seq_lp, gold['rl_seq_logprobs']) < 2e-5
    assert lp_all.size(1) == seq.size(1) + 1
    assert abs(float(loss) - float(gold['rl_loss'])) < 1e-4
    assert set(grads) == set(P) == {k[len('rl_gradnorm/'):] for k in gold.files if k.startswith('rl_gradnorm/')}
    for k, g in grads.items():
        gn = float(gold['rl_gradnorm/' + k])
        assert abs(float(g.double().norm()) - gn) <= 1e-5 + 1e-4 * gn, (k, float(g.double().norm()), gn)
        flat = g.reshape(-1)
        stride = max(1, flat.numel() // 16)                      # make_golden.grad_summary
        sl = gold['rl_gradslice/' + k]
        assert maxerr(flat[::stride][:16], sl) <= 2e-5 + 1e-4 * float(g.abs().max()), k


@pytest.mark.parametrize('name', RL_TIERS)
def test_rl_helper_is_the_forced_id_sample_and_fp64_agrees_with_fp32(name):
    """Without dropout the helper must BE sample_greedy(force_ids) -> rl_criterion -> backward (same ops on the same numbers:
    equal bit for bit), and its fp64 run must agree with the fp32 one within the GPU suite's bar, which is what licenses
    the fp32 oracle at the benchmarked sizes."""
    from oracle import rfn_oracle as O
    cfg, P, fc, att, top, gold, loss, grads, seq, seq_lp, lp_all = _helper(name)
    raw = torch.from_numpy(gold['rl_raw_ids'])
    Pg = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    r_seq, r_lp, r_all, r_reason = O.sample_greedy(cfg, Pg, fc, att, force_ids=raw)
    r_loss = O.rl_criterion(cfg, r_lp, r_seq, torch.from_numpy(gold['rl_reward']), r_all, 0.01, r_reason, top, 1.0)
    r_loss.backward()
    assert torch.equal(r_seq, seq) and tuple(r_all.shape) == tuple(lp_all.shape)
    assert torch.equal(r_lp.detach(), seq_lp) and torch.equal(r_all.detach(), lp_all)
    assert float(r_loss.detach()) == float(loss)
    for k, g in grads.items():
        want = Pg[k].grad if Pg[k].grad is not None else torch.zeros_like(Pg[k])
        assert torch.equal(g, want), k
    loss64, grads64, seq64, lp64, all64 = _helper(name, torch.float64)[6:]
    assert all64.dtype == torch.float64 and all(g.dtype == torch.float64 for g in grads64.values())
    assert torch.equal(seq64, seq)
    assert maxerr(all64, lp_all) < 1e-3 and maxerr(lp64, seq_lp) < 1e-3
    assert abs(float(loss64) - float(loss)) < 1e-4 * max(1.0, abs(float(loss64)))
    rep = compare_grads(grads, grads64, grad_bar)
    assert rep['ratio'] <= 1.0


def test_rl_helper_shapes_of_the_early_exit_and_its_refusals():
    """The early exit from the fed tokens alone: a zero in column t finishes the row, the pass stops at the first step
    with no unfinished row, later (unmasked) tokens of finished rows are fed but masked out of `seq`."""
    from oracle import rfn_oracle as O
    cfg, P, fc, att, top, gold = load_rl_case('tiny1')
    B, S = fc[0].size(0), cfg.seq_length
    fed = torch.zeros(B, S + 1, dtype=torch.long)
    fed[:, 1:] = torch.tensor([[4, 0, 9, 9, 9], [7, 8, 3, 0, 3], [1, 2, 6, 0, 5]])
    reward = torch.tensor([[0.5], [-1.0], [2.0]])
    loss, grads, seq, seq_lp, lp_all = O.rl_step_loss_and_grads(cfg, P, fc, att, fed, reward, top, 0.01, 1.0)
    assert seq.tolist() == [[4, 0, 0], [7, 8, 3], [1, 2, 6]] and tuple(lp_all.shape) == (B, 4, cfg.vocab_size + 1)
    r_seq, r_lp, r_all, _ = O.sample_greedy(cfg, P, fc, att, force_ids=fed[:, 1:])
    assert torch.equal(r_seq, seq) and torch.equal(r_lp, seq_lp) and torch.equal(r_all, lp_all)
    # tokens after the exit step never ran: changing them changes nothing
    fed2 = fed.clone()
    fed2[:, 5:] = 11
    again = O.rl_step_loss_and_grads(cfg, P, fc, att, fed2, reward, top, 0.01, 1.0)
    assert float(again[0]) == float(loss) and all(torch.equal(again[1][k], grads[k]) for k in grads)
    # the unmasked token of a finished row IS fed (:637): that row's later distributions move, but every term they enter
    # is masked (:56-61), so the loss stays
    fed3 = fed.clone()
    fed3[0, 3] = 17
    third = O.rl_step_loss_and_grads(cfg, P, fc, att, fed3, reward, top, 0.01, 1.0)
    assert torch.equal(third[2], seq) and not torch.equal(third[4][0, 3], lp_all[0, 3]) and torch.equal(third[4][1:], lp_all[1:])
    assert float(third[0]) == float(loss)
    with pytest.raises(ValueError):
        O.rl_step_loss_and_grads(cfg, P, fc, att, torch.zeros(B, S + 1, dtype=torch.long), reward, top, 0.01, 1.0)
    with pytest.raises(ValueError):
        O.rl_step_loss_and_grads(cfg, P, fc, att, fed, torch.zeros(B, 2), top, 0.01, 1.0)


def _dicts():
    g = torch.Generator().manual_seed(0)
    want = {'a.weight': torch.randn(7, 5, generator=g), 'b.weight': torch.randn(7, 5, generator=g) * 1e-3,
            'a.bias': torch.randn(7, generator=g), 'scalar': torch.randn((), generator=g)}
    return want, {k: v.clone() for k, v in want.items()}


def test_comparator_passes_within_the_bar_and_reports_the_worst_element():
    want, got = _dicts()
    assert compare_grads(got, want, grad_bar)['ratio'] == 0.0
    bar = grad_bar(want['b.weight'])
    got['b.weight'][3, 2] += 0.5 * bar
    got['a.weight'][1, 1] += 0.25 * grad_bar(want['a.weight'])
    rep = compare_grads(got, want, grad_bar)
    assert rep['name'] == 'b.weight' and rep['index'] == (3, 2) and abs(rep['ratio'] - 0.5) < 1e-3
    assert rep['want'] == float(want['b.weight'][3, 2]) and rep['got'] == float(got['b.weight'][3, 2]) and not rep['failures']


def test_comparator_fails_on_one_element_moved_by_twice_the_bar():
    want, got = _dicts()
    got['b.weight'][6, 4] -= 2.0 * grad_bar(want['b.weight'])
    with pytest.raises(AssertionError, match=r'b\.weight\[6, 4\]'):
        compare_grads(got, want, grad_bar)
    rep = compare_grads(got, want, grad_bar, check=False)
    assert rep['name'] == 'b.weight' and rep['index'] == (6, 4) and abs(rep['ratio'] - 2.0) < 1e-2 and len(rep['failures']) == 1
    # a tensor-wide norm would not see it: that is the gap the element-wise check closes
    assert abs(float(got['b.weight'].norm()) - float(want['b.weight'].norm())) < 3e-3 * float(want['b.weight'].norm())


def test_comparator_fails_on_two_swapped_tensors_of_equal_shape():
    want, got = _dicts()
    got['a.weight'], got['b.weight'] = got['b.weight'], got['a.weight']
    with pytest.raises(AssertionError):
        compare_grads(got, want, grad_bar)
    assert len(compare_grads(got, want, grad_bar, check=False)['failures']) == 2
    # a sign error and a transposed square block keep every norm and fail here
    want, got = _dicts()
    got['a.bias'] = -got['a.bias']
    with pytest.raises(AssertionError, match=r'a\.bias'):
        compare_grads(got, want, grad_bar)
    want, got = _dicts()
    got['a.weight'][:5, :5] = got['a.weight'][:5, :5].t().clone()
    with pytest.raises(AssertionError, match=r'a\.weight'):
        compare_grads(got, want, grad_bar)


def test_comparator_fails_on_a_tensor_missing_on_either_side():
    want, got = _dicts()
    del got['a.bias']
    with pytest.raises(AssertionError, match='missing from the result'):
        compare_grads(got, want, grad_bar)
    want, got = _dicts()
    del want['scalar']
    with pytest.raises(AssertionError, match='without a reference'):
        compare_grads(got, want, grad_bar)
    want, got = _dicts()
    got['a.bias'] = None                                        # a parameter backward never reached
    with pytest.raises(AssertionError, match='no gradient'):
        compare_grads(got, want, grad_bar)
    want, got = _dicts()
    got['a.weight'] = got['a.weight'].t().contiguous()          # a wrong layout is not broadcast away
    with pytest.raises(AssertionError, match='shape'):
        compare_grads(got, want, grad_bar)
    want, got = _dicts()
    got['a.weight'][0, 0] = float('nan')
    with pytest.raises(AssertionError, match='non-finite'):
        compare_grads(got, want, grad_bar)
    assert np.isfinite(compare_grads(*reversed(_dicts()), grad_bar)['ratio'])
