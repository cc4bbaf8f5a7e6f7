"""RecurrentFusionModel.rl_loss (INTEGRATION.md "Policy-gradient loss from the logits"): the teacher-forced replay of given captions
and the reward criterion as one call whose policy and entropy terms come straight from the logits -- no (rows, T, V+1)
logprobs_all, no gradient of it, d logits written in place (rfn_decoder_logits_fwd / _bwd, rfn_rl_logits_fwd / _bwd).

  a. the golden RL tiers (the reference's drawn ids and rewards) against the fp64 oracle, every element of every gradient at
     rl_grad_check.grad_bar, the loss within 1e-4 * max(1, |loss|), last_rl['logprobs'] within LOGP_TOL -- the bars of
     tests/test_rl_grads_gpu.py -- and against the two-call form (sample_group(force_ids) + ReviewNetRewardCriterion) on the same
     model at the same bar; with entropy_reg = 0.01 and with PPO;
  b. n = 3 rows per image: captions from sample_group under no_grad, ragged attention maps, an att_feats tensor that requires grad;
  c. training mode with dropout: the two forms draw the same masks from the same torch seed;
  d. a second backward over the same graph, every refusal, and sample_group's bits before and after rl_loss has run."""
import pytest
import torch

from rl_grad_check import compare_grads, fed_from_raw, grad_bar, load_rl_case
from test_model_gpu import LOGP_TOL, build, maxerr

pytestmark = pytest.mark.gpu

ENTROPY_REG = 0.01


def _to(ts, dev):
    return [t.to(dev) for t in ts]


def _grads_of(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def _pad(seq, S):
    out = torch.zeros(seq.size(0), S, dtype=torch.long, device=seq.device)
    out[:, :seq.size(1)] = seq
    return out


def _two_call(model, cfg, fc, att, top, seq, reward, n, entropy_reg, old=None, att_lens=None, seed=None):
    """sample_group(force_ids) + ReviewNetRewardCriterion + backward -> (loss, grads, seq_lp)."""
    import recurrent_fusion_network_amd as R
    if seed is not None:
        torch.manual_seed(seed)
    cfg.use_ppo, cfg.ppo_clip = int(old is not None), 0.2
    seq2, seq_lp, lp_all, reason = model.sample_group(fc, att, n, {'force_ids': _pad(seq, cfg.seq_length)}, att_lens=att_lens)
    assert torch.equal(seq2, seq)
    rw = reward.expand(seq.size(0), seq.size(1)).contiguous()
    loss = R.ReviewNetRewardCriterion(cfg)(seq_lp, seq2, rw, lp_all, entropy_reg, reason, top, 1.0, old, cfg)
    model.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach().clone(), _grads_of(model), seq_lp.detach().clone()


def _fused(model, fc, att, top, seq, reward, n, entropy_reg, old=None, att_lens=None, seed=None, scale=1.0):
    if seed is not None:
        torch.manual_seed(seed)
    loss, reason = model.rl_loss(fc, att, seq, reward, top, entropy_reg=entropy_reg, n=n, old_logprobs=old, att_lens=att_lens)
    assert len(reason) == model.num_feat_array + 1 and loss.dim() == 0
    model.zero_grad(set_to_none=True)
    (loss * scale).backward()
    return loss.detach().clone(), _grads_of(model), model.last_rl


def _same(got, want, tag):
    rep = compare_grads(got, want, grad_bar, check=False)
    print('%s: worst err/bar %.4f at %s' % (tag, rep['ratio'], rep['name']))
    assert not rep['failures'], (tag, rep['failures'][:10])
    return rep


def _golden(name, dev):
    cfg, P, fc, att, top, gold = load_rl_case(name)
    seq = torch.from_numpy(gold['rl_seq']).long()
    reward = torch.from_numpy(gold['rl_reward']).float().reshape(seq.size(0), -1)
    return cfg, P, fc, att, top, seq, reward


@pytest.mark.parametrize('mode', ['reinforce', 'entropy', 'ppo'])
@pytest.mark.parametrize('name', ['tiny0', 'odd', 'tinymax', 'mid'])
def test_rl_loss_against_the_fp64_oracle_and_the_two_call_form(dev, name, mode):
    from oracle import rfn_oracle as O
    cfg, P, fc, att, top, seq, reward = _golden(name, dev)
    rows, T = seq.shape
    reward = reward.expand(rows, T).contiguous()
    ent = 0.0 if mode == 'reinforce' else ENTROPY_REG
    cfg.use_ppo, cfg.ppo_clip = int(mode == 'ppo'), 0.2            # what the oracle's criterion and the two-call form read
    model = build(cfg, P, dev)
    fcd, attd, topd, seqd, rwd = _to(fc, dev), _to(att, dev), top.to(dev), seq.to(dev), reward.to(dev)
    old = None
    if mode == 'ppo':
        # rewards of 1 +- 0.1 on every other row put ratio * reward on both sides of the clamp (tests/test_rl_grads_gpu.py)
        reward = reward.clone()
        reward[0::2] = 1.0 + 0.1 * torch.randn(reward[0::2].shape, generator=torch.Generator().manual_seed(22))
        rwd = reward.to(dev)
        with torch.no_grad():
            model.rl_loss(fcd, attd, seqd, rwd, topd)
        noise = 0.3 * torch.randn(rows, T, generator=torch.Generator().manual_seed(9))
        old = (model.last_rl['logprobs'] + noise.to(dev)).contiguous()
    loss, grads, last = _fused(model, fcd, attd, topd, seqd, rwd, 1, ent, old)
    fed = fed_from_raw(_pad(seq, cfg.seq_length))
    o_loss, o_grads, o_seq, o_lp, _ = O.rl_step_loss_and_grads(cfg, P, fc, att, fed, reward, top, ent, 1.0,
                                                               old_logprobs=None if old is None else old.cpu(), dtype=torch.float64)
    assert torch.equal(o_seq, seq)
    lp_err, loss_err = maxerr(last['logprobs'], o_lp), abs(float(loss) - float(o_loss))
    rep = compare_grads(grads, o_grads, grad_bar, check=False)
    print('rl_loss/%s/%s: worst err/bar %.4f at %s, log-prob err %.3g, loss err %.3g' % (name, mode, rep['ratio'], rep['name'], lp_err,
                                                                                       loss_err))
    assert set(grads) == set(o_grads)
    assert lp_err < LOGP_TOL
    assert loss_err < 1e-4 * max(1.0, abs(float(o_loss)))
    assert not rep['failures'], rep['failures'][:10]
    # the two terms of the loss, and the detached log-probs
    assert not last['logprobs'].requires_grad and tuple(last['logprobs'].shape) == (rows, T)
    assert last['policy'].dim() == 0 and last['entropy'].dim() == 0
    if ent == 0.0:
        assert float(last['entropy']) == 0.0
    # the two-call form on the same model
    loss2, grads2, seq_lp2 = _two_call(model, cfg, fcd, attd, topd, seqd, rwd, 1, ent, old)
    assert abs(float(loss.detach()) - float(loss2)) < 1e-4 * max(1.0, abs(float(loss2)))
    assert maxerr(last['logprobs'], seq_lp2.cpu()) < LOGP_TOL
    _same(grads, grads2, 'two-call/%s/%s' % (name, mode))


@pytest.mark.parametrize('name', ['tiny0', 'odd'])
def test_three_rows_per_image_with_ragged_maps_and_feature_gradients(dev, name):
    cfg, P, fc, att, top, seq, reward = _golden(name, dev)
    n, B = 3, fc[0].size(0)
    model = build(cfg, P, dev)
    fcd, topd = _to(fc, dev), top.to(dev)
    lens = [torch.tensor([1 + (3 * b + i) % L for b in range(B)], dtype=torch.int32, device=dev) for i, L in enumerate(model.att_num)]
    torch.manual_seed(5)
    with torch.no_grad():
        seq3 = model.sample_group(fcd, _to(att, dev), n, att_lens=lens)[0].contiguous()
    rows, T = seq3.shape
    assert rows == B * n and 1 <= T <= cfg.seq_length
    rw = (torch.randn(rows, 1, generator=torch.Generator().manual_seed(3)) * 1.5).to(dev)
    att_a = [a.to(dev).requires_grad_(True) for a in att]
    loss, grads, last = _fused(model, fcd, att_a, topd, seq3, rw, n, ENTROPY_REG, att_lens=lens)
    d_att = [a.grad.detach().clone() for a in att_a]
    att_b = [a.to(dev).requires_grad_(True) for a in att]
    loss2, grads2, seq_lp2 = _two_call(model, cfg, fcd, att_b, topd, seq3, rw, n, ENTROPY_REG, att_lens=lens)
    assert abs(float(loss.detach()) - float(loss2)) < 1e-4 * max(1.0, abs(float(loss2)))
    assert maxerr(last['logprobs'], seq_lp2.cpu()) < LOGP_TOL
    _same(grads, grads2, 'n=3/%s' % name)
    _same({'att%d' % i: g for i, g in enumerate(d_att)}, {'att%d' % i: a.grad for i, a in enumerate(att_b)}, 'n=3/%s/att_feats' % name)
    assert all(float(g.abs().max()) > 0 for g in d_att)
    # (rows, 1) and (rows, T) rewards are the same call
    loss_t, grads_t, _ = _fused(model, fcd, _to(att, dev), topd, seq3, rw.expand(rows, T).contiguous(), n, ENTROPY_REG, att_lens=lens)
    assert torch.equal(loss_t, loss) and all(torch.equal(grads_t[k], grads[k]) for k in grads)


def test_training_mode_dropout_masks_follow_the_torch_seed_and_a_second_backward_recomputes(dev):
    cfg, P, fc, att, top, seq, reward = _golden('mid', dev)
    cfg.drop_prob_lm, cfg.drop_prob_reason, cfg.drop_prob_fusion = 0.3, 0.2, 0.1
    model = build(cfg, P, dev, train=True)
    fcd, attd, topd, seqd = _to(fc, dev), _to(att, dev), top.to(dev), seq.to(dev)
    rwd = reward.expand(*seq.shape).contiguous().to(dev)
    loss2, want, _ = _two_call(model, cfg, fcd, attd, topd, seqd, rwd, 1, ENTROPY_REG, seed=3)
    torch.manual_seed(3)
    loss, _ = model.rl_loss(fcd, attd, seqd, rwd, topd, entropy_reg=ENTROPY_REG)
    model.zero_grad(set_to_none=True)
    (loss * 0.75).backward(retain_graph=True)           # the upstream gradient reaches d logits through the device scalar
    got = _grads_of(model)
    assert abs(float(loss.detach()) - float(loss2)) < 1e-4 * max(1.0, abs(float(loss2)))
    _same(got, {k: 0.75 * v for k, v in want.items()}, 'dropout')
    # not vacuous: another seed draws other masks
    _, other, _ = _fused(model, fcd, attd, topd, seqd, rwd, 1, ENTROPY_REG, seed=4, scale=0.75)
    assert compare_grads(other, {k: 0.75 * v for k, v in want.items()}, grad_bar, check=False)['ratio'] > 10.0
    # a second backward over the retained graph recomputes the pass: the first one overwrote the logits with their gradient
    model.zero_grad(set_to_none=True)
    (loss * 0.75).backward()
    _same(_grads_of(model), got, 'second backward')


def test_refusals_by_name_before_any_launch(dev):
    import copy
    import recurrent_fusion_network_amd as R
    import recurrent_fusion_network_amd._native as N
    cfg, P, fc, att, top, seq, reward = _golden('tiny0', dev)
    model = build(cfg, P, dev)
    fcd, attd, topd, seqd = _to(fc, dev), _to(att, dev), top.to(dev), seq.to(dev)
    rows, T = seq.shape
    rwd = reward.expand(rows, T).contiguous().to(dev)
    long_seq = torch.ones(rows, cfg.seq_length + 1, dtype=torch.long, device=dev)
    with pytest.raises(N.RfnError, match='seq_length'):
        model.rl_loss(fcd, attd, long_seq, torch.ones(rows, 1, device=dev), topd)
    with pytest.raises(N.RfnError, match='seq must be int64'):
        model.rl_loss(fcd, attd, seqd[:-1], rwd[:-1], topd)
    with pytest.raises(N.RfnError, match='seq must be int64'):
        model.rl_loss(fcd, attd, seqd.int(), rwd, topd)
    with pytest.raises(N.RfnError, match='seq must be int64'):
        model.rl_loss(fcd, attd, seqd, rwd, topd, n=2)                     # rows != images * n
    with pytest.raises(N.RfnError, match='reward must be'):
        model.rl_loss(fcd, attd, seqd, rwd[:, :-1] if T > 2 else rwd[:1], topd)
    with pytest.raises(N.RfnError, match='old_logprobs must be'):
        model.rl_loss(fcd, attd, seqd, rwd, topd, old_logprobs=rwd[:, :1])
    with pytest.raises(ValueError, match='n >= 1'):
        model.rl_loss(fcd, attd, seqd, rwd, topd, n=0)
    model.path_flags = N.PATH_OPT_DEC_UNHOISTED
    with pytest.raises(N.RfnError, match='hoisted decoder cell'):
        model.rl_loss([f.repeat_interleave(1, 0) for f in fcd], attd, seqd.repeat_interleave(2, 0), rwd.repeat_interleave(2, 0), topd, n=2)
    model.path_flags = 0
    model.fixed_decoder_steps = 3                                          # what a GraphedTrainStep sets while it owns the model
    with pytest.raises(N.RfnError, match='GraphedTrainStep'):
        model.rl_loss(fcd, attd, seqd, rwd, topd)
    model.fixed_decoder_steps = None
    mcfg = copy.copy(cfg)
    mcfg.use_mos, mcfg.num_expert = 1, 3
    mos = R.RecurrentFusionModel(mcfg).to(dev)
    with pytest.raises(ValueError, match='use_mos: rl_loss'):
        mos.rl_loss(fcd, attd, seqd, rwd, topd)
    assert model.last_rl is None                                           # nothing ran


def test_sample_group_bits_are_untouched_by_rl_loss(dev):
    """A model on which rl_loss was never called gives the same sample_group bits -- tokens, log-probs, loss and every gradient --
    before and after the new entry points have run in the process (compared with tensors kept in this test run)."""
    cfg, P, fc, att, top, seq, reward = _golden('odd', dev)
    fcd, attd, topd = _to(fc, dev), _to(att, dev), top.to(dev)
    B, n = fc[0].size(0), 2

    def group_step():
        import recurrent_fusion_network_amd as R
        model = build(cfg, P, dev)
        torch.manual_seed(11)
        s, lp, lp_all, reason = model.sample_group(fcd, attd, n)
        rw = (torch.randn(s.size(0), 1, generator=torch.Generator().manual_seed(2)) * 1.5).to(dev).expand(*s.shape).contiguous()
        loss = R.ReviewNetRewardCriterion(cfg)(lp, s, rw, lp_all, ENTROPY_REG, reason, topd, 1.0, None, cfg)
        loss.backward()
        return s.clone(), lp.detach().clone(), lp_all.detach().clone(), loss.detach().clone(), _grads_of(model)

    before = group_step()
    other = build(cfg, P, dev)
    s = before[0]
    _fused(other, fcd, attd, topd, s.contiguous(), torch.ones(s.size(0), 1, device=dev), n, ENTROPY_REG)
    after = group_step()
    for a, b in zip(before[:4], after[:4]):
        assert torch.equal(a, b)
    assert all(torch.equal(before[4][k], after[4][k]) for k in before[4])
