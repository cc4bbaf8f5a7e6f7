"""Self-critical RL gradients of the HIP path, element-wise, through the pass that training differentiates.

Every case compares EVERY element of EVERY parameter gradient with the CPU oracle (oracle/rfn_oracle.py
rl_step_loss_and_grads, pinned to the reference's own RL gradients by tests/test_rl_oracle_cpu.py) at the project's bar
1e-5 + 1e-3 * max|g_oracle| per tensor, log-probs within LOGP_TOL, the loss within 1e-4 * max(1, |loss|), equal key sets.

  a. the reference's drawn ids replayed through `force_ids`, every RL golden tier, c2 on both GEMM modes;
  b. `sample(sample_max=0)` as train_rl.py calls it -- the step-wise sampled pass (rfn_decoder_fwd_sampled), eval mode and
     training mode with dropout 0.1 / 0.2 / 0.3: its gradients equal, BIT FOR BIT, those of a batched teacher-forced pass on the
     tokens it fed (the header's promise that the sampled pass "leaves the workspace ready for rfn_decoder_bwd"), every
     drawn token is the inverse CDF of the previous step's distribution at its uniform, and the gradients agree with the
     oracle given the product's own dropout masks; the same identity for forward() with ss_prob = 0.25;
  c. the PPO surrogate and the dense entropy term through the whole model;
  d. early-exit and finished-row shapes by constructed ids;
  e. the sizes the benchmark runs: c5 at B = 128 and c2 at B = 64 (tile and block variants follow the row count).

With RFN_RL_PARITY_JSON set to a path, every case appends its measured figures there (profiles/rl_grad_parity.json is
such a run)."""
import json
import os
import time

import pytest
import torch

from conftest import load_case, load_drop_case
from rl_grad_check import RL_TIERS, compare_grads, fed_from_raw, grad_bar, load_rl_case
from test_dropout_parity_gpu import product_masks
from test_model_gpu import LOGP_TOL, _gemm_mode, build, maxerr

pytestmark = pytest.mark.gpu

ENTROPY_REG = 0.01


def _record(case, **figures):
    path = os.environ.get('RFN_RL_PARITY_JSON')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, **figures), sort_keys=True) + '\n')


def _to(ts, dev):
    return [t.to(dev) for t in ts]


def _row_reward(B, seed):
    return torch.randn(B, 1, generator=torch.Generator().manual_seed(seed)) * 1.5


def _grads_of(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def _criterion_backward(model, cfg, seq, seq_lp, lp_all, reason, reward_row, top, entropy_reg, old=None):
    """ReviewNetRewardCriterion + backward from clean gradients -> (loss, {name: grad})."""
    import recurrent_fusion_network_amd as R
    dev = seq_lp.device
    reward = reward_row.reshape(seq.size(0), -1).to(dev)
    if reward.size(1) == 1:
        reward = reward.expand(seq.size(0), seq.size(1)).contiguous()
    loss = R.ReviewNetRewardCriterion(cfg)(seq_lp, seq, reward, lp_all, entropy_reg, reason, top.to(dev), 1.0, old, cfg)
    model.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach(), _grads_of(model)


def _against_oracle(case, got, want, oracle_seconds, **extra):
    """got = (loss, grads, seq, seq_lp, lp_all) of the product, want = the oracle's: every figure, then every assertion."""
    loss, grads, seq, seq_lp, lp_all = got
    o_loss, o_grads, o_seq, o_lp, o_all = want
    assert tuple(seq.shape) == tuple(o_seq.shape) and tuple(lp_all.shape) == tuple(o_all.shape), (seq.shape, o_seq.shape)
    assert torch.equal(seq.cpu(), o_seq)
    lp_err = max(maxerr(lp_all, o_all), maxerr(seq_lp, o_lp))
    loss_err = abs(float(loss) - float(o_loss))
    rep = compare_grads(grads, o_grads, grad_bar, check=False)
    print('%s: worst err/bar %.4f at %s%s (got %r want %r), log-prob err %.3g, loss err %.3g, oracle %.1f s' % (
        case, rep['ratio'], rep['name'], list(rep['index'] or ()), rep['got'], rep['want'], lp_err, loss_err, oracle_seconds))
    _record(case, worst_ratio=rep['ratio'], worst_tensor=rep['name'], logprob_err=lp_err, loss_err=loss_err,
            oracle_cpu_seconds=round(oracle_seconds, 2), steps=int(lp_all.size(1)), rows=int(seq.size(0)), **extra)
    assert set(grads) == set(o_grads)
    assert lp_err < LOGP_TOL
    assert loss_err < 1e-4 * max(1.0, abs(float(o_loss)))
    assert not rep['failures'], rep['failures'][:10]
    assert rep['ratio'] <= 1.0
    return rep


def _oracle(cfg, P, fc, att, fed, reward_row, top, entropy_reg=ENTROPY_REG, old=None, drop=None, dtype=torch.float64):
    from oracle import rfn_oracle as O
    t0 = time.time()
    out = O.rl_step_loss_and_grads(cfg, P, fc, att, fed.cpu(), reward_row, top, entropy_reg, 1.0, old_logprobs=old, drop=drop,
                                   dtype=dtype)
    return out, time.time() - t0


# ---------------------------------------------------------------------------------------------------------------
# a. forced ids, eval mode
# ---------------------------------------------------------------------------------------------------------------
def _forced_run(model, cfg, fc, att, top, raw, reward, dev, entropy_reg=ENTROPY_REG, old_of=None):
    seq, seq_lp, lp_all, reason = model.sample(_to(fc, dev), _to(att, dev), {'sample_max': 0, 'force_ids': raw})
    old = None if old_of is None else old_of(seq_lp.detach())
    loss, grads = _criterion_backward(model, cfg, seq, seq_lp, lp_all, reason, reward, top, entropy_reg, old)
    return (loss, grads, seq, seq_lp.detach(), lp_all.detach()), old


@pytest.mark.parametrize('name,gemm', [(n, 'exact') for n in RL_TIERS] + [('c2', 'bf16x3')])
def test_forced_ids_every_gradient_element_against_the_fp64_oracle(dev, name, gemm):
    cfg, P, fc, att, top, gold = load_rl_case(name)
    model = _gemm_mode(build(cfg, P, dev), gemm)
    raw, reward = torch.from_numpy(gold['rl_raw_ids']), torch.from_numpy(gold['rl_reward'])
    got, _ = _forced_run(model, cfg, fc, att, top, raw, reward, dev)
    assert torch.equal(got[2].cpu(), torch.from_numpy(gold['rl_seq']))
    want, secs = _oracle(cfg, P, fc, att, fed_from_raw(raw), reward, top)
    _against_oracle('forced/%s/%s' % (name, gemm), got, want, secs)


# ---------------------------------------------------------------------------------------------------------------
# b. the sampled pass is the pass that is differentiated
# ---------------------------------------------------------------------------------------------------------------
def _case(name, train):
    """(cfg, P, batch) of a tier; training mode: with the drop tier's 0.1 / 0.2 / 0.3."""
    from oracle import make_golden as G
    if train and name in G.DROP_TIERS:
        cfg, spec, P, batch, gold, _ = load_drop_case(name)
    else:
        cfg, spec, P, batch, gold = load_case(name)
        if train:
            for k, v in G.DROP_PROBS.items():
                setattr(cfg, k, v)
    return cfg, P, batch


def _inverse_cdf_ok(lp_all, fed, u_draw, shift=0):
    """(B, T-1) bool: token fed[:, t] is the inverse CDF of exp(lp_all[:, t-1]) at u_draw[t - shift] (fp64 cumulative sum of
    the product's own log-probs, the 2e-6 * total slack of test_multinomial_pick_is_the_inverse_cdf_of_its_uniform)."""
    T = fed.size(1)
    cdf = torch.cumsum(torch.exp(lp_all.detach().double().cpu()[:, :T - 1]), 2)           # (B, T-1, V1)
    total = cdf[:, :, -1]
    v = fed.cpu()[:, 1:T]
    hi = cdf.gather(2, v.unsqueeze(2)).squeeze(2)
    lo = torch.where(v > 0, cdf.gather(2, (v - 1).clamp(min=0).unsqueeze(2)).squeeze(2), torch.zeros_like(hi))
    tgt = u_draw.double().cpu()[1 - shift:T - shift].t() * total
    tol = 2e-6 * total
    return (lo - tol <= tgt) & (tgt <= hi + tol)


def _sampled_run(model, cfg, fcd, attd, top, train, torch_seed, reward_row, dev):
    """sample(sample_max=0) with known uniforms, criterion, backward; then the same graph built the other way (phase 1 and a
    batched teacher-forced pass on the tokens the sampled pass fed) under the same seed.
    -> (product result, fed ids, dropout seed, the replay's result, u)"""
    from recurrent_fusion_network_amd.fusion_model import _fresh_seed
    B, S = fcd[0].size(0), cfg.seq_length
    u = torch.rand(2, S + 1, B, generator=torch.Generator().manual_seed(torch_seed + 1000)).to(dev)
    torch.manual_seed(torch_seed)
    seed = _fresh_seed() if train else 0          # the seed sample() draws from torch's CPU generator in training mode
    torch.manual_seed(torch_seed)
    model._trace_ss, model._ss_uniforms = True, u
    try:
        seq, seq_lp, lp_all, reason = model.sample(fcd, attd, {'sample_max': 0})
    finally:
        model._ss_uniforms = None
    fed = model._sample_ids
    assert lp_all.requires_grad and tuple(fed.shape) == (B, lp_all.size(1)) and bool((fed[:, 0] == 0).all())
    loss, grads = _criterion_backward(model, cfg, seq, seq_lp, lp_all, reason, reward_row, top, ENTROPY_REG)
    got = (loss, grads, seq, seq_lp.detach(), lp_all.detach())
    # the other way round: _prefix + _decode_teacher_forced on the fed tokens, same derivation of seq / seqLogprobs
    comb, h, c, reason2 = model._prefix(fcd, attd, train, seed)
    logp = model._decode_teacher_forced(fed, comb, h, c, train, seed)
    n = fed.size(1) - 1
    tok = fed[:, 1:]
    seq2 = tok * torch.cumprod((tok > 0).long(), 1)
    seq_lp2 = logp[:, :n].gather(2, tok.unsqueeze(2)).squeeze(2)
    loss2, grads2 = _criterion_backward(model, cfg, seq2, seq_lp2, logp.contiguous(), list(reason2.unbind(0)), reward_row, top,
                                        ENTROPY_REG)
    return got, fed, seed, (loss2, grads2, seq2, seq_lp2.detach(), logp.detach()), u


def _identity(got, replay):
    """Which parts of two runs are equal bit for bit -> (all equal, [names that differ])."""
    assert set(got[1]) == set(replay[1])
    differ = [k for i, k in ((0, 'loss'), (2, 'seq'), (3, 'seq_lp'), (4, 'lp_all')) if not torch.equal(got[i], replay[i])]
    differ += [k for k in sorted(got[1]) if got[1][k] is None or replay[1][k] is None or not torch.equal(got[1][k], replay[1][k])]
    return not differ, differ


def _sampled_case(case, cfg, P, fc, att, top, train, dev, oracle_dtype, torch_seed=31):
    """One full check of (b): identity with the teacher-forced replay, inverse-CDF draws, oracle parity (+ non-vacuity)."""
    model = build(cfg, P, dev, train=train)
    B = fc[0].size(0)
    reward_row = _row_reward(B, torch_seed + 7)
    got, fed, seed, replay, u = _sampled_run(model, cfg, _to(fc, dev), _to(att, dev), top, train, torch_seed, reward_row, dev)
    same, differ = _identity(got, replay)
    # rfn_decoder_fwd_sampled: ids column s is drawn from step s - 1's log-probs with u_draw[s] = uniforms[0][s] (row 0 of
    # u_draw is never read; uniforms[1] are the scheduled-sampling coins, all below ss_prob = 1 here)
    ok = _inverse_cdf_ok(got[4], fed, u[0])
    shifted = _inverse_cdf_ok(got[4], fed, u[0], shift=1)
    dropping = train and max(cfg.drop_prob_fusion, cfg.drop_prob_reason, cfg.drop_prob_lm) > 0
    drop = product_masks(cfg, B, fed.size(1), seed, dev) if dropping else None
    want, secs = _oracle(cfg, P, fc, att, fed, reward_row, top, drop=drop, dtype=oracle_dtype)
    rep = _against_oracle(case, got, want, secs, replay_bit_identical=bool(same), replay_differs=differ[:8],
                          inverse_cdf_draws=int(ok.numel()), inverse_cdf_misses=int((~ok).sum()))
    assert same, 'the sampled pass and the teacher-forced replay differ in %s' % differ[:8]
    assert bool(ok.all()), 'drawn tokens that are not the inverse CDF at their uniform: rows/steps %s' % (~ok).nonzero().tolist()[:8]
    assert not bool(shifted.all()), 'the draws do not tell which row of u_draw served which step'
    if dropping:
        # not vacuous: without the product's masks the oracle is far from this run
        eval_want, _ = _oracle(cfg, P, fc, att, fed, reward_row, top, drop=None, dtype=oracle_dtype)
        assert compare_grads(got[1], eval_want[1], grad_bar, check=False)['ratio'] > 10.0
    return rep


@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('name', ['mid', 'tinymax', 'c2'])
def test_sampled_pass_gradients_are_the_teacher_forced_replays_and_the_oracles(dev, name, train):
    """Bit-identity of the step-wise sampled pass and the batched pass, through backward: both leave the same workspace and
    the backward launch (rfn_decoder_bwd, same B and S, same seed) is the same call, so every gradient is torch.equal."""
    cfg, P, batch = _case(name, train)
    fc, att, labels, masks, top = batch
    _sampled_case('sampled/%s/%s' % (name, 'train' if train else 'eval'), cfg, P, fc, att, top, train, dev, torch.float64)


@pytest.mark.parametrize('name', ['mid', 'tinymax', 'c2'])
def test_scheduled_sampling_gradients_are_the_teacher_forced_replays(dev, name):
    """forward() with ss_prob = 0.25 (the published recipe) under dropout: the step-wise pass that draws between its steps
    must leave, bit for bit, the gradients of a batched teacher-forced pass on the tokens it ended up feeding
    (model._ss_ids), XE criterion.  Rows whose coin is below ss_prob got the inverse-CDF draw, the others kept their label."""
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.fusion_model import _fresh_seed
    cfg, P, batch = _case(name, True)
    fc, att, labels, masks, top = batch
    model = build(cfg, P, dev, train=True)
    fcd, attd, lab, msk, topd = _to(fc, dev), _to(att, dev), labels.to(dev), masks.to(dev), top.to(dev)
    B, S = labels.size(0), model._decoder_steps(lab)
    u = torch.rand(2, S, B, generator=torch.Generator().manual_seed(5)).to(dev)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    torch.manual_seed(41)
    seed = _fresh_seed()
    torch.manual_seed(41)
    model.ss_prob, model._trace_ss, model._ss_uniforms = 0.25, True, u
    try:
        lp, reason = model(fcd, attd, lab)
    finally:
        model._ss_uniforms = None
    fed = model._ss_ids
    loss = crit(lp, lab[:, 1:], msk[:, 1:], reason, topd, 1.0)
    model.zero_grad(set_to_none=True)
    loss.backward()
    grads = _grads_of(model)
    model.ss_prob = 0.0
    comb, h, c, reason2 = model._prefix(fcd, attd, True, seed)
    tf = model._decode_teacher_forced(fed, comb, h, c, True, seed)
    loss2 = crit(tf, lab[:, 1:], msk[:, 1:], list(reason2.unbind(0)), topd, 1.0)
    model.zero_grad(set_to_none=True)
    loss2.backward()
    grads2 = _grads_of(model)
    differ = [k for k in sorted(grads) if grads[k] is None or grads2[k] is None or not torch.equal(grads[k], grads2[k])]
    # the coins: uniforms[1][s][b] < ss_prob redraws column s (rfn_multinomial_pick), anything else keeps the label
    redrawn = (u[1] < 0.25).t().cpu()[:, 1:]
    kept = fed.cpu()[:, 1:] == labels[:, 1:S]
    ok = _inverse_cdf_ok(lp, fed, u[0])
    _record('scheduled_sampling/%s' % name, replay_bit_identical=not differ and torch.equal(tf, lp), replay_differs=differ[:8],
            redrawn=int(redrawn.sum()), inverse_cdf_misses=int((~ok & redrawn).sum()))
    assert tuple(fed.shape) == (B, S) and set(grads) == set(grads2) == set(P)
    assert torch.equal(tf.detach(), lp.detach()) and float(loss2.detach()) == float(loss.detach())
    assert not differ, 'the scheduled-sampling pass and the teacher-forced replay differ in %s' % differ[:8]
    assert int(redrawn.sum()) > 0 and int((~redrawn).sum()) > 0
    assert bool(kept[~redrawn].all()) and bool(ok[redrawn].all())
    assert not bool(kept[redrawn].all())


# ---------------------------------------------------------------------------------------------------------------
# c. PPO and the dense entropy term through the model
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mid', 'odd'])
def test_ppo_surrogate_and_entropy_term_through_the_whole_model(dev, name):
    """use_ppo = 1 (ppo_clip 0.2, old log-probs = the sample's + 0.3 * randn) with entropy_reg 0.01 and 0.0, each against the
    fp64 oracle element-wise.

    That the entropy term is exercised is shown on its own gradient D = g(0.01) - g(0.0) of logit.weight: the product's D
    must equal the oracle's within a tenth of the oracle's max|D| (a dropped, halved or sign-flipped entropy term misses that
    by 1.0, 0.5 and 2.0 of it).  The plainer form, "g(0.0) differs from g(0.01) by more than the gradient bar", is false
    for the ORACLE on these tiers: their uniform(+-0.1) weights give near-uniform distributions, where the entropy has no
    slope -- fp64 oracle max|D| is 9.8e-6 on `mid` and 9.0e-6 on `odd` against bars of 1.6e-4 and 3.8e-5 -- so that form
    would fail on a correct product.  The tenth: each fp32 gradient carries about 2^-24 * a few tens of accumulated terms *
    max|g| (0.15 on `mid`) ~ 1e-7 of error, two of them 2e-7, against 0.1 * 9e-6 = 9e-7."""
    cfg, P, fc, att, top, gold = load_rl_case(name)
    cfg.use_ppo, cfg.ppo_clip = 1, 0.2
    model = build(cfg, P, dev)
    raw = torch.from_numpy(gold['rl_raw_ids'])
    # the reference clamps ratio * reward to 1 +- ppo_clip (misc/utils.py:64-66), and ratio = exp(0.3 * randn) here: rows with a
    # reward near 1 sit on both sides of the clamp, rows with any other reward (the golden's are all below 0.3 on `mid`) only
    # outside it -- so every other row gets a reward of 1 +- 0.1, the rest keep a normal draw
    reward = _row_reward(raw.size(0), 21)
    reward[0::2] = 1.0 + 0.1 * torch.randn(reward[0::2].shape, generator=torch.Generator().manual_seed(22))
    reward = reward.expand(raw.size(0), gold['rl_seq'].shape[1]).contiguous()
    noise = torch.Generator().manual_seed(9)

    def old_of(seq_lp):
        return seq_lp + (0.3 * torch.randn(seq_lp.shape, generator=noise)).to(seq_lp.device)

    got, old = _forced_run(model, cfg, fc, att, top, raw, reward, dev, old_of=old_of)
    want, secs = _oracle(cfg, P, fc, att, fed_from_raw(raw), reward, top, old=old.cpu())
    # both branches of the surrogate carry gradient: the clamp (misc/utils.py:64-66) is active on some unmasked elements
    # and inactive on others
    seq, o_lp = want[2], want[3]
    mask = torch.cat([torch.ones(seq.size(0), 1, dtype=torch.bool), (seq > 0)[:, :-1]], 1)
    surr1 = torch.exp(o_lp) / (1e-5 + torch.exp(old.cpu().double())) * reward.double()
    clamped = (surr1 < 1 - cfg.ppo_clip) | (surr1 > 1 + cfg.ppo_clip)
    assert bool((clamped & mask).any()) and bool((~clamped & mask).any())
    _against_oracle('ppo/%s/entropy_0.01' % name, got, want, secs)
    got0, _ = _forced_run(model, cfg, fc, att, top, raw, reward, dev, entropy_reg=0.0, old_of=lambda lp: old)
    want0, secs0 = _oracle(cfg, P, fc, att, fed_from_raw(raw), reward, top, entropy_reg=0.0, old=old.cpu())
    _against_oracle('ppo/%s/entropy_0' % name, got0, want0, secs0)
    k = 'logit.weight'
    d_got, d_want = (got[1][k] - got0[1][k]).cpu(), want[1][k] - want0[1][k]
    d_max = float(d_want.abs().max())
    print('ppo/%s: entropy-only gradient of %s: oracle max %.3g, product off by %.3g; gradient bar %.3g' % (
        name, k, d_max, maxerr(d_got, d_want), grad_bar(want[1][k])))
    _record('ppo/%s/entropy_only' % name, oracle_max=d_max, product_err=maxerr(d_got, d_want), gradient_bar=grad_bar(want[1][k]))
    assert d_max > 0.0
    compare_grads({k: d_got}, {k: d_want}, lambda d: 0.1 * float(d.abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# d. early-exit and finished-row shapes
# ---------------------------------------------------------------------------------------------------------------
def _exit_ids(kind, B, S, V):
    raw = torch.randint(1, V + 1, (B, S), generator=torch.Generator().manual_seed(12))
    if kind == 'all_finish_by_step_3':          # the last rows draw their 0 from step 3's distribution: 4 decoder steps
        for b, z in enumerate([3, 1, 2, 3, 0, 1][:B]):
            raw[b, z] = 0                       # what follows stays non-zero: fed, never scored
        return raw, 3
    if kind == 'one_row_draws_0_first':
        raw[2, 0] = 0
        return raw, S
    if kind == 'no_row_finishes':
        return raw, S
    if kind == 'finished_rows_keep_drawing':
        raw[1, 4], raw[3, 9], raw[4, 0] = 0, 0, 0
        assert bool((raw[1, 5:] > 0).all()) and bool((raw[3, 10:] > 0).all())
        return raw, S
    raise KeyError(kind)


@pytest.mark.parametrize('kind', ['all_finish_by_step_3', 'one_row_draws_0_first', 'no_row_finishes', 'finished_rows_keep_drawing'])
def test_early_exit_and_finished_rows_against_the_fp64_oracle(dev, kind):
    cfg, P, fc, att, top, gold = load_rl_case('mid')
    B, S, V1 = fc[0].size(0), cfg.seq_length, cfg.vocab_size + 1
    raw, n_seq = _exit_ids(kind, B, S, cfg.vocab_size)
    reward = _row_reward(B, 3)
    model = build(cfg, P, dev)
    got, _ = _forced_run(model, cfg, fc, att, top, raw, reward, dev)
    assert tuple(got[2].shape) == (B, n_seq) and tuple(got[4].shape) == (B, n_seq + 1, V1)
    want, secs = _oracle(cfg, P, fc, att, fed_from_raw(raw), reward, top)
    _against_oracle('early_exit/%s' % kind, got, want, secs)
    if kind == 'finished_rows_keep_drawing':
        # the unmasked draws of the finished rows were fed: with zeros fed instead those rows' later log-probs move
        zeroed = raw * torch.cumprod((raw > 0).long(), 1)
        with torch.no_grad():
            lp0 = model.sample(_to(fc, dev), _to(att, dev), {'sample_max': 0, 'force_ids': zeroed})[2]
        assert maxerr(lp0[1, 6:], got[4][1, 6:].cpu()) > 10 * LOGP_TOL and torch.equal(lp0[0], got[4][0])


# ---------------------------------------------------------------------------------------------------------------
# e. the benchmarked sizes
# ---------------------------------------------------------------------------------------------------------------
def test_config5_rl_step_at_its_benchmarked_batch_128_every_gradient_element(dev):
    """The model of test_config5_at_its_stated_batch_128...: bench.py's c5 workload (M = 4, L = 196, D = 2048) at B = 128,
    training mode with dropout 0, through sample(sample_max=0) as the benchmark's c5_rl leg runs it; fp32 oracle on the fed
    tokens (tests/test_rl_oracle_cpu.py licenses fp32)."""
    import bench as HB
    from oracle import rfn_oracle as O
    w = HB.WORKLOADS['c5']
    assert w['B'] == 128
    cfg = HB.make_cfg(w)
    P = O.seeded_params(cfg, 71)
    fc, att, labels, masks, top = O.synthetic_batch(cfg, w['B'], seed=72)
    _sampled_case('benchmarked/c5_B128', cfg, P, fc, att, top, True, dev, None)


def test_config2_rl_step_at_batch_64_under_dropout_every_gradient_element(dev):
    import bench as HB
    from oracle import make_golden as G
    from oracle import rfn_oracle as O
    w = HB.WORKLOADS['c2']
    assert w['B'] == 64
    cfg = HB.make_cfg(w)
    for k, v in G.DROP_PROBS.items():
        setattr(cfg, k, v)
    P = O.seeded_params(cfg, 61)
    fc, att, labels, masks, top = O.synthetic_batch(cfg, w['B'], seed=62)
    _sampled_case('benchmarked/c2_B64_dropout', cfg, P, fc, att, top, True, dev, None)
