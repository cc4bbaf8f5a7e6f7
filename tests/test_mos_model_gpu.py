"""GPU: RecurrentFusionModel with opt.use_mos = 1 (a mixture-of-softmaxes head in place of log_softmax(logit(h)),
misc/ReviewNetModel.py:59-60,122-125): forward against the fp64 restatement applied to the decoder's own hidden rows, the loss
form against forward + criterion, decoding self-consistency, the ensemble, the optimizer bucket, the refusals."""
import copy
import os

import numpy as np
import pytest
import torch

import mos_cpu as MC
from conftest import load_case
from test_model_gpu import to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3


def build_mos(name, dev, train=False, **extra):
    """The golden configuration `name` with use_mos = 1, num_expert = 3: the tier's weights, and head weights of the scale the
    kernel tests use (tests/mos_cpu.random_params), so that the distributions are far from uniform."""
    import recurrent_fusion_network_amd as R
    cfg, spec, P, batch, gold = load_case(name)
    cfg = copy.copy(cfg)
    cfg.use_mos, cfg.num_expert = 1, K
    for k, v in extra.items():
        setattr(cfg, k, v)
    model = R.RecurrentFusionModel(cfg)
    head = MC.random_params(cfg.rnn_size, cfg.rnn_size, K, cfg.vocab_size + 1, 31)
    sd = dict(P)
    sd.update({'mos.' + k: v for k, v in head.items()})
    model.load_state_dict(sd)
    model = model.to(dev)
    model.train(train)
    return cfg, model, head, to_dev(batch, dev)


@pytest.mark.parametrize('name', ['tiny0', 'odd'])
def test_forward_equals_the_restatement_on_the_hidden_rows(dev, name):
    cfg, model, head, (fc, att, labels, masks, top) = build_mos(name, dev)
    with torch.no_grad():
        log_prob, reason = model(fc, att, labels)
        hid = model.decoder_hidden(fc, att, labels)
    B, S, V1 = log_prob.shape
    assert hid.shape == (B, S, cfg.rnn_size) and V1 == cfg.vocab_size + 1 and len(reason) == model.num_feat_array + 1
    ref = MC.log_prob(head, hid.cpu().reshape(B * S, -1)).view(B, S, V1)
    assert float((log_prob.double().cpu() - ref).abs().max()) <= 1e-5
    assert float((torch.exp(log_prob.double()).sum(2) - 1).abs().max()) <= 1e-5


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize('name', ['tiny0', 'odd'])
@pytest.mark.parametrize('smooth', [0, 1])
def test_forward_loss_equals_forward_plus_criterion(dev, name, smooth):
    import recurrent_fusion_network_amd as R
    cfg, model, head, (fc, att, labels, masks, top) = build_mos(name, dev, use_label_smoothing=smooth)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    model.zero_grad()
    lp, reason = model(fc, att, labels)
    want_loss = crit(lp, labels[:, 1:], masks[:, 1:], reason, top, 1.0)
    want_loss.backward()
    want = _grads(model)
    assert all(k in want for k in model.state_dict() if k.startswith('mos.'))
    assert float(want['mos.decoder.weight'].abs().max()) > 0 and float(want['logit.weight'].abs().max()) == 0.0
    model.zero_grad()
    got_loss, reason = model.forward_loss(fc, att, labels, masks, top, crit, 1.0)
    got_loss.backward()
    got = _grads(model)
    assert abs(float(got_loss.detach()) - float(want_loss.detach())) <= 2e-6 * max(1.0, abs(float(want_loss.detach())))
    for k, w in want.items():
        tol = 1e-7 + 2e-5 * float(w.abs().max())
        assert float((got[k] - w).abs().max()) <= tol, (k, float((got[k] - w).abs().max()), tol)


def _feed(seq, S):
    """The (B, S + 2) label matrix whose words are `seq` (column 0 = BOS, zeros behind the caption)."""
    lab = torch.zeros(seq.size(0), S + 2, dtype=torch.long, device=seq.device)
    lab[:, 1:1 + seq.size(1)] = seq
    return lab


@pytest.mark.parametrize('name', ['tiny0', 'odd'])
def test_greedy_beam_score_and_ensemble_are_consistent(dev, name):
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    cfg, model, head, (fc, att, labels, masks, top) = build_mos(name, dev)
    S = model.seq_length
    with torch.no_grad():
        seq, seq_lp, logp_all, _ = model.sample(fc, att, {'sample_max': 1})
        # feeding the returned sequence through forward: each row's argmax is the next token, seq_lp its log-prob
        lp, _ = model(fc, att, _feed(seq, S))
        n = seq.size(1)
        alive = torch.ones(seq.size(0), dtype=torch.bool, device=dev)
        for t in range(min(n, lp.size(1))):
            tok = lp[:, t].argmax(1)
            assert torch.equal((tok * alive)[alive], seq[:, t][alive]), t
            got = lp[:, t].gather(1, seq[:, t:t + 1]).squeeze(1)
            assert float((got - seq_lp[:, t])[alive].abs().max()) <= 1e-5
            alive = alive & (seq[:, t] > 0)
        # beam_size = 1 through sample_beam is greedy
        b_seq, b_lp, _, _, _ = model.sample_beam(fc, att, {'beam_size': 1})
        assert torch.equal(b_seq[:, :n], seq) and int(b_seq[:, n:].abs().sum()) == 0
        # a wider beam: its log-prob is model.score's, and no worse than greedy's
        w_seq, w_lp, top_seq, top_prob, _ = model.sample_beam(fc, att, {'beam_size': 3})
        sc = model.score(fc, att, w_seq, {'include_end': True})
        tok = sc['token_logprobs'][:, :w_lp.size(1)]          # a caption's words and its END, as the beam's seqLogprobs
        assert int((w_lp != 0).sum()) >= w_lp.size(0)
        assert float((tok - w_lp)[w_lp != 0].abs().max()) <= 1e-5
        assert bool((w_lp.double().sum(1) >= seq_lp.double().sum(1) - 1e-5 * S).all())
        # a one-member ensemble is the model, bit for bit
        ens = EnsembleDecoder([model])
        e_seq, e_lp, e_all = ens.sample(fc, att, {})
        assert torch.equal(e_seq, seq) and torch.equal(e_lp, seq_lp) and torch.equal(e_all, logp_all)
        eb_seq, eb_lp, _, _ = ens.sample_beam(fc, att, {'beam_size': 3})
        assert torch.equal(eb_seq, w_seq) and torch.equal(eb_lp, w_lp)
        # one_time_step hands out the same rows as the first greedy step
        comb, _, state = model.get_thought_vectors(fc, att)
        row, _ = model.one_time_step(torch.zeros(seq.size(0), dtype=torch.long, device=dev), fc, comb, state)
        assert float((torch.log_softmax(row, 1) - logp_all[:, 0]).abs().max()) <= 1e-5


def test_optimizer_bucket_hook_order_and_state_dict(dev):
    import recurrent_fusion_network_amd as R
    from oracle import rfn_oracle as O
    cfg, model, head, (fc, att, labels, masks, top) = build_mos('tiny0', dev)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    before = {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items() if k.startswith('mos.')}
    kw = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, grad_clip=1.0)
    opt = R.FusedClampAdam(model, **kw)
    assert model.bucket_names()[:2] == ['mos', 'decoder'] and 'mos' in opt.flat
    seen = []
    model.grad_ready_hook = lambda name, flat: seen.append(name)
    opt.zero_grad()
    loss, _ = model.forward_loss(fc, att, labels, masks, top, crit, 1.0)
    loss.backward()
    assert seen[:2] == ['mos', 'decoder'] and sorted(seen) == sorted(model.bucket_names())
    grads = {k: p.grad.detach().double().cpu().clone() for k, p in model.named_parameters() if k.startswith('mos.')}
    opt.step()
    after = dict(model.named_parameters())
    moved = 0
    for k, g in grads.items():
        want = O.clip_and_adam({k: before[k].clone()}, {k: g}, {}, **kw)[k]
        sel = g.abs() > 1e-5          # the first Adam step is lr * g / (|g| + eps): compare where |g| >> eps
        if bool(sel.any()):
            assert float((after[k].detach().double().cpu() - want)[sel].abs().max()) < 5e-6, k
            moved += 1
    assert moved >= 5
    # state_dict: the reference's keys and shapes under `mos.`, and the golden module's own dict loads
    V1, R_ = cfg.vocab_size + 1, cfg.rnn_size
    sd = model.state_dict()
    assert [k for k in sd if k.startswith('mos.')] == ['mos.' + k for k in MC.param_names(K)]
    assert sd['mos.prior.weight'].shape == (K, R_) and sd['mos.latent.2.0.weight'].shape == (R_, R_)
    assert sd['mos.latent.0.0.bias'].shape == (R_,) and sd['mos.decoder.weight'].shape == (V1, R_) and sd['mos.decoder.bias'].shape == (V1,)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'mos_ref.npz'))
    gold = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('t0.') and k[3:] not in ('h', 'prob')}
    mod = R.MixtureOfSoftmax(24, 24, 3, 37)
    mod.load_state_dict(gold)
    mod = mod.to(dev)
    p = mod(torch.from_numpy(z['t0.h']).to(dev))
    ref = torch.from_numpy(z['t0.prob'])
    live = ref >= 1e-30
    assert float((torch.log(p.detach().double().cpu()) - torch.log(ref.double()))[live].abs().max()) <= 1e-5
    # the stand-alone module is differentiable through autograd
    h = torch.from_numpy(z['t0.h']).to(dev).requires_grad_(True)
    mod.log_prob(h)[:, 5].sum().backward()
    b = MC.backward(gold, torch.from_numpy(z['t0.h']), torch.nn.functional.one_hot(torch.full((5,), 5), 37).double())
    assert float((h.grad.double().cpu() - b['d_h']).abs().max()) <= 1e-7 + 2e-5 * float(b['d_h'].abs().max())
    gw = mod.decoder.weight.grad.double().cpu()
    assert float((gw - b['grads']['decoder.weight']).abs().max()) <= 1e-7 + 2e-5 * float(b['grads']['decoder.weight'].abs().max())


def test_refused_combinations_raise_by_name(dev):
    import recurrent_fusion_network_amd as R
    import recurrent_fusion_network_amd._native as N
    from recurrent_fusion_network_amd.distill import TopKTeacher  # noqa: F401
    cfg, model, head, (fc, att, labels, masks, top) = build_mos('tiny0', dev)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    err = (ValueError, N.RfnError)
    model.ss_prob = 0.25
    with pytest.raises(err, match='ss_prob'):
        model(fc, att, labels)
    with pytest.raises(err, match='ss_prob'):
        model.forward_loss(fc, att, labels, masks, top, crit, 1.0)
    model.ss_prob = 0.0
    with torch.no_grad():
        with pytest.raises(err, match='sample_max'):
            model.sample(fc, att, {'sample_max': 0})
        with pytest.raises(err, match='sample_group'):
            model.sample_group(fc, att, 2)
        with pytest.raises(err, match='sample_distinct'):
            model.sample_distinct(fc, att, 2)
        with pytest.raises(err, match='require'):
            model.sample_beam(fc, att, {'beam_size': 2, 'require': [[[1, 2]]] * fc[0].size(0)})
    with pytest.raises(err, match='under grad'):
        model.sample(fc, att, {'sample_max': 1})
    with pytest.raises(err, match='teacher'):
        model.forward_loss(fc, att, labels, masks, top, crit, 1.0,
                           teacher=torch.zeros(labels.size(0), labels.size(1), cfg.vocab_size + 1, device=dev))
    model.dedup_seq_per_img = 2
    with pytest.raises(err, match='dedup_seq_per_img'):
        model(fc, att, labels)
    model.dedup_seq_per_img = 0
    with pytest.raises(err, match='use_mos'):
        R.GraphedTrainStep(model, crit, R.FusedClampAdam(model, lr=0.0), fc, att, labels, masks, top)
    for bit in (N.PATH_OPT_PERSIST_DEC_FWD, N.PATH_OPT_PERSIST_S2_BWD, N.PATH_OPT_DEC_UNHOISTED):
        model.path_flags = bit
        with pytest.raises(err, match='RFN_PATH_OPT'):
            model(fc, att, labels)
        with torch.no_grad(), pytest.raises(err, match='RFN_PATH_OPT'):
            model.sample(fc, att, {'sample_max': 1})
    model.path_flags = 0
    with pytest.raises(ValueError, match='num_expert'):
        c2 = copy.copy(cfg)
        c2.num_expert = 17
        R.RecurrentFusionModel(c2)


def test_a_model_without_the_option_is_unchanged(dev):
    import recurrent_fusion_network_amd as R
    cfg, spec, P, batch, gold = load_case('tiny0')
    fc, att, labels, masks, top = to_dev(batch, dev)
    assert not hasattr(cfg, 'use_mos')
    c0 = copy.copy(cfg)
    c0.use_mos, c0.num_expert = 0, 10
    outs = []
    for c in (cfg, c0):
        model = R.RecurrentFusionModel(c)
        model.load_state_dict(P)
        model = model.to(dev).eval()
        assert not hasattr(model, 'mos') and model.bucket_names()[0] == 'decoder'
        assert not any(k.startswith('mos.') for k in model.state_dict())
        with torch.no_grad():
            outs.append(model(fc, att, labels)[0])
    assert torch.equal(outs[0], outs[1])
