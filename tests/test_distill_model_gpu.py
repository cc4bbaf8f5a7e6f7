"""RecurrentFusionModel.forward_loss(..., teacher=) -- the distillation loss straight from the logits (rfn_kd_logits_fwd / _bwd) --
against the torch composition of the same definition on `model(...)`'s log-probs, with the bounds of test_forward_loss_gpu.py;
self-distillation, kd_alpha = 0, and EnsembleDecoder.teacher_logits as the teacher."""
import numpy as np
import pytest
import torch

from conftest import load_case
from test_model_gpu import build, to_dev

pytestmark = pytest.mark.gpu

TIERS = ['tiny0', 'odd', 'mid']


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def perturbed(P, seed, scale=0.05):
    """The tier's parameters plus scale * randn from a fixed seed: a teacher near the student, so that the kd gradients are
    O(1) and nothing cancels."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    return {k: v + scale * torch.randn(v.shape, generator=g, dtype=v.dtype) for k, v in P.items()}


def teacher_of(cfg, P, dev, batch, seed=11):
    fc, att, labels, masks, top = batch
    with torch.no_grad():
        return build(cfg, perturbed(P, seed), dev)(fc, att, labels)[0]


def composed(model, crit, batch, teacher, alpha, temperature, scale=1.0):
    """The definition (rfn.h) in torch ops on the model's log-probs, plus the criterion's reason term; backward run."""
    from recurrent_fusion_network_amd.criteria import _MLMFn
    fc, att, labels, masks, top = batch
    model.zero_grad()
    lp, reason = model(fc, att, labels)
    B, S, V1 = lp.shape
    eps = float(crit.label_smoothing_epsilon) if crit.use_label_smoothing else 0.0
    it = float(np.float32(1.0 / temperature))
    m = masks[:, 1:S + 1].float()
    q = torch.full_like(lp, eps / V1)
    q.scatter_(2, labels[:, 1:S + 1].unsqueeze(2), 1 - eps + eps / V1)
    xe = (m * -(q * lp).sum(2)).sum() / B
    z = teacher[:, :S]
    log_pt, log_ps = torch.log_softmax(z * it, 2), torch.log_softmax(lp * it, 2)
    kd = (m * (log_pt.exp() * (log_pt - log_ps)).sum(2)).sum() / (it * it) / B
    loss = (1 - alpha) * xe + alpha * kd + _MLMFn.apply(1.0 / len(reason), top, *reason)
    (loss * scale).backward()
    return loss.detach().clone(), xe.detach().clone(), kd.detach().clone(), grads_of(model)


def assert_grads(got, want, tag):
    for k, w in want.items():
        tol = 1e-7 + 2e-5 * float(w.abs().max())
        err = float((got[k] - w).abs().max())
        assert err <= tol, (tag, k, err, tol)


@pytest.mark.parametrize('name', TIERS)
@pytest.mark.parametrize('smooth', [0, 1])
def test_fused_distillation_equals_the_composed_form(dev, name, smooth):
    import recurrent_fusion_network_amd as R
    cfg, spec, P, batch, gold = load_case(name)
    cfg.use_label_smoothing = smooth
    batch = to_dev(batch, dev)
    fc, att, labels, masks, top = batch
    crit = R.ReviewNetEnsembleCriterion(cfg)
    model = build(cfg, P, dev)
    t = teacher_of(cfg, P, dev, batch)
    want_loss, want_xe, want_kd, want = composed(model, crit, batch, t, 0.5, 2.0)
    model.zero_grad()
    version = t._version
    loss, reason = model.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=t, kd_alpha=0.5, kd_temperature=2.0)
    assert len(reason) == model.num_feat_array + 1
    loss.backward()
    loss = loss.detach()
    got = grads_of(model)
    ld = model.last_distill
    print('%s smooth %d: loss %.7g (composed %.7g)  xe %.7g (%.7g)  kd %.7g (%.7g)'
          % (name, smooth, float(loss.detach()), float(want_loss), float(ld['xe']), float(want_xe), float(ld['kd']), float(want_kd)))
    assert abs(float(loss) - float(want_loss)) <= 2e-6 * max(1.0, abs(float(want_loss)))
    assert ld['xe'].dim() == 0 and ld['kd'].dim() == 0 and ld['xe'].device == loss.device and not ld['kd'].requires_grad
    assert abs(float(ld['xe']) - float(want_xe)) <= 2e-6 * max(1.0, abs(float(want_xe)))
    assert abs(float(ld['kd']) - float(want_kd)) <= 2e-6 * max(1.0, abs(float(want_kd)))
    assert float(want_kd) > 1e-4                             # the teacher differs: there is a kd term to get wrong
    assert_grads(got, want, name)
    assert t.grad is None and t._version == version          # a constant, left alone


def test_distillation_in_training_mode_with_dropout_and_a_scaled_loss(dev):
    """The same dropout seed (torch RNG) gives both forms the same masks; the loss scale reaches d logits through the device
    scalar; a second backward over the retained graph recomputes the pass."""
    import recurrent_fusion_network_amd as R
    cfg, spec, P, batch, gold = load_case('mid')
    cfg.drop_prob_lm, cfg.drop_prob_reason, cfg.drop_prob_fusion = 0.3, 0.2, 0.1
    batch = to_dev(batch, dev)
    fc, att, labels, masks, top = batch
    crit = R.ReviewNetEnsembleCriterion(cfg)
    t = teacher_of(cfg, P, dev, batch)
    model = build(cfg, P, dev, train=True)
    torch.manual_seed(3)
    want_loss, _, _, want = composed(model, crit, batch, t, 0.5, 2.0, scale=0.75)
    torch.manual_seed(3)
    model.zero_grad()
    loss, _ = model.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=t, kd_alpha=0.5, kd_temperature=2.0)
    assert abs(float(loss.detach()) - float(want_loss)) <= 2e-6 * max(1.0, abs(float(want_loss)))
    (loss * 0.75).backward(retain_graph=True)
    assert_grads(grads_of(model), want, 'first backward')
    model.zero_grad()
    (loss * 0.75).backward()
    assert_grads(grads_of(model), want, 'second backward')


@pytest.mark.parametrize('name', TIERS)
@pytest.mark.parametrize('temperature', [1.0, 2.0])
def test_self_distillation_has_no_kd_term(dev, name, temperature):
    """The teacher is the student's own no-grad log-probs: kd vanishes and the language gradients are (1 - alpha) times those
    of the plain call (the reason term is switched off in both calls: it is not scaled by 1 - alpha)."""
    import recurrent_fusion_network_amd as R
    cfg, spec, P, batch, gold = load_case(name)
    fc, att, labels, masks, top = to_dev(batch, dev)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    model = build(cfg, P, dev)
    alpha = 0.25
    model.zero_grad()
    plain, _ = model.forward_loss(fc, att, labels, masks, top, crit, 0.0)
    plain.backward()
    want = {k: (1 - alpha) * v for k, v in grads_of(model).items()}
    with torch.no_grad():
        t = model(fc, att, labels)[0]
    model.zero_grad()
    loss, _ = model.forward_loss(fc, att, labels, masks, top, crit, 0.0, teacher=t, kd_alpha=alpha, kd_temperature=temperature)
    loss.backward()
    xe, kd = float(model.last_distill['xe']), float(model.last_distill['kd'])
    print('%s T %g: xe %.7g  kd %.3e  (bound %.3e)' % (name, temperature, xe, kd, 1e-6 * abs(xe)))
    assert abs(kd) <= 1e-6 * abs(xe)
    assert xe == float(plain.detach())                       # the xe term is the plain call's language loss, bit for bit
    assert_grads(grads_of(model), want, name)


@pytest.mark.parametrize('name', TIERS)
def test_alpha_zero_with_a_teacher_is_the_call_without_one(dev, name):
    import recurrent_fusion_network_amd as R
    cfg, spec, P, batch, gold = load_case(name)
    cfg.use_label_smoothing = 1
    batch = to_dev(batch, dev)
    fc, att, labels, masks, top = batch
    crit = R.ReviewNetEnsembleCriterion(cfg)
    model = build(cfg, P, dev)
    t = teacher_of(cfg, P, dev, batch)
    model.zero_grad()
    a, _ = model.forward_loss(fc, att, labels, masks, top, crit, 1.0)
    a.backward()
    want = grads_of(model)
    assert model.last_distill is None
    model.zero_grad()
    b, _ = model.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=t, kd_alpha=0.0, kd_temperature=2.0)
    b.backward()
    got = grads_of(model)
    assert torch.equal(a, b) and model.last_distill['kd'] is None
    for k, w in want.items():
        assert torch.equal(got[k], w), k


def test_ensemble_teacher(dev):
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.ensemble import EnsembleDecoder
    cfg, spec, P, batch, gold = load_case('odd')
    batch = to_dev(batch, dev)
    fc, att, labels, masks, top = batch
    crit = R.ReviewNetEnsembleCriterion(cfg)
    student = build(cfg, P, dev)
    m1, m2 = build(cfg, perturbed(P, 11), dev), build(cfg, perturbed(P, 12), dev)
    S, V1 = student._decoder_steps(labels), cfg.vocab_size + 1
    B = labels.size(0)
    # one member: its logits are its log-probs up to a per-row shift, so the losses agree to rounding
    t1 = EnsembleDecoder([m1]).teacher_logits(fc, att, labels)
    assert tuple(t1.shape) == (B, S, V1) and tuple(t1.stride()) == (V1, B * V1, 1) and t1.transpose(0, 1).is_contiguous()
    assert not t1.requires_grad
    with torch.no_grad():
        lp1 = m1(fc, att, labels)[0]
    shift = (t1 - lp1).amax(2) - (t1 - lp1).amin(2)
    assert float(shift.max()) < 1e-4                         # the same rows up to a constant
    a, _ = student.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=t1, kd_alpha=0.5, kd_temperature=2.0)
    b, _ = student.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=lp1, kd_alpha=0.5, kd_temperature=2.0)
    print('one-member ensemble teacher: loss %.7g, forward log-probs: %.7g' % (float(a.detach()), float(b.detach())))
    assert abs(float(a.detach()) - float(b.detach())) <= 2e-6 * abs(float(b.detach()))
    # two members: the mean of the members' logits
    t2 = EnsembleDecoder([m2]).teacher_logits(fc, att, labels)
    t12 = EnsembleDecoder([m1, m2]).teacher_logits(fc, att, labels)
    assert tuple(t12.shape) == (B, S, V1) and t12.transpose(0, 1).is_contiguous()
    assert float((t12 - 0.5 * (t1 + t2)).abs().max()) < 1e-5
    assert float((t1 - t2).abs().max()) > 1e-3               # the members differ
    loss, _ = student.forward_loss(fc, att, labels, masks, top, crit, 1.0, teacher=t12)
    loss.backward()
    assert torch.isfinite(loss) and float(student.last_distill['kd']) > 0
