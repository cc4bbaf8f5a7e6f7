"""GraphedTrainStep(device_rng=True): the graph-replayed XE train step under the reference's training recipe -- dropout > 0
and scheduled sampling (train_recurrent_fusion_model.sh:15-29).

What changes per step lives in device memory the wrapper refills before each replay: the dropout seed (the cell kernels
read their Philox key from a one-element tensor: RFN_PATH_OPT_SEED_DEV / rfn_dropout_mask_dev, include/rfn.h) and the
(2, S, B) scheduled-sampling uniforms.  Both are drawn exactly as the eager forward draws them, so every comparison here is
bit for bit: masks, forward + backward of the path with the key handed over either way, and whole train steps (loss,
parameters, gradients, Adam moments) replayed against eager steps started from the same generator states."""
from unittest import mock

import pytest
import torch

from conftest import load_drop_case
from test_trainer_contract_gpu import build, load_case, to_dev

pytestmark = pytest.mark.gpu

OFF_STAGE2, OFF_DECODER = 1 << 20, 1 << 21        # RFN_DROP_OFFSET_STAGE2 / _DECODER (include/rfn.h)
KW = dict(lr=5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5, grad_clip=0.01)      # a clamp that bites, a big lr


def _mask(N, dev, n, p, offset, seed=None, seed_dev=None):
    keep = torch.full((n,), -1.0, device=dev)
    if seed_dev is not None:
        N.check(N.lib.rfn_dropout_mask_dev(seed_dev.data_ptr(), offset, n, p, keep.data_ptr(), N.stream_ptr()), 'rfn_dropout_mask_dev')
    else:
        N.check(N.lib.rfn_dropout_mask(seed, offset, n, p, keep.data_ptr(), N.stream_ptr()), 'rfn_dropout_mask')
    return keep


def test_mask_of_a_device_seed_equals_the_mask_of_the_same_value(dev):
    import recurrent_fusion_network_amd._native as N
    held = torch.zeros(1, dtype=torch.int64, device=dev)
    cases = [(1, 0, 1, 0.5), (0, 7, 300, 0.3), (2 ** 62 - 1, OFF_STAGE2 + 3, 50 * 512, 0.2), (0x1234_5678_9ABC_DEF0 >> 2, OFF_DECODER + 16, 4097, 0.9),
             (17, 5 * 8 + 4, 256, 0.1)]
    for seed, offset, n, p in cases:
        held.fill_(seed)
        got = _mask(N, dev, n, p, offset, seed_dev=held)
        want = _mask(N, dev, n, p, offset, seed=seed)
        assert torch.equal(got, want), (seed, offset, n, p)
        assert bool(((got == 0) | (got == 1)).all())
    # the key is read when the launch runs: the identical call after a refill gives the other seed's mask
    seed, offset, n, p = 11, OFF_DECODER + 2, 50 * 512, 0.3
    held.fill_(seed)
    first = _mask(N, dev, n, p, offset, seed_dev=held)
    held.fill_(seed + 1)
    second = _mask(N, dev, n, p, offset, seed_dev=held)
    assert not torch.equal(first, second)
    assert torch.equal(second, _mask(N, dev, n, p, offset, seed=seed + 1))
    assert abs(float(first.mean()) - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5 + 1e-3
    # p = 0 keeps everything
    assert bool((_mask(N, dev, 1000, 0.0, 3, seed_dev=held) == 1).all())


def _forward_backward(model, crit, d):
    for p in model.parameters():
        p.grad = None
    log_prob, reason = model(d[0], d[1], d[2])
    loss = crit(log_prob, d[2][:, 1:], d[3][:, 1:], reason, d[4], 1.0)
    loss.backward()
    torch.cuda.synchronize()
    return (log_prob.detach().clone(), [r.detach().clone() for r in reason], loss.detach().clone(),
            {k: p.grad.detach().clone() for k, p in model.named_parameters()})


@pytest.mark.parametrize('name', ['mid', 'tiny0', 'tinymax'])
def test_path_with_the_seed_in_device_memory_is_bit_identical_to_the_seed_by_value(dev, name):
    """Tiers mid_drop / tiny0_drop / tinymax_drop (dropout 0.1 / 0.2 / 0.3): forward + backward with the seed as a kernel
    argument, and with the same value in a device tensor and RFN_PATH_OPT_SEED_DEV set."""
    import recurrent_fusion_network_amd as R
    import recurrent_fusion_network_amd._native as N
    cfg, spec, P, batch, gold, _ = load_drop_case(name)
    d = to_dev(batch, dev)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    model = build(cfg, P, dev, train=True)
    seed = 0x2545_F491_4F6C_DD1D >> 2
    with mock.patch('recurrent_fusion_network_amd.fusion_model._fresh_seed', lambda: seed):
        by_value = _forward_backward(model, crit, d)
        assert not (model._dims_for(True).path_flags & N.PATH_OPT_SEED_DEV)
        held = torch.full((1,), seed, dtype=torch.int64, device=dev)
        model._seed_dev = held
        try:
            assert model._dims_for(True).path_flags & N.PATH_OPT_SEED_DEV
            by_address = _forward_backward(model, crit, d)
            held.fill_(seed + 1)                 # not vacuous: another key in the same tensor is another pass
            other = _forward_backward(model, crit, d)
        finally:
            model._seed_dev = None
    assert torch.equal(by_value[0], by_address[0])
    for a, b in zip(by_value[1], by_address[1]):
        assert torch.equal(a, b)
    assert torch.equal(by_value[2], by_address[2])
    for k, g in by_value[3].items():
        assert torch.equal(g, by_address[3][k]), k
    assert not torch.equal(by_value[0], other[0])


def _permuted_batches(batch, dev):
    fc, att, labels, masks, top = to_dev(batch, dev)
    B = labels.size(0)
    perms = [torch.arange(B, device=dev), torch.arange(B, device=dev).flip(0), torch.roll(torch.arange(B, device=dev), 2)]
    return [([f[p] for f in fc], [a[p] for a in att], labels[p], masks[p], top[p]) for p in perms]


def _reseed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed(s)


def _eager_steps(cfg, P, dev, crit, batches, steps, s, ss_prob=0.0, trace=False):
    import recurrent_fusion_network_amd as R
    model = build(cfg, P, dev, train=True)
    model.ss_prob = ss_prob
    opt = R.FusedClampAdam(model, **KW)
    model.fixed_decoder_steps = steps          # the launches of the captured step (its full-length decoder)
    model._trace_ss = trace
    losses, fed = [], []
    _reseed(s)
    for b in batches:
        opt.zero_grad()
        lp, reason = model(b[0], b[1], b[2])
        loss = crit(lp, b[2][:, 1:], b[3][:, 1:], reason, b[4], 1.0)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
        if trace:
            fed.append(model._ss_ids.clone())
    return model, opt, losses, fed


def _assert_same_training_state(model, opt, eager, eager_opt):
    for (k, p), (_, q) in zip(model.named_parameters(), eager.named_parameters()):
        assert torch.equal(p, q), k
        assert torch.equal(p.grad, q.grad), k
    for name in eager_opt.flat:      # the moments of every parameter (the 16-B padding between parameters holds no state)
        params, offs, _ = model.bucket_layout(name)
        for p_, o in zip(params, offs):
            for k in ('m', 'v'):
                assert torch.equal(eager_opt.flat[name][k][o:o + p_.numel()], opt.flat[name][k][o:o + p_.numel()]), (name, k)


def _drop_cfg():
    cfg, spec, P, batch, gold = load_case('mid')
    cfg.drop_prob_lm = cfg.drop_prob_reason = cfg.drop_prob_fusion = 0.3
    return cfg, P, batch


def test_replay_equals_eager_with_dropout(dev):
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.graphed import GraphedTrainStep
    cfg, P, batch = _drop_cfg()
    batches = _permuted_batches(batch, dev)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    steps = batches[0][2].size(1) - 1
    s = 1234
    eager, o1, want, _ = _eager_steps(cfg, P, dev, crit, batches, steps, s)

    model = build(cfg, P, dev, train=True)
    o2 = R.FusedClampAdam(model, **KW)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    _reseed(99)
    cpu_state, cuda_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    g = GraphedTrainStep(model, crit, o2, *batches[0], device_rng=True)
    assert g.steps == steps and model.fixed_decoder_steps is None and model._seed_dev is None
    # constructing the wrapper neither trains nor draws from anybody's random stream
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), cuda_state)
    assert o2.step_count == 0 and all(torch.equal(p, before[k]) for k, p in model.named_parameters())
    _reseed(s)
    for b, w in zip(batches, want):
        loss = g(*b)
        assert torch.equal(loss.detach(), w)
    assert o2.step_count == 3
    _assert_same_training_state(model, o2, eager, o1)
    assert len({float(w) for w in want}) == 3


def test_every_replay_draws_fresh_masks_and_a_pinned_seed_repeats_them(dev):
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.graphed import GraphedTrainStep
    cfg, P, batch = _drop_cfg()
    b = _permuted_batches(batch, dev)[0]
    crit = R.ReviewNetEnsembleCriterion(cfg)
    model = build(cfg, P, dev, train=True)
    opt = R.FusedClampAdam(model, **KW)
    g = GraphedTrainStep(model, crit, opt, *b, device_rng=True)
    snap = opt.snapshot()
    torch.manual_seed(5)
    first = g(*b).detach().clone()
    opt.restore(snap)
    second = g(*b).detach().clone()             # same batch, same parameters, the generator has moved on
    assert not torch.equal(first, second)
    pinned = []
    for _ in range(2):
        opt.restore(snap)
        with mock.patch('recurrent_fusion_network_amd.fusion_model._fresh_seed', lambda: 424242):
            pinned.append(g(*b).detach().clone())
    assert torch.equal(pinned[0], pinned[1])
    opt.restore(snap)
    torch.manual_seed(5)                        # ... and so does reseeding
    assert torch.equal(g(*b).detach(), first)


def test_replay_equals_eager_with_scheduled_sampling(dev):
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.graphed import GraphedTrainStep
    cfg, P, batch = _drop_cfg()
    batches = _permuted_batches(batch, dev)
    crit = R.ReviewNetEnsembleCriterion(cfg)
    steps = batches[0][2].size(1) - 1
    s = 4321
    eager, o1, want, fed = _eager_steps(cfg, P, dev, crit, batches, steps, s, ss_prob=0.25, trace=True)

    model = build(cfg, P, dev, train=True)
    model.ss_prob = 0.25
    model._trace_ss = True
    o2 = R.FusedClampAdam(model, **KW)
    _reseed(7)
    cpu_state, cuda_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    g = GraphedTrainStep(model, crit, o2, *batches[0], device_rng=True)
    assert torch.equal(torch.get_rng_state(), cpu_state) and torch.equal(torch.cuda.get_rng_state(dev), cuda_state)
    assert tuple(g.ss_uniforms.shape) == (2, steps, batches[0][2].size(0)) and model._ss_uniforms is None
    _reseed(s)
    got_fed = []
    for b, w in zip(batches, want):
        loss = g(*b)
        assert torch.equal(loss.detach(), w)
        got_fed.append(model._ss_ids.clone())      # the captured pass's token matrix (a static buffer: copy it)
    assert o2.step_count == 3
    _assert_same_training_state(model, o2, eager, o1)
    for i, (a, e, b) in enumerate(zip(got_fed, fed, batches)):
        assert torch.equal(a, e), i
        assert bool((a != b[2][:, :steps]).any(1).any()), i     # some rows were fed a sampled token
        assert torch.equal(a[:, 0], b[2][:, 0])                 # never the BOS column
    # the same batch twice: consecutive replays draw different coins and tokens
    g(*batches[0])
    one = model._ss_ids.clone()
    g(*batches[0])
    two = model._ss_ids.clone()
    assert not torch.equal(one, two)


def test_refusals_that_remain_with_device_rng(dev):
    import recurrent_fusion_network_amd as R
    from recurrent_fusion_network_amd.graphed import GraphedTrainStep
    cfg, P, batch = _drop_cfg()
    b = _permuted_batches(batch, dev)[0]
    crit = R.ReviewNetEnsembleCriterion(cfg)
    hooked = build(cfg, P, dev, train=True)
    hooked.grad_ready_hook = lambda name, flat: None
    with pytest.raises(R._native.RfnError, match='grad_ready_hook'):
        GraphedTrainStep(hooked, crit, R.FusedClampAdam(hooked, **KW), *b, device_rng=True)
    # the default stays a refusal
    plain = build(cfg, P, dev, train=True)
    with pytest.raises(R._native.RfnError):
        GraphedTrainStep(plain, crit, R.FusedClampAdam(plain, **KW), *b)

    model = build(cfg, P, dev, train=True)
    model.ss_prob = 0.25
    opt = R.FusedClampAdam(model, **KW)
    g = GraphedTrainStep(model, crit, opt, *b, device_rng=True)
    g(*b)
    # the probabilities are still kernel arguments of the captured launches
    model.drop_prob_lm = 0.5
    with pytest.raises(R._native.RfnError, match='dropout'):
        g(*b)
    model.drop_prob_lm = 0.3
    model.ss_prob = 0.5
    with pytest.raises(R._native.RfnError, match='ss_prob'):
        g(*b)
    model.ss_prob = 0.25
    model.eval()
    with pytest.raises(R._native.RfnError, match='training'):
        g(*b)
    model.train()
    g(*b)
    assert opt.step_count == 2
