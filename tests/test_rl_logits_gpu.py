"""rfn_rl_logits_fwd / _bwd through the C ABI against the float64 restatement (tests/rl_logits_cpu.py), at the edges of their code
paths: the element-wise form (V1 = 37), the vector form with most lanes idle (64), exactly one f32x4 per lane (1024) and the
register limit (10240), element-wise again past it (10244), with a padded row stride and with a base one float off a 16-B
boundary; rewards of both signs and an exact zero, PPO with `old` below, inside and above the clamp, finished rows, a row that
draws 0 first, an id out of range.  Bounds: those of test_forward_loss_gpu.py::test_xe_logits_kernels_against_float64 (loss 1e-5 *
max(1, |ref|), log-sum-exp 1e-5, gradient 1e-6), the gradient's scaled -- as test_distill_gpu.py scales it -- by what the
gradient's magnitude grows by over the XE case the 1e-6 was set for: max(1, max |mk * d pol / d lp_tok|) of the fp64 reference.

With RFN_RL_LOSS_JSON set to a path, every case appends its measured error / bound figures there (profiles/rl_loss.json holds
such a run)."""
import json
import os

import numpy as np
import pytest
import torch

import rl_logits_cpu as RL

pytestmark = pytest.mark.gpu

SHAPES = ((3, 4, 37), (2, 3, 64), (2, 2, 1024), (1, 2, 10240), (1, 2, 10244))
MODES = ((0.0, False), (0.01, False), (0.0, True), (0.01, True))          # (entropy_reg, ppo)
PPO_CLIP = 0.2


def _record(case, **figures):
    path = os.environ.get('RFN_RL_LOSS_JSON')
    if path:
        with open(path, 'a') as f:
            f.write(json.dumps(dict(case=case, **figures), sort_keys=True) + '\n')


def run(dev, c, entropy_reg, ppo, ldl=None, offset=0, terms=True):
    """Forward and backward through the C ABI on time-major rows -> float64 arrays in (b, t) order and the raw device tensors.
    ldl: the row stride (slack columns hold NaN); offset: floats between a 16-B boundary and the first row."""
    import recurrent_fusion_network_amd._native as N
    x = torch.from_numpy(c['x'])
    B, T, V1 = x.shape
    ldl = V1 if ldl is None else ldl
    xbuf = torch.full((T * B * ldl + offset,), float('nan'), device=dev)[offset:].view(T * B, ldl)
    assert xbuf.data_ptr() % 16 == 4 * offset
    xs = xbuf[:, :V1]
    xs.copy_(x.transpose(0, 1).reshape(T * B, V1))          # time-major rows r = t * B + b
    seq = torch.from_numpy(c['seq']).to(dev)
    rw = torch.from_numpy(c['reward']).to(dev)
    old = torch.from_numpy(c['old']).to(dev) if ppo else None
    stats, scratch = torch.empty(3 * T * B, device=dev), torch.empty(3 * B * T, device=dev)
    tok_lp = torch.full((B, T + 1), float('nan'), device=dev)
    loss, tm = torch.zeros(1, device=dev), torch.full((2,), float('nan'), device=dev)
    st = N.stream_ptr()
    common = (B, T, V1, seq.data_ptr(), seq.stride(0), rw.data_ptr(), rw.stride(0), entropy_reg, N.ptr(old),
              0 if old is None else old.stride(0), int(ppo), PPO_CLIP)
    N.check(N.lib.rfn_rl_logits_fwd(xbuf.data_ptr(), ldl, *common, stats.data_ptr(), tok_lp.data_ptr(), tok_lp.stride(0),
                                    scratch.data_ptr(), loss.data_ptr(), 0, tm.data_ptr() if terms else None, st), 'rfn_rl_logits_fwd')
    # the log-probs rfn_log_softmax_fwd writes for the same rows, (B, T, V1)
    logp = torch.empty(B, T, V1, device=dev)
    N.check(N.lib.rfn_log_softmax_fwd(xbuf.data_ptr(), ldl, T * B, V1, B, T * V1, V1, logp.data_ptr(), st), 'rfn_log_softmax_fwd')
    gdev = torch.full((1,), 0.5, device=dev)
    N.check(N.lib.rfn_rl_logits_bwd(xbuf.data_ptr(), ldl, *common, stats.data_ptr(), 2.0, gdev.data_ptr(), st),      # 2 * 0.5 = 1
            'rfn_rl_logits_bwd')
    return dict(loss=float(loss), policy=float(tm[0]), entropy=float(tm[1]), loss_t=loss, xbuf=xbuf, stats_t=stats, tok_lp_t=tok_lp,
                logp=logp, seq=seq, stats=stats.view(3, T, B).transpose(1, 2).double().cpu().numpy(),
                tok_lp=tok_lp[:, :T].double().cpu().numpy(), grad=xs.view(T, B, V1).transpose(0, 1).double().cpu().numpy())


def check(got, c, entropy_reg, ppo, tag):
    B, T, V1 = c['x'].shape
    ref = RL.rl_logits(c['x'], c['seq'], c['reward'], entropy_reg, c['old'] if ppo else None, PPO_CLIP)
    seq = c['seq']
    mk = np.concatenate([np.ones((B, 1), bool), seq[:, :-1] > 0], 1)
    m0 = seq > 0
    dead = ~mk & ~m0
    # max |mk * d pol / d lp_tok| from the reference's own log-probs (PPO: the larger of the two branches' slopes)
    dpol = np.zeros((B, T))
    lp = ref['tok_lp']
    for b in range(B):
        for t in range(T):
            if not mk[b, t]:
                continue
            rw = float(c['reward'][b, t])
            if not ppo:
                dpol[b, t] = abs(rw)
            else:
                ratio = np.exp(lp[b, t]) / (1e-5 + np.exp(float(c['old'][b, t])))
                dpol[b, t] = max(abs(ratio * rw), abs(ratio * rw * rw))
    g_tol = 1e-6 * max(1.0, float(dpol.max()))
    e_lse = float(np.abs(got['stats'][0] - ref['lse']).max())
    e_hm = float(np.abs(got['stats'][1] - ref['Hm']).max())
    e_lp = max(float(np.abs(got['stats'][2] - ref['tok_lp']).max()), float(np.abs(got['tok_lp'] - ref['tok_lp']).max()))
    e_grad = float(np.abs(got['grad'] - ref['grad']).max())
    l_tol = 1e-5 * max(1.0, abs(ref['loss']))
    print('%s: loss %.7g (ref %.7g)  policy %.7g (%.7g)  entropy %.7g (%.7g)  lse err %.2e  Hm err %.2e  lp_tok err %.2e  grad err '
          '%.2e (tol %.2e)' % (tag, got['loss'], ref['loss'], got['policy'], ref['policy'], got['entropy'], ref['entropy'], e_lse, e_hm,
                               e_lp, e_grad, g_tol))
    _record(str(tag), loss_err_over_bar=abs(got['loss'] - ref['loss']) / l_tol, stats_err_over_bar=max(e_lse, e_hm, e_lp) / 1e-5,
            grad_err_over_bar=e_grad / g_tol, grad_bar=g_tol)
    assert abs(got['loss'] - ref['loss']) < l_tol, tag
    assert abs(got['policy'] - ref['policy']) < 1e-5 * max(1.0, abs(ref['policy'])), tag
    assert abs(got['entropy'] - ref['entropy']) < 1e-5 * max(1.0, abs(ref['entropy'])), tag
    assert e_lse < 1e-5 and e_hm < 1e-5 and e_lp < 1e-5, tag
    assert e_grad < g_tol, tag
    # the token's log-prob carries the bits rfn_log_softmax_fwd puts at that position; the slack column is not written
    tok = torch.where((got['seq'] < 0) | (got['seq'] >= V1), torch.zeros_like(got['seq']), got['seq'])
    assert torch.equal(got['tok_lp_t'][:, :T], got['logp'].gather(2, tok.unsqueeze(2)).squeeze(2)), tag
    assert torch.isnan(got['tok_lp_t'][:, T]).all(), tag
    # masked rows: exact zeros
    if B > 1 and T > 1:
        assert dead.any(), tag
    assert (got['grad'][dead] == 0).all(), tag
    if entropy_reg == 0.0:
        assert not got['stats'][1].any() and got['entropy'] == 0.0, tag
    return ref


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_rl_logits_kernels_against_float64(dev, shape):
    for k, (ent, ppo) in enumerate(MODES):
        c = RL.make_case(*shape, seed=500 + k)
        got = run(dev, c, ent, ppo)
        check(got, c, ent, ppo, (shape, ent, ppo))
        again = run(dev, c, ent, ppo)                        # no atomics: two runs give the same bits
        assert torch.equal(got['xbuf'], again['xbuf']) and torch.equal(got['loss_t'], again['loss_t'])
        assert torch.equal(got['stats_t'], again['stats_t']) and torch.equal(got['tok_lp_t'][:, :shape[1]], again['tok_lp_t'][:, :shape[1]])


@pytest.mark.parametrize('V1', [64, 1024])
def test_misaligned_rows_take_the_element_wise_form_and_agree(dev, V1):
    """A row stride of V1 + 2 and a base one float off a 16-B boundary: the same data as the aligned call, to the same bounds --
    and the slack columns of the padded rows are not written."""
    B, T = 3, 4
    for ent, ppo in ((0.01, True), (0.0, False)):
        c = RL.make_case(B, T, V1, seed=600)
        vec = run(dev, c, ent, ppo)
        ref = check(vec, c, ent, ppo, (V1, 'aligned', ent, ppo))
        for tag, kw in (('ldl = V1 + 2', dict(ldl=V1 + 2)), ('base + 4 B', dict(offset=1))):
            got = run(dev, c, ent, ppo, **kw)
            check(got, c, ent, ppo, (V1, tag, ent, ppo))
            assert abs(got['loss'] - vec['loss']) < 1e-5 * max(1.0, abs(ref['loss'])), tag
            if 'ldl' in kw:
                assert torch.isnan(got['xbuf'][:, V1:]).all(), tag


def test_zero_reward_rows_and_missing_terms(dev):
    """A zero reward without an entropy term is an exactly zero row (it contributes nothing, whatever its tokens are); with the
    entropy term the row carries that term alone.  terms_out = NULL changes no bit of the loss."""
    c = RL.make_case(3, 4, 64, seed=700)
    c['reward'][:] = 0.0
    got = run(dev, c, 0.0, False)
    assert not got['grad'].any() and got['loss'] == 0.0
    ent = run(dev, c, 0.01, False)
    check(ent, c, 0.01, False, 'zero reward, entropy')
    assert ent['grad'][c['seq'] > 0].any() and ent['policy'] == 0.0
    c2 = RL.make_case(3, 4, 64, seed=701)
    a, b = run(dev, c2, 0.01, True), run(dev, c2, 0.01, True, terms=False)
    assert torch.equal(a['loss_t'], b['loss_t']) and torch.equal(a['xbuf'], b['xbuf'])
