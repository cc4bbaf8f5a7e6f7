"""rfn_kd_logits_fwd / _bwd through the C ABI against the float64 restatement (tests/distill_cpu.py), at the edges of their code
paths: the scalar form (V1 = 5 under one pass, 301 odd, 10244 a multiple of 4 past the register limit), the vector form (1024 =
exactly one f32x4 per lane, 1028 one past that, 10240 the register limit, 9488 the workload's own), the teacher time-major,
batch-major and padded, a teacher or a student whose rows are not 16-B aligned (scalar form on the same data), masks with zeros,
targets out of range, -inf teacher entries, NaN teacher rows under a zero mask.  Bounds: those of
test_forward_loss_gpu.py::test_xe_logits_kernels_against_float64, the gradient's scaled by (1 - alpha) + alpha / it, which is
what the gradient's magnitude grows by over the XE case the 1e-6 was set for."""
import numpy as np
import pytest
import torch

import distill_cpu as D

pytestmark = pytest.mark.gpu

ITS = (1.0, 0.5, 2.0, D.f32(1.0 / 3.0))
V1S = (5, 301, 1024, 1028, 10240, 10244, 9488)


def make_rows(seed, B, T, V1, neg_inf=False, nan_rows=False):
    """float32 rows on the host: x, z (B, T, V1), target (B, T + 2) with values out of range, mask (B, T + 2) of {0, 1, 0.5};
    the kernels see columns 1 .. T of the last two."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn(B, T, V1, generator=g) * 3
    z = torch.randn(B, T, V1, generator=g) * 3
    tgt = torch.randint(-3, V1 + 3, (B, T + 2), generator=g)
    tgt[0, 1], tgt[1, 2] = -1, V1                           # out of range on both sides, whatever the draw
    u = torch.rand(B, T + 2, generator=g)
    mask = (u > 0.3).float() * torch.where(u > 0.8, 0.5, 1.0)
    mask[0, 2], mask[1, 1], mask[B - 1, T] = 0.0, 1.0, 0.0
    if neg_inf:
        hole = torch.rand(B, T, V1, generator=g) < 0.1
        hole[..., 0] = False                                 # every row keeps a finite entry
        z[hole] = float('-inf')
    if nan_rows:
        z[mask[:, 1:T + 1] == 0] = float('nan')
    return x, z, tgt, mask


def teacher_on(dev, z, layout):
    """z (B, T, V1) on the device as a strided view indexed (b, t, v)."""
    B, T, V1 = z.shape
    if layout == 'batch':
        zt = torch.empty(B, T, V1, device=dev)
    elif layout == 'time':
        zt = torch.empty(T, B, V1, device=dev).transpose(0, 1)
    elif layout == 'padded':                                 # slack in both strides, still multiples of 4 when V1 is
        zt = torch.full((B, T + 1, V1 + 8), float('nan'), device=dev)[:, :T, :V1]
    elif layout == 'offset':                                 # a slice [1:] of a larger buffer: rows 4 B off a 16-B boundary
        zt = torch.empty(B * T * V1 + 1, device=dev)[1:].view(B, T, V1)
        assert zt.data_ptr() % 16 == 4
    else:
        raise ValueError(layout)
    zt.copy_(z)
    return zt


def run(dev, rows, eps, alpha, it, layout='batch', ldl=None, terms=True):
    """Forward and backward through the C ABI -> float64 arrays in (b, t) order, plus the raw device tensors."""
    import recurrent_fusion_network_amd._native as N
    x, z, tgt, mask = rows
    B, T, V1 = x.shape
    ldl = V1 if ldl is None else ldl
    xbuf = torch.full((T * B, ldl), float('nan'), device=dev)
    xs = xbuf[:, :V1]
    xs.copy_(x.transpose(0, 1).reshape(T * B, V1))          # time-major rows r = t * B + b
    zt = teacher_on(dev, z, layout)
    tg, mk = tgt.to(dev), mask.to(dev)
    stats, scratch = torch.empty(3 * T * B, device=dev), torch.empty(2 * B * T, device=dev)
    loss, tm = torch.zeros(1, device=dev), torch.full((2,), float('nan'), device=dev)
    st = N.stream_ptr()
    common = (B, T, V1, tg[:, 1:].data_ptr(), tg.stride(0), mk[:, 1:].data_ptr(), mk.stride(0), eps, zt.data_ptr(), zt.stride(0),
              zt.stride(1), alpha, it)
    N.check(N.lib.rfn_kd_logits_fwd(xbuf.data_ptr(), ldl, *common, stats.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 0,
                                    tm.data_ptr() if terms else None, st), 'rfn_kd_logits_fwd')
    x_in = xs.clone()
    gdev = torch.full((1,), 0.5, device=dev)
    N.check(N.lib.rfn_kd_logits_bwd(xbuf.data_ptr(), ldl, *common, stats.data_ptr(), 2.0, gdev.data_ptr(), st),      # 2 * 0.5 = 1
            'rfn_kd_logits_bwd')
    return dict(loss=float(loss), xe=float(tm[0]), kd=float(tm[1]), loss_t=loss, terms_t=tm, x_in=x_in, xbuf=xbuf,
                stats_t=stats, stats=stats.view(3, T, B).transpose(1, 2).double().cpu().numpy(),
                grad=xs.view(T, B, V1).transpose(0, 1).double().cpu().numpy(), tg=tg, mk=mk)


def check(got, rows, eps, alpha, it, tag, terms=True):
    x, z, tgt, mask = rows
    B, T, V1 = x.shape
    m = mask[:, 1:T + 1].numpy()
    ref = D.kd_reference(x.numpy(), z.numpy(), tgt[:, 1:T + 1].numpy(), m, eps, alpha, it)
    live = m != 0
    e_stats = float(np.abs(got['stats'] - ref['stats'])[:, live].max())
    e_grad = float(np.abs(got['grad'] - ref['grad']).max())
    g_tol = 1e-6 * max(1.0, (1 - alpha) + alpha / it)
    print('%s: loss %.7g (ref %.7g)  xe %.7g (%.7g)  kd %.7g (%.7g)  stats err %.2e  grad err %.2e (tol %.2e)'
          % (tag, got['loss'], ref['loss'], got['xe'], ref['xe'], got['kd'], ref['kd'], e_stats, e_grad, g_tol))
    assert abs(got['loss'] - ref['loss']) < 1e-5 * max(1.0, abs(ref['loss'])), tag
    if terms:
        assert abs(got['xe'] - ref['xe']) < 1e-5 * max(1.0, abs(ref['xe'])), tag
        assert abs(got['kd'] - ref['kd']) < 1e-5 * max(1.0, abs(ref['kd'])), tag
    assert e_stats < 1e-5, tag
    assert e_grad < g_tol, tag
    assert (~live).any() and live.any() and (got['grad'][~live] == 0).all(), tag          # masked rows: exact zeros
    return ref


@pytest.mark.parametrize('V1', V1S)
def test_kd_logits_kernels_against_float64(dev, V1):
    k = 0
    for it in ITS:
        for alpha in (0.3, 1.0):
            for eps in (0.0, 0.1):
                B, T = ((3, 4), (2, 5))[k % 2]
                rows = make_rows(100 + k, B, T, V1)
                check(run(dev, rows, eps, alpha, it), rows, eps, alpha, it, (V1, B, T, it, alpha, eps))
                k += 1


@pytest.mark.parametrize('V1', [1024, 9488])
@pytest.mark.parametrize('layout', ['time', 'batch', 'padded'])
def test_teacher_layouts(dev, V1, layout):
    for k, (B, T, it, alpha, eps) in enumerate(((3, 4, 0.5, 0.3, 0.1), (2, 5, D.f32(1.0 / 3.0), 1.0, 0.0))):
        rows = make_rows(200 + k, B, T, V1)
        check(run(dev, rows, eps, alpha, it, layout=layout), rows, eps, alpha, it, (V1, layout, B, T))


@pytest.mark.parametrize('V1', [1024, 9488])
def test_misaligned_rows_take_the_scalar_form_and_agree(dev, V1):
    """A teacher base one float off a 16-B boundary, and a student row stride of V1 + 1: the same data as the aligned call, to
    the same bounds -- and the two forms agree with each other to them."""
    B, T, it, alpha, eps = 3, 4, 0.5, 0.3, 0.1
    rows = make_rows(300, B, T, V1)
    vec = run(dev, rows, eps, alpha, it)
    ref = check(vec, rows, eps, alpha, it, (V1, 'aligned'))
    g_tol = 1e-6 * max(1.0, (1 - alpha) + alpha / it)
    for tag, kw in (('teacher + 4 B', dict(layout='offset')), ('ldl = V1 + 1', dict(ldl=V1 + 1))):
        got = run(dev, rows, eps, alpha, it, **kw)
        check(got, rows, eps, alpha, it, (V1, tag))
        assert abs(got['loss'] - vec['loss']) < 1e-5 * max(1.0, abs(ref['loss'])), tag
        assert float(np.abs(got['stats'] - vec['stats']).max()) < 1e-5 and float(np.abs(got['grad'] - vec['grad']).max()) < g_tol, tag
        if 'ldl' in kw:
            assert torch.isnan(got['xbuf'][:, V1]).all()     # the slack column of the student's rows is not written


@pytest.mark.parametrize('V1,layout', [(301, 'batch'), (1024, 'time'), (9488, 'batch')])
def test_minus_infinity_teacher_entries(dev, V1, layout):
    for k, (it, alpha, eps) in enumerate(((1.0, 0.3, 0.1), (2.0, 1.0, 0.0))):
        rows = make_rows(400 + k, 3, 4, V1, neg_inf=True)
        assert 0.05 < float(torch.isinf(rows[1]).float().mean()) < 0.15
        got = run(dev, rows, eps, alpha, it, layout=layout)
        check(got, rows, eps, alpha, it, (V1, '-inf', it))
        assert np.isfinite(got['grad']).all() and np.isfinite(got['stats']).all() and np.isfinite(got['loss'])


@pytest.mark.parametrize('V1', [301, 1024])
def test_nan_teacher_rows_under_a_zero_mask(dev, V1):
    it, alpha, eps = 0.5, 0.3, 0.1
    rows = make_rows(500, 2, 5, V1, nan_rows=True)
    assert torch.isnan(rows[1]).any()
    got = run(dev, rows, eps, alpha, it)
    check(got, rows, eps, alpha, it, (V1, 'nan rows'))
    assert np.isfinite(got['grad']).all() and np.isfinite(got['loss']) and np.isfinite(got['xe']) and np.isfinite(got['kd'])
    clean = make_rows(500, 2, 5, V1)
    ref = run(dev, clean, eps, alpha, it)
    assert got['loss'] == ref['loss'] and got['kd'] == ref['kd'] and np.array_equal(got['grad'], ref['grad'])


@pytest.mark.parametrize('V1', [301, 1024, 9488])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_xe_term_and_first_row_stat_are_the_xe_kernels_bits(dev, V1, eps):
    import recurrent_fusion_network_amd._native as N
    B, T = 3, 4
    rows = make_rows(600, B, T, V1)
    got = run(dev, rows, eps, 0.3, 0.5)
    x = got['x_in'].contiguous()
    lse, scratch, loss = torch.empty(T * B, device=dev), torch.empty(B * T, device=dev), torch.zeros(1, device=dev)
    N.check(N.lib.rfn_xe_logits_fwd(x.data_ptr(), V1, B, T, V1, got['tg'][:, 1:].data_ptr(), got['tg'].stride(0),
                                    got['mk'][:, 1:].data_ptr(), got['mk'].stride(0), eps, lse.data_ptr(), scratch.data_ptr(),
                                    loss.data_ptr(), 0, N.stream_ptr()), 'rfn_xe_logits_fwd')
    assert torch.equal(got['terms_t'][0], loss[0])
    assert torch.equal(got['stats_t'][:T * B], lse)
    # inv_temp == 1: the tempered student row is the row itself
    one = run(dev, rows, eps, 0.3, 1.0)
    assert torch.equal(one['stats_t'][T * B:2 * T * B], one['stats_t'][:T * B]) and torch.equal(one['terms_t'][0], loss[0])


def test_loss_without_terms_out_and_accumulation(dev):
    """terms_out = NULL gives the same loss bits; accumulate_loss adds to what loss_out holds."""
    import recurrent_fusion_network_amd._native as N
    rows = make_rows(700, 3, 4, 1028)
    eps, alpha, it = 0.1, 0.3, 0.5
    a, b = run(dev, rows, eps, alpha, it), run(dev, rows, eps, alpha, it, terms=False)
    check(b, rows, eps, alpha, it, 'no terms_out', terms=False)
    assert torch.equal(a['loss_t'], b['loss_t']) and torch.isnan(b['terms_t']).all()
    x, z, tgt, mask = rows
    B, T, V1 = x.shape
    xs = x.transpose(0, 1).reshape(T * B, V1).contiguous().to(dev)
    zt, tg, mk = z.to(dev), tgt.to(dev), mask.to(dev)
    stats, scratch = torch.empty(3 * T * B, device=dev), torch.empty(2 * B * T, device=dev)
    loss = torch.full((1,), 10.0, device=dev)
    N.check(N.lib.rfn_kd_logits_fwd(xs.data_ptr(), V1, B, T, V1, tg[:, 1:].data_ptr(), tg.stride(0), mk[:, 1:].data_ptr(),
                                    mk.stride(0), eps, zt.data_ptr(), zt.stride(0), zt.stride(1), alpha, it, stats.data_ptr(),
                                    scratch.data_ptr(), loss.data_ptr(), 1, None, N.stream_ptr()), 'rfn_kd_logits_fwd')
    assert abs(float(loss) - (10.0 + a['loss'])) <= 2.0 ** -23 * (10.0 + abs(a['loss']))       # one float32 rounding of the sum
