"""rfn_kd_topk_fwd / _bwd through the C ABI against the float64 restatement (tests/distill_topk_cpu.py), at the code-path edges of
the dense pair's tests (V1 = 5 and 301 scalar, 1024 / 1028 / 10240 / 9488 vector, 10244 past the register limit), K = 1, 5 and
32 (at V1 = 5 mostly padding), the id / value arrays time-major, batch-major, padded and 4 B off a 16-B boundary, constructed
rows (a teacher id on the target, ids 0 and V1 - 1, two ids in one 16-B group, one live entry, the three kinds of padding), and
masked rows whose entries are NaN and out of range.

The student's rows live in a buffer with ldl = V1 + 8 and one guard row in front, all slack NaN: every out-of-range id a test
uses (-1, or V1 .. V1 + 7) would, if a kernel wrongly indexed with it, land in that slack -- inside the allocation -- and the
slack is checked afterwards.  Bounds: those of test_distill_gpu.py."""
import numpy as np
import pytest
import torch

import distill_cpu as D
import distill_topk_cpu as DK

pytestmark = pytest.mark.gpu

ITS = (1.0, 0.5, 2.0, D.f32(1.0 / 3.0))
V1S = (5, 301, 1024, 1028, 10240, 10244, 9488)
NEG_INF = float('-inf')


def make_rows(seed, B, T, V1):
    """x (B, T, V1) float32, target (B, T + 2) with values out of range, mask (B, T + 2) of {0, 1, 0.5} with zeros and ones
    wherever the draw falls; the kernels see columns 1 .. T of the last two."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn(B, T, V1, generator=g) * 3
    tgt = torch.randint(-3, V1 + 3, (B, T + 2), generator=g)
    tgt[0, 1], tgt[1, 2] = -1, V1
    u = torch.rand(B, T + 2, generator=g)
    mask = (u > 0.3).float() * torch.where(u > 0.8, 0.5, 1.0)
    mask[0, 2], mask[1, 1], mask[B - 1, T] = 0.0, 1.0, 0.0
    return x, tgt, mask


def pad_entry(ids, val, b, t, j, kind, V1, slack):
    """Entry j of row (b, t) becomes padding: id -1, an id in [V1, V1 + slack), or a value of -inf (under an id that may well be
    live elsewhere in the row: padding is not a duplicate)."""
    if kind % 3 == 0:
        ids[b, t, j] = -1
    elif kind % 3 == 1:
        ids[b, t, j] = V1 + (b + t + j) % slack
    else:
        val[b, t, j] = NEG_INF


def make_teacher(seed, rows, K, slack=8):
    """ids (B, T, K) int32, val (B, T, K) float32: distinct live ids per row, padding of the three kinds past min(K, V1) and
    in the middle of every third row; rows under a zero mask hold NaN values and out-of-range ids only.  Out-of-range ids are
    -1 or in [V1, V1 + slack): `slack` is the number of slack columns of the student rows the teacher will be run on."""
    x, tgt, mask = rows
    B, T, V1 = x.shape
    g = torch.Generator(device='cpu').manual_seed(seed)
    ids = torch.full((B, T, K), -1, dtype=torch.int32)
    val = torch.randn(B, T, K, generator=g) * 3
    for b in range(B):
        for t in range(T):
            L = min(K, V1)
            ids[b, t, :L] = torch.randperm(V1, generator=g)[:L].int()
            for j in range(L, K):
                if (j + b) % 3 == 2:
                    ids[b, t, j] = ids[b, t, j % L]          # a live id again, under a value of -inf
                pad_entry(ids, val, b, t, j, j + b, V1, slack)
            if (b * T + t) % 3 == 1 and L > 1:
                pad_entry(ids, val, b, t, (b + t) % L, b + t, V1, slack)
            if mask[b, t + 1] == 0:
                ids[b, t] = torch.tensor([-1 if j % 2 else V1 + slack - 1 for j in range(K)], dtype=torch.int32)
                val[b, t] = float('nan')
    return ids, val


def place(dev, a, layout, fill):
    """a (B, T, K) on the device as a strided view indexed (b, t, k)."""
    B, T, K = a.shape
    if layout == 'batch':
        out = torch.empty(B, T, K, dtype=a.dtype, device=dev)
    elif layout == 'time':
        out = torch.empty(T, B, K, dtype=a.dtype, device=dev).transpose(0, 1)
    elif layout == 'padded':                                 # slack in both strides
        out = torch.full((B, T + 1, K + 3), fill, dtype=a.dtype, device=dev)[:, :T, :K]
    elif layout == 'offset':                                 # a slice [1:] of a larger buffer: rows 4 B off a 16-B boundary
        out = torch.empty(B * T * K + 1, dtype=a.dtype, device=dev)[1:].view(B, T, K)
        assert out.data_ptr() % 16 == 4
    else:
        raise ValueError(layout)
    out.copy_(a)
    return out


def run(dev, rows, teacher, eps, alpha, it, layout='batch', ldl=None, terms=True):
    """Forward and backward through the C ABI -> float64 arrays in (b, t) order, plus the raw device tensors."""
    import recurrent_fusion_network_amd._native as N
    from recurrent_fusion_network_amd.distill import TopKTeacher
    x, tgt, mask = rows
    B, T, V1 = x.shape
    ldl = V1 + 8 if ldl is None else ldl
    xbuf = torch.full((T * B + 1, ldl), float('nan'), device=dev)          # row 0 is a guard row
    xs = xbuf[1:, :V1]
    xs.copy_(x.transpose(0, 1).reshape(T * B, V1))          # time-major rows r = t * B + b
    logits = xbuf[1:].data_ptr()
    tk = TopKTeacher(place(dev, teacher[0], layout, V1), place(dev, teacher[1], layout, float('nan')))
    versions = tk.ids._version, tk.logp._version
    tg, mk = tgt.to(dev), mask.to(dev)
    stats, scratch = torch.empty(3 * T * B, device=dev), torch.empty(2 * B * T, device=dev)
    loss, tm = torch.zeros(1, device=dev), torch.full((2,), float('nan'), device=dev)
    st = N.stream_ptr()
    common = (B, T, V1, tg[:, 1:].data_ptr(), tg.stride(0), mk[:, 1:].data_ptr(), mk.stride(0), eps) + tk._abi() + (alpha, it)
    N.check(N.lib.rfn_kd_topk_fwd(logits, ldl, *common, stats.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 0,
                                  tm.data_ptr() if terms else None, st), 'rfn_kd_topk_fwd')
    x_in = xs.clone()
    gdev = torch.full((1,), 0.5, device=dev)
    N.check(N.lib.rfn_kd_topk_bwd(logits, ldl, *common, stats.data_ptr(), 2.0, gdev.data_ptr(), st), 'rfn_kd_topk_bwd')  # 2 * 0.5 = 1
    assert torch.isnan(xbuf[0]).all() and torch.isnan(xbuf[:, V1:]).all()   # the guard row and every row's slack: untouched
    assert (tk.ids._version, tk.logp._version) == versions
    assert torch.equal(tk.ids.cpu(), teacher[0]) and torch.equal(tk.logp.cpu().nan_to_num(7.0), teacher[1].nan_to_num(7.0))
    return dict(loss=float(loss), xe=float(tm[0]), kd=float(tm[1]), loss_t=loss, terms_t=tm, x_in=x_in, xbuf=xbuf, tk=tk,
                stats_t=stats, stats=stats.view(3, T, B).transpose(1, 2).double().cpu().numpy(),
                grad_t=xs.clone(), grad=xs.view(T, B, V1).transpose(0, 1).double().cpu().numpy(), tg=tg, mk=mk)


def check(got, rows, teacher, eps, alpha, it, tag, terms=True):
    x, tgt, mask = rows
    B, T, V1 = x.shape
    m = mask[:, 1:T + 1].numpy()
    ref = DK.kd_topk_reference(x.numpy(), teacher[0].numpy(), teacher[1].numpy(), tgt[:, 1:T + 1].numpy(), m, eps, alpha, it)
    live = m != 0
    e_stats = float(np.abs(got['stats'] - ref['stats']).max())
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
    assert ref['kd'] > 0
    return ref


@pytest.mark.parametrize('V1', V1S)
def test_kd_topk_kernels_against_float64(dev, V1):
    k = 0
    for it in ITS:
        for alpha in (0.3, 1.0):
            for eps in (0.0, 0.1):
                B, T = ((3, 4), (2, 5))[k % 2]
                K = (1, 5, 32)[k % 3]                    # k % 6 walks every (K, (B, T)) pair
                rows = make_rows(100 + k, B, T, V1)
                teacher = make_teacher(150 + k, rows, K)
                check(run(dev, rows, teacher, eps, alpha, it), rows, teacher, eps, alpha, it, (V1, B, T, K, it, alpha, eps))
                k += 1


@pytest.mark.parametrize('V1', [301, 1024])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_constructed_rows(dev, V1, eps):
    B, T, K = 3, 4, 5
    rows = make_rows(800, B, T, V1)
    x, tgt, mask = rows
    mask[:, 1:T + 1] = 1.0
    mask[0, 1], mask[2, 3] = 0.0, 0.0                        # rows (0, 0) and (2, 2) are masked
    ids, val = make_teacher(801, rows, K)
    assert torch.isnan(val[0, 0]).all() and torch.isnan(val[2, 2]).all() and (ids[0, 0] < 0).logical_or(ids[0, 0] >= V1).all()
    # a teacher id equal to the row's target
    tgt[0, 2] = 17
    ids[0, 1] = torch.tensor([40, 17, 3, 250, 99], dtype=torch.int32)
    val[0, 1] = torch.tensor([0.5, 2.0, -1.0, 0.0, 1.0])
    # ids 0 and V1 - 1 in one row
    ids[0, 2] = torch.tensor([V1 - 1, 7, 0, 100, 200], dtype=torch.int32)
    val[0, 2] = torch.tensor([1.0, 0.0, 1.5, -2.0, 0.3])
    # two (here three) ids inside one 16-B group
    ids[1, 0] = torch.tensor([8, 10, 9, 64, 129], dtype=torch.int32)
    val[1, 0] = torch.tensor([1.0, 1.0, 0.2, -0.5, 0.1])
    # exactly one live entry; padding by id = -1, by id >= V1 and by val = -inf
    ids[1, 1] = torch.tensor([-1, V1, 33, 33, V1 + 7], dtype=torch.int32)
    val[1, 1] = torch.tensor([0.3, 0.1, NEG_INF, -4.0, 9.0])
    # a row whose target is out of range (class 0) and whose teacher holds id 0
    tgt[1, 3] = V1 + 2
    ids[1, 2] = torch.tensor([5, 0, 6, -1, 2], dtype=torch.int32)
    val[1, 2] = torch.tensor([0.1, 0.9, NEG_INF, 3.0, 0.4])
    for it, alpha in ((1.0, 0.3), (0.5, 1.0)):
        got = run(dev, rows, (ids, val), eps, alpha, it)
        check(got, rows, (ids, val), eps, alpha, it, (V1, eps, it, alpha, 'constructed'))
        # the one-entry row: p_t is a point mass on id 33, whatever its value
        assert abs(got['stats'][2][1, 1] - (-4.0 * it)) < 1e-6


@pytest.mark.parametrize('V1,K', [(301, 5), (9488, 32)])
@pytest.mark.parametrize('layout', ['time', 'batch', 'padded', 'offset'])
def test_teacher_layouts(dev, V1, K, layout):
    for k, (B, T, it, alpha, eps) in enumerate(((3, 4, 0.5, 0.3, 0.1), (2, 5, D.f32(1.0 / 3.0), 1.0, 0.0))):
        rows = make_rows(200 + k, B, T, V1)
        teacher = make_teacher(250 + k, rows, K)
        base = run(dev, rows, teacher, eps, alpha, it)
        got = run(dev, rows, teacher, eps, alpha, it, layout=layout)
        check(got, rows, teacher, eps, alpha, it, (V1, K, layout, B, T))
        # the layout of the K entries changes no bit: the student is read as before
        assert torch.equal(got['loss_t'], base['loss_t']) and torch.equal(got['grad_t'], base['grad_t'])


@pytest.mark.parametrize('V1', [1024, 9488])
def test_a_student_row_stride_of_v1_plus_1_takes_the_scalar_form(dev, V1):
    B, T, K, it, alpha, eps = 3, 4, 5, 0.5, 0.3, 0.1
    rows = make_rows(300, B, T, V1)
    teacher = make_teacher(301, rows, K, slack=1)            # out-of-range ids: -1 and V1 only
    vec = run(dev, rows, teacher, eps, alpha, it)
    ref = check(vec, rows, teacher, eps, alpha, it, (V1, 'ldl = V1 + 8'))
    got = run(dev, rows, teacher, eps, alpha, it, ldl=V1 + 1)                # run() checks the slack column
    check(got, rows, teacher, eps, alpha, it, (V1, 'ldl = V1 + 1'))
    g_tol = 1e-6 * max(1.0, (1 - alpha) + alpha / it)
    assert abs(got['loss'] - vec['loss']) < 1e-5 * max(1.0, abs(ref['loss']))
    assert float(np.abs(got['stats'] - vec['stats']).max()) < 1e-5 and float(np.abs(got['grad'] - vec['grad']).max()) < g_tol


@pytest.mark.parametrize('V1', [301, 1024, 9488])
@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_xe_term_and_first_row_stat_are_the_xe_kernels_bits(dev, V1, eps):
    import recurrent_fusion_network_amd._native as N
    B, T = 3, 4
    rows = make_rows(600, B, T, V1)
    teacher = make_teacher(601, rows, 5)
    lse, scratch, loss = torch.empty(T * B, device=dev), torch.empty(B * T, device=dev), torch.zeros(1, device=dev)
    for k, alpha in enumerate((0.3, 1.0, 0.0)):              # at any alpha
        got = run(dev, rows, teacher, eps, alpha, 0.5)
        if k == 0:
            x = got['x_in'].contiguous()
            N.check(N.lib.rfn_xe_logits_fwd(x.data_ptr(), V1, B, T, V1, got['tg'][:, 1:].data_ptr(), got['tg'].stride(0),
                                            got['mk'][:, 1:].data_ptr(), got['mk'].stride(0), eps, lse.data_ptr(), scratch.data_ptr(),
                                            loss.data_ptr(), 0, N.stream_ptr()), 'rfn_xe_logits_fwd')
        assert torch.equal(got['terms_t'][0], loss[0]), alpha
        assert torch.equal(got['stats_t'][:T * B], lse), alpha
    one = run(dev, rows, teacher, eps, 0.3, 1.0)             # inv_temp == 1: the tempered student row is the row itself
    assert torch.equal(one['stats_t'][T * B:2 * T * B], one['stats_t'][:T * B]) and torch.equal(one['terms_t'][0], loss[0])


@pytest.mark.parametrize('V1,K', [(301, 5), (9488, 32)])
def test_two_runs_are_bit_equal_and_terms_out_may_be_null(dev, V1, K):
    rows = make_rows(700, 3, 4, V1)
    teacher = make_teacher(701, rows, K)
    eps, alpha, it = 0.1, 0.3, 0.5
    a, b = run(dev, rows, teacher, eps, alpha, it), run(dev, rows, teacher, eps, alpha, it)
    for key in ('loss_t', 'terms_t', 'stats_t', 'grad_t'):
        assert torch.equal(a[key], b[key]), key
    c = run(dev, rows, teacher, eps, alpha, it, terms=False)
    check(c, rows, teacher, eps, alpha, it, 'no terms_out', terms=False)
    assert torch.equal(a['loss_t'], c['loss_t']) and torch.isnan(c['terms_t']).all() and torch.equal(a['grad_t'], c['grad_t'])


@pytest.mark.parametrize('V1,K', [(5, 5), (301, 5), (1024, 32), (9488, 32)])
def test_the_sparse_pair_agrees_with_the_dense_pair_on_the_dense_teacher(dev, V1, K):
    """The reference here is the merged dense pair, fed TopKTeacher.dense(V1) of the same entries.  At V1 = 5, K = 5 the teacher
    is a full row."""
    import recurrent_fusion_network_amd._native as N
    for k, (B, T, it, alpha, eps) in enumerate(((3, 4, 0.5, 0.3, 0.1), (2, 5, 2.0, 1.0, 0.0), (3, 4, 1.0, 0.3, 0.0))):
        rows = make_rows(900 + k, B, T, V1)
        x, tgt, mask = rows
        teacher = make_teacher(950 + k, rows, K)
        if V1 == 5:
            assert all(sorted(teacher[0][b, t].tolist()) == [0, 1, 2, 3, 4] for b in range(B) for t in range(T)
                       if mask[b, t + 1] != 0 and (b * T + t) % 3 != 1)
        got = run(dev, rows, teacher, eps, alpha, it)
        z = got['tk'].dense(V1)
        assert tuple(z.shape) == (B, T, V1)
        xd = got['x_in'].contiguous()
        stats, scratch = torch.empty(3 * T * B, device=dev), torch.empty(2 * B * T, device=dev)
        loss, tm = torch.zeros(1, device=dev), torch.empty(2, device=dev)
        common = (V1, B, T, V1, got['tg'][:, 1:].data_ptr(), got['tg'].stride(0), got['mk'][:, 1:].data_ptr(), got['mk'].stride(0),
                  eps, z.data_ptr(), z.stride(0), z.stride(1), alpha, it)
        N.check(N.lib.rfn_kd_logits_fwd(xd.data_ptr(), *common, stats.data_ptr(), scratch.data_ptr(), loss.data_ptr(), 0,
                                        tm.data_ptr(), N.stream_ptr()), 'rfn_kd_logits_fwd')
        one = torch.ones(1, device=dev)
        N.check(N.lib.rfn_kd_logits_bwd(xd.data_ptr(), *common, stats.data_ptr(), 1.0, one.data_ptr(), N.stream_ptr()),
                'rfn_kd_logits_bwd')
        ref_loss, ref_xe, ref_kd = float(loss), float(tm[0]), float(tm[1])
        live = (mask[:, 1:T + 1] != 0).numpy()
        ref_stats = stats.view(3, T, B).transpose(1, 2).double().cpu().numpy()
        e_stats = float(np.abs(got['stats'] - ref_stats)[:, live].max())
        e_grad = float((got['grad_t'] - xd).abs().max())
        g_tol = 1e-6 * max(1.0, (1 - alpha) + alpha / it)
        print('V1 %d K %d: loss %.7g (dense %.7g)  xe %.7g (%.7g)  kd %.7g (%.7g)  stats err %.2e  grad err %.2e (tol %.2e)'
              % (V1, K, got['loss'], ref_loss, got['xe'], ref_xe, got['kd'], ref_kd, e_stats, e_grad, g_tol))
        assert abs(got['loss'] - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))
        assert abs(got['xe'] - ref_xe) < 1e-5 * max(1.0, abs(ref_xe)) and abs(got['kd'] - ref_kd) < 1e-5 * max(1.0, abs(ref_kd))
        assert e_stats < 1e-5 and e_grad < g_tol and ref_kd > 0
