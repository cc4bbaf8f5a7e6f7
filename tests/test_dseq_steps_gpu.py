"""rfn_attn_context_bwd_dseq_steps (rfn.h) against fp64 numpy (tests/input_grads_cases.py).

Per element the bar is derived, not measured: 2 * (T + 1) * 2^-24 * (|prev| + sum_t |alpha_t * dz_t|).  Cases: the issue's own
shapes and one on each side of every edge the launcher has (D tile, both row-chunk sizes, the LDS limit with its first refused
size); accumulate 0 and 1 each.  Padded strides with guard values; a base pointer one float off takes the scalar form and gives
the aligned run's bits; ragged lengths with NaN in the padded rows of alpha and of the map; two runs are bit-identical."""
import numpy as np
import pytest
import torch

import input_grads_cases as IC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 12345.0


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def operands(T, B, L, D, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)     # noqa: E731
    return f(T, B, L), f(T, B, D), f(B, L, D)


def call(T, alpha, alpha_st, dz, dz_st, lddz, B, L, D, out, sb, sl, acc, lens=None):
    N = native()
    return N.lib.rfn_attn_context_bwd_dseq_steps(T, alpha.data_ptr(), alpha_st, dz.data_ptr(), dz_st, lddz, B, L, D, out.data_ptr(),
                                                 sb, sl, acc, N.ptr(lens), N.stream_ptr())


def run_packed(alpha, dz, prev, acc, lens=None, off=0):
    """The call on packed device copies; `off`: floats by which the map's and dz's base pointers are moved off 16 bytes."""
    T, B, L = alpha.shape
    D = dz.shape[2]
    a = torch.from_numpy(alpha).to(DEV)
    g = torch.zeros(T * B * D + off, device=DEV)
    g[off:] = torch.from_numpy(dz).to(DEV).reshape(-1)
    o = torch.zeros(B * L * D + off, device=DEV)
    o[off:] = torch.from_numpy(prev).to(DEV).reshape(-1)
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    rc = call(T, a, B * L, g[off:], B * D, D, B, L, D, o[off:], L * D, D, acc, ln)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return o[off:].reshape(B, L, D).cpu()


def check(got, alpha, dz, prev, acc, lens=None, what=''):
    T = alpha.shape[0]
    want, mag = IC.dseq_steps_ref(alpha, dz, prev, acc, lens)
    err = np.abs(got.double().numpy() - want)
    tol = IC.bar(T, mag)
    with np.errstate(invalid='ignore'):
        live = np.isfinite(want)
        worst = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)[live])) if live.any() else 0.0
    print('%s acc %d: max err %.3g, worst err / bar %.3g' % (what, acc, float(err[live].max()) if live.any() else 0.0, worst))
    assert (err[live] <= tol[live]).all(), (what, acc, worst)
    return want


@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('case', IC.CASES, ids=lambda c: 'T%d_B%d_L%d_D%d' % c)
def test_against_fp64(case, acc):
    T, B, L, D = case
    alpha, dz, prev = operands(T, B, L, D, seed=T + 7 * L + D)
    got = run_packed(alpha, dz, prev, acc)
    check(got, alpha, dz, prev, acc, what=str(case))
    if not acc:      # the overwrite never reads the map: NaN there changes nothing
        assert torch.equal(got, run_packed(alpha, dz, np.full_like(prev, np.nan), 0))


@pytest.mark.parametrize('case', IC.REFUSED, ids=lambda c: 'T%d_B%d_L%d_D%d' % c)
def test_first_size_past_the_lds_limit_is_refused_untouched(case):
    T, B, L, D = case
    a = torch.zeros(T * B * L, device=DEV)
    g = torch.zeros(T * B * D, device=DEV)
    o = torch.full((B * L * D,), GUARD, device=DEV)
    assert call(T, a, B * L, g, B * D, D, B, L, D, o, L * D, D, 0) == -1
    torch.cuda.synchronize()
    assert bool((o == GUARD).all())


@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('D, pad', [(8, 4), (8, 3), (7, 2), (1028, 4)], ids=['vec', 'vec_map_scalar_strides', 'scalar', 'two_tiles'])
def test_padded_strides_and_guards(D, pad, acc):
    """sb, sl, lddz, dz_st and alpha_st larger than packed; everything between the rows is a guard value and stays one."""
    T, B, L = 3, 2, 9
    alpha, dz, prev = operands(T, B, L, D, seed=5 + D)
    sl, lddz = D + pad, D + pad
    sb, dz_st, alpha_st = L * sl + 2 * pad, B * lddz + 4, B * L + 5
    a = torch.full((T * alpha_st,), GUARD, device=DEV)
    a.view(T, alpha_st)[:, :B * L] = torch.from_numpy(alpha).to(DEV).reshape(T, B * L)
    g = torch.full((T * dz_st,), GUARD, device=DEV)
    gv = g.view(T, dz_st)[:, :B * lddz].view(T, B, lddz)
    gv[:, :, :D] = torch.from_numpy(dz).to(DEV)
    o = torch.full((B * sb + 16,), GUARD, device=DEV)
    ov = o[:B * sb].view(B, sb)[:, :L * sl].view(B, L, sl)
    ov[:, :, :D] = torch.from_numpy(prev).to(DEV)
    before = o.clone()
    assert call(T, a, alpha_st, g, dz_st, lddz, B, L, D, o, sb, sl, acc) == 0
    torch.cuda.synchronize()
    got = ov[:, :, :D].cpu()
    check(got, alpha, dz, prev, acc, what='strided D %d pad %d' % (D, pad))
    mask = torch.ones_like(o, dtype=torch.bool)
    mask[:B * sb].view(B, sb)[:, :L * sl].view(B, L, sl)[:, :, :D] = False
    assert torch.equal(o[mask], before[mask]) and bool((o[mask] == GUARD).all())
    # the packed run of the same values: the same chain, the same bits
    assert torch.equal(got, run_packed(alpha, dz, prev, acc))


@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('case', [(8, 3, 49, 64), (3, 2, 9, 1028), (9, 2, 6, 12)], ids=lambda c: 'T%d_B%d_L%d_D%d' % c)
def test_pointer_one_float_off_takes_the_scalar_form_same_bits(case, acc):
    T, B, L, D = case
    alpha, dz, prev = operands(T, B, L, D, seed=11)
    aligned = run_packed(alpha, dz, prev, acc)
    shifted = run_packed(alpha, dz, prev, acc, off=1)
    assert torch.equal(aligned, shifted)
    check(shifted, alpha, dz, prev, acc, what='off by one float %s' % (case,))


@pytest.mark.parametrize('acc', [0, 1])
@pytest.mark.parametrize('L, D', [(11, 8), (11, 7), (37, 1028)], ids=['vec', 'scalar', 'two_tiles'])
def test_ragged_lengths_never_load_the_padding(L, D, acc):
    T, B = 4, 5
    lens = [L, 1, 0, L + 3, L // 2]                    # full, one row, 0 (clamped to 1), past the map (clamped), a middle value
    alpha, dz, prev = operands(T, B, L, D, seed=13 + D)
    n = np.clip(lens, 1, L)
    for b in range(B):
        alpha[:, b, n[b]:] = np.nan
        prev[b, n[b]:] = np.nan
    got = run_packed(alpha, dz, prev, acc, lens)
    check(got, alpha, dz, prev, acc, lens, what='ragged L %d D %d' % (L, D))
    for b in range(B):
        pad = got[b, n[b]:]
        if acc:
            assert bool(torch.isnan(pad).all())          # left alone
        else:
            assert bool((pad == 0).all())                # exact zeros
        assert bool(torch.isfinite(got[b, :n[b]]).all())
    # full lengths are the call without lengths, bit for bit
    alpha, dz, prev = operands(T, B, L, D, seed=14)
    assert torch.equal(run_packed(alpha, dz, prev, acc, [L] * B), run_packed(alpha, dz, prev, acc))


def test_two_runs_are_bit_identical():
    for case in ((8, 2, 196, 2048), (9, 2, 6, 12), (2, IC.MIN_BLOCKS, IC.LC_BIG + 1, 4)):
        alpha, dz, prev = operands(*case, seed=17)
        for acc in (0, 1):
            assert torch.equal(run_packed(alpha, dz, prev, acc), run_packed(alpha, dz, prev, acc))


def test_steps_cut_in_two_calls_continue_the_same_chain():
    """What rfn_prefix_bwd_inputs does past the LDS limit: the later call accumulates, the chain per element is the same."""
    T, B, L, D = 9, 2, 6, 12
    alpha, dz, prev = operands(T, B, L, D, seed=19)
    whole = run_packed(alpha, dz, prev, 0)
    first = run_packed(alpha[:5], dz[:5], prev, 0)
    both = run_packed(np.ascontiguousarray(alpha[5:]), np.ascontiguousarray(dz[5:]), first.numpy(), 1)
    assert torch.equal(whole, both)
