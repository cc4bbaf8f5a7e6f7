"""rfn_attn_fwd_ragged / rfn_attn_bwd_ragged (csrc/rfn_attn.hip) through the C ABI, over the case table of tests/ragged_cases.py.

Per case, with the padded rows of proj and att_seq filled with zeros and then with N(0, 1e4^2) noise:
  1. every image's alpha[:n], z, dproj[:n], dhproj and the column sum of dw_part against fp64 attention over that image's first
     n rows alone, with the tolerances of tests/test_attention_edges_gpu.py unchanged (same operand regime);
  2. alpha[n:] == 0 exactly; dproj[n:] == 0 exactly without accumulate, the accumulated-onto bits untouched with it;
  3. every output equal (==) between the two paddings;
  4. len = [L] * B and len = NULL bit-identical to rfn_attn_fwd_het / rfn_attn_bwd_het on the same buffers;
  5. len = 1: alpha = [1, 0, ...] and z == att_seq[b, 0] exactly;
  6. the error contract: bad ngroups RFN_ERR_SHAPE, a NULL required pointer RFN_ERR_ARG, outputs untouched.
Outputs are NaN-filled before every call, so an element that was not written shows."""
import ctypes as C

import pytest
import torch

import ragged_cases as RC

pytestmark = pytest.mark.gpu

NAN = float('nan')
ERR_SHAPE, ERR_ARG = -1, -5


def N():
    import recurrent_fusion_network_amd._native as n
    return n


def ints(v):
    return (C.c_int * len(v))(*v)


def bits(t):
    return t.contiguous().view(torch.int32)


class Run:
    """One forward + backward of a case on the device.  lens: per encoder a list, None (NULL entry), or 'null_array'."""

    def __init__(self, c, ops, lens, accumulate=0, entry='ragged', in_place=False, dev='cuda:0'):
        n = N()
        B, A, ng = c['B'], c['A'], len(c['maps'])
        d = lambda t: t.to(dev).contiguous()  # noqa: E731
        self.ops = [{k: d(v) for k, v in o.items()} for o in ops]
        Ls, Ds = [m[0] for m in c['maps']], [m[1] for m in c['maps']]
        self.scr = [torch.full((B, L), NAN, device=dev) for L in Ls]
        self.alpha = [torch.full((B, L), NAN, device=dev) for L in Ls]
        self.z = [torch.full((B, D), NAN, device=dev) for D in Ds]
        self.len_t = None
        len_arr = None
        if lens is not None and lens != 'null_array':     # None: the _het entries take no lengths at all
            self.len_t = [None if v is None else torch.tensor(v, dtype=torch.int32, device=dev) for v in lens]
            len_arr = n.ptr_array(self.len_t)
        col = lambda k: n.ptr_array([o[k] for o in self.ops])  # noqa: E731
        st = n.stream_ptr()
        if entry == 'ragged':
            self.rc_fwd = n.lib.rfn_attn_fwd_ragged(ng, col('proj'), col('hproj'), col('w'), col('bo'), col('x'), B, ints(Ls), A,
                                                    ints(Ds), n.ptr_array(self.scr), n.ptr_array(self.alpha), n.ptr_array(self.z),
                                                    len_arr, st)
        else:
            self.rc_fwd = n.lib.rfn_attn_fwd_het(ng, col('proj'), col('hproj'), col('w'), col('bo'), col('x'), B, ints(Ls), A,
                                                 ints(Ds), n.ptr_array(self.scr), n.ptr_array(self.alpha), n.ptr_array(self.z), st)
        if in_place:
            self.dproj = [o['proj'].clone() for o in self.ops]
            proj_in = n.ptr_array(self.dproj)
        else:
            self.dproj = [o['dproj0'].clone() if accumulate else torch.full_like(o['proj'], NAN) for o in self.ops]
            proj_in = col('proj')
        self.dhp = [torch.full((B, A), NAN, device=dev) for _ in Ls]
        self.dw = [torch.full((B, A), NAN, device=dev) for _ in Ls]
        args = [ng, proj_in, col('hproj'), col('w'), n.ptr_array(self.alpha), col('x'), col('dz'), B, ints(Ls), A, ints(Ds),
                n.ptr_array(self.dproj), accumulate, n.ptr_array(self.dhp), n.ptr_array(self.dw)]
        if entry == 'ragged':
            self.rc_bwd = n.lib.rfn_attn_bwd_ragged(*args, len_arr, st)
        else:
            self.rc_bwd = n.lib.rfn_attn_bwd_het(*args, st)
        torch.cuda.synchronize()
        assert self.rc_fwd == 0 and self.rc_bwd == 0, (self.rc_fwd, self.rc_bwd)

    def outputs(self):
        return self.alpha + self.z + self.dproj + self.dhp + self.dw


def err(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def check_against_fp64(c, ops, run, accumulate):
    for g, o in enumerate(ops):
        ref_dw = torch.zeros(c['A'], dtype=torch.float64)
        got = dict(alpha=run.alpha[g].cpu(), z=run.z[g].cpu(), dproj=run.dproj[g].cpu(), dhp=run.dhp[g].cpu(), dw=run.dw[g].cpu())
        for b in range(c['B']):
            n = RC.n_of(c, g, b)
            alpha, z, dproj, dhp, dw = RC.plain_attention(o['proj'][b, :n], o['hproj'][b], o['w'], o['bo'], o['x'][b, :n], o['dz'][b])
            ref_dw += dw
            tag = (c['name'], g, b, n)
            assert err(got['alpha'][b, :n], alpha) < RC.TOL['alpha'], tag
            assert err(got['z'][b], z) < RC.TOL['z'], tag
            want = dproj + o['dproj0'][b, :n].double() if accumulate else dproj
            assert err(got['dproj'][b, :n], want) < RC.TOL['dproj'], tag
            assert err(got['dhp'][b], dhp) < RC.TOL['dhp'], tag
            # 2. exact zeros / untouched
            assert bool((got['alpha'][b, n:] == 0).all()), tag
            if accumulate:
                assert torch.equal(bits(got['dproj'][b, n:]), bits(o['dproj0'][b, n:])), tag
            else:
                assert bool((got['dproj'][b, n:] == 0).all()), tag
            if n == 1:     # 5. one valid row: its weight is exactly 1 and the context is that row
                assert float(got['alpha'][b, 0]) == 1.0 and torch.equal(got['z'][b], o['x'][b, 0]), tag
        assert err(got['dw'].double().sum(0), ref_dw) < RC.TOL['dw'] * max(1.0, float(ref_dw.abs().max())), (c['name'], g)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('name', [c['name'] for c in RC.CASES])
def test_ragged_against_fp64_and_padding(name, accumulate):
    c = RC.CASE_BY_NAME[name]
    base = RC.operands(c)
    zeros, noise = RC.fill_padding(c, base, 0.0), RC.fill_padding(c, base, 1e4)
    r0 = Run(c, zeros, c['lens'], accumulate)
    r1 = Run(c, noise, c['lens'], accumulate)
    check_against_fp64(c, zeros, r0, accumulate)
    check_against_fp64(c, noise, r1, accumulate)
    for a, b in zip(r0.outputs(), r1.outputs()):          # 3. the padding is never read: not one bit moves
        assert not bool(torch.isnan(a).any()) and bool((a == b).all()), name
    if not accumulate:                                    # dproj aliasing proj, as the path calls it
        r2 = Run(c, noise, c['lens'], 0, in_place=True)
        for a, b in zip(r1.outputs(), r2.outputs()):
            assert torch.equal(bits(a), bits(b)), name


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('name', [c['name'] for c in RC.CASES])
def test_full_lengths_are_the_het_calls_bit_for_bit(name, accumulate):
    c = RC.CASE_BY_NAME[name]
    ops = RC.operands(c)
    want = Run(c, ops, None, accumulate, entry='het').outputs()
    full = [[L] * c['B'] for L, _ in c['maps']]
    over = [[L + 5] * c['B'] for L, _ in c['maps']]       # the kernel clamps: beyond L is L
    for lens in (full, [None] * len(c['maps']), 'null_array', over):
        got = Run(c, ops, lens, accumulate).outputs()
        for a, b in zip(want, got):
            assert torch.equal(bits(a), bits(b)), (name, lens)


def test_len_one_and_the_lower_clamp():
    c = dict(RC.CASE_BY_NAME['vec'])
    ops = RC.fill_padding(dict(c, lens=[[1, 1, 1]]), RC.operands(c), 1e4)
    for lens in ([1, 1, 1], [0, -7, 1]):                  # below 1 is 1
        r = Run(c, ops, [lens])
        for b in range(c['B']):
            want = torch.zeros(9)
            want[0] = 1.0
            assert torch.equal(r.alpha[0][b].cpu(), want)
            assert torch.equal(r.z[0][b].cpu(), ops[0]['x'][b, 0])
            assert bool((r.dproj[0][b, 1:] == 0).all())
            # softmax over one entry has no gradient: ds = alpha * (dalpha - alpha * dalpha) = 0
            assert bool((r.dproj[0][b, 0] == 0).all()) and bool((r.dhp[0][b] == 0).all()) and bool((r.dw[0][b] == 0).all())


def test_error_contract():
    n = N()
    dev = 'cuda:0'
    c = RC.CASE_BY_NAME['het']
    ops = [{k: v.to(dev) for k, v in o.items()} for o in RC.operands(c)]
    B, A = c['B'], c['A']
    Ls, Ds = [m[0] for m in c['maps']], [m[1] for m in c['maps']]
    outs = dict(scr=[torch.full((B, L), NAN, device=dev) for L in Ls], alpha=[torch.full((B, L), NAN, device=dev) for L in Ls],
                z=[torch.full((B, D), NAN, device=dev) for D in Ds], dproj=[torch.full((B, L, A), NAN, device=dev) for L in Ls],
                dhp=[torch.full((B, A), NAN, device=dev) for _ in Ls], dw=[torch.full((B, A), NAN, device=dev) for _ in Ls])
    lens = [torch.tensor(c['lens'][0], dtype=torch.int32, device=dev), None]
    col = lambda k: n.ptr_array([o[k] for o in ops])  # noqa: E731
    al_in = [torch.softmax(torch.randn(B, L), 1).to(dev) for L in Ls]

    def fwd(ng=2, proj=None, alpha=None, L=None):
        return n.lib.rfn_attn_fwd_ragged(ng, col('proj') if proj is None else proj, col('hproj'), col('w'), col('bo'), col('x'), B,
                                         ints(L or Ls), A, ints(Ds), n.ptr_array(outs['scr']),
                                         n.ptr_array(outs['alpha']) if alpha is None else alpha, n.ptr_array(outs['z']),
                                         n.ptr_array(lens), n.stream_ptr())

    def bwd(ng=2, proj=None, dproj=None, L=None):
        return n.lib.rfn_attn_bwd_ragged(ng, col('proj') if proj is None else proj, col('hproj'), col('w'), n.ptr_array(al_in),
                                         col('x'), col('dz'), B, ints(L or Ls), A, ints(Ds),
                                         n.ptr_array(outs['dproj']) if dproj is None else dproj, 0, n.ptr_array(outs['dhp']),
                                         n.ptr_array(outs['dw']), n.ptr_array(lens), n.stream_ptr())

    for ng in (0, -1, 9):
        assert fwd(ng=ng) == ERR_SHAPE and bwd(ng=ng) == ERR_SHAPE
    assert fwd(L=[7, 0]) == ERR_SHAPE and bwd(L=[7, 0]) == ERR_SHAPE
    assert fwd(proj=C.c_void_p(None)) == ERR_ARG and bwd(proj=C.c_void_p(None)) == ERR_ARG          # a NULL host array
    assert fwd(proj=n.ptr_array([ops[0]['proj'], None])) == ERR_ARG                                  # a NULL entry
    assert bwd(proj=n.ptr_array([ops[0]['proj'], None])) == ERR_ARG
    assert fwd(alpha=n.ptr_array([outs['alpha'][0], None])) == ERR_ARG
    assert bwd(dproj=n.ptr_array([outs['dproj'][0], None])) == ERR_ARG
    torch.cuda.synchronize()
    for k, ts in outs.items():
        for t in ts:
            assert bool(torch.isnan(t).all()), 'a refused call wrote %s' % k
    assert fwd() == 0 and bwd() == 0                      # the same buffers are fine
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for k in ('alpha', 'z', 'dproj', 'dhp', 'dw') for t in outs[k])
