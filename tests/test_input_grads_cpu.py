"""Gradients of fc_feats / att_feats, the parts that need no GPU: the two new entries are declared in rfn.h, exported and bound,
the ABI version did not move; their refusals that come before any launch (dummy non-NULL pointers: nothing is dereferenced);
and the numpy restatement of rfn_attn_context_bwd_dseq_steps' contract that tests/test_dseq_steps_gpu.py uses as its reference
(tests/input_grads_cases.py, ragged rule included) equals a plain loop; the sweep's case table reaches the launcher's edges."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import input_grads_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('rfn_attn_context_bwd_dseq_steps', 'rfn_prefix_bwd_inputs')
SHAPE, UNSUPPORTED, ARG = -1, -2, -5     # rfn.h RFN_ERR_*


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def test_new_entries_are_declared_exported_and_bound():
    N = native()
    src = open(os.path.join(ROOT, 'include', 'rfn.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(rfn_[a-z0-9_]+)\s*\(', src))
    for s in NEW_SYMBOLS:
        assert s in declared, '%s is not declared in rfn.h' % s
        assert hasattr(N.lib, s), 'librfn_hip.so does not export %s' % s
        assert s in N.EXPORTS, '_native.py does not bind %s' % s
    assert len(N.lib.rfn_attn_context_bwd_dseq_steps.argtypes) == 15
    assert len(N.lib.rfn_prefix_bwd_inputs.argtypes) == 9
    assert re.search(r'#define\s+RFN_PATH_OPT_INPUT_GRADS\s+512u\b', open(os.path.join(ROOT, 'include', 'rfn.h')).read())
    assert N.PATH_OPT_INPUT_GRADS == 512


def test_abi_version_did_not_move():
    N = native()
    assert N.lib.rfn_abi_version() == 9 and N.ABI_VERSION == 9
    assert re.search(r'#define\s+RFN_ABI_VERSION\s+9\b', open(os.path.join(ROOT, 'include', 'rfn.h')).read())


def test_kernel_entry_refuses_before_launching():
    N = native()
    f = N.lib.rfn_attn_context_bwd_dseq_steps
    p = 0x1000     # never dereferenced: every call below is refused on the host

    def call(T=2, alpha=p, dz=p, B=2, L=3, D=4, out=p):
        return f(T, alpha, B * L, dz, B * D, D, B, L, D, out, L * D, D, 0, None, None)

    assert call(T=0) == SHAPE and call(T=-1) == SHAPE
    assert call(L=0) == SHAPE and call(B=0) == SHAPE and call(D=0) == SHAPE
    assert call(alpha=None) == ARG and call(dz=None) == ARG and call(out=None) == ARG
    assert call(T=0, alpha=None) == SHAPE                        # shape checks come first
    # the LDS tile: T * min(Dp, 1024) + 32 * Tp floats <= 64 KiB
    assert call(T=16, D=1024) == SHAPE and call(T=16, D=1021) == SHAPE and call(T=16, D=5000) == SHAPE
    assert call(T=453, D=4) == SHAPE and call(T=453, D=1) == SHAPE


def test_path_entry_refuses_without_the_flag():
    N = native()
    d = N.make_dims(2, 16, 16, 16, 3, 3, 20, 51, [7, 12], [8, 12], [8, 12])
    p = 0x1000
    arr = (C.c_void_p * 2)(p, p)
    f = N.lib.rfn_prefix_bwd_inputs
    assert f(C.byref(d), 3, p, arr, arr, p, 1 << 40, None, None) == UNSUPPORTED
    assert f(C.byref(d), 0, p, arr, arr, p, 1 << 40, None, None) == SHAPE
    assert f(C.byref(d), 3, None, arr, arr, p, 1 << 40, None, None) == ARG
    # with the bit: a workspace of the inference size is refused as such, a smaller one as too small
    g = N.make_dims(2, 16, 16, 16, 3, 3, 20, 51, [7, 12], [8, 12], [8, 12], path_flags=N.PATH_OPT_INPUT_GRADS)
    infer, train = N.lib.rfn_prefix_ws_bytes(C.byref(g), 3, 0), N.lib.rfn_prefix_ws_bytes(C.byref(g), 3, 1)
    assert 0 < infer < train
    assert f(C.byref(g), 3, p, arr, arr, p, infer, None, None) == UNSUPPORTED
    assert f(C.byref(g), 3, p, arr, arr, p, train - 1, None, None) == UNSUPPORTED
    assert f(C.byref(g), 3, p, arr, arr, p, infer - 1, None, None) == -4       # RFN_ERR_WORKSPACE
    # the bit buys T1 d z slices (256-B aligned) instead of one buffer per encoder, and nothing without training
    base = N.lib.rfn_prefix_ws_bytes(C.byref(d), 3, 1)
    assert train - base == 4 * sum(3 * (-(-3 * D // 64) * 64) - (-(-3 * D // 64) * 64) for D in (8, 12))
    assert N.lib.rfn_prefix_ws_bytes(C.byref(d), 3, 0) == infer


def plain_loop(alpha, dz, prev, accumulate, lens):
    T, B, L = alpha.shape
    D = dz.shape[2]
    out = np.array(prev, dtype=np.float64)
    for b in range(B):
        n = L if lens is None else min(max(int(lens[b]), 1), L)
        for l in range(L):
            if l >= n:
                if not accumulate:
                    out[b, l, :] = 0.0
                continue
            for d in range(D):
                acc = out[b, l, d] if accumulate else 0.0
                for t in range(T):
                    acc += float(alpha[t, b, l]) * float(dz[t, b, d])
                out[b, l, d] = acc
    return out


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('lens', [None, [5, 1, 0, 8, 3]])
def test_reference_restatement_is_the_plain_loop(accumulate, lens):
    rng = np.random.default_rng(3)
    T, B, L, D = 3, 5, 5, 6
    alpha, dz, prev = rng.standard_normal((T, B, L)), rng.standard_normal((T, B, D)), rng.standard_normal((B, L, D))
    if lens is not None:
        for b in range(B):
            alpha[:, b, min(max(lens[b], 1), L):] = np.nan          # the padding is never used
    got, mag = IC.dseq_steps_ref(alpha, dz, prev, accumulate, lens)
    want = plain_loop(alpha, dz, prev, accumulate, lens)
    assert np.isfinite(got).all() and np.abs(got - want).max() < 1e-13
    live = np.arange(L)[None, :] < (np.full(B, L) if lens is None else np.clip(lens, 1, L))[:, None]
    assert (mag >= np.abs(got) - 1e-13)[live].all() and (mag[~live] == 0).all()
    if lens is not None and not accumulate:
        assert (got[2, 1:] == 0).all() and (got[1, 1:] == 0).all() and not (got[3] == 0).any()
    if lens is not None and accumulate:
        assert (got[2, 1:] == prev[2, 1:]).all()


def test_case_table_reaches_the_launcher_edges():
    N = native()
    f = N.lib.rfn_attn_context_bwd_dseq_steps
    cases = set(IC.CASES)
    for c in ((1, 1, 1, 1), (3, 2, 5, 7), (8, 3, 49, 64), (8, 2, 196, 2048), (9, 2, 6, 12)):      # the issue's own
        assert c in cases
    ds = {D for _, _, _, D in cases}
    assert {IC.DT - 4, IC.DT, IC.DT + 4} <= ds and any(D % 4 for D in ds)
    for lc in (IC.LC_SMALL, IC.LC_BIG):      # each chunk size at -1, 0, +1 rows
        got = {L - lc for T, B, L, D in cases if IC.rows_per_block(B, L, D) == lc}
        assert {-1, 0, 1} <= got, (lc, sorted(got))
    # the LDS limit from both sides, as the library itself counts it
    assert any(T == IC.max_steps(D) for T, _, _, D in cases)
    for T, B, L, D in IC.CASES:
        assert T <= IC.max_steps(D) and B * L * D <= 1 << 20
    for T, B, L, D in IC.REFUSED:
        assert T == IC.max_steps(D) + 1
        assert f(T, 0x1000, B * L, 0x1000, B * D, D, B, L, D, 0x1000, L * D, D, 0, None, None) == SHAPE
