"""Ragged attention maps (rfn.h rfn_attn_fwd_ragged / rfn_attn_bwd_ragged, rfn_prefix_*_ex): the case table of the kernel
sweep and a plain fp64 restatement of attention over the first len[b] rows of every image, on the CPU.

Constants restated from csrc/rfn_attn.hip (nothing is imported from the C side):
    SC_ROWS 16         rows of one raw-score block: a block whose first row is >= len[b] leaves before it loads anything
    CTX_UNROLL 4       rows per trip of the context kernel's unrolled loop, then a remainder loop
    DAL_GROUP 4        rows a wave walks together in the fused d-alpha sweep (tail: min(4, n - l0) rows)
    SB_WAVES 16, SB_UNROLL 4 -> 64 rows per sweep of the score-backward loop and of the d-alpha loop
    context kernel: 1024 columns per block with 16-byte loads, 256 scalar; block 0 publishes alpha
"""
import torch

SC_ROWS = 16
CTX_UNROLL = 4
DAL_GROUP = 4
SB_WAVES, SB_UNROLL = 16, 4
SWEEP = SB_WAVES * SB_UNROLL
TOL = dict(alpha=2e-6, z=1e-5, dproj=2e-5, dhp=1e-4, dw=1e-4)      # tests/test_attention_edges_gpu.py, unchanged

NEW_SYMBOLS = ['rfn_attn_fwd_ragged', 'rfn_attn_bwd_ragged', 'rfn_prefix_fwd_ex', 'rfn_prefix_fwd_from_state_ex',
               'rfn_prefix_bwd_ex']
ATT_LENS_METHODS = ['forward', 'forward_loss', 'get_thought_vectors', 'sample', 'sample_beam', 'sample_group', 'sample_distinct',
                    'score']
ENSEMBLE_METHODS = ['sample', 'sample_beam', 'score']

L_SC = 2 * SC_ROWS + 1
L_SW = SWEEP + 6


def case(name, B, A, maps, lens):
    """maps: [(L, D)] per encoder; lens: per encoder a list of B counts or None (a NULL entry: every row)."""
    assert len(maps) == len(lens) and all(v is None or len(v) == B for v in lens)
    return dict(name=name, B=B, A=A, maps=list(maps), lens=list(lens))


# (B, L, A, D): the smallest shapes that reach each path
CASES = [
    case('vec', 3, 8, [(9, 8)], [[9, 1, 5]]),                                    # 16-byte instantiations
    case('scalar', 3, 6, [(9, 6)], [[9, 1, 5]]),                                 # scalar instantiations
    # score blocks that fall wholly past a row's length (blocks of SC_ROWS rows)
    case('score_blocks_vec', 4, 8, [(L_SC, 8)], [[SC_ROWS - 1, SC_ROWS, SC_ROWS + 1, L_SC]]),
    case('score_blocks_scalar', 4, 6, [(L_SC, 6)], [[SC_ROWS - 1, SC_ROWS, SC_ROWS + 1, L_SC]]),
    # len % 4 = 0, 1, 2, 3: the context kernel's unroll and its tail, the d-alpha row-group tails
    case('mod4_vec', 4, 8, [(12, 8)], [[8, 5, 6, 7]]),
    case('mod4_scalar', 4, 6, [(12, 6)], [[8, 5, 6, 7]]),
    # ... and the same tails in the second 64-row sweep of the backward loops
    case('second_sweep', 5, 8, [(L_SW, 8)], [[SWEEP, SWEEP + 1, SWEEP + 2, SWEEP + 3, L_SW]]),
    # more than one context block per image (only block 0 writes alpha and its zeros)
    case('two_ctx_blocks_vec', 2, 8, [(9, 1028)], [[5, 9]]),
    case('two_ctx_blocks_scalar', 2, 6, [(9, 258)], [[5, 9]]),
    # heterogeneous launch: the first map gets lengths, the second a NULL entry
    case('het', 3, 8, [(7, 8), (12, 12)], [[7, 1, 4], None]),
    case('het_scalar', 3, 6, [(7, 6), (12, 10)], [[7, 1, 4], None]),
]
CASE_BY_NAME = {c['name']: c for c in CASES}


def n_of(c, g, b):
    L = c['maps'][g][0]
    return L if c['lens'][g] is None else c['lens'][g][b]


def operands(c, seed=0):
    """Unit-normal operands, w_out at scale 0.3 (the regime of test_attention_edges_gpu.py): per encoder a dict of CPU f32
    tensors proj (B, L, A), hproj (B, A), w (A,), bo (1,), x (B, L, D), dz (B, D), dproj0 (B, L, A) (what an accumulating
    backward adds onto)."""
    g = torch.Generator().manual_seed(1234 + seed)
    out = []
    for (L, D) in c['maps']:
        B, A = c['B'], c['A']
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        out.append(dict(proj=r(B, L, A), hproj=r(B, A), w=r(A) * 0.3, bo=r(1), x=r(B, L, D), dz=r(B, D), dproj0=r(B, L, A)))
    return out


def plain_attention(proj, hproj, w, bo, x, dz):
    """fp64 AttentionModelCore forward + the rfn.h backward formulas for ONE image: proj (n, A), hproj (A,), x (n, D), dz (D,)
    -> alpha (n,), z (D,), dproj (n, A), dhproj (A,), dw (A,)."""
    proj, hproj, w, bo, x, dz = (t.double() for t in (proj, hproj, w, bo, x, dz))
    e = torch.tanh(proj + hproj[None, :])
    alpha = torch.softmax(e @ w + bo, 0)
    z = alpha @ x
    dalpha = x @ dz
    ds = alpha * (dalpha - (alpha * dalpha).sum())
    dproj = ds[:, None] * w[None, :] * (1 - e * e)
    return alpha, z, dproj, dproj.sum(0), (ds[:, None] * e).sum(0)


def masked_attention(proj, hproj, w, bo, x, dz, lens):
    """The same for a batch, as a MASK: scores past lens[b] are -inf, everything else runs over all L rows.  -> alpha (B, L),
    z (B, D), dproj (B, L, A), dhproj (B, A), dw_part (B, A); alpha and dproj are exactly 0 past lens[b]."""
    proj, hproj, w, bo, x, dz = (t.double() for t in (proj, hproj, w, bo, x, dz))
    B, L, _ = proj.shape
    keep = torch.arange(L)[None, :] < torch.as_tensor(lens)[:, None]
    e = torch.tanh(proj + hproj[:, None, :])
    scores = (e @ w + bo).masked_fill(~keep, float('-inf'))
    alpha = torch.softmax(scores, 1)
    z = torch.einsum('bl,bld->bd', alpha, torch.where(keep[:, :, None], x, torch.zeros_like(x)))
    dalpha = torch.where(keep, torch.einsum('bld,bd->bl', x, dz), torch.zeros_like(alpha))
    ds = alpha * (dalpha - (alpha * dalpha).sum(1, keepdim=True))
    dproj = ds[:, :, None] * w[None, None, :] * (1 - e * e)
    dproj = torch.where(keep[:, :, None], dproj, torch.zeros_like(dproj))
    return alpha, z, dproj, dproj.sum(1), torch.where(keep[:, :, None], ds[:, :, None] * e, torch.zeros_like(e)).sum(1)


def fill_padding(c, ops, std, seed=99):
    """Copies of the operands with the rows past each image's length of proj and x replaced: zeros (std = 0) or N(0, std^2)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for gi, o in enumerate(ops):
        o = {k: v.clone() for k, v in o.items()}
        for b in range(c['B']):
            n = n_of(c, gi, b)
            for k in ('proj', 'x'):
                pad = o[k][b, n:]
                o[k][b, n:] = torch.randn(pad.shape, generator=g) * std if std else torch.zeros_like(pad)
        out.append(o)
    return out
