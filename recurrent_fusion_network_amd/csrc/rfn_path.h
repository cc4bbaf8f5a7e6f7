// Host-side sequencing of the recurrent-fusion caption-decoder path on one MI355X.
//
// Restates the control flow of RecurrentFusionModel.forward / sample
// (misc/RecurrentFusionModel.py:198-281, 545-658) as a fixed schedule of HIP launches on one stream:
//   phase 1 (rfn_prefix_*): fc2h -> T1 x M fusion-stage-I cells -> reason heads -> state mean ->
//                           T2 fusion-stage-II cells                       (:199-255, 283-343)
//   phase 2 (rfn_decoder_*): embed -> attention-LSTM decoder -> logit + log_softmax (:257-281)
// What is different from the reference's per-step Python loop of ~1500 ATen calls:
//   * every attention feature projection att_2_att_h does not depend on h, so all T1 (stage I),
//     T2 (stage II) step weights of one encoder are applied in ONE grouped MFMA GEMM before the
//     recurrence, and the decoder's is applied once instead of 17 times;
//   * all activations are kept time-major ((step, batch, feature)), so "stack + transpose +
//     contiguous" (:223-227, 246-251) disappears, the stage-II / decoder attention reads the thought
//     vectors through strides, and every weight gradient that is shared across steps is ONE GEMM
//     over (steps*batch) rows;
//   * the teacher-forced i2h(x_t) and logit(h_t) of all steps are batched GEMMs;
//   * backward never materialises tanh outputs: the projection slice is overwritten in place by its
//     gradient, which then feeds the grouped weight-gradient GEMM (the 77 % CPU hotspot).
// No allocation, no synchronisation, no global state: buffers come from the caller's workspace.
// This header is internal to the rfn_path_*.hip translation units: parameter order, GEMM / cell-GEMM launch helpers, workspace
// layouts and the predicates that several phases have to agree on (definitions: rfn_path_common.hip).
#pragma once
#include <stdio.h>
#include <string.h>
#include <initializer_list>

#include <vector>

#include "rfn_internal.h"

// hidden: none of this is part of the exported ABI of librfn_hip.so
namespace rfn_path __attribute__((visibility("hidden"))) {

// ---------------------------------------------------------------------------------------------
// canonical parameter order (names: SURVEY.md 8b)
// ---------------------------------------------------------------------------------------------
struct PIdx {
    int M, T1, T2;
    explicit PIdx(const rfn_dims* d) : M(d->M), T1(d->T1), T2(d->T2) {}
    int fc_w(int i) const { return 2 * i; }
    int fc_b(int i) const { return 2 * i + 1; }
    int embed() const { return 2 * M; }
    int logit_w() const { return 2 * M + 1; }
    int logit_b() const { return 2 * M + 2; }
    // stage I cell (t, i): k = 0 att_2_att_h.w, 1 .b, 2 h_2_att_h.w, 3 .b, 4 att_h_2_out.w, 5 .b,
    //                          6 H2h.w, 7 H2h.b, 8 z2h.w, 9 z2h.b
    int s1(int t, int i, int k) const { return 2 * M + 3 + (t * M + i) * 10 + k; }
    int rind_w(int i) const { return 2 * M + 3 + T1 * M * 10 + 2 * i; }
    int rind_b(int i) const { return rind_w(i) + 1; }
    int s2base(int t) const { return 2 * M + 3 + T1 * M * 10 + 2 * M + t * (2 + 8 * M); }
    int s2_hh_w(int t) const { return s2base(t); }
    int s2_hh_b(int t) const { return s2base(t) + 1; }
    // stage II cell t, encoder i: k = 0 z_2_h.w, 1 .b, 2 att_2_att_h.w, 3 .b, 4 h_2_att_h.w, 5 .b,
    //                                 6 att_h_2_out.w, 7 .b
    int s2(int t, int i, int k) const { return s2base(t) + 2 + 8 * i + k; }
    int r_w() const { return s2base(T2); }
    int r_b() const { return r_w() + 1; }
    // decoder: 0 i2h.w, 1 .b, 2 h2h.w, 3 .b, 4 z2h.w, 5 .b, 6 att_2_att_h.w, 7 .b, 8 h_2_att_h.w,
    //          9 .b, 10 att_h_2_out.w, 11 .b
    int dec(int k) const { return r_w() + 2 + k; }
    int count() const { return r_w() + 2 + 12; }
};

// The `seed` argument of an entry point as the launches carry it: the key itself, or -- RFN_PATH_OPT_SEED_DEV -- the device
// address of the key (rfn.h).  Every entry point resolves it once, before anything is launched.
int path_seed(const rfn_dims* d, uint64_t seed_arg, RfnSeed* out);
int check_dims(const rfn_dims* d);

// ---------------------------------------------------------------------------------------------
// GEMM helpers.  lin(): Y = X W^T + b.  dx(): dX = dY W.  dw(): dW = dY^T X.
// ---------------------------------------------------------------------------------------------
inline rfn_gemm_seg seg_lin(const float* X, long ldx, const float* W, long ldw, int K, const float* bias) {
    rfn_gemm_seg s;
    memset(&s, 0, sizeof(s));
    s.A = X; s.lda = ldx; s.a_kfast = 1;
    s.B = W; s.ldb = ldw; s.b_kfast = 1;
    s.K = K; s.bias = bias;
    return s;
}
// dX[m, k] = sum_n dY[m, n] W[n, k]   (W is (N, Kout) row-major, ld ldw)
inline rfn_gemm_seg seg_dx(const float* dY, long lddy, const float* W, long ldw, int N) {
    rfn_gemm_seg s;
    memset(&s, 0, sizeof(s));
    s.A = dY; s.lda = lddy; s.a_kfast = 1;
    s.B = W; s.ldb = ldw; s.b_kfast = 0;
    s.K = N;
    return s;
}
// dW[n, k] = sum_m dY[m, n] X[m, k]
inline rfn_gemm_seg seg_dw(const float* dY, long lddy, const float* X, long ldx, int rows) {
    rfn_gemm_seg s;
    memset(&s, 0, sizeof(s));
    s.A = dY; s.lda = lddy; s.a_kfast = 0;
    s.B = X; s.ldb = ldx; s.b_kfast = 0;
    s.K = rows;
    return s;
}
// stream + split-K scratch handed to every GEMM of a phase
struct GemmCtx {
    void* st;
    float* ws;
    size_t ws_bytes;
    unsigned flags;   // RFN_GEMM_OPT_* bits of the phase (rfn_dims.gemm_flags)
    int32_t* tickets = nullptr;   // zeroed split-K tile counters of the phase's workspace (rfn_gemm_f32_tk), or NULL
    int n_tickets = 0;
};
const int GEMM_TICKETS = 16384;   // 64 KB of counters per workspace: every split launch of the path has fewer output tiles
inline rfn_gemm_problem prob1(float* C, long ldc, const rfn_gemm_seg& s) {
    rfn_gemm_problem p;
    memset(&p, 0, sizeof(p));
    p.C = C; p.ldc = ldc; p.nseg = 1; p.seg[0] = s;
    return p;
}
// weight gradient + its bias gradient (column sums of dY) in one problem
inline rfn_gemm_problem prob_dw(float* dW, long ldw, float* db, const float* dY, long lddy, const float* X, long ldx,
                         int rows) {
    rfn_gemm_problem p = prob1(dW, ldw, seg_dw(dY, lddy, X, ldx, rows));
    p.a_colsum = db;
    return p;
}
inline int gemm1(int M, int N, const rfn_gemm_seg& s, float* C, long ldc, int acc, const GemmCtx& gx) {
    rfn_gemm_problem p = prob1(C, ldc, s);
    return rfn_gemm_f32_tk(M, N, 1, &p, acc, gx.ws, gx.ws_bytes, gx.flags, gx.tickets, gx.n_tickets, gx.st);
}
inline int gemm_dw(int N, int K, float* dW, long ldw, float* db, const float* dY, long lddy, const float* X, long ldx,
            int rows, const GemmCtx& gx) {
    rfn_gemm_problem p = prob_dw(dW, ldw, db, dY, lddy, X, ldx, rows);
    return rfn_gemm_f32_tk(N, K, 1, &p, 0, gx.ws, gx.ws_bytes, gx.flags, gx.tickets, gx.n_tickets, gx.st);
}
// The vocabulary (V+1 = 9488 at the headline size) is not a multiple of the 128-wide tile: the three logit-layer GEMMs
// are issued as an aligned main part that takes the unchecked fast path plus a thin remainder (< 128 columns / rows /
// reduction elements) on the bounds-checked kernel.  Same sums, same order per output element except the dX split,
// which adds the remainder's partial product last.
inline int aligned_part(int n) { return (n / 128) * 128; }

// rfn_dims.probe_events (rfn.h): the caller's timing events around the dominant launches, recorded on the launch stream
inline int probe_mark(const rfn_dims* d, int idx, void* st) {
    if (!d->probe_events || !d->probe_events[idx]) return RFN_OK;
    return hipEventRecord((hipEvent_t)d->probe_events[idx], (hipStream_t)st) == hipSuccess ? RFN_OK : RFN_ERR_LAUNCH;
}
int gemm_logits(int rows, int V1, const float* h, int R, const float* Wl, const float* bl, float* C, const GemmCtx& gx);
int gemm_logits_dw(int V1, int R, float* dW, float* db, const float* dlg, const float* h, int rows, const GemmCtx& gx);
int gemm_logits_dx(int rows, int R, int V1, const float* dlg, const float* Wl, float* dh, const GemmCtx& gx);
// any number of K segments into one C (chunks of RFN_GEMM_MAXSEG, later chunks accumulate)
int gemm_segs(int M, int N, int nseg, const rfn_gemm_seg* segs, float* C, long ldc, int acc, const GemmCtx& gx);
// any number of same-shape problems (chunks of RFN_GEMM_MAXGROUP); _split_cols: aligned main part + thin remainder
int gemm_groups(int M, int N, int n, const rfn_gemm_problem* p, int acc, const GemmCtx& gx);
int gemm_groups_split_cols(int M, int N, int n, const rfn_gemm_problem* p, int acc, const GemmCtx& gx);
// The GEMM context of a phase on workspace W (split-K scratch at float offset `gws`).  The split-K tile counters at `tk` are
// handed out only with RFN_GEMM_OPT_SPLITK_IN_KERNEL (measured slower: off unless asked for, rfn.h); `zero_tickets`: the entry
// point zeroes them before anything else (every launch leaves them zero).
int phase_gemm(const rfn_dims* d, float* W, size_t gws, size_t tk, bool zero_tickets, void* st, GemmCtx* gx);

// ---------------------------------------------------------------------------------------------
// fused per-step products of the recurrences (csrc/rfn_cellgemm.hip): several outputs per launch, K cut across the
// waves of a block, LSTM forward / backward epilogues.  cell_lin(): Y = X W^T + b;  cell_dx(): dX = dY W.
// ---------------------------------------------------------------------------------------------
inline rfn_cell_out cell_out(float* C, long ldc, int N, int accumulate) {
    rfn_cell_out o;
    memset(&o, 0, sizeof(o));
    o.C = C; o.ldc = ldc; o.N = N; o.accumulate = accumulate; o.epilogue = RFN_CELL_EPI_STORE;
    return o;
}
inline void cell_lin(rfn_cell_out& o, const float* X, long ldx, const float* W, long ldw, int K, const float* bias) {
    if (o.nseg < RFN_CELL_MAXSEG) o.seg[o.nseg] = seg_lin(X, ldx, W, ldw, K, bias);
    ++o.nseg;     // an overflow makes rfn_cell_gemm_supported() say no
}
inline void cell_dx(rfn_cell_out& o, const float* dY, long lddy, const float* W, long ldw, int N) {
    if (o.nseg < RFN_CELL_MAXSEG) o.seg[o.nseg] = seg_dx(dY, lddy, W, ldw, N);
    ++o.nseg;
}
inline void cell_lstm(rfn_cell_out& o, const float* c_prev, long ldcp, float* c_next, long ldcn, float* h_next, long ldh,
               uint64_t drop_offset) {
    o.epilogue = RFN_CELL_EPI_LSTM;
    o.c_prev = c_prev; o.ldcp = ldcp; o.c_next = c_next; o.ldcn = ldcn; o.h_next = h_next; o.ldh = ldh;
    o.drop_offset = drop_offset;
}
inline void cell_lstm_bwd(rfn_cell_out& o, float* gates, long ldg, const float* c_prev, long ldcp, const float* c_next, long ldcn,
                   const float* dh_ext, long lddh, const float* dc_next, long lddcn, float* dc_prev, long lddcp,
                   uint64_t drop_offset) {
    o.epilogue = RFN_CELL_EPI_LSTM_BWD;
    o.gates = gates; o.ldg = ldg; o.c_prev = c_prev; o.ldcp = ldcp; o.c_next = const_cast<float*>(c_next); o.ldcn = ldcn;
    o.dh_ext = dh_ext; o.lddh = lddh; o.dc_next = dc_next; o.lddcn = lddcn; o.dc_prev = dc_prev; o.lddcp = lddcp;
    o.drop_offset = drop_offset;
}
inline bool cell_ok(int B, int n, const rfn_cell_out* outs, int R) {
    for (int i = 0; i < n; ++i)
        if (outs[i].nseg > RFN_CELL_MAXSEG) return false;
    return n <= RFN_CELL_MAXOUT && rfn_cell_gemm_supported(B, n, outs, R) != 0;
}
// variant: 0, or RFN_CELL_VARIANT_DEEP from cell_variant(d) (A/B hook: few-tile launches on the deep-ring kernel)
inline int cell_run(int B, int n, const rfn_cell_out* outs, int R, float drop_p, RfnSeed seed, void* st, int variant) {
    CgPrepared pz;
    RFN_TRY(rfn_cg_prepare(B, n, outs, R, drop_p, seed, variant, &pz));   // rfn_cell_gemm with the key as the path carries it
    return rfn_cg_launch(pz, st);
}
inline int cell_variant(const rfn_dims* d) {
    const int tiles = (d->path_flags & RFN_PATH_OPT_NO_SMALL_TILES) ? 9 : (d->path_flags & RFN_PATH_OPT_SHARED_SMALL_TILES) ? 7 : 0;
    return ((d->path_flags & RFN_PATH_OPT_DEEP_CELLS) ? RFN_CELL_VARIANT_DEEP : 0) | tiles;
}
// the same launch prepared instead of launched: one phase of a recurrence-chain step (rfn_chain.hip)
inline int cell_prepare(int B, int n, const rfn_cell_out* outs, int R, float drop_p, RfnSeed seed, CgPrepared* pz, int variant) {
    return rfn_cg_prepare(B, n, outs, R, drop_p, seed, variant, pz);
}
inline int chain_persist(const rfn_dims* d, uint32_t which) { return (d->path_flags & which) ? 1 : 0; }

// Up to MEM_BATCH copies / zero fills of f32 buffers in ONE launch (src == NULL: zero).  The path's bookkeeping moves (initial
// states into the workspace, gradient slabs zeroed before they are accumulated into) come in twos and threes; each was a
// hipMemcpyAsync / hipMemsetAsync of its own, i.e. a ~5 us launch in the dependent chain.
const int MEM_BATCH = 4;
struct MemOp { float* dst; const float* src; long n; };
int mem_batch(std::initializer_list<MemOp> ops, void* st);
inline int copy_f32(float* dst, const float* src, size_t n, void* st) {
    if (hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)st) != hipSuccess)
        return RFN_ERR_LAUNCH;
    return RFN_OK;
}
inline int zero_f32(float* dst, size_t n, void* st) {
    if (hipMemsetAsync(dst, 0, n * sizeof(float), (hipStream_t)st) != hipSuccess) return RFN_ERR_LAUNCH;
    return RFN_OK;
}

// ---------------------------------------------------------------------------------------------
// workspace layouts (offsets in floats, 256-B aligned)
// ---------------------------------------------------------------------------------------------
// LSTM gate width: [in | forget | out | g] or, with maxout, [in | forget | out | g1 | g2] (max of the last two,
// misc/LSTMSoftMultiAttentionFeatArrayNoInputCore.py:25-27,60-62; misc/LSTMSoftAttentionCore.py:25-28,89-91)
inline int gate_width(int maxout, int R) { return (maxout ? 5 : 4) * R; }

struct Bump {
    size_t off = 0;
    size_t take(size_t n) {
        const size_t o = off;
        off += (n + 63) & ~(size_t)63;
        return o;
    }
};

const size_t GEMM_WS_FLOATS = (size_t)64 << 20;  // 256 MiB of split-K partial tiles (a 4096 x 2208 weight gradient cut 8 ways)
const int FUSED_ATTN_BWD_MIN_B = 96;   // below this the (L/64, B) grid of the split dalpha kernel fills the chip better
const long FUSED_ATTN_BWD_SMALL_MAP = 32768;   // ... unless the map (L x D) is so small that launches, not bytes, are the cost
const size_t STEP_GEMM_WS_FLOATS = GEMM_WS_FLOATS;   // the free-running step makes the same split-K choices as the teacher-forced pass

struct PrefixLayout {
    size_t P1[RFN_MAX_ENC], al1[RFN_MAX_ENC], z1[RFN_MAX_ENC], P2[RFN_MAX_ENC], dz1[RFN_MAX_ENC];
    size_t dz1_st[RFN_MAX_ENC];   // float stride between the stage-I steps' d z slices: 0 (one buffer, reused by every step) unless
                                  // RFN_PATH_OPT_INPUT_GRADS keeps all T1 of them for rfn_prefix_bwd_inputs
    size_t Hs, Cs, hp1, g1, rmat, rarg, h2, c2, hp2, al2, z2, g2;
    size_t dHs, dHpart, dC, dal, dwp, dhp1, dh2e, dhrec, dc2, dz2, dhp2;
    size_t gws;
    size_t bar;     // grid-barrier counters of the persistent recurrence kernels (RFN_CHAIN_BAR_WORDS uint32, rfn_chain.hip)
    size_t tk;      // split-K tile counters (GEMM_TICKETS int32), zeroed at the head of every entry point that splits
    size_t x3;      // plane images + split-K partials of the bf16-plane GEMMs (RFN_GEMM_OPT_BF16X3), 0 floats otherwise
    size_t x3p[RFN_MAX_ENC];   // train: encoder i's dP1 as a k-slow plane image (all T1 steps), kept from the backward
                               // recurrence to its weight-gradient GEMM
    size_t total;
};
// Does encoder i's hoisted projection (and its weight gradient) take the bf16-plane GEMM?  Only when asked for
// (RFN_GEMM_OPT_BF16X3), when the per-step output groups are whole 256-wide tiles and when the product is long enough to
// pay for the two split passes; everything else stays on the exact-f32 kernels.
bool x3_takes(const rfn_dims* d, int B, int i);
inline int x3_row_pad(int rows) { return (rows + 255) / 256 * 256; }   // row pitch of a k-slow image
// Stage-I attention backward, which form runs (decided here, once, because the weight-gradient pass has to know whether the
// attention launches already wrote dP1 as bf16 planes).  The fused kernel (d alpha kept in LDS, one block per batch row and
// encoder) needs enough blocks to stream at the chip's rate: the GROUPED launch of all M encoders counts M * B of them, a
// per-encoder launch B.  Below that the split d-alpha kernel's (L/64, B) grid fills the chip better -- unless the map is so
// small that launches, not bytes, are the cost.
// ONE definition, used by the backward sweep (which launches it) and by the weight-gradient pass (which has to know whether
// encoder i's dP1 already sits in its plane image) -- ADVICE r04: the two used to restate each other's conditions.
//   GROUPED(_KS)  all M encoders of a step in one launch (they share (L, D)); _KS: dP1 written as bf16 planes
//   HET           all M encoders in one launch, maps of different (L, D), exact f32 only
//   FUSED(_KS)    one launch per encoder, d alpha kept in LDS
//   SPLIT         d alpha kernel + score-backward kernel per encoder
// A launch needs enough blocks to stream at the chip's rate: it has (encoders in the launch) x B of them.
enum AttnBwdForm { AB_GROUPED_KS, AB_GROUPED, AB_HET, AB_FUSED_KS, AB_FUSED, AB_SPLIT };
AttnBwdForm attn_bwd_form(const rfn_dims* d, int B, int i, bool dz_in_one_launch);
bool x3_dp_emitted(const rfn_dims* d, int B, int i);   // dP1 of encoder i reaches its k-slow plane image from the attention launches
PrefixLayout prefix_layout(const rfn_dims* d, int B, int train);

const int DEC_KSPLIT = 4;   // the decoder's d gates . W_hh (K = 4R) is computed as this many K-split partial products (rfn_decoder_bwd)
struct DecoderLayout {
    size_t Pd, Ud, xs, gd, hd, cd, hpd, ald, zd, logits;
    size_t dhe, dhrec, dc, dz, dal, dwp, dhpd, dPd, dPi, dUd, dxs;
    size_t gws, tk, bar;
    size_t total;
};
// n = rows per image (rfn.h "multi-sample self-critical"; must divide B): Pd, Ud, dUd and dPi hold B / n images
DecoderLayout decoder_layout(const rfn_dims* d, int B, int S, int train, int n = 1);
int stage1_cell_cus();   // CU count of the current device (cached); 256 when it cannot be read

const uint64_t OFF_STAGE2 = RFN_DROP_OFFSET_STAGE2, OFF_DECODER = RFN_DROP_OFFSET_DECODER;   // rfn.h: rfn_dropout_mask

// The decoder cell's form: z2h hoisted through the attention (rfn_deccell.hip: two dependent launches per step each way)
// unless the caller asks for the three-launch form of rounds 3-5 (A/B hook; the persistent decoder chains are built from it).
inline bool dec_hoisted(const rfn_dims* d) {
    return !(d->path_flags & (RFN_PATH_OPT_DEC_UNHOISTED | RFN_PATH_OPT_PERSIST_DEC_FWD | RFN_PATH_OPT_PERSIST_DEC_BWD));
}
// rfn_decoder_prepare's buffer: [Pd = att_2_att_h(comb) (T2 * Bc, A) | U = comb . W_z^T (T2 * Bc, GD)], U 256-B aligned
inline size_t cproj_u_off(const rfn_dims* d, int Bc) { return ((size_t)d->T2 * Bc * d->A + 63) & ~(size_t)63; }

// One decoder cell call on given buffers (rfn_path_decoder.hip), shared by the teacher-forced, step-wise and free-running passes
int decoder_cell_core(const rfn_dims* d, int B, const float* const* prm, const float* comb, const float* cproj,
                      const float* U, int row_div, const float* h, const float* c, float* h_next, float* c_next,
                      float* hp, float* al, float* z, float* g, const GemmCtx& gx, RfnSeed seed, int step, void* st);

// rfn_decoder_fwd_begin / rfn_decoder_fwd_step with n rows per image (rfn_decoder_fwd_sampled_ex queues them)
int decoder_fwd_begin_n(const rfn_dims* d, int B, int S, int n, const float* const* prm, const float* comb, const float* h0,
                        const float* c0, void* ws, size_t ws_bytes, int train, void* st);
int decoder_fwd_step_n(const rfn_dims* d, int B, int S, int n, int s, const float* const* prm, const float* comb,
                       const int64_t* ids_s, int64_t ld_ids, float* log_prob, void* ws, size_t ws_bytes, int train,
                       uint64_t seed_arg, void* st);

}  // namespace rfn_path
using namespace rfn_path;
