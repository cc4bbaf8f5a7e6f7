/*
 * rfn.h -- C ABI of librfn_hip.so: the MI355X (gfx950) implementation of the recurrent-fusion
 * caption-decoder hot path of cswhjiang/Recurrent_Fusion_Network.
 *
 * The reference has no FFI for this path: its seam is the Python duck type returned by
 * models.setup(opt) (reference models.py:14-38) whose forward()/sample() call nothing but ATen.
 * Each entry point below names the reference code it replaces (paths relative to the reference
 * checkout).  INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain C types only; every pointer is a DEVICE pointer unless its name ends in _host;
 *   - all floating-point data is IEEE fp32, row-major; token / target ids are int64;
 *   - the caller owns every buffer, including workspaces (sizes from the *_ws_bytes queries);
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it, never allocate,
 *     never synchronise, and are re-entrant.  The library reads no environment variable and keeps
 *     no mutable state except write-once, per-device launch attributes of its kernels (dynamic-LDS
 *     opt-in, blocks per CU), so one process may drive several devices; every tuning choice
 *     travels with the call (rfn_dims.gemm_flags, rfn_gemm_f32_opt);
 *   - return RFN_OK (0) or a negative RFN_ERR_* code; nothing is launched on a shape error.
 */
#ifndef RFN_H_
#define RFN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFN_OK 0
#define RFN_ERR_SHAPE (-1)       /* unsupported or inconsistent dimensions */
#define RFN_ERR_UNSUPPORTED (-2) /* configuration the path does not implement (e.g. maxout) */
#define RFN_ERR_LAUNCH (-3)      /* HIP launch failure */
#define RFN_ERR_WORKSPACE (-4)   /* workspace too small */
#define RFN_ERR_ARG (-5)         /* null / misaligned pointer */

#define RFN_MAX_ENC 8
#define RFN_ABI_VERSION 9

/* Model dimensions: the fields RecurrentFusionModel.__init__ reads from `opt`
 * (misc/RecurrentFusionModel.py:118-151).  Limits (RFN_ERR_SHAPE otherwise): M <= RFN_MAX_ENC,
 * T1*M <= 64 and T2*M <= 64 (the reference ships T1 = T2 = 8, M <= 5), dropout probabilities in [0, 1). */
typedef struct rfn_dims {
    int32_t M;                 /* number of encoders, len(opt.feat_array_info)            */
    int32_t R;                 /* opt.rnn_size                                            */
    int32_t A;                 /* opt.att_hid_size                                        */
    int32_t E;                 /* opt.input_encoding_size                                 */
    int32_t T1;                /* opt.num_review_steps_0 (fusion stage I steps)           */
    int32_t T2;                /* opt.num_review_steps   (fusion stage II steps)          */
    int32_t K;                 /* opt.top_words_count                                     */
    int32_t V1;                /* opt.vocab_size + 1                                      */
    int32_t L[RFN_MAX_ENC];    /* feat_array_info[i]['att_num']                           */
    int32_t D[RFN_MAX_ENC];    /* feat_array_info[i]['att_feat_size']                     */
    int32_t F[RFN_MAX_ENC];    /* feat_array_info[i]['fc_feat_size']                      */
    int32_t review_maxout;     /* opt.review_maxout (stage II gates are 5R wide)          */
    int32_t decoder_maxout;    /* opt.maxout        (decoder gates are 5R wide)           */
    float drop_fusion;         /* opt.drop_prob_fusion (stage I)                          */
    float drop_reason;         /* opt.drop_prob_reason (stage II)                         */
    float drop_lm;             /* opt.drop_prob_lm     (decoder)                          */
    uint32_t gemm_flags;       /* RFN_GEMM_OPT_* bits applied to every GEMM of the path (0 = defaults)  */
    uint32_t path_flags;       /* RFN_PATH_OPT_* bits (0 = defaults)                                    */
    /* Measurement hook (NULL = off; bench.py's in-step roofline): an array of 4*M hipEvent_t created by the caller
     * with timing enabled.  rfn_prefix_fwd records events [2i] / [2i+1] on the launch stream right before / after
     * encoder i's hoisted att_2_att_h projection launch (the path's dominant kernel), rfn_prefix_bwd_wgrad records
     * [2M+2i] / [2M+2i+1] around encoder i's att_2_att_h weight-gradient launch.  Recording is asynchronous; the
     * caller reads the pairs after its own synchronisation.  Nothing else in the library looks at it. */
    void* const* probe_events;
} rfn_dims;
/* rfn_dims.path_flags: run the named recurrence -- all of its steps -- inside ONE persistent launch (csrc/rfn_chain.hip: the
 * per-step launches' device bodies, a grid barrier between dependent phases; bit-identical results) instead of three launches
 * per step.  Opt-in: measured on MI355X the in-launch hand-off costs what the launch boundary costs (profiles/r05_chain.md).
 * A/B hooks only: the persistent grid is launched non-cooperatively and relies on all of its blocks (<= CU count, 128 KB of LDS each)
 * being resident at once -- do not set them beside other streams, processes or collectives on the same device (a block that cannot
 * become resident makes its peers spin into a trap).  The decoder bits imply RFN_PATH_OPT_DEC_UNHOISTED (the chains are built
 * from the three-launch decoder cell). */
#define RFN_PATH_OPT_PERSIST_DEC_FWD 1u   /* teacher-forced decoder steps (rfn_decoder_fwd)                   */
#define RFN_PATH_OPT_PERSIST_S2_FWD 2u    /* stage-II steps (rfn_prefix_fwd)                                  */
#define RFN_PATH_OPT_PERSIST_DEC_BWD 4u   /* decoder backward sweep, steps S-1 ... 1 (rfn_decoder_bwd)        */
#define RFN_PATH_OPT_PERSIST_S2_BWD 8u    /* stage-II backward sweep, steps T2-1 ... 1 (rfn_prefix_bwd)       */
#define RFN_PATH_OPT_PERSIST_ALL 15u
#define RFN_PATH_OPT_NO_SMALL_TILES 32u   /* A/B hook: per-step products keep 32-row tiles even when the launch has so few of them
                                           * that the library would take 16-row tiles (rfn_cell_gemm variant 6; same results)  */
#define RFN_PATH_OPT_SHARED_SMALL_TILES 64u /* A/B hook: those 16-row tiles on ring slots shared by the block (rfn_cell_gemm variants
                                           * 4 / 5) instead of wave-private ones (variant 6, the default); same results        */
#define RFN_PATH_OPT_DEC_UNHOISTED 128u   /* A/B hook: the decoder cell of rounds 3-5 (z2h(z) as a per-step product: three
                                           * dependent launches per step each way) instead of the hoisted form (two).  Same
                                           * mathematics, different rounding.  Implied by the PERSIST_DEC_* bits; the beam loop,
                                           * whose rows share their image's thought vectors, has no unhoisted form          */
#define RFN_PATH_OPT_DEEP_CELLS 16u       /* A/B hook: per-step products with no more tiles than CUs on the deep-ring kernel
                                           * (rfn_cell_gemm, RFN_CELL_VARIANT_DEEP) instead of the 3-slot one; not faster      */
/* ABI 9.  The `uint64_t seed` argument of every entry point that takes a `const rfn_dims*` (rfn_prefix_fwd / _bwd,
 * rfn_decoder_fwd / _fwd_step / _fwd_sampled / _bwd, rfn_decoder_step / _step_embedded, rfn_decoder_loop, rfn_beam_loop) is not
 * the dropout key but the DEVICE ADDRESS of one uint64_t holding it (8-byte aligned; 0 -> RFN_ERR_ARG).  The kernels read the key
 * when they run, so a captured graph replays with whatever the host stored there before the replay.  Only the key moves: the
 * call-site offsets (rfn_dropout_mask) are as without the bit, and the same value gives the same bits either way.  The library
 * never writes to that location; the caller keeps its value unchanged from the forward launches of a step until the backward
 * (and recompute) launches of that step have run.  rfn_dropout_mask_dev publishes the masks of such a call. */
#define RFN_PATH_OPT_SEED_DEV 256u
/* Keep what the gradients of fc_feats / att_feats need (rfn_prefix_bwd_inputs, below): the training workspace holds T1 slices
 * (B, D_i) of d z per encoder instead of one buffer reused by every step, and step t of the stage-I backward sweep writes its
 * d z = d gates . W_z[t, i] into slice t.  Nothing else changes: forward outputs, every parameter gradient and dP1 are
 * bit-identical to the run without the bit; without it the workspace size and every launch are what they were. */
#define RFN_PATH_OPT_INPUT_GRADS 512u

int rfn_abi_version(void);
const char* rfn_error_string(int code);

/* ---- parameter table ------------------------------------------------------------------------
 * Parameters and their gradients are passed as arrays of device pointers in ONE canonical order.
 * rfn_param_name() returns the reference state_dict key of slot `idx` (e.g.
 * "review_steps_individual.3.lstm.1.att_model.att_2_att_h.weight"), so a host binds the table by
 * name and never hard-codes the order.  nn.Linear layout (out, in). */
int rfn_param_count(const rfn_dims* d);
int rfn_param_name(const rfn_dims* d, int idx, char* buf, size_t buflen);
/* rows/cols of slot idx (cols = 1 for a bias) */
int rfn_param_shape(const rfn_dims* d, int idx, int64_t* rows, int64_t* cols);

/* ---- primitive operators (exported for unit parity tests and for other hosts) ---------------- */

/* C[M,N] (+)= sum_s op(A_s)[M,K_s] * op(B_s)[N,K_s]^T + sum_s bias_s[N]; exact-fp32 MFMA
 * (v_mfma_f32_32x32x2_f32: each output is a k-ordered fp32 fma chain).  Replaces every nn.Linear
 * / mm / addmm / bmm on the path and their backward
 * matmuls.  *_kfast = 1: the reduction index is the contiguous one (A is [M,K] with row stride
 * lda; B is [N,K] = an nn.Linear weight).  *_kfast = 0: the output index is contiguous (A is
 * [K,M] with row stride lda; B is [K,N]).  Up to RFN_GEMM_MAXSEG K-segments accumulate into one C
 * (gate sums such as H2h(H) + z2h(z), misc/RecurrentFusionModel.py:53); up to RFN_GEMM_MAXGROUP
 * same-shape problems run in one launch (the per-step weights of one encoder).
 *
 * Operands.  Any base pointer and any lda / ldb / ldc >= the row length are accepted.  The 16-byte (float4) staging is
 * taken when EVERY segment of EVERY group has A and B 16-byte aligned, lda % 4 == 0 and ldb % 4 == 0, and whole float4s
 * along the contiguous index: K_s % 4 == 0 for a *_kfast = 1 operand, M % 4 == 0 (A) / N % 4 == 0 (B) for a *_kfast = 0
 * one; otherwise the whole call stages scalars (slower, same results).  C, bias and a_colsum are accessed as scalars by
 * the tile kernels and need no alignment; the separate split-K reduce reads and writes them 16 bytes wide only when
 * N % 4 == 0, every C is 16-byte aligned with ldc % 4 == 0 and every bias is 16-byte aligned.  a_kfast / b_kfast must be
 * the same in every segment and group (RFN_ERR_SHAPE).
 * K rule.  K_s >= 1 (K_s < 0: RFN_ERR_ARG).  K_s = 0 is accepted only when EVERY segment of the problem is empty -- the
 * call then means C (+)= sum_s bias_s -- and refused with RFN_ERR_SHAPE next to a non-empty segment (the tile kernels
 * count an empty segment as no K step but would spend one on it).  Leave an empty segment out instead.
 * M <= 0 or N <= 0: RFN_OK, nothing is written.  A refused call launches nothing and writes nothing.
 *
 * Bit-identical results (the same k-ordered chain per output element, asserted by tests/test_gemm_edges_gpu.py):
 *   - float4 and scalar staging of the same values; any leading dimensions; any tile shape the launcher picks (128 x 128,
 *     64 x 64, the half-height and quarter tiles of a last round); LDS-DMA and register staging: an UNSPLIT product does
 *     not depend on RFN_GEMM_OPT_LDS_LEAN / RFN_GEMM_OPT_NO_DMA at all;
 *   - repeated calls, with or without a K split (the split is a function of the arguments, the partial tiles are added in
 *     K-range order);
 *   - under a K split: RFN_GEMM_OPT_LDS_LEAN == default, always (its 16-deep kernel cuts the K ranges of the layout's
 *     default kernel); the in-kernel ticket finish == the separate reduce; rfn_gemm_f32_lstm == rfn_gemm_f32_ws +
 *     rfn_lstm_fwd_grouped; RFN_GEMM_OPT_NO_DMA == default wherever both cut the same K ranges: always on the 64 x 64
 *     tile and for a_kfast = b_kfast = 1, and for the other layouts of a split big-tile product (default K step 16,
 *     register kernel 32) unless 0 < (K / 32) mod s <= s / 2 -- there the two differ by fp32 re-association only.
 *   A split product differs from the unsplit one by fp32 re-association. */
#define RFN_GEMM_MAXSEG 8
#define RFN_GEMM_MAXGROUP 8
typedef struct rfn_gemm_seg {
    const float* A;
    const float* B;
    const float* bias; /* may be NULL */
    int64_t lda, ldb;
    int32_t K;
    int32_t a_kfast, b_kfast;
    int32_t pad_;
} rfn_gemm_seg;
typedef struct rfn_gemm_problem {
    float* C;
    int64_t ldc;
    int32_t nseg;
    int32_t pad_;
    /* optional, only with a_kfast = 0: a_colsum[m] (=|+=) sum_s sum_k A_s[k, m].  For dW = dY^T X this is
     * the bias gradient colsum(dY), produced by the GEMM that already streams dY (no extra pass). */
    float* a_colsum;
    rfn_gemm_seg seg[RFN_GEMM_MAXSEG];
} rfn_gemm_problem;
int rfn_gemm_f32(int M, int N, int ngroups, const rfn_gemm_problem* problems_host, int accumulate,
                 void* stream);
/* Same, with a scratch buffer (>= 1 MiB, 16-B aligned).  Skinny problems (M = batch rows, few output tiles)
 * are then cut along K across thread blocks; the partial tiles are summed in a fixed order by a second
 * kernel, so the result is deterministic (it differs from the unsplit result only by fp32 re-association).
 * A buffer below 1 MiB or not 16-byte aligned is ignored (the unsplit product, bit for bit; the buffer is not touched).
 * Only whole MiB count: a split into s ranges needs (M * N + M) * ngroups * s floats <= (ws_bytes >> 20) MiB and is
 * capped accordingly; the launch writes the first (M * N [+ M with an a_colsum]) * ngroups * s floats and nothing behind
 * them.  The buffer must not be shared by launches that can overlap. */
int rfn_gemm_f32_ws(int M, int N, int ngroups, const rfn_gemm_problem* problems_host, int accumulate,
                    void* ws, size_t ws_bytes, void* stream);
/* Same, with option bits (every tuning choice travels with the call: the library reads no environment variable and
 * keeps no mutable process state beyond write-once, per-device launch attributes of its kernels).
 *   RFN_GEMM_OPT_LDS_LEAN  the long big-tile GEMMs take 32 KB of LDS per block (64 KB per CU for a one-round
 *                          weight-gradient launch) instead of 64 KB per block, so that kernels of other streams --
 *                          RCCL's under data parallelism -- can co-reside instead of waiting for a
 *                          multi-millisecond GEMM to drain; bit-identical results, split along K or not; same speed
 *                          within 1 %;
 *   RFN_GEMM_OPT_NO_DMA    interior tiles use the register-staged kernel instead of the LDS-DMA one (A/B hook; same k
 *                          order per output element: bit-identical when unsplit and wherever both kernels cut the same K
 *                          ranges -- see the list above -- otherwise equal up to fp32 re-association);
 *   RFN_GEMM_OPT_BF16X3    (rfn_dims.gemm_flags only) the two long products of the path -- the hoisted stage-I feature
 *                          projection and its weight gradient -- run on the bf16 matrix cores with every f32 operand
 *                          held as three bf16 planes and six plane products accumulated in f32 (rfn_x3_*, below):
 *                          f32-level accuracy (at least as close to an f64 product as the f32 MFMA chain), not
 *                          bit-identical to it.  Off by default.  Products too short to pay for the split passes
 *                          (< 2e10 multiply-adds x 2) stay on the exact kernels unless
 *   RFN_GEMM_OPT_BF16X3_ANY_SIZE is also set (parity tests run the small reference-generated tiers through the plane
 *                          GEMM with it). */
#define RFN_GEMM_OPT_LDS_LEAN 1u
#define RFN_GEMM_OPT_NO_DMA 2u
#define RFN_GEMM_OPT_BF16X3 4u
#define RFN_GEMM_OPT_BF16X3_ANY_SIZE 8u
/* (rfn_dims.gemm_flags only) A/B hook: the split-K GEMMs of the path finish inside their launch (rfn_gemm_f32_tk, below)
 * instead of through rfn_gemm_reduce_k.  Bit-identical results; MEASURED SLOWER on MI355X (C3 step 65.6 -> 68.9 ms, C2
 * 5.4 -> 6.6 ms: every K-range block pays an agent-scope release = a write-back of its XCD's L2 before its ticket), which
 * is what the MI355X guide reports for split-K seams kept inside a launch.  Off by default. */
#define RFN_GEMM_OPT_SPLITK_IN_KERNEL 16u
/* Diagnostics (tools/split_probe.py): bits 8-12 force the K split of a medium big-tile product (1 = unsplit). */
#define RFN_GEMM_OPT_FORCE_SPLIT(n) (((unsigned)(n) & 31u) << 8)
int rfn_gemm_f32_opt(int M, int N, int ngroups, const rfn_gemm_problem* problems_host, int accumulate,
                     void* ws, size_t ws_bytes, unsigned flags, void* stream);
/* Same, with split-K finished INSIDE the launch: `tickets` points to n_tickets int32 counters that are ZERO on entry
 * (the library leaves them zero: a caller zeroes them once per workspace and keeps them for its GEMMs).  The K ranges of
 * an output tile draw tickets on the tile's counter; the last one to arrive adds the partial tiles in K-range order
 * (the order the separate reduce kernel uses: bit-identical results) -- no second launch.  Launches with more output
 * tiles than counters (ngroups * ceil(M / tile) * ceil(N / tile), tile = 128 or 64 as the launcher picks: 64 x 64 tiles
 * are the safe count) use the separate reduce kernel and leave every counter alone, as do unsplit launches and
 * rfn_gemm_f32_lstm.  Counters need 4-byte alignment only; a counter that is not zero on entry gives a wrong or unfinished
 * tile.  Launches that can overlap must not share counters. */
int rfn_gemm_f32_tk(int M, int N, int ngroups, const rfn_gemm_problem* problems_host, int accumulate, void* ws,
                    size_t ws_bytes, unsigned flags, int32_t* tickets, int n_tickets, void* stream);
/* Gate GEMM + LSTM update in one call (stage I: misc/RecurrentFusionModel.py:53-73): gates_g[M, 4R] = sum_s A_s W_s^T + b
 * for ngroups cells (problems_host[g].C = cell g's gate buffer, equally spaced), then rfn_lstm_fwd_grouped on them.  When
 * the product is cut along K the update rides on the fixed-order reduce (one launch less); results are those of
 * rfn_gemm_f32_ws followed by rfn_lstm_fwd_grouped either way. */
typedef struct rfn_gemm_lstm {
    const float* c_prev;   /* cell g at c_prev + g * gs_cprev, (M, R) with row stride ldcp; likewise c_next, h_next */
    float* c_next;
    float* h_next;
    int64_t ldcp, ldcn, ldh, gs_cprev, gs_cnext, gs_h;
    float drop_p;
    int32_t pad_;
    uint64_t seed, offset; /* dropout stream of cell g: (seed, offset + g) */
} rfn_gemm_lstm;
int rfn_gemm_f32_lstm(int M, int R, int ngroups, const rfn_gemm_problem* problems_host, void* ws, size_t ws_bytes,
                      unsigned flags, const rfn_gemm_lstm* lstm, void* stream);

/* ---- f32 GEMM on the bf16 matrix cores (csrc/rfn_gemm_x3.hip) -------------------------------------------------------
 * Replaces, when RFN_GEMM_OPT_BF16X3 is set, the two nn.Linear products the reference spends most of its time in:
 * att_2_att_h over all B*L regions (misc/AttentionModelCore.py:33-35, hoisted over the T1 review steps) and its
 * weight gradient (autograd of the same line).
 *
 * A logical operand Y[rows][K] (row = output index, K = reduction index) is held as a PLANE IMAGE: x = x0 + x1 + x2 with
 * x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1) (round to nearest even; exact for finite x below 2^127), stored
 * as 1-KiB pieces in the operand order of v_mfma_f32_16x16x32_bf16: piece (kc, rb, p) at byte
 * ((kc * nrb + rb) * 3 + p) * 1024 holds, at 16 * l, plane p of Y[rb * 16 + l % 16][kc * 32 + 8 * (l / 16) + 0..7];
 * nrb = rows padded to 256, over 16; K is padded to 32; pad rows / columns are zero.  rfn_x3_image_bytes gives the size
 * (6 bytes per padded element). */
size_t rfn_x3_image_bytes(int rows, int K);
/* Image of Y[ngroups * rows][K] whose row block g is the f32 matrix srcs_host[g] (device pointers in a host array;
 * k_fast = 1: element (row, k) at src[row * ld + k], k_fast = 0: at src[k * ld + row]).  rows % 32 == 0 unless
 * ngroups == 1 (RFN_ERR_SHAPE); 1 <= ngroups <= 64, rows, K >= 1, no NULL (RFN_ERR_ARG).  Any ld and any 4-byte aligned
 * source: 16-byte loads are used where a k_fast source allows them (ld % 4 == 0, 16-byte aligned base), and every storage of
 * the same values gives the same image bytes. */
int rfn_x3_split(const float* const* srcs_host, int ngroups, int64_t ld, int rows, int K, int k_fast, void* image,
                 void* stream);
/* C (+)= A . B^T from two images (A: M rows, B: N rows, both with reduction length K): the six plane products
 * a0.b0, a0.b1, a1.b0, a0.b2, a1.b1, a2.b0, smallest first, accumulated in f32 by v_mfma_f32_16x16x32_bf16.
 * The output is cut into groups of gm rows x gn columns, group (i, j) written to C_host[i * ceil(N/gn) + j] with leading
 * dimension ldc (+ bias_host[..][column inside the group] when bias_host and the entry are non-NULL); gm and gn must be
 * multiples of 256 unless they cover the whole dimension; at most 64 groups.  splitk > 1 cuts K over blocks; the partial
 * tiles (part: rfn_x3_part_floats floats) are summed in slice order by a second kernel (deterministic; N % 4 == 0).
 *
 * Stores.  A wave tile (64 x 128 outputs; 128 x 64 for rfn_x3_gemm_ks) that lies wholly inside M x N is stored 16 bytes per
 * lane when accumulate == 0, the address of its first element is a multiple of 16 and ldc % 4 == 0 -- for every wave tile
 * of a launch: every C_host[g] 16-byte aligned and ldc % 4 == 0 (N % 4 == 0 follows for packed groups).  Any other wave
 * tile (ragged, accumulate, an odd ldc, a base one float off) is stored one float at a time.  Both ways store the same
 * bits, acc + bias (+ previous C, in that order), and neither touches the columns between gn and ldc.
 *
 * Split.  With nkc = ceil(K / 32) pieces and per = ceil(nkc / splitk), slice s holds the pieces [s * per, min((s + 1) * per,
 * nkc)); 1 <= splitk <= nkc (RFN_ERR_SHAPE beyond), so trailing slices may be EMPTY (nkc = 10, splitk = 7: per = 2, slices 5
 * and 6) and then contribute zeros.  Slice s writes all of part[s][M][N]; the result is ((p_0 + p_1) + ... + p_(splitk-1)) + bias
 * + previous C in f32, p_s bit-identical to the unsplit product over the slice's k range.  part is read with 16-byte loads:
 * N % 4 == 0 and gn % 4 == 0 (RFN_ERR_ARG otherwise, as for part == NULL), and the caller keeps part 16-byte aligned (not
 * checked).
 *
 * Limits.  Offsets inside a block tile are 32-bit: 256 * ldc * 4 < 2^32 (ldc < 2^22; with splitk > 1: 256 * N * 4), and for
 * rfn_x3_gemm_ks 96 * Mp * 2 < 2^32 per image; RFN_ERR_SHAPE otherwise.  M, N, K >= 1 and non-NULL images and C_host, else
 * RFN_ERR_ARG.  A refused call launches nothing and writes nothing. */
int rfn_x3_gemm(int M, int N, int K, const void* imageA, const void* imageB, int gm, int gn, float* const* C_host,
                const float* const* bias_host, int64_t ldc, int accumulate, int splitk, float* part, void* stream);
/* K-SLOW images: a logical operand stored reduction-index-major in memory, Y[K][cols] (the weight gradient's two operands:
 * dproj[(b,l)][a] and att[(b,l)][d]), keeps that orientation: element (k, plane, m) at ((k * 3 + plane) * Mp + m) * 2
 * bytes, Mp = ngroups * cols padded to 256, k padded to 32 with zero rows; rfn_x3_image_bytes(ngroups * cols, K) bytes.
 * Column block g comes from srcs_host[g][k * ld + c] (cols % 4 == 0, ld % 4 == 0, 16-B aligned).  No transposing pass:
 * rfn_x3_gemm_ks forms the MFMA operands with the transposing LDS read (ds_read_b64_tr_b16). */
int rfn_x3_split_ks(const float* const* srcs_host, int ngroups, int64_t ld, int K, int cols, void* image, void* stream);
/* rfn_x3_gemm with BOTH operands given as k-slow images (A: M columns, B: N columns, K rows each). */
int rfn_x3_gemm_ks(int M, int N, int K, const void* imageA, const void* imageB, int gm, int gn, float* const* C_host,
                   const float* const* bias_host, int64_t ldc, int accumulate, int splitk, float* part, void* stream);
size_t rfn_x3_part_floats(int M, int N, int splitk);
/* the number of K slices with which one round of blocks covers the chip (1 for launches of many tiles) */
int rfn_x3_splitk_for(int M, int N, int K);

/* out[n] (+)= sum_r X[r*ldx + n]   (bias gradients) */
int rfn_colsum_f32(const float* X, int64_t ldx, int rows, int cols, float* out, int accumulate,
                   void* stream);
/* the same for `ngroups` matrices X + g*group_stride, each into its own outs_host[g] (one launch) */
int rfn_colsum_grouped_f32(const float* X, int64_t group_stride, int64_t ldx, int rows, int cols,
                           float* const* outs_host, int ngroups, void* stream);
/* the same, every sum also written to outs2_host[g] where that is not NULL (two parameters that enter one pre-activation
 * share one bias gradient: H2h.bias / z2h.bias, LSTMFusionNoInputCore.py:42; att_2_att_h.bias / h_2_att_h.bias,
 * AttentionModelCore.py:36-38) */
int rfn_colsum_grouped2_f32(const float* X, int64_t group_stride, int64_t ldx, int rows, int cols,
                            float* const* outs_host, float* const* outs2_host, int ngroups, void* stream);

/* outs_host[g][0..n) = value for `ngroups` small device buffers in one launch */
int rfn_fill_small_f32(float* const* outs_host, int ngroups, int n, float value, void* stream);
/* dst_host[g][0..n) = src_host[g][0..n) for `ngroups` small device buffer pairs in one launch */
int rfn_copy_small_f32(float* const* dst_host, const float* const* src_host, int ngroups, int n, void* stream);

/* Additive soft attention, AttentionModelCore.forward (misc/AttentionModelCore.py:31-48; inlined
 * copy misc/LSTMSoftAttentionCore.py:64-79), split at the GEMM boundary:
 *   proj[b,l,:] = att_2_att_h(att_seq[b,l,:])  (hoisted GEMM, :32-34)
 *   hproj[b,:]  = h_2_att_h(pre_h[b,:])        (GEMM, :36)
 * scores:  alpha[b,:] = softmax_l( w . tanh(proj[b,l,:] + hproj[b,:]) + b_o )      (:39-44)
 * context: z[b,:]     = sum_l alpha[b,l] * att_seq[b,l,:]                          (:45-47)
 * Element (b,l,x) of proj / att_seq lives at base + b*stride_b + l*stride_l + x.
 *
 * Alignment and strides (every rfn_attn_* entry): any float-aligned pointer and any stride is accepted.  The fast case is
 * the aligned one: 16-byte loads / stores are used for proj and dproj when A % 4 == 0, both pointers are 16-byte aligned and
 * all their strides are multiples of 4 floats; for att_seq and z when D % 4 == 0, the pointers are 16-byte aligned and
 * sb, sl, ldz are multiples of 4 (the fused backward decides for att_seq independently of proj / dproj).  Otherwise the
 * same entry runs its scalar instantiation: same results to rounding (another summation order within a row), not the same
 * bits.  hproj, w_out, b_out, alpha, dalpha, dz (any lddz) and the raw-score scratch are only ever accessed as scalars and
 * never matter.  In a grouped or heterogeneous launch the decision is all-or-nothing: one encoder off these conditions
 * puts every encoder of the launch on the scalar kernels.  rfn_attn_small_bwd takes its 16-byte form only when ALL of
 * A % 4 == 0, D % 4 == 0, every stride (lddz included) a multiple of 4 and proj, att_seq, dproj, dhproj, dw_part, datt_seq
 * 16-byte aligned hold; rfn_attn_small_fwd decides per encoder from A and proj alone.
 *
 * Limits (RFN_ERR_SHAPE, nothing launched, no output touched -- the raw-score scratch included); Xp = X rounded up to 4:
 *   every extent (B, L, A, D) >= 1; 1 <= ngroups <= RFN_MAX_ENC;
 *   rfn_attn_scores_fwd, rfn_attn_fwd[_grouped|_het]:      2 * Ap floats <= 64 KiB                      (A <= 8192)
 *   rfn_attn_context_fwd, rfn_attn_fwd[_grouped|_het]:     L floats <= 64 KiB                           (L <= 16384)
 *   rfn_attn_context_bwd_dalpha:                           Dp floats <= 64 KiB                          (D <= 16384)
 *   rfn_attn_scores_bwd:                                   34 * Ap + 16 + L floats <= 150 KiB
 *   rfn_attn_bwd[_grouped|_grouped_ks|_het]:               34 * Ap + 16 + 2 * Lp + Dp floats <= 150 KiB (largest L, D of the launch)
 *   rfn_attn_small_fwd:                                    L <= 1024 and 2 * Ap + L floats <= 64 KiB
 *   rfn_attn_small_bwd:                                    L <= 1024 and 2 * Ap + Dp + 2 * Lp floats <= 64 KiB
 *   rfn_attn_context_bwd_dseq:                             none beyond the extents.
 *   rfn_attn_context_bwd_dseq_steps:                       T >= 1; T * min(Dp, 1024) + 32 * Tp floats <= 64 KiB (T <= 15 at D >= 1021)
 * A NULL required pointer (or host array, or array entry) is RFN_ERR_ARG; b_out, its array, and datt_seq of
 * rfn_attn_small_bwd may be NULL.
 *
 * Aliasing: dproj may be proj itself (same pointer and strides: in place) in every
 * backward entry; scores_scratch must not be alpha (RFN_ERR_ARG).  No other output may overlap an input or another
 * output; inputs may overlap each other freely.  (tests/test_attention_edges_gpu.py pins all of the above.)
 *
 * Ragged maps (rfn_attn_fwd_ragged / rfn_attn_bwd_ragged; tests/test_ragged_attention_gpu.py): `len` is a HOST array of
 * ngroups DEVICE pointers, len[g] a (B,) int32 vector or NULL; the array itself may be NULL.  Image b of encoder g has
 * n = clamp(len[g][b], 1, L_g) valid rows (NULL: n = L_g); the clamp happens on the device, nothing is read back.  Same
 * limits (LDS is sized by L_g, not by n), alignment rules, aliasing rules and error contract as above; `len` is never a
 * required pointer.  Forward: raw scores, softmax and context run over l < n in the order of the full-length kernels,
 * alpha[b, l] = 0 exactly for l >= n, and rows l >= n of proj and att_seq are never loaded (the raw-score scratch past n is
 * not written).  Backward: dalpha, the softmax / tanh backward, dhproj and dw_part cover l < n; dproj[b, l, :] is written as
 * exact zeros for l >= n when accumulate_dproj == 0 (so a consumer may read all B * L rows) and left alone otherwise.  The
 * row count is uniform within a block: a shorter trip count, no mask multiply.  With every n == L_g the results are the
 * _het calls', bit for bit; those calls forward here with len = NULL. */
int rfn_attn_scores_fwd(const float* proj, int64_t proj_sb, int64_t proj_sl, const float* hproj,
                        const float* w_out, const float* b_out, int B, int L, int A, float* alpha,
                        void* stream);
int rfn_attn_context_fwd(const float* att_seq, int64_t sb, int64_t sl, const float* alpha, int B,
                         int L, int D, float* z, int64_t ldz, void* stream);
/* rfn_attn_scores_fwd + rfn_attn_context_fwd in two launches instead of three: the context kernel normalises the
 * raw scores itself.  scores_scratch: B*L floats, must not alias alpha.  Results are bit-identical to the pair. */
int rfn_attn_fwd(const float* proj, int64_t proj_sb, int64_t proj_sl, const float* hproj, const float* w_out,
                 const float* b_out, const float* att_seq, int64_t sb, int64_t sl, int B, int L, int A, int D,
                 float* scores_scratch, float* alpha, float* z, int64_t ldz, void* stream);
/* The same for `ngroups` encoders that share (L, A, D) and every stride, two launches in total; arrays are host
 * arrays of device pointers, one entry per encoder. */
int rfn_attn_fwd_grouped(int ngroups, const float* const* proj, int64_t proj_sb, int64_t proj_sl,
                         const float* const* hproj, const float* const* w_out, const float* const* b_out,
                         const float* const* att_seq, int64_t sb, int64_t sl, int B, int L, int A, int D,
                         float* const* scores_scratch, float* const* alpha, float* const* z, int64_t ldz,
                         void* stream);
/* dalpha[b,l] = <dz[b,:], att_seq[b,l,:]> */
int rfn_attn_context_bwd_dalpha(const float* att_seq, int64_t sb, int64_t sl, const float* dz,
                                int64_t lddz, int B, int L, int D, float* dalpha, void* stream);
/* datt_seq[b,l,:] += alpha[b,l] * dz[b,:]   (only for differentiable att_seq: stages II, decoder) */
int rfn_attn_context_bwd_dseq(const float* alpha, const float* dz, int64_t lddz, int B, int L,
                              int D, float* datt_seq, int64_t sb, int64_t sl, void* stream);
/* The same over T steps in ONE pass over the map (stage I: the context's share of d att_feats, rfn_prefix_bwd_inputs):
 *   datt_seq[b,l,d] (=|+=) sum_{t < T} alpha[t * alpha_st + b * L + l] * dz[t * dz_st + b * lddz + d]
 * Every map element is written once, and read once only when accumulate != 0; T calls of rfn_attn_context_bwd_dseq read
 * and write the whole map T times.  Arithmetic: one fmaf chain per element, t ascending, starting from the previous value
 * (accumulate != 0) or from 0: deterministic, and -- unlike the entries above -- the 16-byte and the scalar instantiation
 * give the SAME bits.  datt_seq is accessed 16 bytes wide under the rule above (D % 4 == 0, sb and sl multiples of 4, a
 * 16-byte aligned pointer); dz is read 16 bytes wide when lddz % 4 == 0, dz_st % 4 == 0 and it is 16-byte aligned, otherwise
 * as scalars; alpha is only ever read as scalars.  The T dz rows of a block's D tile (at most 1024 columns) and the alpha of
 * its rows (at most 32, T rounded up to Tp, a multiple of 4) are staged in LDS: T * min(Dp, 1024) + 32 * Tp floats <= 64 KiB,
 * RFN_ERR_SHAPE beyond (nothing launched; a caller with more steps issues several calls, the later ones accumulating -- the
 * chain is then the same).  The grid is tiled over (image, row chunk, D tile): 32
 * rows per block, 8 when that would leave fewer than 1024 blocks.
 * len: NULL, or a (B,) int32 DEVICE vector; n = clamp(len[b], 1, L) on the device.  Rows l >= n are written as exact zeros
 * when accumulate == 0 and left alone otherwise; alpha and the map are never loaded there.
 * T, B, L, D >= 1 (RFN_ERR_SHAPE); alpha, dz, datt_seq non-NULL (RFN_ERR_ARG); datt_seq must not overlap alpha or dz.
 * (tests/test_dseq_steps_gpu.py pins all of the above.) */
int rfn_attn_context_bwd_dseq_steps(int T, const float* alpha, int64_t alpha_st, const float* dz, int64_t dz_st, int64_t lddz,
                                    int B, int L, int D, float* datt_seq, int64_t sb, int64_t sl, int accumulate,
                                    const int32_t* len, void* stream);
/* softmax + tanh backward.  ds = alpha*(dalpha - <alpha,dalpha>); dproj[b,l,a] (=|+=)
 * ds[b,l]*w[a]*(1-e^2), e = tanh(proj+hproj); dhproj[b,a] = sum_l dproj[b,l,a];
 * dw_part[b,a] = sum_l ds[b,l]*e[b,l,a]  (caller column-sums dw_part over b).
 * dproj may alias proj (in-place).  */
int rfn_attn_scores_bwd(const float* proj, int64_t proj_sb, int64_t proj_sl, const float* hproj,
                        const float* w_out, const float* alpha, const float* dalpha, int B, int L,
                        int A, float* dproj, int64_t dproj_sb, int64_t dproj_sl,
                        int accumulate_dproj, float* dhproj, float* dw_part, void* stream);

/* rfn_attn_context_bwd_dalpha + rfn_attn_scores_bwd in one launch, one block per batch row: dalpha never leaves
 * the CU.  Results are bit-identical to the pair.  (d att_seq is not produced here: the stage-I feature gradient is a pass of its own
 * over all steps, rfn_attn_context_bwd_dseq_steps / rfn_prefix_bwd_inputs.) */
int rfn_attn_bwd(const float* proj, int64_t proj_sb, int64_t proj_sl, const float* hproj, const float* w_out,
                 const float* alpha, const float* att_seq, int64_t sb, int64_t sl, const float* dz, int64_t lddz,
                 int B, int L, int A, int D, float* dproj, int64_t dproj_sb, int64_t dproj_sl,
                 int accumulate_dproj, float* dhproj, float* dw_part, void* stream);
/* rfn_attn_fwd_grouped / rfn_attn_bwd_grouped for encoders whose feature maps differ in (L_g, D_g) -- the reference ships
 * 196 x 2048, 64 x 1536, 64 x 1280 and 49 x 2208 maps side by side (feat_array.py:240-244, one AttentionModelCore per
 * encoder: misc/RecurrentFusionModel.py:139-146) -- in ONE pair of launches / one launch: the M cells of a stage-I step are
 * independent (misc/RecurrentFusionModel.py:101-114).  Contiguous layouts: proj / dproj (B, L_g, A), att_seq (B, L_g, D_g),
 * z / dz (B, D_g), alpha and the raw-score scratch (B, L_g).  Same kernels and per-row arithmetic as the per-encoder calls:
 * bit-identical results, as long as the per-encoder call takes the same (16-byte or scalar) instantiation -- see the
 * all-or-nothing rule above: a map with D_g % 4 != 0 puts its neighbours on the scalar context / dalpha code as well.
 * L_host / D_host: host arrays of ngroups ints. */
int rfn_attn_fwd_het(int ngroups, const float* const* proj, const float* const* hproj, const float* const* w_out,
                     const float* const* b_out, const float* const* att_seq, int B, const int* L_host, int A,
                     const int* D_host, float* const* scores_scratch, float* const* alpha, float* const* z, void* stream);
int rfn_attn_bwd_het(int ngroups, const float* const* proj, const float* const* hproj, const float* const* w_out,
                     const float* const* alpha, const float* const* att_seq, const float* const* dz, int B,
                     const int* L_host, int A, const int* D_host, float* const* dproj, int accumulate_dproj,
                     float* const* dhproj, float* const* dw_part, void* stream);
int rfn_attn_fwd_ragged(int ngroups, const float* const* proj, const float* const* hproj, const float* const* w_out,
                        const float* const* b_out, const float* const* att_seq, int B, const int* L_host, int A,
                        const int* D_host, float* const* scores_scratch, float* const* alpha, float* const* z,
                        const int32_t* const* len, void* stream);
int rfn_attn_bwd_ragged(int ngroups, const float* const* proj, const float* const* hproj, const float* const* w_out,
                        const float* const* alpha, const float* const* att_seq, const float* const* dz, int B,
                        const int* L_host, int A, const int* D_host, float* const* dproj, int accumulate_dproj,
                        float* const* dhproj, float* const* dw_part, const int32_t* const* len, void* stream);
/* The same for `ngroups` encoders that share (L, A, D) and every stride, one launch (grid = B x ngroups). */
int rfn_attn_bwd_grouped(int ngroups, const float* const* proj, int64_t proj_sb, int64_t proj_sl,
                         const float* const* hproj, const float* const* w_out, const float* const* alpha,
                         const float* const* att_seq, int64_t sb, int64_t sl, const float* const* dz, int64_t lddz,
                         int B, int L, int A, int D, float* const* dproj, int64_t dproj_sb, int64_t dproj_sl,
                         int accumulate_dproj, float* const* dhproj, float* const* dw_part, void* stream);
/* The same launch with dproj delivered as bf16 planes into k-slow plane images (rfn_x3_split_ks layout, one image per
 * encoder, row pitch ks_mp, this call's A columns at column ks_col0; k = b * L + l) instead of f32 -- the operand of
 * rfn_x3_gemm_ks for d att_2_att_h.weight.  A % 4 == 0 and 16-B aligned contiguous rows only. */
int rfn_attn_bwd_grouped_ks(int ngroups, const float* const* proj, int64_t proj_sb, int64_t proj_sl,
                            const float* const* hproj, const float* const* w_out, const float* const* alpha,
                            const float* const* att_seq, int64_t sb, int64_t sl, const float* const* dz, int64_t lddz,
                            int B, int L, int A, int D, void* const* ks_images, int ks_mp, int ks_col0,
                            float* const* dhproj, float* const* dw_part, void* stream);

/* Fused small-L (L <= 1024; meant for a handful) attention of up to RFN_MAX_ENC encoders in one launch: scores + softmax + context
 * (forward) and dalpha + softmax/tanh backward + d att_seq (backward), one block per (batch row, encoder).
 * Used by stage II and the decoder, which attend over the T1 / T2 thought vectors.  Arrays are host arrays of
 * device pointers, one entry per encoder; all encoders share strides and (L, A, D). */
int rfn_attn_small_fwd(int ngroups, const float* const* proj, int64_t proj_sb, int64_t proj_sl,
                       const float* const* hproj, const float* const* w_out, const float* const* b_out,
                       const float* const* att_seq, int64_t sb, int64_t sl, int B, int L, int A, int D,
                       float* const* alpha, float* const* z, int64_t ldz, void* stream);
/* datt_seq (may be NULL) is ACCUMULATED into: datt_seq[g][b,l,:] += alpha*dz; dproj/dhproj/dw_part as in
 * rfn_attn_scores_bwd. */
int rfn_attn_small_bwd(int ngroups, const float* const* proj, int64_t proj_sb, int64_t proj_sl,
                       const float* const* hproj, const float* const* w_out, const float* const* alpha,
                       const float* const* att_seq, int64_t sb, int64_t sl, const float* const* dz,
                       int64_t lddz, int B, int L, int A, int D, float* const* dproj, int64_t dproj_sb,
                       int64_t dproj_sl, int accumulate_dproj, float* const* dhproj, float* const* dw_part,
                       float* const* datt_seq, void* stream);

/* ---- decoder cell with z2h hoisted through the attention (csrc/rfn_deccell.hip, round 6) -------------------------------
 * misc/LSTMSoftAttentionCore.py:64-81 applies z2h to z = sum_l alpha_l v_l over the SAME thought vectors v with the SAME
 * weights on every step; z2h is linear, so z2h(z) = b_z + sum_l alpha_l U_l with U = v . W_z^T computed once per call.
 * rfn_dec_cell_fwd: one launch = scores (:64-75), softmax (:76), gates = (sum_l alpha_l U_l + b_z) + gates_in (:81; gates_in =
 *   i2h(x) + h2h(h) already in `gates`), LSTM update (:83-101) with the dropout mask of (seed, drop_offset); the gate
 *   activations overwrite `gates` (4R wide, 5R with maxout) as rfn_lstm_fwd leaves them.  proj / U rows of batch row b are
 *   those of row b / row_div (beam search: the rows of one image share its thought vectors).  alpha (B, L) out.
 * rfn_dec_attn_bwd: the attention backward of one step from that step's gate gradients: d alpha_l = <dgates, U_l>, softmax
 *   and tanh backward; dproj (accumulated when `accumulate`), dhproj, dw_part as rfn_attn_small_bwd.  GD = 4R or 5R.
 * rfn_dec_du: after the loop, dU[b, l, :] = sum_s alpha[s, b, l] * dgates[s, b, :] (alpha (S, B, L), dgates (S, B, GD)
 *   contiguous; dU strides as U).
 *
 * Operands.  proj (b', l, :) at proj + b' * psb + l * psl and U at U + b' * usb + l * usl with b' = b / row_div: both need
 *   ceil(B / row_div) rows (rfn_dec_attn_bwd has no row_div: B rows).  gates, c_prev, c_next, h_next, dgates have a row stride
 *   (ldg, ldcp, ldcn, ldh); dproj has strides of its own (dpsb, dpsl), dU those handed to rfn_dec_du.  Packed, without a
 *   stride: hproj (B, A), w_out (A), bz (GD), alpha (B, L), dhproj and dw_part (B, A), and rfn_dec_du's alpha (S, B, L) and
 *   dgates (S, B, GD).  c_next may be c_prev (same pointer, same stride: a unit reads its c_prev before it writes; the
 *   free-running decoders call the cell in place), and h_next may be any buffer the call does not read; results are those of the
 *   out-of-place call.  With U = 0 and b_z = 0 the gate activations are rfn_lstm_fwd's bits on the same gates_in; c and h agree
 *   with it to rounding (f * c_prev + i * g is left to the compiler's contraction in both).  The dropout counter of unit j of
 *   row b is b * R + j (rfn_dropout_mask over B * R values) whatever ldh is.
 * Limits (RFN_ERR_SHAPE, nothing launched, no output touched); Xp = X rounded up to 4:
 *   every extent (B, L, A, R, GD, S) >= 1; row_div >= 1; 0 <= drop_p < 1;
 *   rfn_dec_cell_fwd:   L <= 1024; off its fast kernel 2 * Ap + L floats <= 64 KiB
 *   rfn_dec_attn_bwd:   L <= 1024 and 2 * Ap + 2 * Lp + 32 floats <= 64 KiB (whichever kernel would serve the call)
 *   rfn_dec_du:         on its 16-byte kernel (below) the S * L alpha values of a row are staged in LDS: S * L floats <= 64 KiB,
 *                       else refused; the scalar kernel reads alpha from memory and takes any S * L.
 *   A NULL pointer is RFN_ERR_ARG; b_out alone may be NULL (no bias: the results of b_out = {0}).
 * Alignment: any float-aligned pointer and any stride is accepted.
 *   rfn_dec_cell_fwd takes its fast kernel when A % 4 == 0, A <= 512, L <= 8, R % 256 == 0, psb and psl are multiples of 4 and
 *   proj, hproj, w_out are 16-byte aligned; else the general kernel, which reads proj in 16-byte pieces when A % 4 == 0, psb and
 *   psl are multiples of 4 and proj is 16-byte aligned.  A row's results (gates, c, h, alpha) are the same bits on the fast
 *   kernel, whatever the share of a row it gives a block, and on the general kernel with 16-byte proj reads, at any B and any
 *   block size; the general kernel's scalar proj reads sum a score in another order (same results to rounding).
 *   rfn_dec_attn_bwd takes its fast kernel when A % 4 == 0, A <= 512, L <= 8, GD % 4 == 0, every stride (psb, psl, usb, usl, ldg,
 *   dpsb, dpsl) is a multiple of 4 and proj, hproj, w_out, U, dgates, dproj, dhproj, dw_part are 16-byte aligned.  Otherwise
 *   the general kernel decides twice: 16-byte accesses on the (L, A) side when A % 4 == 0, psb, psl, dpsb, dpsl are multiples of
 *   4 and proj, dproj, dhproj, dw_part are aligned; on the GD side when GD % 4 == 0, usb, usl, ldg are multiples of 4 and U,
 *   dgates are aligned.  The five kernels are the same formulas and agree to rounding; bit-equality between two of them is
 *   not promised (contraction is left to the compiler: the fast kernel and the general one with both 16-byte forms fuse
 *   1 - t * t and the d pre-activation products into fmas differently; the fast kernel adds the sums of rows 0..3 and 4..7
 *   separately; the scalar forms sum a dot in another order).  A row's results do not depend on B or on the other rows.
 *   accumulate != 0: dproj = dproj_before + the gradient with one rounding (the gradient's last product is fused into the
 *   sum): within u * (|accumulated| + |overwritten|), u = 2^-24, of dproj_before + the overwrite result, not its bits;
 *   dhproj, dw_part do not depend on accumulate.
 *   rfn_dec_du takes its 16-byte kernel when GD % 4 == 0, usb and usl are multiples of 4 and dgates, dU are 16-byte aligned, else
 *   the scalar one; both add the steps in order from 0 and give the same bits.  Only dU[b, l, 0:GD], l < L, is written. */
int rfn_dec_cell_fwd(const float* proj, int64_t psb, int64_t psl, const float* hproj, const float* w_out,
                     const float* b_out, const float* U, int64_t usb, int64_t usl, const float* bz, float* gates,
                     int64_t ldg, const float* c_prev, int64_t ldcp, float* c_next, int64_t ldcn, float* h_next,
                     int64_t ldh, float* alpha, int B, int L, int A, int R, int maxout, int row_div, float drop_p,
                     uint64_t seed, uint64_t drop_offset, void* stream);
int rfn_dec_attn_bwd(const float* proj, int64_t psb, int64_t psl, const float* hproj, const float* w_out,
                     const float* alpha, const float* U, int64_t usb, int64_t usl, const float* dgates, int64_t ldg,
                     int B, int L, int A, int GD, float* dproj, int64_t dpsb, int64_t dpsl, int accumulate,
                     float* dhproj, float* dw_part, void* stream);
int rfn_dec_du(const float* alpha, const float* dgates, int S, int B, int L, int GD, float* dU, int64_t usb,
               int64_t usl, void* stream);
/* The backward pair with n = row_div rows per image ("multi-sample self-critical" below; misc/LSTMSoftAttentionCore.py:64-81 on
 * n rows that hold the same thought vectors).  Limits, alignment rules and kernels as above; row_div < 1: RFN_ERR_SHAPE.
 * rfn_dec_attn_bwd_ex: proj and U are read at image b / row_div (ceil(B / row_div) rows each), exactly as rfn_dec_cell_fwd reads
 *   them; alpha, dgates, hproj, dhproj, dw_part AND dproj stay per row -- dproj is (b, l, :) at dproj + b * dpsb + l * dpsl for all
 *   B rows, so no two rows of an image ever read-modify-write one address (no atomics; the caller sums the rows afterwards,
 *   rfn_rowgroup_sum).  A row's arithmetic is that of rfn_dec_attn_bwd on physically repeated proj / U: the same bits on the
 *   same kernel.  row_div = 1: rfn_dec_attn_bwd, which forwards here.
 * rfn_dec_du_ex: B % row_div == 0 (RFN_ERR_SHAPE otherwise); dU is (B / row_div images, L, GD) with strides usb / usl and
 *   dU[k, l, :] = sum_j sum_s alpha[s, k * n + j, l] * dgates[s, k * n + j, :]: ONE running sum from 0, the image's rows j
 *   ascending outermost, the steps s ascending inside.  The 16-byte kernel stages row_div * S * L alpha values in LDS (<= 64 KiB,
 *   else refused); the scalar kernel takes any.  Both give the same bits.  row_div = 1: rfn_dec_du, which forwards here. */
int rfn_dec_attn_bwd_ex(const float* proj, int64_t psb, int64_t psl, const float* hproj, const float* w_out,
                        const float* alpha, const float* U, int64_t usb, int64_t usl, const float* dgates, int64_t ldg,
                        int B, int row_div, int L, int A, int GD, float* dproj, int64_t dpsb, int64_t dpsl, int accumulate,
                        float* dhproj, float* dw_part, void* stream);
int rfn_dec_du_ex(const float* alpha, const float* dgates, int S, int B, int L, int GD, int row_div, float* dU, int64_t usb,
                  int64_t usl, void* stream);
/* y[r, 0:cols] = ((0 + x[r * n, :]) + x[r * n + 1, :]) + ... + x[r * n + n - 1, :] for r < rows: every n consecutive rows of x
 * (row stride ldx) summed onto one row of y (row stride ldy), j ascending -- the fan-in of the per-row d att_2_att_h(v) slabs
 * (T2, B, A) onto the images (T2, B / n, A), which is this call with rows = T2 * B / n.  One output chunk per thread (16 bytes when
 * cols % 4 == 0, ldx and ldy are multiples of 4 and x, y are 16-byte aligned, else one float; same bits), no atomics.
 * RFN_ERR_SHAPE: n < 1, rows < 1, cols < 1, a stride below cols.  x and y must not overlap. */
int rfn_rowgroup_sum(const float* x, int64_t ldx, int n, float* y, int64_t ldy, int64_t rows, int cols, void* stream);

/* ---- row-panel GEMM of the recurrences (csrc/rfn_cellgemm.hip) ------------------------------------------------------
 * One launch computes up to RFN_CELL_MAXOUT outputs over the same M (= batch) rows, each with its own destination,
 * weights and K segments:  C_o[M, N_o] (+)= sum_s A_os[M, K_os] * op(B_os) + sum_s bias_os.  Segments are rfn_gemm_seg
 * with a_kfast = 1; b_kfast = 1: B is an nn.Linear weight [N][K] (forward products, K1-K2 / K5 / K8 / K9 of SURVEY.md
 * 2.2); b_kfast = 0: B is [K][N] (dX = dY . W of the backward recurrences).  The K range of an output tile is cut across
 * the waves of ONE block and the partial tiles are added in LDS in wave order: deterministic, no scratch, and an
 * element's k order depends only on K.
 * epilogue RFN_CELL_EPI_STORE: plain store / accumulate (16-B coalesced).
 * epilogue RFN_CELL_EPI_LSTM (b_kfast = 1, N = 4R): C is the gate buffer (B, 4R) [in | forget | out | g]; the sums
 *   (+ C when accumulate: e.g. i2h(x) + h2h(h) produced earlier) go through the LSTM gate math of rfn_lstm_fwd inside
 *   the same launch: activations written back to C, c_next = f c_prev + i g, h_next = dropout(o tanh c_next) with the
 *   mask of (seed, drop_offset) (rfn_dropout_mask).  Replaces misc/RecurrentFusionModel.py:53-73,
 *   misc/LSTMSoftMultiAttentionFeatArrayNoInputCore.py:50-72, misc/LSTMSoftAttentionCore.py:81-101 after the attention.
 * epilogue RFN_CELL_EPI_LSTM_BWD (b_kfast = 0, N = R, one output): the product is the recurrent part of d h of an
 *   EARLIER cell call (the one the backward sweep processes next); the launch finishes that gradient,
 *   dh = product (+ C when accumulate) + dh_ext, and runs rfn_lstm_bwd of that call on it: `gates` holds its activations
 *   on entry and its gate gradients on exit, c_prev / c_next are its cell states, dc_next (may be NULL, may alias
 *   dc_prev) the incoming d c, dc_prev the outgoing one, (seed, drop_offset) its dropout mask.  C (may be NULL unless
 *   accumulate) receives dh.  Replaces the axpby + rfn_lstm_bwd pair at the head of every backward step.
 * Requirements (rfn_cell_gemm_supported; otherwise RFN_ERR_UNSUPPORTED and the caller uses rfn_gemm_f32 + rfn_lstm_*):
 * every K and N a multiple of 32, 16-B aligned operands with leading dimensions that are multiples of 4, R a multiple
 * of 8 for the gate epilogue; any M.  `variant` 0 lets the library pick: the K step and K-wave count -- which fix the k order
 * of every output element -- from the K counts alone, never from M, so a row's arithmetic does not depend on the batch it
 * sits in; the tile height may follow M (16-row tiles on wave-private ring slots, variant 6, for launches with few tiles:
 * the same fma chains, identical bits).  1..6 and 8 force a variant; 7 / 9 = the library's choice restricted to the
 * shared-slot forms 1..5 / to the 64- and 32-row shared-slot forms 1..3 (tests, tools, A/B); bits 4-7 force the ring depth
 * of variants 1..5 (tools).  RFN_CELL_VARIANT_DEEP in `variant` (A/B hook): a launch of the 32-row variant whose tiles do not
 * outnumber the device's CUs runs on the deep-ring kernel (8 ring slots, the whole K range of K <= 512 in flight, a K loop
 * without barriers) -- bit-identical results, measured slower inside the step (profiles/r05_chain.md). */
#define RFN_CELL_VARIANT_DEEP 256
#define RFN_CELL_MAXOUT 10
#define RFN_CELL_MAXSEG 8
#define RFN_CELL_EPI_STORE 0
#define RFN_CELL_EPI_LSTM 1
#define RFN_CELL_EPI_LSTM_BWD 2
typedef struct rfn_cell_out {
    float* C;
    int64_t ldc;
    int32_t N;
    int32_t accumulate;
    int32_t nseg;
    int32_t epilogue;            /* the same for every output of a launch */
    rfn_gemm_seg seg[RFN_CELL_MAXSEG];
    /* RFN_CELL_EPI_LSTM and _LSTM_BWD */
    const float* c_prev;         /* (M, R); forward: may alias c_next */
    int64_t ldcp;
    float* c_next;               /* forward: written; backward: read */
    int64_t ldcn;
    float* h_next;               /* forward only */
    int64_t ldh;
    uint64_t drop_offset;
    /* RFN_CELL_EPI_LSTM_BWD only */
    float* gates;                /* (M, 4R) activations in, gate gradients out */
    int64_t ldg;
    const float* dh_ext;         /* (M, R) gradient of that call's h from outside the recurrence, may be NULL */
    int64_t lddh;
    const float* dc_next;        /* may be NULL */
    int64_t lddcn;
    float* dc_prev;
    int64_t lddcp;
    /* RFN_CELL_EPI_STORE and _LSTM_BWD with accumulate: the sums start from C + S_0 + ... + S_{acc_parts-1}, added in that
     * order, where slab S_p has C's shape and leading dimension and starts at acc_slabs + p * acc_stride (acc_parts = 0: C
     * alone) -- the partial products of an earlier launch: the decoder's K-split d gates . W_hh computed beside the attention
     * backward (csrc/rfn_deccell.hip), the stage-I cells' d gates_j . W_H_j of small batches */
    const float* acc_slabs;
    int32_t acc_parts;
    int64_t acc_stride;
} rfn_cell_out;
int rfn_cell_gemm_supported(int M, int nout, const rfn_cell_out* outs_host, int R);
int rfn_cell_gemm(int M, int nout, const rfn_cell_out* outs_host, int R, float drop_p, uint64_t seed, int variant,
                  void* stream);

/* Dropout masks of the path (nn.Dropout of the three cells: misc/RecurrentFusionModel.py:70,
 * misc/LSTMSoftMultiAttentionFeatArrayNoInputCore.py:69, misc/LSTMSoftAttentionCore.py:98).  A mask is never stored:
 * unit j of batch row b of one cell call is kept iff philox4x32-10(key = seed, counter = (b * R + j, offset)) >= p, with
 * `seed` the 64-bit seed the caller hands to rfn_prefix_fwd / rfn_decoder_fwd / rfn_decoder_step and `offset` the call
 * site: stage-I cell (step t, encoder i) -> t * M + i (p = drop_fusion); stage-II cell t -> RFN_DROP_OFFSET_STAGE2 + t
 * (p = drop_reason); decoder step s -> RFN_DROP_OFFSET_DECODER + s (p = drop_lm).  Forward and backward regenerate it.
 * rfn_dropout_mask writes the keep mask of one call site (n = B * R values, 1.0f = kept, 0.0f = dropped) so that a
 * test can hand the product's own masks to the CPU oracle. */
#define RFN_DROP_OFFSET_STAGE2 (1ull << 20)
#define RFN_DROP_OFFSET_DECODER (1ull << 21)
int rfn_dropout_mask(uint64_t seed, uint64_t offset, int64_t n, float drop_p, float* keep_out, void* stream);
/* The same mask for the key stored at `seed_dev` (device memory, read when the launch runs): what the kernels of a call with
 * RFN_PATH_OPT_SEED_DEV and seed = (uint64_t)seed_dev apply.  Errors as rfn_dropout_mask; a NULL seed_dev is RFN_ERR_ARG. */
int rfn_dropout_mask_dev(const uint64_t* seed_dev, uint64_t offset, int64_t n, float drop_p, float* keep_out, void* stream);

/* LSTM gate epilogue shared by the three cells (misc/RecurrentFusionModel.py:55-73,
 * misc/LSTMSoftMultiAttentionFeatArrayNoInputCore.py:54-72, misc/LSTMSoftAttentionCore.py:83-101):
 * gates[b, 0:4R] = [in | forget | out | g] pre-activations on entry, activations on exit;
 * c_next = f*c_prev + i*g; h_next = dropout(o*tanh(c_next)).  maxout != 0: gates are 5R wide,
 * g = max(chunk 3, chunk 4) without tanh (LSTMSoftMultiAttention...py:60-62, LSTMSoftAttentionCore.py:89-91).  drop_p > 0 draws a Philox mask from
 * (seed, offset) that rfn_lstm_bwd regenerates. */
int rfn_lstm_fwd(float* gates, int64_t ldg, const float* c_prev, int64_t ldcp, float* c_next,
                 int64_t ldcn, float* h_next, int64_t ldh, int B, int R, int maxout, float drop_p,
                 uint64_t seed, uint64_t offset, void* stream);
/* G independent cells in one launch (the M encoders of a stage-I step): group g uses gates + g*gs_gates,
 * c_prev + g*gs_cprev, c_next + g*gs_cnext, h_next + g*gs_h and dropout stream offset + g. */
int rfn_lstm_fwd_grouped(float* gates, int64_t ldg, const float* c_prev, int64_t ldcp, float* c_next,
                         int64_t ldcn, float* h_next, int64_t ldh, int B, int R, int maxout, float drop_p,
                         uint64_t seed, uint64_t offset, int G, int64_t gs_gates, int64_t gs_cprev,
                         int64_t gs_cnext, int64_t gs_h, void* stream);
/* dgates (in place over the activations), dc_prev = dc_next_total * f.
 * dh / dc_next are the TOTAL incoming gradients of h_next / c_next (dc_next may be NULL). */
int rfn_lstm_bwd(float* gates, int64_t ldg, const float* c_prev, int64_t ldcp, const float* c_next,
                 int64_t ldcn, const float* dh, int64_t lddh, const float* dc_next, int64_t lddcn,
                 float* dc_prev, int64_t lddcp, int B, int R, int maxout, float drop_p, uint64_t seed,
                 uint64_t offset, void* stream);

/* grouped backward: c_prev and c_next share gs_c; dc_next and dc_prev share gs_dc */
int rfn_lstm_bwd_grouped(float* gates, int64_t ldg, const float* c_prev, int64_t ldcp, const float* c_next,
                         int64_t ldcn, const float* dh, int64_t lddh, const float* dc_next, int64_t lddcn,
                         float* dc_prev, int64_t lddcp, int B, int R, int maxout, float drop_p,
                         uint64_t seed, uint64_t offset, int G, int64_t gs_gates, int64_t gs_c, int64_t gs_dh,
                         int64_t gs_dc,
                         void* stream);

/* nn.Embedding gather (misc/RecurrentFusionModel.py:276): out[r,:] = W[id(r), :] with
 * id(r) = ids[(r % inner)*ids_s_inner + (r / inner)*ids_s_outer]  (row r = (step, batch) reads
 * ids[batch, step] with inner = B, ids_s_inner = ld_ids, ids_s_outer = 1). */
int rfn_embed_fwd(const float* W, int E, int64_t V1, const int64_t* ids, int inner,
                  int64_t ids_s_inner, int64_t ids_s_outer, int rows, float* out, int64_t ldo,
                  void* stream);
/* dW[v,:] = sum_{r: id(r)==v} dout[r,:]  (fixed order, overwrites all of dW) */
int rfn_embed_bwd(const float* dout, int64_t ldo, const int64_t* ids, int inner,
                  int64_t ids_s_inner, int64_t ids_s_outer, int rows, int E, int64_t V1, float* dW,
                  void* stream);

/* F.log_softmax over the vocabulary (misc/RecurrentFusionModel.py:278).  Row r of `logits`
 * (ld = ldl) is written to out + (r % inner)*out_s_inner + (r / inner)*out_s_outer, which turns
 * the path's time-major (step, batch) rows into the reference's (batch, step, V+1) layout. */
int rfn_log_softmax_fwd(const float* logits, int64_t ldl, int rows, int V1, int inner,
                        int64_t out_s_inner, int64_t out_s_outer, float* out, void* stream);
/* dlogits[r,:] = g[r',:] - exp(logp[r',:]) * sum_v g[r',v]   (r' = the same row mapping) */
int rfn_log_softmax_bwd(const float* g, const float* logp, int rows, int V1, int inner,
                        int64_t s_inner, int64_t s_outer, float* dlogits, int64_t ldd, void* stream);

/* max over steps of the reason heads (misc/RecurrentFusionModel.py:229,253):
 * out[b,k] = max_t X[t,b,k]; arg[b,k] = first t attaining it. */
int rfn_max_over_steps_fwd(const float* X, int T, int B, int K, float* out, int32_t* arg,
                           void* stream);
/* dX[t,b,k] = (arg[b,k]==t) ? dout[b,k] : 0 */
int rfn_max_over_steps_bwd(const float* dout, const int32_t* arg, int T, int B, int K, float* dX,
                           void* stream);
/* The same for `ngroups` heads in one launch: X slabs (T,B,K) back to back, out / arg / dout (B,K) back to back. */
int rfn_max_over_steps_fwd_grouped(const float* X, int T, int B, int K, float* out, int32_t* arg, int ngroups,
                                   void* stream);
int rfn_max_over_steps_bwd_grouped(const float* dout, const int32_t* arg, int T, int B, int K, float* dX,
                                   int ngroups, void* stream);

/* y[r,c] = alpha*x[r,c] + beta*y[r,c]  (state mean misc/RecurrentFusionModel.py:233-235,
 * gradient fan-in) */
int rfn_axpby_2d(float alpha, const float* x, int64_t ldx, float beta, float* y, int64_t ldy,
                 int rows, int cols, void* stream);

/* y[r,c] = y[r,c] / divisor (IEEE division, as `sum / num_feat_array` in the reference) */
int rfn_div_2d(float* y, int64_t ldy, int rows, int cols, float divisor, void* stream);
/* State mean over the M encoder slices of a concatenated (rows, G*gstride) state (misc/RecurrentFusionModel.py:233-235):
 * y_p[r,c] = (x_p[r,c] + x_p[r,gstride+c] + ...) / G, summed in slice order then divided; up to two (x, y) pairs
 * (h and c) per launch.  Arrays are host arrays of device pointers. */
int rfn_mean_over_groups(int npairs, const float* const* x, int64_t ldx, int64_t gstride, int G, float* const* y,
                         int64_t ldy, int rows, int cols, void* stream);
/* Its backward: y_p[r, g*gstride + c] = alpha*x_p[r,c] + beta[p]*y_p[r, g*gstride + c] for every slice g. */
int rfn_bcast_to_groups(int npairs, float alpha, const float* const* x, int64_t ldx, const float* beta,
                        float* const* y, int64_t ldy, int64_t gstride, int G, int rows, int cols, void* stream);

/* ---- criteria (misc/utils.py) --------------------------------------------------------------- */
/* ReviewNetEnsembleCriterion language term (misc/utils.py:163-184): loss_out[0] (+)=
 * -sum_{b,t} mask[b,t]*q[b,t,:].logp[b,t,:] / B with q one-hot (eps = 0) or label-smoothed, and
 * dlogp (same layout as logp, overwritten) = d loss / d logp * gscale.  Either output may be NULL. */
int rfn_xe_loss(const float* logp, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                const float* mask, int64_t ld_mask, float eps, float gscale,
                float* scratch /* B*T floats, needed when loss_out != NULL */, float* loss_out,
                int accumulate_loss, float* dlogp, void* stream);
/* Same, with the upstream gradient also read from a device scalar (autograd hands d loss as a 0-dim tensor):
 * dlogp is scaled by gscale * gscale_dev[0]; gscale_dev may be NULL. */
int rfn_xe_loss_ex(const float* logp, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                   const float* mask, int64_t ld_mask, float eps, float gscale, const float* gscale_dev,
                   float* scratch, float* loss_out, int accumulate_loss, float* dlogp, void* stream);
/* The same language term straight from the LOGITS (log-softmax / NLL / label smoothing and their backward
 * without the (B, T, V+1) log_prob and d log_prob tensors; F.log_softmax of misc/RecurrentFusionModel.py:276 + misc/utils.py:
 * 163-184).  `logits`: time-major rows r = t * B + b with row stride ldl (the layout of the decoder workspace,
 * rfn_decoder_logits).  _fwd: lse[r] (T*B floats) = the row's logsumexp, loss_out[0] (+)= -sum mask * q . (x - lse) / B;
 * scratch: B*T floats.  _bwd overwrites the logits with d loss / d logits * gscale * gscale_dev[0] (gscale_dev may be NULL). */
int rfn_xe_logits_fwd(const float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                      const float* mask, int64_t ld_mask, float eps, float* lse, float* scratch, float* loss_out,
                      int accumulate_loss, void* stream);
int rfn_xe_logits_bwd(float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                      const float* mask, int64_t ld_mask, float eps, const float* lse, float gscale,
                      const float* gscale_dev, void* stream);
/* Distillation: the same language term plus a KL term towards a teacher's distribution, straight from the logits (the loss of
 * RecurrentFusionModel.forward_loss(..., teacher=)).  Rows are (b, t): x = the student's logits row (time-major, as above),
 * z = the teacher's row at teacher + b * z_sb + t * z_st, logits or log-probs (every term is invariant to a per-row shift of
 * z; the two strides serve a batch-major (B, T, V1) tensor and a time-major (T, B, V1) buffer alike), q = the one-hot or
 * label-smoothed target of rfn_xe_logits_*, m = mask[b, t], it = inv_temp = 1 / temperature, alpha in [0, 1]:
 *   p_t(v)  = softmax(z * it)(v)            p_s(v) = softmax(x * it)(v)
 *   KL(b,t) = sum_{v : p_t(v) > 0} p_t(v) * (log p_t(v) - log p_s(v))
 *   xe      = sum_{b,t} m * ( -q . log_softmax(x) ) / B           (exactly rfn_xe_logits_fwd's loss, bit for bit)
 *   kd      = sum_{b,t} m * KL(b,t) / (it*it) / B                 (the usual tau^2 scaling)
 *   loss    = (1 - alpha) * xe + alpha * kd
 *   d loss / d x[v] = m * g / B * ( (1 - alpha) * (softmax(x)[v] - q[v]) + alpha / it * (p_s(v) - p_t(v)) )
 * A -inf teacher entry contributes 0 (constraint-masked log-probs are a legal teacher; no NaN from 0 * inf); a teacher row
 * with no finite entry is the caller's error and is not checked; a row with m == 0 has loss terms of exactly 0 and _bwd writes
 * zeros over its logits, whatever its teacher row holds (NaN included).  Targets are clamped as in rfn_xe_logits_*.
 * _fwd: row_stats (3*T*B floats) = lse(x), lse(x*it), lse(z*it), each as T*B time-major rows; scratch: 2*B*T floats;
 * loss_out[0] (+)= loss; terms_out (may be NULL) = {xe, kd}.  _bwd overwrites the logits with d loss / d logits * gscale *
 * gscale_dev[0] (gscale_dev may be NULL) from the same target / mask / eps / teacher / alpha / inv_temp and _fwd's row_stats.
 * Both rows are read 16 B per lane when the student passes rfn_xe_logits_*'s conditions (V1 % 4 == 0, V1 <= 10240, ldl % 4 == 0,
 * 16-B aligned) and the teacher is 16-B aligned with z_sb % 4 == 0 and z_st % 4 == 0; otherwise element-wise.
 * RFN_ERR_SHAPE: the checks of rfn_xe_logits_*, alpha outside [0, 1], inv_temp not finite or <= 0, |z_sb| or |z_st| < V1. */
int rfn_kd_logits_fwd(const float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                      const float* mask, int64_t ld_mask, float eps, const float* teacher, int64_t z_sb, int64_t z_st,
                      float alpha, float inv_temp, float* row_stats, float* scratch, float* loss_out, int accumulate_loss,
                      float* terms_out, void* stream);
int rfn_kd_logits_bwd(float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                      const float* mask, int64_t ld_mask, float eps, const float* teacher, int64_t z_sb, int64_t z_st,
                      float alpha, float inv_temp, const float* row_stats, float gscale, const float* gscale_dev,
                      void* stream);
/* The same pair with a COMPACT teacher: row (b, t) of the teacher is the K <= 32 pairs
 *   (t_ids[b * i_sb + t * i_st + k], t_val[b * v_sb + t * v_st + k]),  k < K,
 * e.g. the lists rfn_log_softmax_topk writes, batch-major or time-major (two strides each, in elements).  Their meaning is
 * exactly rfn_kd_logits_*'s on the dense row z with z[id_k] = val_k and -inf everywhere else:
 *   p_t(k)  = softmax over the K entries of val * it          p_s(v) = softmax(x * it)(v)
 *   KL(b,t) = sum_k p_t(k) * (log p_t(k) - log p_s(id_k))
 * and xe, kd, loss and d loss / d x are as written above (p_t(v) = 0 off the K ids): the teacher's tail mass is dropped and the
 * K entries are renormalised.  val may be logits or log-probs (every term is invariant to a per-row shift).
 * An entry is padding when its id is outside [0, V1) or its val is -inf: it contributes 0 and its id is never used as an index,
 * so a row may hold fewer than K live entries.  The live ids of a row must be distinct (not checked here: the caller's
 * contract); a row without a live entry is the caller's error, as a dense row without a finite entry is.  A row with m == 0 has
 * loss terms of exactly 0, _bwd writes zeros over its logits, and neither its ids nor its values are read.
 * row_stats (3*T*B) = lse(x), lse(x*it), lse over the live entries of val*it (0 for a row with m == 0): the dense pair's layout;
 * scratch: 2*B*T floats; loss_out, terms_out, gscale, gscale_dev as above.  The xe term and lse(x) are rfn_xe_logits_fwd's bits
 * at any alpha.  No atomics: the K entries are reduced by one wave's shuffles in a fixed order, so two runs give the same bits.
 * The student's row is read 16 B per lane under rfn_xe_logits_*'s conditions and element-wise otherwise, whatever the alignment
 * of t_ids / t_val (K elements per row, read one per lane).  _bwd writes in place: it gathers x[id_k] before any lane of the
 * row's block writes, writes the teacher-free gradient over the row, and rewrites the K elements behind a block barrier.
 * RFN_ERR_SHAPE: the checks of rfn_xe_logits_*, alpha / inv_temp as rfn_kd_logits_*, K < 1, K > 32, |i_sb|, |i_st|, |v_sb| or
 * |v_st| < K.  RFN_ERR_ARG: a NULL pointer (gscale_dev and terms_out may be NULL).  Shape checks come first. */
int rfn_kd_topk_fwd(const float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                    const float* mask, int64_t ld_mask, float eps, const int32_t* t_ids, int64_t i_sb, int64_t i_st,
                    const float* t_val, int64_t v_sb, int64_t v_st, int K, float alpha, float inv_temp, float* row_stats,
                    float* scratch, float* loss_out, int accumulate_loss, float* terms_out, void* stream);
int rfn_kd_topk_bwd(float* logits, int64_t ldl, int B, int T, int V1, const int64_t* target, int64_t ld_target,
                    const float* mask, int64_t ld_mask, float eps, const int32_t* t_ids, int64_t i_sb, int64_t i_st,
                    const float* t_val, int64_t v_sb, int64_t v_st, int K, float alpha, float inv_temp, const float* row_stats,
                    float gscale, const float* gscale_dev, void* stream);
/* ReviewNetRewardCriterion policy + entropy terms (misc/utils.py:50-72):
 * loss_out[0] (+)= [ -sum pol(b,t)*mask(b,t) + entropy_reg * sum mask0(b,t) * sum_v lp*exp(lp) ] / B with
 * mask0 = seq > 0, mask = [1, mask0[:, :-1]], pol = input*reward or the reference's PPO-clip surrogate.
 * d_input (B,T) and d_logprobs_all rows t < T (same strides convention) are overwritten when non-NULL. */
int rfn_rl_loss(const float* input, int64_t ld_in, const int64_t* seq, int64_t ld_seq, const float* reward,
                int64_t ld_rw, const float* logprobs_all, int64_t lp_sb, int64_t lp_st, int B, int T, int V1,
                float entropy_reg, const float* old_logprobs, int64_t ld_old, int use_ppo, float ppo_clip,
                float* scratch /* B*T floats when loss_out != NULL */, float* loss_out, int accumulate_loss,
                float* d_input, int64_t ld_din, float* d_logprobs_all, int64_t dlp_sb, int64_t dlp_st,
                void* stream);
/* Same, for an autograd host: the upstream gradient is read from a device scalar (d_input and d_logprobs_all are scaled
 * by gscale_dev[0]; NULL = 1), and logprobs_all / d_logprobs_all hold T_all >= T steps per caption (sample() returns
 * seq_length + 1 of them, misc/RecurrentFusionModel.py:655-658): rows t in [T, T_all) of d_logprobs_all are written as
 * zeros by the same launch, so the caller needs neither a zero fill nor a scaling pass over the (B, T_all, V+1) tensor. */
int rfn_rl_loss_ex(const float* input, int64_t ld_in, const int64_t* seq, int64_t ld_seq, const float* reward,
                   int64_t ld_rw, const float* logprobs_all, int64_t lp_sb, int64_t lp_st, int B, int T, int T_all, int V1,
                   float entropy_reg, const float* old_logprobs, int64_t ld_old, int use_ppo, float ppo_clip,
                   const float* gscale_dev, float* scratch, float* loss_out, int accumulate_loss, float* d_input,
                   int64_t ld_din, float* d_logprobs_all, int64_t dlp_sb, int64_t dlp_st, void* stream);
/* ---- policy-gradient loss from the logits ----------------------------------------------------------------------------------
 * The same policy + entropy terms straight from the LOGITS of a teacher-forced replay of given captions (the loss of
 * RecurrentFusionModel.rl_loss): neither logprobs_all (B, T, V+1) nor its gradient exists, so captions drawn by the no-grad
 * device loops (rfn_decoder_loop_ex2, the beam loops, stochastic beam search) can be trained on.  `logits`: time-major rows
 * r = t * B + b with row stride ldl, as rfn_xe_logits_* take them.  Per row, with lp_v = x_v - lse, p_v = exp(lp_v),
 * tok = seq[b, t] (clamped into [0, V1) as rfn_xe_logits_* clamp targets), m0 = seq[b, t] > 0, mk = 1 at t == 0 and
 * seq[b, t - 1] > 0 after it, rw = reward[b * ld_rw + t]:
 *   Hm   = sum_v lp_v * p_v                                  (only evaluated where entropy_reg * m0 != 0; 0 otherwise)
 *   pol  = lp_tok * rw, or rfn_rl_loss's PPO-clip surrogate of lp_tok, old_logprobs[b, t] and ppo_clip (it clamps surr1)
 *   loss_out[0] (+)= sum_{b,t} ( -pol * mk + entropy_reg * m0 * Hm ) / B     (rfn_rl_loss's loss; terms summed in a fixed order)
 *   d x_v = a * ([v == tok] - p_v) + e * p_v * (lp_v - Hm),  a = -(g / B) * mk * d pol / d lp_tok,  e = (g / B) * entropy_reg * m0
 * _fwd: row_stats (3*T*B floats) = lse, Hm, lp_tok as T*B time-major rows; tok_lp (B, ld_tok_lp >= T) = lp_tok, the expression
 * x[tok] - lse: the bits rfn_log_softmax_fwd writes at that position; scratch: B*T floats, 3*B*T with terms_out; terms_out (may be
 * NULL) = {sum -pol * mk / B, sum entropy_reg * m0 * Hm / B}, the two terms each summed on its own.  _bwd overwrites the logits with
 * d loss / d logits, g = gscale * gscale_dev[0] (gscale_dev may be NULL), from the same seq / reward / old_logprobs and _fwd's
 * row_stats.  A row with a == 0 and e == 0 (mk == 0 and m0 == 0; a zero reward without an entropy term) is written as exact
 * zeros; with e == 0 the entropy expression is not evaluated.  No atomics: two runs give the same bits.  Rows are read 16 B per
 * lane under rfn_xe_logits_*'s conditions and element-wise otherwise.
 * RFN_ERR_SHAPE: B, T or V1 < 1, ldl < V1, ld_tok_lp < T.  RFN_ERR_ARG: a NULL pointer (old_logprobs may be NULL unless
 * use_ppo; gscale_dev and terms_out may be NULL).  Shape checks come first. */
int rfn_rl_logits_fwd(const float* logits, int64_t ldl, int B, int T, int V1, const int64_t* seq, int64_t ld_seq,
                      const float* reward, int64_t ld_rw, float entropy_reg, const float* old_logprobs, int64_t ld_old,
                      int use_ppo, float ppo_clip, float* row_stats, float* tok_lp, int64_t ld_tok_lp, float* scratch,
                      float* loss_out, int accumulate_loss, float* terms_out, void* stream);
int rfn_rl_logits_bwd(float* logits, int64_t ldl, int B, int T, int V1, const int64_t* seq, int64_t ld_seq,
                      const float* reward, int64_t ld_rw, float entropy_reg, const float* old_logprobs, int64_t ld_old,
                      int use_ppo, float ppo_clip, const float* row_stats, float gscale, const float* gscale_dev, void* stream);
/* nn.MultiLabelMarginLoss, mean reduction (misc/utils.py:186-190), scaled by `scale`:
 * loss_out[0] (+)= scale * MLM(pred, target); dpred (overwritten) = scale * gscale * dMLM/dpred. */
int rfn_multilabel_margin(const float* pred, int B, int K, const int64_t* target, float scale,
                          float gscale, float* scratch /* B floats when loss_out != NULL */,
                          float* loss_out, int accumulate_loss, float* dpred, void* stream);

/* All M+1 reasoning heads of ReviewNetEnsembleCriterion in one launch (misc/utils.py:186-190: the per-head
 * losses are added one after the other, which the fixed-order finish reproduces).  preds / dpreds: host arrays of
 * nheads device pointers ((B,K) each; dpreds or its entries may be NULL); scratch: nheads*B floats when loss_out. */
int rfn_multilabel_margin_grouped(int nheads, const float* const* preds, int B, int K, const int64_t* target,
                                  float scale, float gscale, const float* gscale_dev, float* scratch,
                                  float* loss_out, int accumulate_loss, float* const* dpreds, void* stream);

/* clip_gradient + Adam with L2 weight decay (misc/utils.py:292-296, train.py:69-71,162-163),
 * one pass: g = clamp(g, +-clip) + wd*p; m,v update; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps).
 * grad_scale multiplies g first (1/world_size after a sum all-reduce). */
int rfn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, float grad_clip, float grad_scale,
                  int step, void* stream);
/* The same update of up to RFN_ADAM_MAXBUCKET flat buckets in ONE launch (same hyper-parameters and step for all, as
 * torch.optim.Adam applies them to the reference's single param group, train.py:69-71): bit-identical to one rfn_adam_step
 * per bucket, without the per-launch ramp and tail (2.15 -> 1.95 ms at C3).  Host arrays of nbuckets entries. */
#define RFN_ADAM_MAXBUCKET 16
int rfn_adam_step_multi(int nbuckets, float* const* p, const float* const* g, float* const* m, float* const* v,
                        const int64_t* n_host, float lr, float beta1, float beta2, float eps, float weight_decay,
                        float grad_clip, float grad_scale, int step, void* stream);
/* The same launch with its two step-dependent scalars read from DEVICE memory: coef_dev[0] = lr / (1 - beta1^step),
 * coef_dev[1] = 1 / sqrt(1 - beta2^step), computed by the host exactly as rfn_adam_step_multi computes them (in double, then
 * rounded to float) and written there before the launch.  Everything else of the call is step-independent, so a HIP graph
 * that captured it can be replayed for every step (kernel arguments are frozen by a capture; train.py:162-163 steps the
 * optimizer once per iteration).  Bit-identical to rfn_adam_step_multi for the same coefficients. */
int rfn_adam_step_multi_coef(int nbuckets, float* const* p, const float* const* g, float* const* m, float* const* v,
                             const int64_t* n_host, const float* coef_dev, float beta1, float beta2, float eps,
                             float weight_decay, float grad_clip, float grad_scale, void* stream);

/* greedy pick of sample() (misc/RecurrentFusionModel.py:619-649) for one step t >= 1:
 * it = argmax_v logp[b,:] (first maximum), lp_out[b] = that value,
 * with torch.max's order on degenerate rows: NaN ranks above every number, so a row holding NaN picks its first NaN
 * (lp_out[b] = NaN), and a row of all -inf picks token 0; `it` is always in [0, V1).
 * unf_out[b] = (t==1 ? 1 : unf_prev[b]) & (it>0), seq_out[b] = it*unf_out[b],
 * next_ids[b] = it (UNMASKED: the reference embeds the raw argmax, :637).
 * Keeping one unf_out row per step lets the host apply the reference's early exit (:645) with a
 * single device read after the loop instead of one sync per step. */
int rfn_greedy_pick(const float* logp, int64_t ldl, int B, int V1, int t, int64_t* next_ids,
                    int64_t* seq_out, int64_t ld_seq, float* lp_out, int64_t ld_lp,
                    const int32_t* unf_prev, int32_t* unf_out, void* stream);

/* The same bookkeeping for a token chosen elsewhere (given != NULL, e.g. a multinomial draw; may alias next_ids):
 * it = given[b], lp_out[b] = logp[b, it], unf / seq / next_ids as above.  given == NULL: rfn_greedy_pick. */
int rfn_pick_record(const float* logp, int64_t ldl, int B, int V1, int t, const int64_t* given, int64_t* next_ids,
                    int64_t* seq_out, int64_t ld_seq, float* lp_out, int64_t ld_lp, const int32_t* unf_prev,
                    int32_t* unf_out, void* stream);

/* multinomial pick of sample() (misc/RecurrentFusionModel.py:623-631) and of scheduled sampling (:260-270), on the
 * device: ids[b] = inverse-CDF draw from p[v] ~ exp(logp[b,v] * inv_temperature) with the caller's uniform u[b] in
 * [0,1) -- a deterministic function of (logp, u).  With coin != NULL only rows with coin[b] < keep_prob are redrawn,
 * the others keep the token ids[b] already holds (the scheduled-sampling mask).  Element b of ids lives at
 * ids[b * ld_ids].  (The reference draws on the host with torch.multinomial; RNG streams are not portable, the
 * distribution is the same.) */
int rfn_multinomial_pick(const float* logp, int64_t ldl, int B, int V1, float inv_temperature, const float* u,
                         const float* coin, float keep_prob, int64_t* ids, int64_t ld_ids, void* stream);

/* Batched beam-search bookkeeping of sample_beam (misc/RecurrentFusionModel.py:451-531) for step t in [1, S]:
 * one block per image consumes the log-probs of its W beam rows (rows k*W .. k*W+W-1 of `logp`), reproduces the
 * reference's candidate order / stable sort / fork / done-beam rules on the device and emits
 *   order[r]    source row whose recurrent state row r continues (feed rfn_gather_rows),
 *   next_ids[r] token row r feeds to the next decoder step,
 * updating beam_seq / beam_lp (S, NB, W), beam_sum (NB, W), the done-beam arrays (NB, max_done, ...) and
 * active[k] (0 once image k has no candidate left, :480).  W <= 16 (rfn_beam_step_topk: W <= 32), S <= 64. */
int rfn_beam_step(const float* logp, int64_t ldl, int V1, int W, int S, int t, int NB, int max_done,
                  int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* next_ids,
                  int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active,
                  void* stream);
/* The same step fed with every beam row's W best log-probs and tokens (rfn_log_softmax_topk, (NB * W, W) each) instead
 * of the full rows -- all the reference ever reads of them (:463-466). */
int rfn_beam_step_topk(const float* topv, const int32_t* topi, int V1, int W, int S, int t, int NB, int max_done,
                       int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* next_ids,
                       int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active, void* stream);
/* log-softmax of every row + its W <= 32 best entries, ordered (value descending, token ascending) as a descending
 * sort lists them; the log-prob bits are those rfn_log_softmax_fwd writes, which are not materialised here. */
int rfn_log_softmax_topk(const float* logits, int64_t ldl, int rows, int V1, int W, float* topv, int32_t* topi,
                         void* stream);
/* ---- decoding constraints (off by default; the reference has none) ---------------------------------------------------------
 * All of them edit a row's log-probs AFTER the log-softmax, by setting entries to -inf without renormalising: the log-prob
 * recorded for a chosen token stays the model's own.  The history of a row is the tokens it has emitted so far (BOS
 * excluded); step t >= 1 picks the t-th token, so the history then holds t - 1 tokens.  For a row that has not finished
 * (history empty or its last token != 0; a finished row is left alone, its list is empty):
 *   - banned[i] (0 < id < V1) is blocked at every step;
 *   - block_ngram = n in [2, 4] (0 = off), t >= n: with g the last n - 1 tokens of the history, every token that followed an
 *     earlier occurrence of g in the history is blocked, except token 0 (END);
 *   - token 0 is blocked when the last token of the history is one of bad_endings (at t = S as at any other step: the search's
 *     forced close at t = S is not a token choice and stays as it is).
 * rfn_decode_blocklist writes the blocked ids of `rows` rows: blk (rows, RFN_DECODE_MAX_IDS + S) int32, row r holding blk_n[r]
 * ids (banned first, then the n-gram continuations in history order, then 0) padded with -1; the list may hold duplicates.
 * Token j of row r is hist[src * s_row + j * s_tok], src = order ? order[r] : r -- a (B, S) matrix (s_row = its row stride,
 * s_tok = 1), or the beam arrays (S, NB, W) (s_row = 1, s_tok = NB * W): with order == NULL as rfn_beam_step leaves them
 * (already forked, row r = beam r), with the step's order[] when they have NOT been forked yet (row r continues beam
 * order[r]).  Limits (RFN_ERR_SHAPE): 1 <= t <= S <= 64, n_banned, n_bad <= RFN_DECODE_MAX_IDS.  Ids outside [0, V1) are
 * dropped, so are banned ids <= 0. */
#define RFN_DECODE_MAX_IDS 64
int rfn_decode_blocklist(const int64_t* hist, int64_t s_row, int64_t s_tok, const int32_t* order, int rows, int S, int t,
                         int block_ngram, const int32_t* banned, int n_banned, const int32_t* bad_endings, int n_bad, int V1,
                         int32_t* blk, int32_t* blk_n, void* stream);
/* logp[r, blk[r, i]] = -inf for i < blk_n[r], in place; everything else keeps its bits (ldl >= V1: the row stride). */
int rfn_logp_mask_rows(float* logp, int64_t ldl, int rows, int V1, const int32_t* blk, int64_t ld_blk, const int32_t* blk_n,
                       void* stream);
/* rfn_log_softmax_topk of the masked rows: the log-sum-exp is taken over ALL V1 logits (an unblocked entry carries exactly the
 * bits rfn_log_softmax_topk / rfn_log_softmax_fwd give it), blocked tokens rank as -inf -- the list a stable descending sort of
 * the masked log-prob row gives, so a row with fewer than W unblocked tokens is filled with its lowest -inf ids in ascending
 * order.  blk == NULL: rfn_log_softmax_topk, bit for bit.  V1 <= 393216 with a block list (one bit per token in LDS). */
int rfn_log_softmax_topk_masked(const float* logits, int64_t ldl, int rows, int V1, int W, const int32_t* blk, int64_t ld_blk,
                                const int32_t* blk_n, float* topv, int32_t* topi, void* stream);
/* What the loop entry points below take: the id lists live in device memory (uploaded once per call by the host), blk / blk_n
 * are scratch of (rows, RFN_DECODE_MAX_IDS + S) and (rows) int32 for the rows of the loop (B, or NB * W). */
typedef struct rfn_decode_constraints {
    int32_t block_ngram;          /* 0 = off, else 2 .. 4 */
    int32_t n_banned, n_bad;      /* <= RFN_DECODE_MAX_IDS each */
    int32_t pad_;
    const int32_t* banned;        /* device, may be NULL when n_banned = 0 */
    const int32_t* bad_endings;   /* device, may be NULL when n_bad = 0 */
    int32_t* blk;
    int32_t* blk_n;
} rfn_decode_constraints;
/* ---- truncated sampling: top-k and nucleus (top-p) (off by default; the reference has neither) -----------------------------
 * Another edit of a row's log-probs after the log-softmax (and after the constraints' masking), again without renormalising.
 * x[0 .. V1): log-probs, possibly holding -inf already; inv_temperature > 0, top_k, top_p.
 *   - weight w_v = exp(x_v * inv_temperature); a -inf entry has weight 0 and is never kept;
 *   - the order is x descending, then token id ascending (the order rfn_log_softmax_topk lists);
 *   - top_k = k > 0: the first min(k, number of finite entries) in that order are kept -- ties at the cut go to the lower ids,
 *     so exactly that many; top_k <= 0 or >= V1: off;
 *   - top_p = p, 0 < p < 1, over the survivors of top-k: with c_j the sum of the first j weights and c_n the sum of all, the
 *     first J = min{ j : c_j >= p * c_n } are kept (J >= 1); p >= 1: off;
 *   - every entry not kept becomes -inf, kept entries keep their bits: the log-prob recorded for a drawn token stays the model's
 *     own, and rfn_multinomial_pick normalises by the sum of what is left;
 *   - a row with no finite entry, or one holding a NaN, is left untouched (the pick's own rules then apply).
 * rfn_logp_truncate_rows does this in place for `rows` rows of stride ldl >= V1, one launch, one block per row, without sorting
 * (a radix select on the integer image of the floats; masses are exact 64-bit integer sums of fp64 weights rounded down to 2^-47
 * of the row's largest, so the kept set is a function of the row alone: the same in any launch, at any row position, rows and
 * ldl).  kept_n (rows, or NULL): the number of kept entries (0 for a row without finite entry, -1 for one holding a NaN).
 * RFN_ERR_SHAPE: rows <= 0, V1 <= 0, ldl < V1, !(inv_temperature > 0), top_p not in (0, +inf); RFN_ERR_ARG: logp NULL; both
 * knobs off: RFN_OK, nothing launched; V1 > 65536: RFN_ERR_UNSUPPORTED. */
int rfn_logp_truncate_rows(float* logp, int64_t ldl, int rows, int V1, int top_k, float top_p, float inv_temperature,
                           int32_t* kept_n, void* stream);
/* What rfn_decoder_loop_ex2 takes besides the constraints. */
typedef struct rfn_decode_sampling {
    int32_t top_k;            /* <= 0: off */
    float top_p;              /* >= 1: off */
    int32_t rows_per_image;   /* n >= 1 draws per image (0 reads as 1) */
    int32_t pad_;
} rfn_decode_sampling;
/* ---- diverse beam search: beam groups with a Hamming penalty (off by default; the reference has none) -----------------------
 * The W beams of an image are G groups of Wg = W / G beams, group g owning beams g*Wg .. g*Wg+Wg-1.  One step t (1 .. S) of
 * one image runs the groups in order g = 0 .. G-1, all groups at the same t (no stagger in time); each group follows the rules
 * of rfn_beam_step restricted to its own beams:
 *   - live rows: at t == 1 the group's first row only, else its Wg rows; a row whose last token is 0 gives no candidates;
 *   - count[v], v != 0: the number of beams that groups 0 .. g-1 newly selected at this step with token v.  Token 0 (END) is
 *     never counted and never penalised (the exemption n-gram blocking makes: diversity never decides whether a caption may
 *     end); a beam that kept its previous state (vix >= the number of new beams) is not counted;
 *   - candidates in (column c of the row's top list outer, beam q inner) order over the live rows, with today's values
 *     local = ys[q][c] and p = fp32(beam_sum[q] + local);
 *   - ranking key: p where count[v] == 0, else fp32(beam_sum[q] + fp32(local - fp32(lambda * count[v]))) -- three operations,
 *     each rounded to fp32 on its own, never fused;
 *   - stable descending order by key; the first min(Wg, candidates) become the group's beams 0 .. Wg-1;
 *   - beam_lp, beam_sum, done_lp and done_p get the unaugmented local / p: lambda decides which hypotheses survive, never a
 *     reported log-probability;
 *   - a selected candidate that emits 0, or any selected candidate at t == S, is appended to the image's done beams in
 *     construction order (group, then rank), done_group[k, slot] = g beside it; max_done = W * S bounds them as before;
 *   - a group without a candidate leaves its rows inert (order = identity, next_ids = 0); active[k] becomes 0 only when no
 *     group of the image has one.
 * The constraints act on the top lists before the step sees them, the length penalty ranks the done beams afterwards: both
 * unchanged.  Keys that are NaN (a NaN log-prob) are not ordered; the step then stays in bounds but selects no defined set.
 *
 * Why the W best entries of a row suffice.  Define the search on full rows: every row's V1 entries sorted descending (value,
 * then token id), candidates taken in (column, beam) order.  At group g at most g * Wg <= W - Wg distinct tokens are
 * penalised.  A candidate beyond column W of its row therefore has at least Wg unpenalised entries of the same row in earlier
 * columns; their keys are not smaller (they are p values of larger or equal local on the same beam_sum, the fp32 add is
 * monotone, and a penalty only lowers a key), and on a tie they come earlier in construction order.  So that candidate is
 * never among the first Wg, and a stable sort keeps the relative order of the ones that remain.  With V1 < W the list is the
 * whole row.
 *
 * rfn_beam_step_div: rfn_beam_step_topk's arguments plus G, lambda and done_group (NB, max_done) int32.  One block per image,
 * the groups in a serial loop, every candidate computing its own rank (no single-thread sort).  G == 1 forwards to
 * rfn_beam_step_topk (lambda is ignored, done_group may be NULL).  RFN_ERR_SHAPE: G < 1, W % G != 0, !(lambda >= 0). */
int rfn_beam_step_div(const float* topv, const int32_t* topi, int V1, int W, int G, float lambda, int S, int t, int NB,
                      int max_done, int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* next_ids,
                      int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* done_group, int32_t* active,
                      void* stream);
/* What rfn_beam_loop_ex2 takes besides the constraints. */
typedef struct rfn_beam_diversity {
    int32_t groups;           /* G >= 1, W % G == 0; 1: the plain search */
    float lambda;             /* >= 0 */
    int32_t* done_group;      /* (NB, max_done), device; may be NULL when groups == 1 */
} rfn_beam_diversity;
/* ---- lexically constrained beam search: required words (off by default; the reference has none) -----------------------------
 * After Anderson et al. 2017, "Guided open vocabulary image captioning with constrained beam search".  Per image there are C
 * constraint sets, 0 <= C <= RFN_LEX_MAX_SETS; a set is a disjunction of token ids in [1, V1) (token 0, END, is never in one)
 * and is satisfied once the caption holds any of its ids.  The host hands over the image's unique ids, want (NB, NW) int32
 * padded with -1, and want_bits (NB, NW) int32 with bit i set when the id is in set i (an id in two sets carries two bits);
 * NW <= RFN_LEX_MAX_IDS.  init_state (NB) int32 holds the bits of the image's EMPTY sets: an image with fewer than C sets has its
 * missing sets satisfied from the start.
 *
 * Search state.  G = 2^C states (bit masks of satisfied sets), each owning a beam of Wb rows: state s owns rows s*Wb ..
 * s*Wb+Wb-1 of the image's W = G * Wb <= 32 rows.  state_n (NB, G) int32 counts the occupied rows of every state; occupied rows
 * are packed at the front.  Before step 1 only the first row of state init_state[k] is occupied (at t == 1 the step takes the
 * occupancy from init_state and does not read state_n).  Unoccupied rows are inert: order = identity, next_ids = 0, no
 * candidates; their beam_seq / beam_lp / beam_sum entries are whatever an earlier step left there and mean nothing.
 *
 * One step t (1 .. S) of one image visits the target states in ascending order s = 0 .. G-1, every one reading the beams as they
 * were BEFORE the step:
 *   - a live row is an occupied row whose last token is not 0 (at t == 1 the single occupied row is live);
 *   - a stay candidate of live row q in state s' is an entry (local, v) of the row's top list whose destination s' | bits(v)
 *     equals s' (bits(v) = 0 for a token that is not wanted), taken in (column outer, row inner) order;
 *   - a move candidate of row q is a want entry j with bits_j & ~s' != 0: local = wantv[q][j], destination s' | bits_j, taken in
 *     (want index outer, row inner) order.  A want token whose sets are all satisfied already is only ever a stay candidate, so
 *     no token is offered twice;
 *   - a candidate whose local is -inf is dropped: a blocked or absent token cannot occupy a row;
 *   - the candidates of target s are listed by source state ascending; within a source state come its stay candidates when
 *     s' == s and its move candidates with destination s otherwise;
 *   - p = fp32(beam_sum[q] + local); the order is stable and descending by p; the first min(Wb, candidates) become rows 0 .. of
 *     state s and state_n[k, s] is that count.  DEPARTURE from rfn_beam_step: a state with fewer candidates than Wb does not keep
 *     stale rows -- the rest of its rows are unoccupied;
 *   - a selected candidate that emits 0, or any selected candidate at t == S, is appended to the done beams in construction order
 *     (state, then rank), done_state[k, slot] = s beside it; max_done = W * S bounds them as before; beam_lp, beam_sum, done_lp
 *     and done_p are handled exactly as in rfn_beam_step_topk;
 *   - active[k] becomes 0 when no state has a candidate.
 * Keys that are NaN are not ordered; the step then stays in bounds but selects no defined set (as the diverse search).
 *
 * Why the W best entries of a row suffice.  Define the search on full rows (every row's V1 entries sorted descending by value,
 * then token id).  Move candidates come from the want values, not from the lists.  Of a row's first W columns at most NW change
 * the state, so at least W - NW stay; a row can place at most Wb candidates in its own state, and a stay candidate beyond column
 * W has at least W - NW stay candidates of the same row before it, with p not smaller (the fp32 add is monotone) and earlier in
 * construction order.  With NW <= W - Wb that candidate is never among the first Wb, and a stable sort keeps the relative order
 * of the rest: the search on the W-wide lists equals the search on full rows.  With V1 < W the list is the whole row.  The entry
 * points refuse NW > W - Wb.
 *
 * The returned caption (host, torch ops on the device): done beams ordered by the number of satisfied sets descending, within
 * that by p (or p / len^alpha) descending, ties in construction order.
 *
 * rfn_log_softmax_topk_want: rfn_log_softmax_topk_masked plus wantv (rows, NW): wantv[r, j] = the log-prob of token
 * want[r / row_div, j] (want has row stride ld_want >= NW) in the bits rfn_log_softmax_fwd writes, -inf for an id outside
 * [0, V1) (the -1 padding) or a blocked token.  topv / topi are bit for bit rfn_log_softmax_topk_masked's.  want == NULL forwards
 * to rfn_log_softmax_topk_masked.  RFN_ERR_SHAPE: as there, NW < 1, NW > RFN_LEX_MAX_IDS, ld_want < NW, row_div < 1.
 *
 * rfn_beam_step_lex: one block per image, the target states in a serial loop, every candidate computing its own rank.  C == 0
 * forwards to rfn_beam_step_topk.  RFN_ERR_SHAPE: C < 0 or > RFN_LEX_MAX_SETS, W % 2^C != 0, NW < 0 or > RFN_LEX_MAX_IDS,
 * NW > W - Wb, W > 32, S > 64. */
#define RFN_LEX_MAX_SETS 3
#define RFN_LEX_MAX_IDS 16
int rfn_log_softmax_topk_want(const float* logits, int64_t ldl, int rows, int V1, int W, int row_div, const int32_t* want,
                              int64_t ld_want, int NW, const int32_t* blk, int64_t ld_blk, const int32_t* blk_n, float* topv,
                              int32_t* topi, float* wantv, void* stream);
int rfn_beam_step_lex(const float* topv, const int32_t* topi, const float* wantv, const int32_t* want, const int32_t* want_bits,
                      int NW, int C, int V1, int W, int S, int t, int NB, int max_done, int64_t* beam_seq, float* beam_lp,
                      float* beam_sum, int32_t* order, int64_t* next_ids, int64_t* done_seq, float* done_lp, float* done_p,
                      int32_t* done_n, int32_t* state_n, int32_t* done_state, const int32_t* init_state, int32_t* active,
                      void* stream);
/* What rfn_beam_loop_ex3 takes besides the constraints and the diversity. */
typedef struct rfn_beam_lexical {
    int32_t n_sets;               /* C in 1 .. RFN_LEX_MAX_SETS; W % 2^C == 0 */
    int32_t n_want;               /* NW in 1 .. RFN_LEX_MAX_IDS, NW <= W - W / 2^C */
    const int32_t* want;          /* (NB, n_want), device, padded with -1 */
    const int32_t* want_bits;     /* (NB, n_want), device */
    const int32_t* init_state;    /* (NB), device */
    float* wantv;                 /* (NB * W, n_want) scratch */
    int32_t* state_n;             /* (NB, 2^C) */
    int32_t* done_state;          /* (NB, max_done) */
} rfn_beam_lexical;
/* ---- stochastic beam search: W distinct sampled captions (off by default; the reference has none) -------------------------
 * After Kool, van Hoof and Welling 2019, "Stochastic beams and where to find them": one beam search of width W on
 * Gumbel-perturbed log-probabilities returns W distinct captions that are an exact sample WITHOUT replacement from the model's
 * distribution over captions; row 0 is an exact ordinary sample, and the perturbed scores give importance weights.
 *
 * Noise.  The search has a 64-bit seed and a 64-bit offset0.  Row r = k * W + j (image k, beam row j), step t in [1, S], token
 * v: n = the upper 24 bits (word >> 8) of word 0 of Philox4x32-10 with key = seed and counter = (idx = r * V1 + v, offset =
 * offset0 + t), the layout of rfn_dropout_mask; u = (n + 0.5) / 2^24, never 0 or 1; e = -ln(-ln u).  All in fp64.
 *
 * State.  Every row holds, in fp64, phi (the log-probability of its prefix) and G (its perturbed log-probability), and the
 * flags live and finished (finished: live, and its last token is 0).  Before step 1 only row 0 of an image is live, with phi = 0
 * and G = the draw e of (r = k * W, v = 0, t = 0); the other rows are dead (phi = G = -inf).  The root's G must be a Gumbel(0)
 * draw and not the constant 0: the maximum of the captions' perturbed scores is such a draw, and fixing it conditions every G
 * below it -- the SET drawn is the same either way (G' is increasing in G_j), but the weights below assume unconditional scores
 * and come out biased under the constant (their sum averages 0.83 instead of 1 on the 40-caption model of tests/sbs_cpu.py).
 * rfn_beam_sbs_begin writes that state (one launch); rfn_beam_loop_ex4 calls it.
 *
 * Step t of image k:
 *   - a live, unfinished row j with log-prob row x -- the fp32 bits rfn_log_softmax_fwd writes, -inf where the decoding
 *     constraints blocked a token; a -inf or NaN entry is never a candidate -- has, per token v, key_v = double(x_v) + e,
 *     gamma_v = phi_j + key_v and Z_j = max_v gamma_v.  Candidate (j, v) has phi' = phi_j + double(x_v) and
 *     G' = -ln(exp(-G_j) - exp(-Z_j) + exp(-gamma_v)), evaluated as d = G_j - gamma_v + log1mexp(gamma_v - Z_j), G' = G_j -
 *     max(0, d) - log1p(exp(-|d|)), with log1mexp(a) = ln(-expm1(a)) for a > -ln 2 and log1p(-exp(a)) otherwise; the argmax
 *     child (the first entry of the row's list: largest key, lowest token among equals) gets G' = G_j exactly;
 *   - a live finished row has the single candidate "itself": token 0, token log-prob 0, phi and G unchanged.  Carrying finished
 *     rows as candidates is what makes the sample exact;
 *   - the new rows are the min(W, candidates) candidates of largest G', stored in descending G', ties by source row ascending,
 *     then token ascending.  Rows beyond that are dead: live = 0, phi = G = -inf, tokens and token log-probs 0, order = identity,
 *     next_ids = 0.  A row becomes finished when its token is 0; at t = S every row is closed as it stands;
 *   - G' is non-decreasing in gamma_v for a fixed row, so the image's W best candidates lie inside each row's W best key_v: the
 *     per-row lists of rfn_log_softmax_topk_gumbel are all a row has to hand over.
 * Weights after step S: with kappa = G of the last live row, live rows before the last get weight = exp(phi) / q, q =
 * -expm1(-exp(phi - kappa)); the last live row and the dead rows get 0 -- Kool et al.'s estimator over W - 1 samples with the
 * W-th as threshold: sum_i weight_i f(caption_i) is an unbiased estimate of E f.  With decoding constraints the weights are
 * RELATIVE: the restricted distribution is not renormalised (phi sums the model's own log-probs), so they estimate sums over the
 * allowed captions, not expectations under a renormalised model.
 *
 * rfn_log_softmax_topk_gumbel: one block per row, the structure and limits of rfn_log_softmax_topk_masked (W <= 32, the same
 * log-sum-exp, hence the same log-prob bits; blk == NULL: no block list).  Rows with live[r] == 0 are skipped, none of their
 * outputs is written.  Per live row the W best candidates by key (descending, token ascending): topk64 (rows, W) fp64 keys, topv
 * their own fp32 log-probs, topi their tokens; a row with fewer than W candidates fills the rest with (-inf, -inf, 0).  offset is
 * offset0 + t of the step that READS the lists.  Error codes as rfn_log_softmax_topk_masked; live or topk64 NULL: RFN_ERR_ARG.
 *
 * rfn_beam_step_sbs: one block per image.  beam_seq / beam_lp keep the (S, NB, W) layout of rfn_beam_step (zero-initialised by the
 * caller), so rfn_decode_blocklist reads them as it does there: a finished row's history ends in 0 and is left alone.  phi /
 * gumbel (NB, W) fp64 and live (NB * W) int32 are the state above; order / next_ids as in rfn_beam_step_topk (a finished row
 * continues the row it came from and feeds token 0, a dead row continues itself).  weight (NB, W) fp64 and n_live (NB) int32 are
 * written at t == S only.  RFN_ERR_SHAPE: W > 32, S > 64, t outside [1, S]; RFN_ERR_ARG: a NULL pointer. */
int rfn_log_softmax_topk_gumbel(const float* logits, int64_t ldl, int rows, int V1, int W, const int32_t* blk, int64_t ld_blk,
                                const int32_t* blk_n, const int32_t* live, uint64_t seed, uint64_t offset, double* topk64,
                                float* topv, int32_t* topi, void* stream);
int rfn_beam_sbs_begin(int NB, int W, int V1, uint64_t seed, uint64_t offset0, double* phi, double* gumbel, int32_t* live,
                       void* stream);
int rfn_beam_step_sbs(const double* topk64, const float* topv, const int32_t* topi, int V1, int W, int S, int t, int NB,
                      int64_t* beam_seq, float* beam_lp, double* phi, double* gumbel, int32_t* live, int32_t* order,
                      int64_t* next_ids, double* weight, int32_t* n_live, void* stream);
/* What rfn_beam_loop_ex4 takes besides the constraints, the diversity and the required words. */
typedef struct rfn_beam_stochastic {
    uint64_t seed, offset0;       /* the noise of step t is drawn at (seed, offset0 + t) */
    double* phi;                  /* (NB, W), device */
    double* gumbel;               /* (NB, W), device */
    int32_t* live;                /* (NB * W), device; the loop sets all three with rfn_beam_sbs_begin */
    double* weight;               /* (NB, W), written by the last step */
    int32_t* n_live;              /* (NB), written by the last step */
    double* topk64;               /* (NB * W, W) scratch: the rows' keys */
} rfn_beam_stochastic;
/* dst[r,:] = src[order[r],:]  (src != dst) */
int rfn_gather_rows(const float* src, float* dst, const int32_t* order, int rows, int R, void* stream);

/* ---- whole-path entry points ---------------------------------------------------------------- */
/* Phase 1 = get_init_state + get_thought_vectors (misc/RecurrentFusionModel.py:333-343, 283-331;
 * the same code is inlined in forward :199-255 and sample :557-612): fc2h, T1 fusion-stage-I steps
 * over M encoders, reason heads, state mean, T2 stage-II steps.
 * Inputs : params (rfn_param_count pointers), fc_feats[i] (B,F_i), att_feats[i] (B,L_i,D_i).
 * Outputs: comb (T2,B,R) time-major thought_vectors_comb; h_out,c_out (B,R) = state_review;
 *          reason_pred (M+1,B,K).
 * `ws` keeps every activation rfn_prefix_bwd needs (size rfn_prefix_ws_bytes; with train = 0 a
 * smaller inference workspace suffices and rfn_prefix_bwd must not be called). */
size_t rfn_prefix_ws_bytes(const rfn_dims* d, int B, int train);
/* `train` selects the workspace layout (activations kept for rfn_prefix_bwd); dropout is applied whenever the
 * probabilities in `d` are non-zero (masks from `seed`), with or without `train`. */
int rfn_prefix_fwd(const rfn_dims* d, int B, const float* const* params,
                   const float* const* fc_feats, const float* const* att_feats, float* comb,
                   float* h_out, float* c_out, float* reason_pred, void* ws, size_t ws_bytes,
                   int train, uint64_t seed, void* stream);
/* get_thought_vectors(fc_feats, att_feats, state_list) with the caller's stage-I state (:283-331): init_h[i],
 * init_c[i] are (B,R) contiguous, one pair per encoder; inference only (workspace of train = 0). */
int rfn_prefix_fwd_from_state(const rfn_dims* d, int B, const float* const* params,
                              const float* const* init_h, const float* const* init_c,
                              const float* const* att_feats, float* comb, float* h_out, float* c_out,
                              float* reason_pred, void* ws, size_t ws_bytes, void* stream);
/* Gradients of phase 1.  d_comb (T2,B,R), d_h, d_c (B,R), d_reason_pred (M+1,B,K) are the incoming
 * gradients (any may be NULL = zero).  Every slot of grads[] (same table as params) that belongs
 * to phase 1 is OVERWRITTEN exactly once (no zero-fill needed); phase-2 slots are not touched. */
int rfn_prefix_bwd(const rfn_dims* d, int B, const float* const* params,
                   const float* const* fc_feats, const float* const* att_feats,
                   const float* d_comb, const float* d_h, const float* d_c,
                   const float* d_reason_pred, float* const* grads, void* ws, size_t ws_bytes,
                   uint64_t seed, int defer_wgrad, void* stream);
/* With defer_wgrad != 0, rfn_prefix_bwd leaves out the stage-I weight gradients of the encoders
 * (review_steps_individual.{t}.lstm.{enc}.{att_model.att_2_att_h, att_model.h_2_att_h, H2h, z2h}.{weight,bias}
 * for all t); this call produces them for one encoder from the same workspace.  `parts` bit 0: H2h, z2h,
 * h_2_att_h (0.27 GB of gradients, short GEMMs); bit 1: att_2_att_h (34 MB, the longest GEMM of backward).
 * A data-parallel host issues part 1, all-reduces that bucket under part 2's GEMM, and so on: only the last
 * encoder's 34 MB bucket remains exposed at the end of backward.  Part 1 of an encoder must be issued before its
 * part 2: att_2_att_h.bias and h_2_att_h.bias have the same gradient, which part 1 computes once and writes to both. */
int rfn_prefix_bwd_wgrad(const rfn_dims* d, int B, const float* const* att_feats, float* const* grads,
                         void* ws, size_t ws_bytes, int enc, int parts, void* stream);
/* Ragged attention maps through stage I: the three entries above plus `att_len`, a HOST array of M DEVICE pointers
 * (att_len[i]: (B,) int32 valid rows of encoder i's map per image, or NULL = all L_i; the array may be NULL).  The lengths
 * reach the stage-I attention launches only (rfn_attn_fwd_ragged / rfn_attn_bwd_ragged: clamped to [1, L_i] on the device);
 * the projection GEMMs still run over all B * L_i rows, so padded rows of att_feats must be FINITE; stage II and the decoder
 * attend over thought vectors and do not change.  The backward call must get the lengths of its forward call.  The padded
 * rows of dP1 are exact zeros, so rfn_prefix_bwd_wgrad needs no lengths.  Without lengths these are the entries above, bit
 * for bit (they forward here).  With lengths, RFN_ERR_UNSUPPORTED -- before anything is launched -- for forms that were not
 * taught them: RFN_PATH_OPT_PERSIST_S2_FWD / _S2_BWD, and RFN_GEMM_OPT_BF16X3 where it makes a length-carrying encoder's
 * attention backward write dP1 as bf16 planes (rfn_attn_bwd_grouped_ks).  The two-kernel backward (rfn_attn_context_bwd_dalpha
 * + rfn_attn_scores_bwd, what small batches with large maps take) has no ragged form either: with lengths those encoders
 * run the one-launch rfn_attn_bwd_ragged instead (same results to the bit as the pair, rfn_attn_bwd). */
int rfn_prefix_fwd_ex(const rfn_dims* d, int B, const float* const* params,
                      const float* const* fc_feats, const float* const* att_feats, float* comb,
                      float* h_out, float* c_out, float* reason_pred, void* ws, size_t ws_bytes,
                      int train, uint64_t seed, const int32_t* const* att_len, void* stream);
int rfn_prefix_fwd_from_state_ex(const rfn_dims* d, int B, const float* const* params,
                                 const float* const* init_h, const float* const* init_c,
                                 const float* const* att_feats, float* comb, float* h_out, float* c_out,
                                 float* reason_pred, void* ws, size_t ws_bytes, const int32_t* const* att_len, void* stream);
int rfn_prefix_bwd_ex(const rfn_dims* d, int B, const float* const* params,
                      const float* const* fc_feats, const float* const* att_feats,
                      const float* d_comb, const float* d_h, const float* d_c,
                      const float* d_reason_pred, float* const* grads, void* ws, size_t ws_bytes,
                      uint64_t seed, int defer_wgrad, const int32_t* const* att_len, void* stream);
/* Gradients of phase 1 with respect to its INPUTS (encoder fine-tuning, saliency).  With x_i = att_feats[i]:
 *   d x_i[b,l,:] = sum_t dP1_i[t][b,l,:] . W_att2att[t,i]     (A) the hoisted projections: one product, K = T1 * A
 *                + sum_t alpha_i[t][b,l] * d z_i[t][b,:]      (B) the attention contexts: rfn_attn_context_bwd_dseq_steps
 *   d fc_i       = (d h0_i + d c0_i) . W_fc2h[i]              (C) get_init_state sets c0 = h0 = fc2h(fc)
 * Called after rfn_prefix_bwd[_ex] on the same workspace, with rfn_dims.path_flags carrying RFN_PATH_OPT_INPUT_GRADS in the
 * forward, the backward and this call; before or after the rfn_prefix_bwd_wgrad calls (it only READS dP1, the attention
 * rows, the d z slices and the stage-I state gradients).  d_att[i] (B, L_i, D_i) and d_fc[i] (B, F_i) are contiguous and
 * OVERWRITTEN; either array, or any entry, may be NULL: that gradient is not produced (no launch for it -- the long product
 * (A) included).  att_len: the lengths of the forward call; rows past an image's length come out as exact zeros.
 * RFN_ERR_UNSUPPORTED, before anything is launched: path_flags without RFN_PATH_OPT_INPUT_GRADS (the workspace has no d z
 * slices); RFN_GEMM_OPT_BF16X3 where it makes the attention backward write a requested encoder's dP1 as bf16 planes only;
 * a workspace of the inference size (smaller than that: RFN_ERR_WORKSPACE). */
int rfn_prefix_bwd_inputs(const rfn_dims* d, int B, const float* const* params, float* const* d_fc, float* const* d_att,
                          void* ws, size_t ws_bytes, const int32_t* const* att_len, void* stream);

/* Phase 2 = the teacher-forced decoder loop of forward() (misc/RecurrentFusionModel.py:257-281):
 * for s < S: xt = embed(ids[b,s]); decoder cell (misc/LSTMSoftAttentionCore.py:60-102);
 * log_prob[b,s,:] = log_softmax(logit(h)).  `ids` is (B, ld_ids) int64, column s feeds step s.
 * The caller derives S from the reference's break rule (:274).
 * log_prob may be NULL: the pass then stops at the logits, which stay in the workspace as time-major rows r = s * B + b of
 * V1 floats (rfn_decoder_logits returns their address) -- the operand of rfn_xe_logits_fwd / _bwd, the loss-only form of
 * the step (RecurrentFusionModel.forward_loss). */
size_t rfn_decoder_ws_bytes(const rfn_dims* d, int B, int S, int train);
float* rfn_decoder_logits(const rfn_dims* d, int B, int S, int train, void* ws);
int rfn_decoder_fwd(const rfn_dims* d, int B, int S, const float* const* params, const float* comb,
                    const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids,
                    float* log_prob /* (B,S,V1) */, void* ws, size_t ws_bytes, int train,
                    uint64_t seed, void* stream);
/* The same pass one step at a time, for scheduled sampling (misc/RecurrentFusionModel.py:260-270: the token fed at
 * step s may be drawn from the distribution of step s-1, so the host interleaves its draws with the steps).
 * rfn_decoder_fwd_begin + rfn_decoder_fwd_step for s = 0 .. S-1 leave `ws` and log_prob[:, 0..S-1, :] exactly as
 * rfn_decoder_fwd on the final ids does (bit for bit), so rfn_decoder_bwd runs on the result unchanged: the sampled
 * pass IS the differentiated pass.  ids_s points at the B tokens of step s (element b at ids_s[b * ld_ids]). */
int rfn_decoder_fwd_begin(const rfn_dims* d, int B, int S, const float* const* params, const float* comb,
                          const float* h0, const float* c0, void* ws, size_t ws_bytes, int train, void* stream);
int rfn_decoder_fwd_step(const rfn_dims* d, int B, int S, int s, const float* const* params, const float* comb,
                         const int64_t* ids_s, int64_t ld_ids, float* log_prob /* (B,S,V1) base */, void* ws,
                         size_t ws_bytes, int train, uint64_t seed, void* stream);
/* d_log_prob (B,S,V1) in; d_comb (T2,B,R), d_h0, d_c0 (B,R) out (overwritten); the phase-2 slots of
 * grads[] (embed, logit, decoder.*) are overwritten.  log_prob == d_log_prob == NULL: the workspace's logits rows
 * already hold d loss / d logits (rfn_xe_logits_bwd wrote them there). */
int rfn_decoder_bwd(const rfn_dims* d, int B, int S, const float* const* params, const float* comb,
                    const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids,
                    const float* log_prob, const float* d_log_prob, float* d_comb, float* d_h0,
                    float* d_c0, float* const* grads, void* ws, size_t ws_bytes, uint64_t seed,
                    void* stream);

/* One free-running decoder step for sample()/sample_beam()/one_time_step
 * (misc/RecurrentFusionModel.py:345-350, 616-653, 526-527): state (h,c) is updated in place,
 * logits (B,V1) pre-softmax and/or logp (B,V1) are written when non-NULL.
 * cproj (rfn_decoder_cproj_floats(d, B) floats) must have been filled by rfn_decoder_prepare: the loop-invariant products of
 * the thought vectors, [att_2_att_h(comb) (T2*B, A) | U = comb . z2h.weight^T (T2*B, 4R or 5R), 256-B aligned] -- the
 * reference recomputes the first every step (misc/LSTMSoftAttentionCore.py:64-66) and applies z2h to the context every step
 * (:81); z2h(sum_l alpha_l v_l) = z2h.bias + sum_l alpha_l U_l (csrc/rfn_deccell.hip).
 * The step is computed with the operation sequence of step `step` of rfn_decoder_fwd: with d->drop_lm > 0 it applies
 * the dropout mask of (seed, step) that rfn_decoder_fwd(train, seed) applies at that step, and its log-probs are
 * bit-identical to the teacher-forced pass fed the same tokens -- the reference samples (scheduled sampling :260-270,
 * multinomial sample :623-631) from the very distribution it differentiates.  Hosts pass drop_lm = 0 outside
 * training mode. */
size_t rfn_decoder_step_ws_bytes(const rfn_dims* d, int B);
size_t rfn_decoder_cproj_floats(const rfn_dims* d, int B);
int rfn_decoder_prepare(const rfn_dims* d, int B, const float* const* params, const float* comb,
                        float* cproj, void* stream);
int rfn_decoder_step(const rfn_dims* d, int B, const float* const* params, const float* comb,
                     const float* cproj, const int64_t* ids, float* h, float* c, float* logits,
                     float* logp, int64_t ld_logp /* row stride of logp, >= V1 */, void* ws,
                     size_t ws_bytes, uint64_t seed, int step, void* stream);
/* The same step fed with an already embedded token xt (B, E) -- the literal signature of the reference's
 * one_time_step(xt, thought_vectors_comb, state) (misc/RecurrentFusionModel.py:345-350), whose callers do
 * xt = model.embed(it) themselves (eval_utils.py:368,516,539). */
int rfn_decoder_step_embedded(const rfn_dims* d, int B, const float* const* params, const float* comb,
                              const float* cproj, const float* xt, int64_t ld_xt, float* h, float* c,
                              float* logits, float* logp, int64_t ld_logp, void* ws, size_t ws_bytes,
                              uint64_t seed, int step, void* stream);

/* ---- whole decode loops queued by ONE call: the device-resident decoder loop (SURVEY.md 8b "decoder_loop") ------------
 * Each is the sequence of per-step launches its host loop would issue (embedding K10, decoder cell a5, logit +
 * log-softmax K11, the pick / beam bookkeeping between steps) with the host removed from the loop: nothing is read back,
 * nothing is decided on the host between steps, results are bit for bit those of the step-by-step calls.
 * They are NOT one persistent kernel, on purpose: a decoder step is three dependent all-to-all products, and on MI355X a
 * grid-wide barrier inside a launch (4-7 us) costs more than the kernel boundary it replaces (1.5-2 us) -- the same
 * trade the in-launch split-K finish lost when it was measured (RFN_GEMM_OPT_SPLITK_IN_KERNEL); DESIGN.md section 13.
 *
 * rfn_decoder_loop: sample() free-running decode (misc/RecurrentFusionModel.py:616-653), `steps` = seq_length + 1 steps.
 *   mode 0 greedy (argmax of the previous step's log-probs, first maximum), mode 1 multinomial (inverse-CDF draw with the
 *   caller's uniforms u[(t-1) * B + b], temperature 1 / inv_temperature).  h, c: decoder state in / out (B, R).
 *   logp_all[b * ld_b + t * ld_t + v]: log-probs of step t.  seq / seq_lp (B, steps - 1) with row strides ld_seq / ld_lp:
 *   token (0 once the row has finished) and its log-prob per step, as :647-649.  unf (steps, B) int32: unfinished flags
 *   per step (row 0 unused), for the caller's single early-exit read-back (:645).  ids: B int64 of scratch (last fed
 *   tokens).  ws: rfn_decoder_step_ws_bytes. */
int rfn_decoder_loop(const rfn_dims* d, int B, int steps, const float* const* params, const float* comb,
                     const float* cproj, float* h, float* c, int mode, float inv_temperature, const float* u,
                     float* logp_all, int64_t ld_b, int64_t ld_t, int64_t* seq, int64_t ld_seq, float* seq_lp,
                     int64_t ld_lp, int32_t* unf, int64_t* ids, void* ws, size_t ws_bytes, uint64_t seed, void* stream);
/* rfn_decoder_fwd_sampled: the step-wise TRAINING decoder with draws between the steps (scheduled sampling :260-270 with
 *   probability ss_prob; ss_prob = 1: the multinomial sample() with grad, train_rl.py:160) = rfn_decoder_fwd_begin + S x
 *   (rfn_multinomial_pick, rfn_decoder_fwd_step).  ids (B, S) in / out (column 0 = BOS is never redrawn); u_draw, u_coin
 *   (S, B) uniforms in [0, 1) (row 0 unused).  Leaves the workspace ready for rfn_decoder_bwd. */
int rfn_decoder_fwd_sampled(const rfn_dims* d, int B, int S, const float* const* params, const float* comb,
                            const float* h0, const float* c0, int64_t* ids, int64_t ld_ids, float ss_prob,
                            float inv_temperature, const float* u_draw, const float* u_coin, float* log_prob, void* ws,
                            size_t ws_bytes, int train, uint64_t seed, void* stream);
/* rfn_beam_loop: sample_beam's search (:451-531) for NB images x W beams: S x (rfn_beam_step, two rfn_gather_rows,
 *   rfn_decoder_step on the NB * W rows, ending in rfn_log_softmax_topk instead of the full log-softmax).  comb (T2, NB, R)
 *   and cproj = rfn_decoder_prepare(d, NB, ...) are per IMAGE: the W beam rows of image k read row k (the reference feeds
 *   beam_size copies of the image's thought vectors, :417-420).  h / c
 *   (NB * W, R) in / out, h_alt / c_alt same-size scratch, logp: 2 * NB * W * W floats of scratch (the rows' top-W lists);
 *   the beam / done arrays as rfn_beam_step (zero-initialised by the caller; active = 1). */
int rfn_beam_loop(const rfn_dims* d, int NB, int W, int S, const float* const* params, const float* comb,
                  const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp, int64_t* beam_seq,
                  float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids, int64_t* done_seq, float* done_lp,
                  float* done_p, int32_t* done_n, int32_t* active, int max_done, void* ws, size_t ws_bytes, uint64_t seed,
                  void* stream);

/* The same loops under decoding constraints (above): per step one rfn_decode_blocklist, then rfn_logp_mask_rows before the pick
 * (rfn_decoder_loop_ex: the masked entries of logp_all read -inf afterwards) or rfn_log_softmax_topk_masked in place of
 * rfn_log_softmax_topk (rfn_beam_loop_ex).  A row left without any unblocked token picks token 0, as rfn_greedy_pick does on
 * a row of -inf (a multinomial draw of such a row keeps the token the row fed last).  cons == NULL: the calls and the bits
 * of rfn_decoder_loop / rfn_beam_loop, which forward here.  rfn_decoder_loop_ex needs steps - 1 <= 64 with constraints. */
int rfn_decoder_loop_ex(const rfn_dims* d, int B, int steps, const float* const* params, const float* comb,
                        const float* cproj, float* h, float* c, int mode, float inv_temperature, const float* u,
                        float* logp_all, int64_t ld_b, int64_t ld_t, int64_t* seq, int64_t ld_seq, float* seq_lp,
                        int64_t ld_lp, int32_t* unf, int64_t* ids, void* ws, size_t ws_bytes, uint64_t seed,
                        const rfn_decode_constraints* cons, void* stream);
/* rfn_decoder_loop_ex with truncated sampling and n draws per image.  Per step t >= 1: rfn_decode_blocklist and
 * rfn_logp_mask_rows (cons), rfn_logp_truncate_rows (mode 1 only: the argmax is always kept), rfn_multinomial_pick,
 * rfn_pick_record; the cut entries of logp_all read -inf afterwards.  rows_per_image = n > 1: B counts ROWS, B % n == 0, row
 * k * n + j is draw j of image k and reads image k's thought vectors: comb is (T2, B / n, R) and cproj comes from
 * rfn_decoder_prepare(d, B / n, ...), as for the beam rows of rfn_beam_loop; h / c are (B, R), u and the workspace as for B
 * rows.  n > 1 needs the hoisted decoder cell (RFN_ERR_UNSUPPORTED with RFN_PATH_OPT_DEC_UNHOISTED or the persistent decoder
 * chains).  samp == NULL: rfn_decoder_loop_ex, which forwards here. */
int rfn_decoder_loop_ex2(const rfn_dims* d, int B, int steps, const float* const* params, const float* comb,
                         const float* cproj, float* h, float* c, int mode, float inv_temperature, const float* u,
                         float* logp_all, int64_t ld_b, int64_t ld_t, int64_t* seq, int64_t ld_seq, float* seq_lp,
                         int64_t ld_lp, int32_t* unf, int64_t* ids, void* ws, size_t ws_bytes, uint64_t seed,
                         const rfn_decode_constraints* cons, const rfn_decode_sampling* samp, void* stream);
int rfn_beam_loop_ex(const rfn_dims* d, int NB, int W, int S, const float* const* params, const float* comb,
                     const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp, int64_t* beam_seq,
                     float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids, int64_t* done_seq, float* done_lp,
                     float* done_p, int32_t* done_n, int32_t* active, int max_done, void* ws, size_t ws_bytes, uint64_t seed,
                     const rfn_decode_constraints* cons, void* stream);
/* rfn_beam_loop_ex as a diverse beam search (above): rfn_beam_step_div in place of rfn_beam_step_topk, on the same top-W lists;
 * div->done_group (NB, max_done) receives the group of every done beam.  div == NULL or div->groups == 1: the calls and the
 * bits of rfn_beam_loop_ex, which forwards here.  RFN_ERR_SHAPE as rfn_beam_step_div; RFN_ERR_ARG: groups > 1 without done_group. */
int rfn_beam_loop_ex2(const rfn_dims* d, int NB, int W, int S, const float* const* params, const float* comb,
                      const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp, int64_t* beam_seq,
                      float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids, int64_t* done_seq, float* done_lp,
                      float* done_p, int32_t* done_n, int32_t* active, int max_done, void* ws, size_t ws_bytes, uint64_t seed,
                      const rfn_decode_constraints* cons, const rfn_beam_diversity* div, void* stream);
/* rfn_beam_loop_ex2 as a lexically constrained search (above): per step rfn_log_softmax_topk_want in place of
 * rfn_log_softmax_topk_masked and rfn_beam_step_lex in place of rfn_beam_step_topk; W counts all rows of an image (2^C states of
 * W / 2^C beams).  cons composes: a blocked token is -inf in the lists and in the want values.  lex == NULL: the calls and the bits
 * of rfn_beam_loop_ex2, which forwards here.  RFN_ERR_UNSUPPORTED: lex with div->groups > 1.  RFN_ERR_SHAPE as rfn_beam_step_lex
 * (and n_sets < 1, n_want < 1); RFN_ERR_ARG: a NULL member of lex. */
int rfn_beam_loop_ex3(const rfn_dims* d, int NB, int W, int S, const float* const* params, const float* comb,
                      const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp, int64_t* beam_seq,
                      float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids, int64_t* done_seq, float* done_lp,
                      float* done_p, int32_t* done_n, int32_t* active, int max_done, void* ws, size_t ws_bytes, uint64_t seed,
                      const rfn_decode_constraints* cons, const rfn_beam_diversity* div, const rfn_beam_lexical* lex,
                      void* stream);
/* rfn_beam_loop_ex3 as a stochastic beam search (above): per step rfn_beam_step_sbs in place of rfn_beam_step_topk and
 * rfn_log_softmax_topk_gumbel in place of rfn_log_softmax_topk_masked (and one rfn_beam_sbs_begin before the first step), the two rfn_gather_rows and the optional rfn_decode_blocklist
 * as they were -- the launch count per step is the plain search's.  beam_sum, the done-beam arrays and active are not used and may
 * be NULL with sbs; beam_seq / beam_lp are required.  cons composes (the weights are then relative, see above).  sbs == NULL: the
 * calls and the bits of rfn_beam_loop_ex3, which forwards here.  RFN_ERR_UNSUPPORTED: sbs with div->groups > 1 or with lex;
 * RFN_ERR_SHAPE: S > 64; RFN_ERR_ARG: a NULL member of sbs. */
int rfn_beam_loop_ex4(const rfn_dims* d, int NB, int W, int S, const float* const* params, const float* comb,
                      const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp, int64_t* beam_seq,
                      float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids, int64_t* done_seq, float* done_lp,
                      float* done_p, int32_t* done_n, int32_t* active, int max_done, void* ws, size_t ws_bytes, uint64_t seed,
                      const rfn_decode_constraints* cons, const rfn_beam_diversity* div, const rfn_beam_lexical* lex,
                      const rfn_beam_stochastic* sbs, void* stream);

/* ---- self-critical reward: CIDEr-D of token-id captions (get_rewards.py:39-112, cider/pyciderevalcap/ciderD) ---------
 * CiderD(n=4, sigma) as compute_reward calls it (csrc/rfn_reward.hip).  A caption is the ids of its row up to and including
 * the first 0, or all of them when there is none (array_to_str); the end token 0 is a word.  Score row r is caption
 * res[r, :T_res] of image row_img[r], scored against references gts[row_img[r], j, :T_gt] for j < n_refs[image].
 * Document frequencies:
 *   - corpus mode (table == NULL): df[g] = sum over images whose references contain g of the number of score rows pointing at
 *     that image, ref_len = log(n_rows) -- compute_reward's crefs, one entry per score row;
 *   - table mode: a table built by rfn_ciderd_table_build (the reference's df='coco-train-idxs' pickle), ref_len =
 *     log(ref_docs) (113287 for coco-train, 123287 for coco-all, 5000 for coco-val).
 * Arithmetic is fp64 in fixed orders: scores are bitwise reproducible run to run; the only atomics are integer df counts.
 * A row whose caption, or one of whose image's references, holds an id outside [0, vocab] (or whose row_img / n_refs is out of
 * range) scores NaN; other rows are unaffected (a bad reference's n-grams are left out of the corpus df).
 * Limits (RFN_ERR_SHAPE otherwise): 1 <= T_res, T_gt <= 64, 1 <= max_refs <= 32, 0 <= vocab <= 32767.
 * Four launches in corpus mode, three in table mode; no allocation, no synchronisation (capturable in a graph).
 * res, gts: int64; row_img (n_rows), n_refs (n_img): int32; scores: n_rows doubles; ws: rfn_ciderd_ws_bytes, 16-B aligned.
 * table: rfn_ciderd_table_bytes(slots) bytes (slots a power of two).  ngram_ids: n_entries x 4 int32, the n-gram's ids
 * followed by -1 padding; counts: its df (doubles).  Keys must be unique; entries with an id above vocab are skipped.  At most
 * slots / 2 entries. */
size_t rfn_ciderd_ws_bytes(int n_rows, int T_res, int n_img, int max_refs, int T_gt, int corpus);
size_t rfn_ciderd_table_bytes(int64_t slots);
int rfn_ciderd_table_build(const int32_t* ngram_ids, const double* counts, int64_t n_entries, int vocab, void* table, int64_t slots,
                           void* stream);
int rfn_ciderd_score(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                     const int32_t* n_refs, int n_img, int max_refs, int T_gt, const void* table, int64_t slots, double ref_docs,
                     int vocab, double sigma, double* scores, void* ws, size_t ws_bytes, void* stream);
/* train_rl.py's reward from the scores of B sampled rows followed by B greedy rows: reward[b, :] = weight * (s[b] - s[B + b])
 * (use_baseline) or weight * s[b], broadcast over T; out (B, T) f32 and / or out64 (B, T) f64, either may be NULL. */
int rfn_scst_reward(const double* scores, int B, int T, double weight, int use_baseline, float* out, double* out64,
                    void* stream);

/* ---- self-critical reward: BLEU-D of token-id captions (cider/pyciderevalcap/bleuD, BleuD(4), option 'closest') ------------
 * The same captions, rows, references and limits as rfn_ciderd_score.  Per score row: testlen = the caption's word count (the
 * end token counts), guess[n] = max(0, testlen - n + 1), correct[n] = sum over the row's distinct n-grams of min(its count, the
 * largest count in any one reference of the image), reflen = the reference length closest to testlen (the shorter on a tie);
 * scores[r, k] = (prod_{j <= k} (correct[j] + 1e-15) / (guess[j] + 1e-9)) ^ (1 / (k + 1)), times exp(1 - 1 / ratio) when
 * ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1.  corpus: the same formula over the sums of the rows' components.
 * Integer counting, then fp64 in one thread per row: bitwise reproducible, no atomics.  A row whose caption, or one of whose
 * image's references, holds an id outside [0, vocab] (or whose row_img / n_refs is out of range) scores NaN in all four
 * columns, has zero components and is left out of the corpus sums; other rows are unaffected.
 * Two launches, a third when corpus != NULL; no allocation, no synchronisation (capturable in a graph).
 * scores: n_rows x 4 doubles; comps: NULL or n_rows x 10 int32 (testlen, reflen, guess[4], correct[4]); corpus: NULL or 4
 * doubles; ws: rfn_bleud_ws_bytes (0 for sizes outside the limits; T_res takes part in the limits only), 16-B aligned. */
size_t rfn_bleud_ws_bytes(int n_rows, int T_res, int n_img, int max_refs, int T_gt);
int rfn_bleud_score(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                    const int32_t* n_refs, int n_img, int max_refs, int T_gt, int vocab, double* scores, int32_t* comps,
                    double* corpus, void* ws, size_t ws_bytes, void* stream);
/* compute_reward's mix of the two: reward[b, :] = ((b4 * bleu4_weight) + (c * cider_weight)) + 0.0 with b4 = bleu[b, 3] -
 * bleu[B + b, 3] and c = cider[b] - cider[B + b] (use_baseline) or the sampled row's score alone; every product and sum is
 * rounded on its own, as numpy does.  cider: NULL or 2B doubles, bleu: NULL or 2B x 4 doubles (not both NULL); a NULL term is
 * the 0 * weight the reference adds.  out (B, T) f32 and / or out64 (B, T) f64, either may be NULL. */
int rfn_scst_reward_mix(const double* cider, double cider_weight, const double* bleu, double bleu4_weight, int B, int T,
                        int use_baseline, float* out, double* out64, void* stream);

/* ---- validation captions (eval_utils.language_eval: coco-caption/pycocoevalcap Bleu(4), Rouge(), Cider()) -------------------
 * eval_utils.decode_sequence stops BEFORE the first 0, so a validation caption carries no end token.  The _ex forms of the two
 * score calls take flags: with RFN_CAPTION_END_EXCLUDED a hypothesis or reference is the ids strictly before its first 0 (all
 * T when there is none) and may be empty; without it they are rfn_ciderd_score / rfn_bleud_score bit for bit.  An empty
 * hypothesis scores like pycocoevalcap's (BLEU 0 through its brevity penalty, CIDEr 0, ROUGE-L 0); an image with an empty
 * reference (which the loader never produces) is treated like one with an out-of-range id: its rows score NaN.  Unknown flag
 * bits: RFN_ERR_ARG.  Cider() is rfn_ciderd_score_ex in corpus mode with one score row per image (df per image, ref_len =
 * log(n_img)); Bleu(4)'s corpus four are the `corpus` output. */
#define RFN_CAPTION_END_EXCLUDED 1u
int rfn_ciderd_score_ex(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                        const int32_t* n_refs, int n_img, int max_refs, int T_gt, const void* table, int64_t slots, double ref_docs,
                        int vocab, double sigma, unsigned flags, double* scores, void* ws, size_t ws_bytes, void* stream);
int rfn_bleud_score_ex(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                       const int32_t* n_refs, int n_img, int max_refs, int T_gt, int vocab, unsigned flags, double* scores,
                       int32_t* comps, double* corpus, void* ws, size_t ws_bytes, void* stream);
/* ROUGE-L (rouge/rouge.py): lcs[r, j] = the length of the longest common subsequence of row r's caption and reference j of its
 * image (integer, one 64-bit bit-vector recurrence per pair); p = max_j lcs / len(caption), q = max_j lcs / len(reference j);
 * scores[r] = (1 + beta^2) p q / (q + beta^2 p) when both are non-zero, else 0 (beta: 1.2 in the reference; must be > 0).
 * Captions, rows, references, limits, flags and the NaN rule as above (both caption conventions).  One launch, one fp64 formula
 * per row, no atomics: bitwise reproducible; no allocation, no synchronisation (capturable in a graph).
 * scores: n_rows doubles; lcs: NULL or n_rows x max_refs int32 (0 behind an image's references and on a NaN row); ws:
 * rfn_rougel_ws_bytes (0 outside the limits, else one 256-byte block: the single launch keeps nothing in it), 16-B aligned. */
size_t rfn_rougel_ws_bytes(int n_rows, int T_res, int n_img, int max_refs, int T_gt);
int rfn_rougel_score(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                     const int32_t* n_refs, int n_img, int max_refs, int T_gt, int vocab, unsigned flags, double beta, double* scores,
                     int32_t* lcs, void* ws, size_t ws_bytes, void* stream);
/* The corpus mean of a score column: *mean = the mean of scores[0], scores[stride], ... (n values) that are not NaN (NaN when
 * none is left), *n_skipped (NULL or one int64) = how many were.  One workgroup, fp64 in a fixed order (strided partial sums,
 * then a binary tree): bitwise reproducible, no atomics.  n, stride >= 1 (RFN_ERR_SHAPE otherwise). */
int rfn_score_mean(const double* scores, int64_t n, int64_t stride, double* mean, int64_t* n_skipped, void* stream);

/* ---- multi-sample self-critical ------------------------------------------------------------------------------------------
 * train_rl.py:160-203 draws one caption per row and pays a second, greedy decode for the baseline.  Here n captions are drawn
 * per image and a draw's baseline is the mean score of the image's other n - 1 draws: no greedy pass, n policy-gradient samples
 * per run of stages I / II (misc/RecurrentFusionModel.py:199-255).
 *   Rows are image-major: row r = k * n + j is draw j of image k (as rows_per_image of rfn_decoder_loop_ex2 and the beam rows).
 *   B counts rows, B % n == 0, Bc = B / n counts images.
 *   comb is (T2, Bc, R).  h0 and c0 stay per row (B, R): the host fans them out and sums their gradients back.
 *   d_comb comes back (T2, Bc, R), already summed over each image's n rows.
 *   Dropout: stages I / II draw one mask per image (they run once per image); the decoder's mask is per ROW, counter b * R + unit
 *   with b the row (rfn_dropout_mask over B * R values at RFN_DROP_OFFSET_DECODER + step).
 *   Only the hoisted decoder cell has this form: RFN_PATH_OPT_DEC_UNHOISTED (or a persistent decoder chain) with n > 1 is
 *   RFN_ERR_UNSUPPORTED, as in rfn_decoder_loop_ex2.  n < 1 or B % n != 0: RFN_ERR_SHAPE (rfn_decoder_ws_bytes_ex: 0).
 * The _ex forms below are rfn_decoder_ws_bytes / _fwd / _fwd_sampled / _bwd (misc/RecurrentFusionModel.py:257-281, 623-631) with
 * rows_per_image = n; the old names forward with 1, and with 1 every launch and every bit is theirs.
 *   Forward: att_2_att_h(comb) and U = comb . z2h.weight^T (misc/LSTMSoftAttentionCore.py:64-66, 81) are computed once per image
 *   (T2 * Bc GEMM rows); every step's cell reads them at image b / n (rfn_dec_cell_fwd's row_div).  Everything else is per row,
 *   so a row's log-probs are the bits of the old call on comb physically repeated n times.
 *   Backward: the sweep as before with rfn_dec_attn_bwd_ex(row_div = n), d Pd kept per row; then rfn_dec_du_ex (sum over j, s as
 *   documented there), rfn_rowgroup_sum of d Pd onto the images (j ascending), d_comb = dPd_img . W_att + dU . W_z over T2 * Bc
 *   rows, and d att_2_att_h / d z2h.weight from dPd_img / dU against comb over T2 * Bc rows.  All other gradients are per row.
 *   The workspace grows by the per-image d Pd (T2 * Bc * A floats) when n > 1; Pd, U and dU shrink to Bc rows.  The logits-only
 *   form (log_prob == NULL, rfn_decoder_logits) exists for one row per image only: RFN_ERR_ARG with n > 1. */
size_t rfn_decoder_ws_bytes_ex(const rfn_dims* d, int B, int S, int train, int rows_per_image);
int rfn_decoder_fwd_ex(const rfn_dims* d, int B, int S, const float* const* params, const float* comb /* (T2,B/n,R) */,
                       const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids, float* log_prob, void* ws,
                       size_t ws_bytes, int train, uint64_t seed, int rows_per_image, void* stream);
int rfn_decoder_fwd_sampled_ex(const rfn_dims* d, int B, int S, const float* const* params, const float* comb,
                               const float* h0, const float* c0, int64_t* ids, int64_t ld_ids, float ss_prob,
                               float inv_temperature, const float* u_draw, const float* u_coin, float* log_prob, void* ws,
                               size_t ws_bytes, int train, uint64_t seed, int rows_per_image, void* stream);
int rfn_decoder_bwd_ex(const rfn_dims* d, int B, int S, const float* const* params, const float* comb,
                       const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids, const float* log_prob,
                       const float* d_log_prob, float* d_comb /* (T2,B/n,R) */, float* d_h0, float* d_c0,
                       float* const* grads, void* ws, size_t ws_bytes, uint64_t seed, int rows_per_image, void* stream);
/* The leave-one-out reward (compute_reward's mix, get_rewards.py:39-112, with the grouped baseline in place of the greedy row).
 * For a score vector s of B rows and group size n:
 *   baseline 1 (leave-one-out, n >= 2): base[k*n+j] = (((0.0 + s[k*n+i0]) + s[k*n+i1]) + ...) / (n - 1) over i != j ascending;
 *                                       diff = s - base.        baseline 0 (none): diff = s.
 *   reward[r, :] = ((diff_bleu4[r] * bleu4_weight) + (diff_cider[r] * cider_weight)) + 0.0, broadcast over T.
 * Every sum, product and quotient is rounded on its own in fp64 (no contraction; the division is correctly rounded).  A NULL
 * scorer is the reference's 0 * weight.  A NaN score poisons its image's group through the arithmetic, and only that group.
 * cider: NULL or B doubles; bleu: NULL or B x 4 doubles (column 3 is used); out (B, T) f32 = the cast of out64 (B, T) f64, either
 * may be NULL.  One launch, no allocation, no synchronisation (capturable in a graph).
 * RFN_ERR_SHAPE: B < 1, T < 1, n < 1, B % n != 0, baseline not 0 or 1, n == 1 with baseline 1.  RFN_ERR_ARG: both scores NULL or
 * both outputs NULL. */
int rfn_scst_reward_group(const double* cider, double cider_weight, const double* bleu, double bleu4_weight, int B, int n, int T,
                          int baseline, float* out, double* out64, void* stream);
/* The logits-only pair with n rows per image (additive: rfn_decoder_fwd_ex / _bwd_ex keep refusing log_prob == NULL with n > 1).
 * rfn_decoder_logits_fwd issues rfn_decoder_fwd_ex's launches as far as the logit product and leaves the time-major rows
 * r = t * B + b at rfn_decoder_logits_ex(d, B, S, train, n, ws) (row stride V1); the workspace is rfn_decoder_ws_bytes_ex(d, B, S,
 * train, n) bytes and train = 1 keeps what the backward needs.  rfn_decoder_logits_bwd is rfn_decoder_bwd_ex started from the
 * d loss / d logits a criterion left over those rows (rfn_xe_logits_bwd, rfn_rl_logits_bwd): the log-softmax backward is the only
 * step that reads log_prob, everything behind it takes its row counts from B and n.  d_comb comes back (T2, B / n, R), summed
 * over each image's rows.  n > 1 needs the hoisted cell (RFN_ERR_UNSUPPORTED), shapes and pointers are checked as in the _ex
 * forms. */
int rfn_decoder_logits_fwd(const rfn_dims* d, int B, int S, const float* const* params, const float* comb /* (T2,B/n,R) */,
                           const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids, void* ws, size_t ws_bytes,
                           int train, uint64_t seed, int rows_per_image, void* stream);
float* rfn_decoder_logits_ex(const rfn_dims* d, int B, int S, int train, int rows_per_image, void* ws);
int rfn_decoder_logits_bwd(const rfn_dims* d, int B, int S, const float* const* params, const float* comb, const int64_t* ids,
                           int64_t ld_ids, float* d_comb /* (T2,B/n,R) */, float* d_h0, float* d_c0, float* const* grads, void* ws,
                           size_t ws_bytes, uint64_t seed, int rows_per_image, void* stream);
/* The reward of a DISTINCT-sample set: the n rows of image k are a sample without replacement (stochastic beam search) with
 * importance weights w (rfn_beam_step_sbs's `weight`, B doubles).  The normalised importance-weighted policy-gradient estimator
 * with its built-in baseline (Kool, van Hoof and Welling, "Stochastic Beams and Where to Find Them", ICML 2019).  With
 * s_j = ((bleu4_j * bleu4_weight) + (cider_j * cider_weight)) + 0.0 (a NULL scorer is 0 * weight), over the rows of the image
 * with w_j > 0 only, j ascending:
 *   Wsum = ((0.0 + w_j0) + w_j1) + ...        q_j = w_j / Wsum        base = ((0.0 + q_j0 * s_j0) + q_j1 * s_j1) + ...  (baseline 1)
 *   reward[k*n+j, :] = (q_j * (s_j - base)) * n, broadcast over T;      baseline 0: base = 0.
 * Rows with w_j <= 0 (dead rows, the threshold row) or a NaN weight enter no sum and get exactly 0.0 whatever their score; an
 * image without a weighted row, or with a non-finite Wsum, gets zeros.  The factor n puts the reward on the group step's scale:
 * the criterion divides by B = images * n, and sum_j q_j stands where the group step has (1 / n) sum_j.  A NaN score on a
 * weighted row poisons its own image only.  fp64, every sum, product and quotient rounded on its own; out / out64 as above; one
 * launch, no allocation, no synchronisation.
 * RFN_ERR_SHAPE: B < 1, T < 1, n < 1, B % n != 0, baseline not 0 or 1, baseline 1 with n < 3 (n = 2 leaves one weighted row,
 * whose coefficient is identically 0).  RFN_ERR_ARG: both scores NULL, weight NULL or both outputs NULL. */
int rfn_scst_reward_distinct(const double* cider, double cider_weight, const double* bleu, double bleu4_weight, const double* weight,
                             int B, int n, int T, int baseline, float* out, double* out64, void* stream);

/* ---- consensus reranking (minimum-Bayes-risk decoding under CIDEr-D; off by default, the reference has none) ---------------------
 * Of the n candidate captions of an image, keep the one that agrees most with the others under CIDEr-D (csrc/rfn_reward.hip).
 * Inputs: cands (n_img, n, T) int64 ids; n_cand (n_img) int32, only the first n_cand[k] candidates of image k are valid (NULL:
 * all n); weights (n_img, n) fp64 (NULL: every weight is 1); the df source, sigma, vocab and flags as rfn_ciderd_score_ex takes
 * them (RFN_CAPTION_END_EXCLUDED is honoured).
 *   Pairwise utility: U[k][i][j] is what rfn_ciderd_score_ex returns for the one row cands[k][i] against the single reference
 *   cands[k][j]: the per-order clipped similarity, divided by both norms only when both are non-zero, times the Gaussian length
 *   penalty, then ((((0 + s0) + s1) + s2) + s3) / 4 * 10, fp64 in that scorer's summation orders (both kernels run one device
 *   function per pair).  The diagonal is computed like any other entry; U is not symmetric (min(w_h, w_r) * w_r).
 *   df source: table mode as rfn_ciderd_score_ex, with the caller's ref_docs.  Corpus mode (table == NULL): a document is an
 *   image, df(g) = the sum of n_cand[k] over the images whose valid candidates hold g, ref_docs = the sum of all n_cand[k] --
 *   exactly what rfn_ciderd_score_ex computes in corpus mode when the compacted valid candidates are passed as `res` and the
 *   candidates as `gts`.  So in both modes the mean over the valid j of U[k][i][j] is that call's score of candidate i (up to the
 *   last rounding).  An image whose n_cand is outside [1, n] adds nothing to either sum; an image that is bad for another reason
 *   adds its n_cand to ref_docs and nothing to df, as a bad image's rows do there.
 *   Consensus score: c[k][i] = (sum_{j != i, j < n_cand[k]} w_j * U[k][i][j]) / (sum_{j != i} w_j), j ascending, each product, each
 *   sum and the quotient rounded on its own (no contraction).  A weight sum of 0 (which includes n_cand[k] = 1) gives c = 0.
 *   Pick: best[k] = the lowest i with c[k][i] equal to the maximum.
 *   Bad inputs: a valid candidate holding an id outside [0, vocab], a negative or NaN weight on a valid candidate, n_cand[k]
 *   outside [1, n], or (under RFN_CAPTION_END_EXCLUDED) an empty valid candidate make all of image k's c and U NaN and best[k] = -1;
 *   other images are unaffected.  Entries of c and U at or beyond n_cand[k] are NaN.
 *   Limits (RFN_ERR_SHAPE otherwise; rfn_consensus_ws_bytes: 0): 1 <= T <= 64, 1 <= n <= 32, 0 <= vocab <= 32767 -- the reward's,
 *   whose n-gram packing is shared.  Checks in rfn_ciderd_score_ex's precedence: shape, then arg (unknown flag bits; cands, c,
 *   best or ws NULL, ws not 16-B aligned), then workspace.
 * Launches: the candidate counts, [clear the corpus df], cook the candidates once (as references), their tf-idf vectors and norms,
 * the pairs (one workgroup per (image, candidate)), the pick (one wave per image): 5 in table mode, 6 in corpus mode.  No
 * floating-point atomics, fixed orders: bitwise repeatable.  No allocation, no synchronisation (capturable in a graph).
 * U: NULL or n_img * n * n doubles; c: n_img * n doubles; best: n_img int64. */
size_t rfn_consensus_ws_bytes(int n_img, int n, int T, int corpus);
int rfn_consensus_ciderd(const int64_t* cands, int n_img, int n, int T, const int32_t* n_cand, const double* weights,
                         const void* table, int64_t slots, double ref_docs, int vocab, double sigma, unsigned flags, double* U,
                         double* c, int64_t* best, void* ws, size_t ws_bytes, void* stream);
/* The pick's gather as a launch of its own: row best[k] of image k's n rows goes to row k of the output, for each array pair
 * given: seq (n_img, n, S) int64 -> (n_img, S), lp (n_img, n, S) f32 -> (n_img, S), p (n_img, n) f32 -> (n_img).  best[k] outside
 * [0, n) (a bad image's -1) writes zeros.  RFN_ERR_SHAPE: n_img, n or S < 1; RFN_ERR_ARG: best NULL, no pair given, or a pair
 * with only one side. */
int rfn_consensus_gather(const int64_t* best, int n_img, int n, int S, const int64_t* seq_in, int64_t* seq_out, const float* lp_in,
                         float* lp_out, const float* p_in, float* p_out, void* stream);

/* ---- caption-set diversity (how different an image's n captions are from each other; the reference has nothing of the kind) -------
 * Div-m, mBLEU and Self-CIDEr of caption sets, from the candidates cooked once as consensus reranking cooks them
 * (csrc/rfn_reward.hip).  Inputs: cands (n_img, n, T) int64 ids, n_cand (n_img) int32 (NULL: all n), the df source, sigma, vocab and
 * flags exactly as rfn_consensus_ciderd takes them (corpus mode counts the df from the candidates as that call does).
 *   Bad images: n_cand[k] outside [1, n], a valid candidate holding an id outside [0, vocab], or (RFN_CAPTION_END_EXCLUDED) an empty
 *   valid candidate -- rfn_consensus_ciderd's conditions.  Every double output of a bad image is NaN, every integer output 0; other
 *   images are unaffected (in corpus mode a bad image changes the df, as there).
 *   Div-m, m = 1..4: distinct[k][m-1] = the number of distinct m-grams over image k's valid candidates; words[k] = the sum of their
 *   word counts (a caption's words as the flags define them); div[k][m-1] = distinct / (1e-6 + words), one fp64 add and one
 *   division.  Defined for n_cand[k] = 1.
 *   mBLEU: row (k, i) is BLEU-D of candidate i against the references {cands[k][j] : j != i, j < n_cand[k]} by rfn_bleud_score's
 *   rules (clip each n-gram count against the largest count in any one reference; the closest reference length, the shorter on a
 *   tie; the same formula).  mbleu (n_img, n, 4); mbleu_comps (n_img, n, 10) int32 in rfn_bleud_score's component layout (zeros
 *   for a NaN row); mbleu_corpus (n, 4): row i is that formula over the integer sums of slot i's components across the images whose
 *   row (k, i) is not NaN, NaN when there is none.  Rows at or beyond n_cand[k], and the one row of an image with n_cand[k] = 1
 *   (nothing to compare with), are NaN and left out of the sums.  The reported mBleu_m is the mean of mbleu_corpus[:, m-1] over the
 *   slots that are not NaN.
 *   Self-CIDEr: U[k] is rfn_consensus_ciderd's pairwise utility with unit weights, the same bits.  K = (U + U^T) / 2 / 10 over the
 *   valid candidates ((U_ij + U_ji) / 2, then / 10; CIDEr-D clips, so U itself is not symmetric, and a number read off one triangle
 *   would change when the candidates are permuted).  eig (n_img, n): the eigenvalues of K ascending (fp64 cyclic Jacobi, fixed
 *   rotation order and stopping rule), NaN at or beyond n_cand[k].  Eigenvalues below 1e-12 * lambda_max count as 0 -- part of the
 *   definition: duplicate captions give exact zero eigenvalues that a solver returns as +-1e-16, whose square root would be 1e-8 of
 *   noise.  With s_i = sqrt(lambda_i) of what is left, summed ascending, self_cider[k] = -log(max_i s_i / sum_i s_i) / log(n_cand[k]);
 *   NaN when n_cand[k] = 1 or lambda_max <= 0.
 *   Limits and checks: rfn_consensus_ciderd's (RFN_ERR_SHAPE outside 1 <= T <= 64, 1 <= n <= 32, 0 <= vocab <= 32767, and
 *   rfn_capset_ws_bytes returns 0; then RFN_ERR_ARG for unknown flag bits, cands or ws NULL, ws not 16-B aligned; then
 *   RFN_ERR_WORKSPACE).  Every output pointer may be NULL, and a NULL output skips its launches: distinct / words / div need the
 *   cooking and one launch (one workgroup per image); the mbleu outputs one launch (one workgroup per (image, candidate)) plus one
 *   for mbleu_corpus; U the tf-idf vectors and the pairs; eig / self_cider U (kept in the workspace when U is NULL) and one launch
 *   (one wave per image).  Integer outputs are exact; fp64 in fixed orders, no floating-point atomics: bitwise repeatable, and in
 *   table mode an image's outputs do not depend on the batch around it.  No allocation, no synchronisation (capturable). */
size_t rfn_capset_ws_bytes(int n_img, int n, int T, int corpus);
int rfn_capset_diversity(const int64_t* cands, int n_img, int n, int T, const int32_t* n_cand, const void* table, int64_t slots,
                         double ref_docs, int vocab, double sigma, unsigned flags, int32_t* distinct, int32_t* words, double* div,
                         double* mbleu, int32_t* mbleu_comps, double* mbleu_corpus, double* U, double* eig, double* self_cider,
                         void* ws, size_t ws_bytes, void* stream);
/* Best-of-n, its lowest index and mean-of-n of a score column: scores[(k * n + j) * stride] is the score of candidate j of image k;
 * over j < n_cand[k] (NULL: n) best[k] = the maximum, arg[k] = its lowest index, mean[k] = the sum (ascending, from 0.0) divided
 * once by n_cand[k].  One NaN among an image's valid entries, or n_cand[k] outside [1, n], gives NaN, -1, NaN.  Any output may be
 * NULL.  One launch.  RFN_ERR_SHAPE: n_img, n or stride < 1; RFN_ERR_ARG: scores NULL or every output NULL. */
int rfn_score_group_stats(const double* scores, int64_t stride, int n_img, int n, const int32_t* n_cand, double* best, int64_t* arg,
                          double* mean, void* stream);

/* ---- caption scoring (how likely the model finds a caption it is GIVEN; the reference has nothing of the kind) ------------------
 * The decoding entry points produce captions; these score given ones: per position the log-prob of the given token, its rank in
 * the step's distribution and the distribution's entropy, per caption the sum and the length -- straight from the logits rows, so
 * the (rows, S, V+1) log-prob tensor that rfn_decoder_fwd + a gather would write and read back is never materialised
 * (csrc/rfn_score.hip; one block of 256 per row, the row read once).
 *   logits: time-major rows r = i * B + b (i < T) of V1 floats, row stride ldl >= V1: steps t0 .. t0+T-1 of B captions.
 *   target (B, ld_target) int64: column t is the token scored at step t.  An id outside [0, V1) reads as 0, everywhere below.
 *   Live rule: position (b, t) is LIVE iff target[b, t'] != 0 for every t' < t, and (include_end != 0 or target[b, t] != 0).
 *   include_end = 1 covers a caption's words and its first 0 (the positions the XE criterion's mask covers); 0 the words only
 *   (eval_utils' sum(seqLogprobs * (seq > 0))).  Whatever follows the first 0 is never live.
 *   Outputs at [b * ld_out + t], t = t0 + i, with x the row and tg = target[b, t]:
 *     tok_lp   = x[tg] - lse, lse the row's log-sum-exp: the bits rfn_log_softmax_fwd writes for that entry       dead: 0
 *     tok_rank = #{v : x[v] > x[tg] or (x[v] == x[tg] and v < tg)}  (may be NULL)                                   dead: -1
 *                Tie rule: the position of tg in a stable descending sort of the row, 0 = the argmax -- the order of
 *                rfn_log_softmax_topk's lists.
 *     tok_ent  = -sum_v p_v * (x[v] - lse), p_v = exp(x[v] - lse), entries with p_v == 0 count 0  (may be NULL)    dead: 0
 *   A dead position's block returns before it reads its logits row.  Reductions run in a fixed order (no float atomics): the
 *   outputs are a function of the row alone, whatever B, T or t0 -- one step at a time (T = 1, t0 = t) gives the bits of one call.
 *   A row holding a NaN gives NaN tok_lp / tok_ent and a rank that counts only the comparisons that are true; other rows are
 *   unaffected.  A -inf target gives tok_lp = -inf; -inf entries leave the entropy finite.
 *   RFN_ERR_SHAPE: B, T or V1 <= 0, t0 < 0, ldl < V1, ld_out < t0 + T.  RFN_ERR_ARG: logits, target or tok_lp NULL. */
int rfn_score_logits(const float* logits, int64_t ldl, int B, int T, int t0, int V1, const int64_t* target,
                     int64_t ld_target, int include_end, float* tok_lp, int32_t* tok_rank, float* tok_ent,
                     int64_t ld_out, void* stream);
/* Summation order: cap_lp[b] = ((0.0 + tok_lp[b,0]) + tok_lp[b,1]) + ... over the LIVE positions t < T ascending, in fp64, one IEEE
 * add each (a host loop over the same floats reproduces it exactly); cap_len[b] (may be NULL) = the number of live positions.  One
 * thread per caption.  RFN_ERR_SHAPE: B, T or V1 <= 0, ld_lp < T.  RFN_ERR_ARG: tok_lp, target or cap_lp NULL. */
int rfn_score_captions(const float* tok_lp, int64_t ld_lp, const int64_t* target, int64_t ld_target, int B, int T, int V1,
                       int include_end, double* cap_lp, int32_t* cap_len, void* stream);
/* The whole pass: rfn_decoder_fwd_ex's teacher-forced pass with train = 0 -- no dropout, whatever d->drop_lm says -- and
 * rows_per_image = n as far as the time-major logits, rfn_score_logits over all S * B rows (T = S, t0 = 0), and rfn_score_captions
 * when cap_lp is given.  Log-probs are never written; a position's tok_lp is the bits rfn_decoder_fwd_ex's log_prob holds there.
 *   ids (B, ld_ids): column s is the token fed at step s (column 0 = BOS); target (B, ld_target): column s is scored at step s.  The
 *   two may be views of one matrix M (B, S + 1) with column 0 = BOS: ids = M, target = M + 1, the same stride.
 *   comb (T2, B / n, R), h0 / c0 (B, R), rows image-major, as rfn_decoder_fwd_ex; n > 1 needs the hoisted cell
 *   (RFN_ERR_UNSUPPORTED otherwise); n < 1 or B % n != 0: RFN_ERR_SHAPE (rfn_decoder_score_ws_bytes: 0).
 *   tok_lp (B, ld_out >= S); tok_rank, tok_ent, cap_lp, cap_len may be NULL (cap_len needs cap_lp).
 *   The workspace is rfn_decoder_ws_bytes_ex(d, B, S, 0, n): its logits slab is S * B * V1 floats, so a host bounds it by
 *   splitting the rows between images -- no bit changes, the batched products are never split along K. */
size_t rfn_decoder_score_ws_bytes(const rfn_dims* d, int B, int S, int rows_per_image);
int rfn_decoder_score(const rfn_dims* d, int B, int S, const float* const* params, const float* comb /* (T2, B/n, R) */,
                      const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids /* column s feeds step s */,
                      const int64_t* target, int64_t ld_target /* column s is scored at step s */, int include_end,
                      float* tok_lp, int32_t* tok_rank, float* tok_ent, int64_t ld_out, double* cap_lp, int32_t* cap_len,
                      void* ws, size_t ws_bytes, int rows_per_image, void* stream);

/* ---- mixture of softmaxes (opts.py --use_mos / --num_expert; misc/MixtureOfSoftmax.py) ------------------------------------------
 * An output head that replaces log_softmax(logit(h)): K experts tanh(Linear(h)) share one vocabulary projection, a softmax prior
 * over the experts mixes their softmaxes.  Per hidden row h (R floats), with the reference's state_dict names:
 *   c_k    = prior.weight[k] . h                           log pi_k = c_k - LSE_j c_j
 *   z_k    = tanh(latent.k.0.weight . h + latent.k.0.bias)                                  (E floats)
 *   x_kv   = decoder.weight[v] . z_k + decoder.bias[v]     lse_k = LSE_v x_kv
 *   a_kv   = log pi_k + x_kv - lse_k
 *   logp_v = LSE_k a_kv
 * The reference takes log(sum_k pi_k softmax(x_k)) in linear f32 space, which is -inf where the sum underflows; the log-sum-exp
 * form is the same function and stays finite for every finite input.
 * Backward, G_v = dL / dlogp_v:  r_kv = exp(a_kv - logp_v), p_kv = exp(x_kv - lse_k), s_k = sum_v G_v r_kv,
 *   dx_kv = G_v r_kv - p_kv s_k,  dc_k = s_k - pi_k sum_j s_j;  dz, dh and the parameter gradients follow by the chain rule.
 * Loss form: G_v = -(g / B) * mask * q_v with q the one-hot or label-smoothed target of rfn_xe_logits_* (targets clamped alike).
 *
 * Parameters and gradients: arrays of device pointers in state_dict order -- prior.weight (K, R); latent.k.0.weight (E, R) and
 * latent.k.0.bias (E) for k < K; decoder.weight (V1, E); decoder.bias (V1) -- rfn_mos_param_count = 2 K + 3 slots, names and
 * shapes as rfn_param_name / rfn_param_shape give them (cols = 1 for a bias).  1 <= K <= RFN_MOS_MAXK, R, E >= 1, V1 >= 2:
 * RFN_ERR_SHAPE otherwise (rfn_mos_ws_bytes: 0).
 *
 * Workspace (rfn_mos_ws_bytes(md, rows, train) bytes, 16-B aligned; every slab rounded up to 64 floats):
 *   c (rows, K) | log pi (rows, K) | lse (K, rows) | z (K, rows, E) | x (K, rows, V1)
 *   train: + d z (K, rows, E) | d c (rows, K) | 64 MiB of split-K scratch for the weight gradients.
 * Expert k's rows lie at row k * rows + r of z and x, so the vocabulary projection is ONE product over K * rows rows.  No softmax
 * of any expert is written: the mix kernels (one block of 256 per hidden row) take the K log-sum-exps, then stream the K expert
 * rows once more, 16 B per lane when V1 % 4 == 0, V1 <= 10240 and the outputs are 16-B aligned with strides % 4 == 0, element-wise
 * otherwise.  Reductions run in a fixed order: results are bitwise reproducible.
 *
 * rfn_mos_fwd: h (rows, ldh >= R) -> logp, row r at logp + (r % inner) * out_s_inner + (r / inner) * out_s_outer (the remap of
 *   rfn_log_softmax_fwd: time-major rows r = s * B + b reach a (B, S, V1) tensor with inner = B, strides S * V1 and V1).  The
 *   workspace keeps c, log pi, lse, z and x for rfn_mos_bwd whatever `train` is; `train` only sizes the backward's slabs.
 * rfn_mos_loss_fwd: the masked, label-smoothed NLL of rfn_xe_logits_fwd straight from x, for time-major rows r = t * B + b:
 *   loss_out[0] (+)= -sum mask * q . logp / B, summed in rfn_xe_logits_fwd's order; logp is never written.  scratch: B * T floats.
 * rfn_mos_bwd: from d_logp (laid out as rfn_mos_fwd's logp) on the workspace either forward left.  Writes d x over x, then
 *   d_h (rows, R) and every gradient slot (overwritten).  rfn_mos_loss_bwd: the same from (target, mask, eps, gscale *
 *   gscale_dev[0]) on rfn_mos_loss_fwd's (or rfn_mos_fwd's) workspace; a row whose mask is 0 gets exactly zero in d x, d c and d_h.
 *   Both need a workspace of the train size.
 * RFN_ERR_SHAPE: rows (B, T) < 1, ldh < R, inner < 1, eps outside [0, 1).  RFN_ERR_ARG: a NULL pointer (gscale_dev may be
 * NULL), a workspace that is not 16-B aligned.  RFN_ERR_WORKSPACE: ws_bytes below rfn_mos_ws_bytes. */
#define RFN_MOS_MAXK 16
typedef struct rfn_mos_dims {
    int32_t R, E, K, V1;
} rfn_mos_dims;
int rfn_mos_param_count(const rfn_mos_dims* md);
int rfn_mos_param_name(const rfn_mos_dims* md, int idx, char* buf, size_t buflen);
int rfn_mos_param_shape(const rfn_mos_dims* md, int idx, int64_t* rows, int64_t* cols);
size_t rfn_mos_ws_bytes(const rfn_mos_dims* md, int64_t rows, int train);
/* addresses inside a workspace of `rows` rows: lse (K, rows), log pi (rows, K), x (K, rows, V1), d c (rows, K; train) */
float* rfn_mos_ws_lse(const rfn_mos_dims* md, int64_t rows, void* ws);
float* rfn_mos_ws_logpi(const rfn_mos_dims* md, int64_t rows, void* ws);
float* rfn_mos_ws_x(const rfn_mos_dims* md, int64_t rows, void* ws);
float* rfn_mos_ws_dc(const rfn_mos_dims* md, int64_t rows, void* ws);
int rfn_mos_fwd(const rfn_mos_dims* md, int rows, const float* h, int64_t ldh, const float* const* params, int inner,
                int64_t out_s_inner, int64_t out_s_outer, float* logp, void* ws, size_t ws_bytes, int train, void* stream);
int rfn_mos_loss_fwd(const rfn_mos_dims* md, int B, int T, const float* h, int64_t ldh, const float* const* params,
                     const int64_t* target, int64_t ld_target, const float* mask, int64_t ld_mask, float eps, float* scratch,
                     float* loss_out, int accumulate_loss, void* ws, size_t ws_bytes, void* stream);
int rfn_mos_bwd(const rfn_mos_dims* md, int rows, const float* h, int64_t ldh, const float* const* params, const float* d_logp,
                int inner, int64_t s_inner, int64_t s_outer, float* d_h, float* const* grads, void* ws, size_t ws_bytes,
                void* stream);
int rfn_mos_loss_bwd(const rfn_mos_dims* md, int B, int T, const float* h, int64_t ldh, const float* const* params,
                     const int64_t* target, int64_t ld_target, const float* mask, int64_t ld_mask, float eps, float gscale,
                     const float* gscale_dev, float* d_h, float* const* grads, void* ws, size_t ws_bytes, void* stream);

/* The decoder path beside such a head (additive; rfn_decoder_fwd_ex / _bwd_ex keep their launches and bits):
 * rfn_decoder_fwd_hidden is rfn_decoder_fwd_ex (one row per image) stopped before the logit product; rfn_decoder_hidden returns
 * the address of the (S * B, R) time-major rows r = s * B + b the logit layer would read -- under dropout the dropped-out
 * outputs (misc/LSTMSoftAttentionCore.py:98-101).  rfn_decoder_bwd_hidden is rfn_decoder_bwd_ex started from d_hidden (S * B, R)
 * in place of the log-softmax and logit-layer backward: the logit.* gradient slots are zero-filled, everything else is
 * overwritten as there.  The workspace is rfn_decoder_ws_bytes's.  RFN_ERR_UNSUPPORTED with RFN_PATH_OPT_DEC_UNHOISTED or a
 * persistent decoder chain (RFN_PATH_OPT_PERSIST_DEC_*). */
int rfn_decoder_fwd_hidden(const rfn_dims* d, int B, int S, const float* const* params, const float* comb, const float* h0,
                           const float* c0, const int64_t* ids, int64_t ld_ids, void* ws, size_t ws_bytes, int train,
                           uint64_t seed, void* stream);
float* rfn_decoder_hidden(const rfn_dims* d, int B, int S, int train, void* ws);
int rfn_decoder_bwd_hidden(const rfn_dims* d, int B, int S, const float* const* params, const float* comb, const float* h0,
                           const float* c0, const int64_t* ids, int64_t ld_ids, const float* d_hidden, float* d_comb,
                           float* d_h0, float* d_c0, float* const* grads, void* ws, size_t ws_bytes, uint64_t seed,
                           void* stream);

/* ---- attention maps (where the model looked when it wrote a word; the reference never returns its attention weights) ------------
 * Every forward kernel writes its softmax weights because the backward needs them; these entry points hand them out and compose
 * the three levels into one word-to-region map per (caption row, encoder) (csrc/rfn_attnmap.hip).  Notation: T1, T2, M, L_i of
 * rfn_dims; rows = B * n caption rows, image-major, image k = row / n; S decoder steps.
 *
 * Accessors: addresses inside the workspace of a FINISHED forward pass, valid until the next call on that workspace.
 *   rfn_prefix_alpha1(d, B, train, i, ws): a1_i[t1, b, l], (T1, B, L_i) contiguous -- stage I, encoder i over its regions; under
 *     ragged maps (rfn_prefix_fwd_ex with att_len) columns l >= the image's length hold exact zeros.
 *   rfn_prefix_alpha2(d, B, train, ws):    a2[t2, i, b, t1], (T2, M, B, T1) contiguous -- stage II over encoder i's thought vectors.
 *   rfn_decoder_alpha(d, B, S, train, n, ws): aD[s, row, t2], (S, B, T2) contiguous, B counting rows -- the decoder over the fused
 *     thought vectors, from rfn_decoder_fwd[_ex] / _fwd_hidden / _logits_fwd / rfn_decoder_score.
 *   (d, B, S, train, n) are those of the pass.  Workspaces of BOTH sizes keep every step's weights at the same offsets, and every
 *   form of the passes (persistent chains, the un-hoisted decoder cell) writes them there, so an inference-size pass (train = 0)
 *   suffices; a caller that wants inference weights passes dims whose dropout probabilities are 0.  NULL for bad dims, B or S < 1,
 *   an encoder outside [0, M), n that does not divide B, or ws == NULL.  No existing entry point changed for these.
 *
 * rfn_attn_rollout, one launch per encoder: for every row r, k = r / n, every step s < S and every region l < L
 *   G[r, s, l] = sum_{t2 < T2} aD[s, r, t2] * ( sum_{t1 < T1} a2[t2, k, t1] * a1[t1, k, l] )
 *   in exactly this nesting, both sums ascending from 0.f (products may be contracted into the adds); no atomics: two runs give
 *   the same bits.  Rows of row-stochastic inputs give a row-stochastic G.  This composes attention WEIGHTS only; it is not a
 *   gradient attribution (the LSTM states carry information too).
 *   aD at aD[s * d_ss + r * d_sr + t2]; a2 (this encoder's slab) at a2[t2 * a2_st + k * a2_sb + t1] -- for the accessor's layout
 *   a2 = rfn_prefix_alpha2(..) + i * B * T1, a2_st = M * B * T1, a2_sb = T1; a1 at a1[t1 * a1_st + k * a1_sb + l]; out at
 *   out[r * o_sr + s * o_ss + l], unit stride in l.
 *   len (rows,) int32 or NULL (every step live), clamped to [0, S]: steps s >= len[r] are written as exact zeros, and a row with
 *   len 0 loads nothing.  att_len (rows / n,) int32 or NULL, clamped to [1, L] as the ragged forward clamps it: columns
 *   l >= att_len[k] are written as exact zeros and a1 is not loaded there.
 *   One wave per (row, tile of 256 columns): 16 B per lane where L % 4 == 0, a1 and out are 16-B aligned and a1_st, a1_sb, o_sr,
 *   o_ss are multiples of 4; element-wise with 64-column tiles otherwise (same sums, same bits).  The row's aD (S x T2), the
 *   image's a2 (T2 x T1) and the inner sums of the tile (T2 x tile) are staged in LDS; the a1 rows of a tile are read once.
 *   LDS limit: (S * T2 + T2 * T1 + T2 * tile) floats (the first two rounded up to 4) <= 64 KiB.  A map that qualifies for the
 *   16-B form but whose 256-column tile does not fit takes the 64-column element-wise form; what does not fit that either is
 *   RFN_ERR_UNSUPPORTED -- there is no kernel without the LDS stage.
 *   Checks, in this order: RFN_ERR_SHAPE for rows, n, S, T1, T2 or L < 1, rows % n != 0, o_sr or o_ss < L, d_sr < T2,
 *   a2_sb < T1, a1_sb or a1_st < L; RFN_ERR_ARG for aD, a2, a1 or out NULL; then RFN_ERR_UNSUPPORTED.
 *
 * rfn_attn_map_stats, one launch per encoder over G (G[r * g_sr + s * g_ss + l]); per (row, step), at [r * S + s]:
 *   peak int32: the first argmax over l;  entropy f32: -sum_l G log G in nats, 0 log 0 = 0;  mass f32: the sum of G[r, s, l] over the
 *   l with region_mask[r * m_sr + s * m_ss + l] != 0 (uint8) -- written only when a mask is given (mass may then not be NULL).
 *   Dead steps (s >= len[r]) get peak = -1, entropy = 0, mass = 0 and their map row is not read.  One wave per (row, step), lane-
 *   strided partial sums then xor shuffles: a fixed order.  RFN_ERR_SHAPE: rows, S or L < 1, g_sr or g_ss < L, with a mask m_sr or
 *   m_ss < L.  RFN_ERR_ARG: G, peak or entropy NULL, a mask without mass.
 *
 * rfn_attn_decoder_copy: out[r * o_sr + s * o_ss + t2] = s < len[r] ? aD[s * d_ss + r * d_sr + t2] : 0 -- the decoder weights
 *   caption-major with the rollout's zeroing; dead steps are not loaded.  RFN_ERR_SHAPE: rows, S or T2 < 1, d_sr, o_sr or o_ss < T2.
 *   RFN_ERR_ARG: aD or out NULL.
 * No allocation, no synchronisation (capturable in a graph). */
float* rfn_prefix_alpha1(const rfn_dims* d, int B, int train, int enc, void* ws);
float* rfn_prefix_alpha2(const rfn_dims* d, int B, int train, void* ws);
float* rfn_decoder_alpha(const rfn_dims* d, int B, int S, int train, int rows_per_image, void* ws);
int rfn_attn_rollout(const float* aD, int64_t d_ss, int64_t d_sr, const float* a2, int64_t a2_st, int64_t a2_sb, const float* a1,
                     int64_t a1_st, int64_t a1_sb, const int32_t* len, const int32_t* att_len, int rows, int n, int S, int T1, int T2,
                     int L, float* out, int64_t o_sr, int64_t o_ss, void* stream);
int rfn_attn_map_stats(const float* G, int64_t g_sr, int64_t g_ss, const int32_t* len, const uint8_t* region_mask, int64_t m_sr,
                       int64_t m_ss, int rows, int S, int L, int32_t* peak, float* entropy, float* mass, void* stream);
int rfn_attn_decoder_copy(const float* aD, int64_t d_ss, int64_t d_sr, const int32_t* len, int rows, int S, int T2, float* out,
                          int64_t o_sr, int64_t o_ss, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RFN_H_ */
