// Phase 2, training: the teacher-forced attention-LSTM decoder (embed -> cell steps -> logit + log_softmax), its step-wise form for
// scheduled sampling and its backward pass.  decoder_cell_core is also the cell of the free-running step (rfn_path_decode.hip).
#include "rfn_path.h"

// =============================================================================================
// phase 2: teacher-forced decoder
// =============================================================================================
// single-encoder forms of the fused small-L attention (decoder: one attention over the T2 fused thoughts)
static int attn1_fwd(const float* proj, long psb, long psl, const float* hp, const float* w, const float* bo,
                     const float* x, long sb, long sl, int B, int L, int A, int D, float* al, float* z, long ldz,
                     void* st) {
    return rfn_attn_small_fwd(1, &proj, psb, psl, &hp, &w, &bo, &x, sb, sl, B, L, A, D, &al, &z, ldz, st);
}
static int attn1_bwd(const float* proj, long psb, long psl, const float* hp, const float* w, const float* al,
                     const float* x, long sb, long sl, const float* dz, long lddz, int B, int L, int A, int D,
                     float* dproj, long dpsb, long dpsl, int acc, float* dhp, float* dwp, float* dx, void* st) {
    return rfn_attn_small_bwd(1, &proj, psb, psl, &hp, &w, &al, &x, sb, sl, &dz, lddz, B, L, A, D, &dproj, dpsb, dpsl,
                              acc, &dhp, &dwp, &dx, st);
}

// rows_per_image = n > 1 (rfn.h "multi-sample self-critical"): the rows k * n .. k * n + n - 1 are n draws of image k and read
// its thought vectors; comb, Pd, U, dU and d_comb count the Bc = B / n images, everything else the B rows.  Hoisted cell only.
static int rows_per_image_ok(const rfn_dims* d, int B, int n) {
    if (n < 1 || B % n) return RFN_ERR_SHAPE;
    return (n > 1 && !dec_hoisted(d)) ? RFN_ERR_UNSUPPORTED : RFN_OK;
}
extern "C" size_t rfn_decoder_ws_bytes_ex(const rfn_dims* d, int B, int S, int train, int rows_per_image) {
    if (check_dims(d) != RFN_OK || B < 1 || S < 1 || rows_per_image < 1 || B % rows_per_image) return 0;
    return decoder_layout(d, B, S, train, rows_per_image).total * sizeof(float);
}
extern "C" size_t rfn_decoder_ws_bytes(const rfn_dims* d, int B, int S, int train) {
    return rfn_decoder_ws_bytes_ex(d, B, S, train, 1);
}

// One decoder cell call on given buffers (g already holds i2h(x)): h_2_att_h(h), attention over the fused thoughts,
// h2h(h) + z2h(z) accumulated onto the gates, LSTM update with the dropout mask of (seed, step).  Shared by the batched,
// the step-wise and the free-running pass, so the three are bit-identical by construction.
// K1 of every form: h_2_att_h(h) and g += h2h(h) in one launch (they share h).
static void decoder_k1(const rfn_dims* d, const float* const* prm, const float* h, float* hp, float* g, rfn_cell_out* k1) {
    const PIdx P(d);
    const int R = d->R, A = d->A, GD = gate_width(d->decoder_maxout, R);
    k1[0] = cell_out(hp, A, A, 0);
    cell_lin(k1[0], h, R, prm[P.dec(8)], R, R, prm[P.dec(9)]);
    k1[1] = cell_out(g, GD, GD, 1);
    cell_lin(k1[1], h, R, prm[P.dec(2)], R, R, prm[P.dec(3)]);
}
// The fused three-launch form of that step, prepared: K1; the attention; K3 = g += z2h(z) with the LSTM update as its epilogue.
// h_next / c_next may alias h / c (free-running step).  false: the cell GEMM cannot take the step (maxout, widths).
static bool decoder_cell_prepare(const rfn_dims* d, int B, const float* const* prm, const float* comb, const float* cproj,
                                 const float* h, const float* c, float* h_next, float* c_next, float* hp, float* al, float* z,
                                 float* g, RfnSeed seed, int step, ChainStep* cs) {
    const PIdx P(d);
    const int R = d->R, A = d->A, T2 = d->T2;
    const int GD = gate_width(d->decoder_maxout, R);
    const long BR = (long)B * R, BA = (long)B * A;
    if (d->decoder_maxout) return false;
    rfn_cell_out k1[2], k3;
    decoder_k1(d, prm, h, hp, g, k1);
    k3 = cell_out(g, GD, GD, 1);
    cell_lin(k3, z, R, prm[P.dec(4)], R, R, prm[P.dec(5)]);
    cell_lstm(k3, c, R, c_next, R, h_next, R, OFF_DECODER + (uint64_t)step);
    if (!cell_ok(B, 2, k1, R) || !cell_ok(B, 1, &k3, R)) return false;
    const float *w = prm[P.dec(10)], *bo = prm[P.dec(11)];
    return cell_prepare(B, 2, k1, R, 0.f, RfnSeed{}, &cs->g0, cell_variant(d)) == RFN_OK &&
           rfn_attn_small_prepare_fwd(1, &cproj, A, BA, &hp, &w, &bo, &comb, R, BR, B, T2, A, R, &al, &z, R, &cs->at) == RFN_OK &&
           cell_prepare(B, 1, &k3, R, d->drop_lm, seed, &cs->g2, cell_variant(d)) == RFN_OK;
}

// Hoisted form (default, rfn_deccell.hip; 2 launches): K1, then ONE per-row launch = scores, softmax,
// gates += b_z + sum_l alpha_l U_l, LSTM update.  `U` = comb . W_z^T (Bc = B / row_div rows per thought vector; the rows
// b of one beam-search image share row b / row_div of cproj / U).  z is not computed.
// Otherwise the three-launch form, or -- when the cell GEMM refuses it -- its products on the plain GEMM.
int rfn_path::decoder_cell_core(const rfn_dims* d, int B, const float* const* prm, const float* comb, const float* cproj,
                                const float* U, int row_div, const float* h, const float* c, float* h_next, float* c_next,
                                float* hp, float* al, float* z, float* g, const GemmCtx& gx, RfnSeed seed, int step, void* st) {
    const PIdx P(d);
    const int R = d->R, A = d->A, T2 = d->T2;
    const int GD = gate_width(d->decoder_maxout, R);
    const long BR = (long)B * R, BA = (long)B * A;
    rfn_cell_out k1[2];
    if (dec_hoisted(d)) {
        const int Bc = B / row_div;
        decoder_k1(d, prm, h, hp, g, k1);
        if (cell_ok(B, 2, k1, R)) {
            RFN_TRY(cell_run(B, 2, k1, R, 0.f, RfnSeed{}, st, cell_variant(d)));
        } else {
            RFN_TRY(gemm1(B, A, k1[0].seg[0], hp, A, 0, gx));
            RFN_TRY(gemm1(B, GD, k1[1].seg[0], g, GD, 1, gx));
        }
        return rfn_dec_cell_fwd(cproj, A, (long)Bc * A, hp, prm[P.dec(10)], prm[P.dec(11)], U, GD, (long)Bc * GD, prm[P.dec(5)], g,
                                GD, c, R, c_next, R, h_next, R, al, B, T2, A, R, d->decoder_maxout, row_div, d->drop_lm, seed,
                                OFF_DECODER + (uint64_t)step, st);
    }
    if (row_div != 1) return RFN_ERR_UNSUPPORTED;   // the three-launch form reads comb per row
    {
        ChainStep cs;
        if (decoder_cell_prepare(d, B, prm, comb, cproj, h, c, h_next, c_next, hp, al, z, g, seed, step, &cs))
            return rfn_chain_run(&cs, 1, 0, nullptr, st);   // one step: its three launches
    }
    decoder_k1(d, prm, h, hp, g, k1);
    RFN_TRY(gemm1(B, A, k1[0].seg[0], hp, A, 0, gx));
    RFN_TRY(attn1_fwd(cproj, A, BA, hp, prm[P.dec(10)], prm[P.dec(11)], comb, R, BR, B, T2, A, R, al, z, R, st));
    const rfn_gemm_seg segs[2] = {k1[1].seg[0], seg_lin(z, R, prm[P.dec(4)], R, R, prm[P.dec(5)])};
    RFN_TRY(gemm_segs(B, GD, 2, segs, g, GD, 1, gx));
    return rfn_lstm_fwd(g, GD, c, R, c_next, R, h_next, R, B, R, d->decoder_maxout, d->drop_lm, seed,
                        OFF_DECODER + (uint64_t)step, st);
}

// The slabs of step s on the training workspace (gd[s] already holds i2h(x_s))
struct DecStepBufs {
    float *h, *c, *hp, *al, *z, *g;
    DecStepBufs(const rfn_dims* d, int B, int s, float* W, const DecoderLayout& Lo)
        : h(W + Lo.hd + s * (long)B * d->R), c(W + Lo.cd + s * (long)B * d->R), hp(W + Lo.hpd + s * (long)B * d->A),
          al(W + Lo.ald + (long)s * B * d->T2), z(W + Lo.zd + s * (long)B * d->R),
          g(W + Lo.gd + (long)s * B * gate_width(d->decoder_maxout, d->R)) {}
};
// The decoder cell of step s: h_2_att_h, attention over the fused thoughts, h2h + z2h accumulated onto the gates, LSTM
// epilogue with the dropout mask of (seed, s).
static int decoder_fwd_cell(const rfn_dims* d, int B, int n, int s, const float* const* prm, const float* comb, float* W,
                            const DecoderLayout& Lo, const GemmCtx& gx, RfnSeed seed, void* st) {
    const DecStepBufs b(d, B, s, W, Lo);
    const long BR = (long)B * d->R;
    return decoder_cell_core(d, B, prm, comb, W + Lo.Pd, W + Lo.Ud, n, b.h, b.c, b.h + BR, b.c + BR, b.hp, b.al, b.z, b.g, gx, seed, s, st);
}
// its three-launch form prepared instead of launched; false: the cell GEMM cannot take the step
static bool decoder_fwd_cell_prepare(const rfn_dims* d, int B, int s, const float* const* prm, const float* comb, float* W,
                                     const DecoderLayout& Lo, RfnSeed seed, ChainStep* cs) {
    const DecStepBufs b(d, B, s, W, Lo);
    const long BR = (long)B * d->R;
    return decoder_cell_prepare(d, B, prm, comb, W + Lo.Pd, b.h, b.c, b.h + BR, b.c + BR, b.hp, b.al, b.z, b.g, seed, s, cs);
}

// Loop-invariant part of phase 2: projection of the fused thoughts (applied once instead of every step) and the
// initial state.  The batched products of the pass (this projection, i2h, logits) are never split along K: the
// free-running step (rfn_decoder_prepare / rfn_decoder_step) and the step-wise training pass (rfn_decoder_fwd_step)
// compute the same products for one step's rows with the same unsplit k order, so log-probs of the same tokens are
// bit-identical across all three whatever the batch size (split-K choices depend on the row count).  The per-step
// products (h_2_att_h, h2h + z2h) have the same shape everywhere and take the same split.
static int decoder_fwd_begin(const rfn_dims* d, int B, int n, const float* const* prm, const float* comb, const float* h0,
                             const float* c0, float* W, const DecoderLayout& Lo, void* st) {
    const PIdx P(d);
    const int R = d->R, A = d->A, T2 = d->T2, Bc = B / n;   // the projections: once per image
    const GemmCtx gx_whole{st, nullptr, 0, d->gemm_flags};
    RFN_TRY(gemm1(T2 * Bc, A, seg_lin(comb, R, prm[P.dec(6)], R, R, prm[P.dec(7)]), W + Lo.Pd, A, 0, gx_whole));
    if (dec_hoisted(d)) {   // U = comb . W_z^T, no bias: z2h of every thought vector, once (misc/LSTMSoftAttentionCore.py:78-81)
        const int GD = gate_width(d->decoder_maxout, R);
        RFN_TRY(gemm1(T2 * Bc, GD, seg_lin(comb, R, prm[P.dec(4)], R, R, nullptr), W + Lo.Ud, GD, 0, gx_whole));
    }
    return mem_batch({{W + Lo.hd, h0, (long)B * R}, {W + Lo.cd, c0, (long)B * R}}, st);
}

// The teacher-forced pass on a checked call: everything rfn_decoder_fwd_ex launches, on the workspace laid out as `Lo`.  log_prob
// == NULL stops at the time-major logits (W + Lo.logits), with any n: rfn_decoder_score reads them there.
static int decoder_fwd_body(const rfn_dims* d, int B, int S, int n, const float* const* prm, const float* comb, const float* h0,
                            const float* c0, const int64_t* ids, int64_t ld_ids, float* log_prob, float* W,
                            const DecoderLayout& Lo, RfnSeed seed, void* st, bool head = true) {
    const PIdx P(d);
    const int R = d->R, E = d->E, V1 = d->V1;
    const int GD = gate_width(d->decoder_maxout, R);
    const GemmCtx gx{st, W + Lo.gws, GEMM_WS_FLOATS * sizeof(float), d->gemm_flags};
    const GemmCtx gx_whole{st, nullptr, 0, d->gemm_flags};
    RFN_TRY(decoder_fwd_begin(d, B, n, prm, comb, h0, c0, W, Lo, st));
    // all token embeddings and their i2h projections in one go (teacher forcing: ids are known)
    RFN_TRY(rfn_embed_fwd(prm[P.embed()], E, V1, ids, B, ld_ids, 1, S * B, W + Lo.xs, E, st));
    RFN_TRY(gemm1(S * B, GD, seg_lin(W + Lo.xs, E, prm[P.dec(0)], E, E, prm[P.dec(1)]), W + Lo.gd, GD, 0, gx_whole));
    if (dec_hoisted(d)) {   // the S cell steps, two launches each (rfn_deccell.hip)
        for (int s = 0; s < S; ++s) RFN_TRY(decoder_fwd_cell(d, B, n, s, prm, comb, W, Lo, gx, seed, st));
    } else {   // three-launch form: one persistent launch (rfn_chain.hip) when every step takes the fused form, else step by step
        std::vector<ChainStep> steps((size_t)S);
        bool fused = true;
        for (int s = 0; s < S && fused; ++s) fused = decoder_fwd_cell_prepare(d, B, s, prm, comb, W, Lo, seed, &steps[s]);
        if (fused) {
            RFN_TRY(rfn_chain_run(steps.data(), S, chain_persist(d, RFN_PATH_OPT_PERSIST_DEC_FWD), (uint32_t*)(W + Lo.bar), st));
        } else {
            for (int s = 0; s < S; ++s) RFN_TRY(decoder_fwd_cell(d, B, 1, s, prm, comb, W, Lo, gx, seed, st));
        }
    }
    if (!head) return RFN_OK;   // rfn_decoder_fwd_hidden: another output layer reads the rows at W + Lo.hd + B * R
    // logits of all steps, then log-softmax written in the reference's (B, S, V+1) layout
    RFN_TRY(gemm_logits(S * B, V1, W + Lo.hd + (long)B * R, R, prm[P.logit_w()], prm[P.logit_b()], W + Lo.logits, gx_whole));
    if (log_prob) RFN_TRY(rfn_log_softmax_fwd(W + Lo.logits, V1, S * B, V1, B, (long)S * V1, V1, log_prob, st));
    return RFN_OK;      // log_prob == NULL: the logits stay in the workspace for rfn_xe_logits_fwd (rfn_decoder_logits)
}
extern "C" int rfn_decoder_fwd_ex(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb,
                                  const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids, float* log_prob,
                                  void* ws, size_t ws_bytes, int train, uint64_t seed_arg, int rows_per_image, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1 || S < 1) return RFN_ERR_SHAPE;
    const int n = rows_per_image;
    RFN_TRY(rows_per_image_ok(d, B, n));
    if (!prm || !comb || !h0 || !c0 || !ids || !ws) return RFN_ERR_ARG;
    if (n > 1 && !log_prob) return RFN_ERR_ARG;   // the logits-only form is found through rfn_decoder_logits: one row per image
    const DecoderLayout Lo = decoder_layout(d, B, S, train, n);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    return decoder_fwd_body(d, B, S, n, prm, comb, h0, c0, ids, ld_ids, log_prob, (float*)ws, Lo, seed, st);
}

// ---- caption scoring (rfn.h): the inference pass as far as the logits, then rfn_score_logits over all S * B rows -------------
// train = 0 and no dropout whatever d->drop_lm says (the key is never read); n rows per image reach the logits-only form here.
extern "C" size_t rfn_decoder_score_ws_bytes(const rfn_dims* d, int B, int S, int rows_per_image) {
    return rfn_decoder_ws_bytes_ex(d, B, S, 0, rows_per_image);
}
extern "C" int rfn_decoder_score(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb, const float* h0,
                                 const float* c0, const int64_t* ids, int64_t ld_ids, const int64_t* target, int64_t ld_target,
                                 int include_end, float* tok_lp, int32_t* tok_rank, float* tok_ent, int64_t ld_out,
                                 double* cap_lp, int32_t* cap_len, void* ws, size_t ws_bytes, int rows_per_image, void* st) {
    RFN_TRY(check_dims(d));
    if (B < 1 || S < 1 || ld_out < S) return RFN_ERR_SHAPE;
    const int n = rows_per_image;
    RFN_TRY(rows_per_image_ok(d, B, n));
    if (!prm || !comb || !h0 || !c0 || !ids || !target || !tok_lp || !ws || (cap_len && !cap_lp)) return RFN_ERR_ARG;
    rfn_dims dn = *d;
    dn.drop_lm = 0.f;
    const DecoderLayout Lo = decoder_layout(&dn, B, S, 0, n);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    float* W = (float*)ws;
    RFN_TRY(decoder_fwd_body(&dn, B, S, n, prm, comb, h0, c0, ids, ld_ids, nullptr, W, Lo, rfn_seed_value(0), st));
    RFN_TRY(rfn_score_logits(W + Lo.logits, dn.V1, B, S, 0, dn.V1, target, ld_target, include_end, tok_lp, tok_rank, tok_ent, ld_out, st));
    if (cap_lp) RFN_TRY(rfn_score_captions(tok_lp, ld_out, target, ld_target, B, S, dn.V1, include_end, cap_lp, cap_len, st));
    return RFN_OK;
}
extern "C" int rfn_decoder_fwd(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb,
                               const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids, float* log_prob,
                               void* ws, size_t ws_bytes, int train, uint64_t seed_arg, void* st) {
    return rfn_decoder_fwd_ex(d, B, S, prm, comb, h0, c0, ids, ld_ids, log_prob, ws, ws_bytes, train, seed_arg, 1, st);
}

// ---- the pass without its output layer (rfn.h "mixture of softmaxes"): the same launches as far as the last cell step -------
extern "C" int rfn_decoder_fwd_hidden(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb, const float* h0,
                                      const float* c0, const int64_t* ids, int64_t ld_ids, void* ws, size_t ws_bytes, int train,
                                      uint64_t seed_arg, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1 || S < 1) return RFN_ERR_SHAPE;
    if (!dec_hoisted(d)) return RFN_ERR_UNSUPPORTED;
    if (!prm || !comb || !h0 || !c0 || !ids || !ws) return RFN_ERR_ARG;
    const DecoderLayout Lo = decoder_layout(d, B, S, train, 1);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    return decoder_fwd_body(d, B, S, 1, prm, comb, h0, c0, ids, ld_ids, nullptr, (float*)ws, Lo, seed, st, false);
}
extern "C" float* rfn_decoder_hidden(const rfn_dims* d, int B, int S, int train, void* ws) {
    if (check_dims(d) != RFN_OK || B < 1 || S < 1 || !ws) return nullptr;
    return (float*)ws + decoder_layout(d, B, S, train).hd + (size_t)B * d->R;
}
// rfn.h "attention maps": the (S, B, T2) attention weights every form of the teacher-forced pass leaves in its workspace
extern "C" float* rfn_decoder_alpha(const rfn_dims* d, int B, int S, int train, int rows_per_image, void* ws) {
    if (check_dims(d) != RFN_OK || B < 1 || S < 1 || rows_per_image < 1 || B % rows_per_image != 0 || !ws) return nullptr;
    return (float*)ws + decoder_layout(d, B, S, train, rows_per_image).ald;
}

extern "C" float* rfn_decoder_logits(const rfn_dims* d, int B, int S, int train, void* ws) {
    if (check_dims(d) != RFN_OK || B < 1 || S < 1 || !ws) return nullptr;
    return (float*)ws + decoder_layout(d, B, S, train).logits;
}

// Step-wise form of the same pass for scheduled sampling (misc/RecurrentFusionModel.py:260-270): the token fed at
// step s may be drawn from the distribution of step s-1, so the host interleaves its draws with the steps.  begin +
// S steps leave the workspace and log_prob exactly as rfn_decoder_fwd on the final ids does (bit for bit), so
// rfn_decoder_bwd runs on it unchanged -- the sampled pass IS the differentiated pass, nothing is computed twice.
int rfn_path::decoder_fwd_begin_n(const rfn_dims* d, int B, int S, int n, const float* const* prm, const float* comb,
                                  const float* h0, const float* c0, void* ws, size_t ws_bytes, int train, void* st) {
    RFN_TRY(check_dims(d));
    if (B < 1 || S < 1) return RFN_ERR_SHAPE;
    RFN_TRY(rows_per_image_ok(d, B, n));
    if (!prm || !comb || !h0 || !c0 || !ws) return RFN_ERR_ARG;
    const DecoderLayout Lo = decoder_layout(d, B, S, train, n);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    return decoder_fwd_begin(d, B, n, prm, comb, h0, c0, (float*)ws, Lo, st);
}
extern "C" int rfn_decoder_fwd_begin(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb,
                                     const float* h0, const float* c0, void* ws, size_t ws_bytes, int train, void* st) {
    return decoder_fwd_begin_n(d, B, S, 1, prm, comb, h0, c0, ws, ws_bytes, train, st);
}

extern "C" int rfn_decoder_fwd_step(const rfn_dims* d, int B, int S, int s, const float* const* prm, const float* comb,
                                    const int64_t* ids_s, int64_t ld_ids, float* log_prob, void* ws, size_t ws_bytes,
                                    int train, uint64_t seed_arg, void* st) {
    return decoder_fwd_step_n(d, B, S, 1, s, prm, comb, ids_s, ld_ids, log_prob, ws, ws_bytes, train, seed_arg, st);
}
int rfn_path::decoder_fwd_step_n(const rfn_dims* d, int B, int S, int n, int s, const float* const* prm, const float* comb,
                                 const int64_t* ids_s, int64_t ld_ids, float* log_prob, void* ws, size_t ws_bytes,
                                 int train, uint64_t seed_arg, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1 || S < 1 || s < 0 || s >= S) return RFN_ERR_SHAPE;
    RFN_TRY(rows_per_image_ok(d, B, n));
    if (!prm || !comb || !ids_s || !log_prob || !ws) return RFN_ERR_ARG;
    const DecoderLayout Lo = decoder_layout(d, B, S, train, n);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    const PIdx P(d);
    const int R = d->R, E = d->E, V1 = d->V1;
    const int GD = gate_width(d->decoder_maxout, R);
    float* W = (float*)ws;
    const GemmCtx gx{st, W + Lo.gws, GEMM_WS_FLOATS * sizeof(float), d->gemm_flags};
    const GemmCtx gx_whole{st, nullptr, 0, d->gemm_flags};
    float* xs = W + Lo.xs + (long)s * B * E;
    float* lg = W + Lo.logits + (long)s * B * V1;
    RFN_TRY(rfn_embed_fwd(prm[P.embed()], E, V1, ids_s, B, ld_ids, 1, B, xs, E, st));
    RFN_TRY(gemm1(B, GD, seg_lin(xs, E, prm[P.dec(0)], E, E, prm[P.dec(1)]), W + Lo.gd + (long)s * B * GD, GD, 0, gx_whole));
    RFN_TRY(decoder_fwd_cell(d, B, n, s, prm, comb, W, Lo, gx, seed, st));
    RFN_TRY(gemm_logits(B, V1, W + Lo.hd + (long)(s + 1) * B * R, R, prm[P.logit_w()], prm[P.logit_b()], lg, gx_whole));
    return rfn_log_softmax_fwd(lg, V1, B, V1, B, (long)S * V1, V1, log_prob + (long)s * V1, st);
}

namespace {
// rfn_decoder_bwd's operands: the caller's arrays and the slabs of its workspace, shared by the two sweeps and the tail
struct DecBwd {
    const rfn_dims* d;
    const PIdx P;
    int B, n, Bc, S, R, A, E, T2, V1, GD;   // n rows per image, Bc = B / n images (rfn.h "multi-sample self-critical")
    long BR, BA;
    const float* const* prm;
    const float* comb;
    const int64_t* ids;
    int64_t ld_ids;
    float *d_comb, *d_h0, *d_c0;
    float* const* grd;
    float* W;
    DecoderLayout Lo;
    RfnSeed seed;
    void* st;
    GemmCtx gx;
    float *hd, *cd, *gd, *dhe, *dhrec, *dc, *dz, *dPd;

    // LSTM backward of step s as a launch of its own: d h = dhe[s] (the recurrent part already added), d c from step s + 1
    int lstm_bwd_of(int s) const {
        return rfn_lstm_bwd(gd + (long)s * B * GD, GD, cd + s * BR, R, cd + (s + 1) * BR, R, dhe + s * BR, R, (s < S - 1) ? dc : nullptr,
                            R, dc, R, B, R, d->decoder_maxout, d->drop_lm, seed, OFF_DECODER + (uint64_t)s, st);
    }
    // The product that ends a fused step of either form: d h_rec (+ `parts` partial slabs behind it) += d hproj_s . W_h, whose
    // epilogue completes d h of step s-1 (+ the logit layer's share dhe[s-1]) and runs that step's LSTM backward -- the next
    // thing the sweep needs.  Step 0's is a plain accumulate.
    void kb2_of(int s, int parts, rfn_cell_out& kb2) const {
        kb2 = cell_out(dhrec, R, R, 1);
        if (parts) {
            kb2.acc_slabs = dhrec + BR;
            kb2.acc_parts = parts;
            kb2.acc_stride = BR;
        }
        cell_dx(kb2, W + Lo.dhpd + s * BA, A, prm[P.dec(8)], R, A);
        if (s > 0)
            cell_lstm_bwd(kb2, gd + (long)(s - 1) * B * GD, GD, cd + (s - 1) * BR, R, cd + s * BR, R, dhe + (s - 1) * BR, R,
                          dc, R, dc, R, OFF_DECODER + (uint64_t)(s - 1));
    }
    // the hoisted attention backward of step s from that step's gate gradients: f = rfn_dec_attn_bwd_ex (last = the stream) or
    // rfn_dec_attn_bwd_args (last = the argument block, nothing launched)
    template <class F, class Last>
    int attn_bwd_hoisted(F f, int s, Last last) const {
        return f(W + Lo.Pd, A, (long)Bc * A, W + Lo.hpd + s * BA, prm[P.dec(10)], W + Lo.ald + (long)s * B * T2, W + Lo.Ud, GD,
                 (long)Bc * GD, gd + (long)s * B * GD, GD, B, n, T2, A, GD, dPd, A, BA, 1, W + Lo.dhpd + s * BA, W + Lo.dwp + s * BA,
                 last);
    }
    int attn_bwd_unhoisted(int s) const {
        return attn1_bwd(W + Lo.Pd, A, BA, W + Lo.hpd + s * BA, prm[P.dec(10)], W + Lo.ald + (long)s * B * T2, comb, R, BR, dz, R, B, T2,
                         A, R, dPd, A, BA, 1, W + Lo.dhpd + s * BA, W + Lo.dwp + s * BA, d_comb, st);
    }
    int sweep_hoisted() const;
    int sweep_unhoisted() const;
    int tail(bool hoisted) const;
};

// ---- z2h hoisted (rfn_deccell.hip): per step the attention backward from that step's gate gradients, then ONE product
// d h = [d gates_s | d hproj_s] . [W_hh ; W_h] whose epilogue finishes d h of step s-1 (+ the logit layer's share) and
// runs that step's LSTM backward.  d thoughts / d W_z / d att_2_att_h follow in the tail from dU and dPd.
// The fused form of a step, two launches: X = the step's attention-backward rows BESIDE the tiles of d gates_s . W_hh cut
// DEC_KSPLIT ways along K into partial slabs (neither depends on the other; one grid, rfn_cg_launch_with_rows), then
// Y = d hproj_s . W_h + the slabs (kb2_of).
int DecBwd::sweep_hoisted() const {
    RFN_TRY(mem_batch({{dPd, nullptr, (long)T2 * BA}}, st));
    auto kx_of = [&](int s, rfn_cell_out* kx) {
        const int Kp = GD / DEC_KSPLIT;
        for (int j = 0; j < DEC_KSPLIT; ++j) {
            kx[j] = cell_out(dhrec + (long)j * BR, R, R, 0);
            cell_dx(kx[j], gd + (long)s * B * GD + (long)j * Kp, GD, prm[P.dec(2)] + (long)j * Kp * R, R, Kp);
        }
    };
    rfn_cell_out kx[DEC_KSPLIT], ky;
    bool fused = !d->decoder_maxout && GD % (DEC_KSPLIT * 32) == 0;
    for (int s = 0; s < S && fused; ++s) {
        kx_of(s, kx);
        kb2_of(s, DEC_KSPLIT - 1, ky);
        fused = cell_ok(B, DEC_KSPLIT, kx, R) && cell_ok(B, 1, &ky, R);
    }
    if (fused) RFN_TRY(lstm_bwd_of(S - 1));   // the last step: nothing recurrent flows into it
    for (int s = S - 1; s >= 0; --s) {
        float* g = gd + (long)s * B * GD;
        float* dhp = W + Lo.dhpd + s * BA;
        if (!fused) {
            if (s < S - 1) RFN_TRY(rfn_axpby_2d(1.f, dhrec, R, 1.f, dhe + s * BR, R, B, R, st));
            RFN_TRY(lstm_bwd_of(s));
            RFN_TRY(attn_bwd_hoisted(rfn_dec_attn_bwd_ex, s, st));
            rfn_gemm_seg sg[2] = {seg_dx(g, GD, prm[P.dec(2)], R, GD), seg_dx(dhp, A, prm[P.dec(8)], R, A)};
            RFN_TRY(gemm_segs(B, R, 2, sg, dhrec, R, 0, gx));
            continue;
        }
        kx_of(s, kx);
        CgPrepared px;
        DecAttnBwdArgs da;
        RFN_TRY(cell_prepare(B, DEC_KSPLIT, kx, R, 0.f, RfnSeed{}, &px, cell_variant(d)));
        RFN_TRY(attn_bwd_hoisted(rfn_dec_attn_bwd_args, s, &da));
        const int rc = rfn_cg_launch_with_rows(px, da, B, st);
        if (rc == RFN_ERR_UNSUPPORTED) {   // shapes the fused grid does not take: the same two bodies as two launches
            RFN_TRY(attn_bwd_hoisted(rfn_dec_attn_bwd_ex, s, st));
            RFN_TRY(rfn_cg_launch(px, st));
        } else {
            RFN_TRY(rc);
        }
        kb2_of(s, DEC_KSPLIT - 1, ky);
        RFN_TRY(cell_run(B, 1, &ky, R, d->drop_lm, seed, st, cell_variant(d)));
    }
    return RFN_OK;
}

// ---- three-launch form (A/B hook; the persistent chain is built from it).  Fused form of a backward step: Kb1 =
// [dh_rec | dz] = dgates . [W_hh | W_z] in one launch (they share the gate gradients); the attention backward; Kb2 (kb2_of).
// Every step's operands are validated before the fused form is chosen (see the stage-II sweep in rfn_prefix_bwd).
int DecBwd::sweep_unhoisted() const {
    RFN_TRY(mem_batch({{d_comb, nullptr, (long)T2 * BR}, {dPd, nullptr, (long)T2 * BA}}, st));
    auto kb1_of = [&](int s, rfn_cell_out* kb1) {
        float* g = gd + (long)s * B * GD;
        kb1[0] = cell_out(dhrec, R, R, 0);
        cell_dx(kb1[0], g, GD, prm[P.dec(2)], R, GD);
        kb1[1] = cell_out(dz, R, R, 0);
        cell_dx(kb1[1], g, GD, prm[P.dec(4)], R, GD);
    };
    rfn_cell_out kb1[2], kb2;
    bool fused = !d->decoder_maxout;
    for (int s = 0; s < S && fused; ++s) {
        kb1_of(s, kb1);
        kb2_of(s, 0, kb2);
        fused = cell_ok(B, 2, kb1, R) && cell_ok(B, 1, &kb2, R);
    }
    if (fused) RFN_TRY(lstm_bwd_of(S - 1));   // the last step: nothing recurrent flows into it
    int s_hi = S - 1;
    if (fused && S >= 3) {
        // steps S-1 ... 1 share one form (Kb2 carries the LSTM backward of the step below): one persistent launch
        // (rfn_chain.hip); step 0, whose Kb2 is a plain accumulate, follows as its three launches
        std::vector<ChainStep> steps((size_t)(S - 1));
        bool ok = true;
        for (int s = S - 1; s >= 1 && ok; --s) {
            ChainStep& cs = steps[(size_t)(S - 1 - s)];
            kb1_of(s, kb1);
            kb2_of(s, 0, kb2);
            const float *proj = W + Lo.Pd, *hp = W + Lo.hpd + s * BA, *w = prm[P.dec(10)], *al = W + Lo.ald + (long)s * B * T2;
            const float *dzc = dz, *x = comb;
            float *dpr = dPd, *dhp = W + Lo.dhpd + s * BA, *dwp = W + Lo.dwp + s * BA, *dxc = d_comb;
            ok = cell_prepare(B, 2, kb1, R, 0.f, RfnSeed{}, &cs.g0, cell_variant(d)) == RFN_OK &&
                 rfn_attn_small_prepare_bwd(1, &proj, A, BA, &hp, &w, &al, &x, R, BR, &dzc, R, B, T2, A, R, &dpr, A, BA, 1, &dhp,
                                            &dwp, &dxc, &cs.at) == RFN_OK &&
                 cell_prepare(B, 1, &kb2, R, d->drop_lm, seed, &cs.g2, cell_variant(d)) == RFN_OK;
        }
        if (ok) {
            RFN_TRY(rfn_chain_run(steps.data(), S - 1, chain_persist(d, RFN_PATH_OPT_PERSIST_DEC_BWD), (uint32_t*)(W + Lo.bar), st));
            s_hi = 0;
        }
    }
    for (int s = s_hi; s >= 0; --s) {
        kb1_of(s, kb1);
        kb2_of(s, 0, kb2);
        if (fused) {
            RFN_TRY(cell_run(B, 2, kb1, R, 0.f, RfnSeed{}, st, cell_variant(d)));
            RFN_TRY(attn_bwd_unhoisted(s));
            RFN_TRY(cell_run(B, 1, &kb2, R, d->drop_lm, seed, st, cell_variant(d)));
            continue;
        }
        if (s < S - 1) RFN_TRY(rfn_axpby_2d(1.f, dhrec, R, 1.f, dhe + s * BR, R, B, R, st));
        RFN_TRY(lstm_bwd_of(s));
        const rfn_gemm_problem pr[2] = {prob1(dhrec, R, kb1[0].seg[0]), prob1(dz, R, kb1[1].seg[0])};
        RFN_TRY(gemm_groups(B, R, 2, pr, 0, gx));
        RFN_TRY(attn_bwd_unhoisted(s));
        RFN_TRY(gemm1(B, R, kb2.seg[0], dhrec, R, 1, gx));
    }
    return RFN_OK;
}

// What follows either sweep: the state gradients, d thoughts and the gradients of the weights shared across steps (one GEMM over
// (S*B) time-major rows each, bias gradients ride along).  Hoisted: d thoughts and d z2h.weight come from dU instead of z,
// and d z2h.bias is copied from d h2h.bias (b_z enters every step's gates as b_h2h does: the same column sums).
int DecBwd::tail(bool hoisted) const {
    float* dUd = W + Lo.dUd;
    float* dPi = n > 1 ? W + Lo.dPi : dPd;   // d Pd per image
    RFN_TRY(mem_batch({{d_h0, dhrec, BR}, {d_c0, dc, BR}, {grd[P.dec(11)], nullptr, 1}}, st));
    if (hoisted) {   // d U = sum_s alpha_s (x) d gates_s; d thoughts = dPd . W_att + dU . W_z (one product, two K segments)
        // n rows per image: dU sums them (rfn_dec_du_ex), the per-row d Pd slabs are summed onto the image (j ascending) first
        RFN_TRY(rfn_dec_du_ex(W + Lo.ald, gd, S, B, T2, GD, n, dUd, GD, (long)Bc * GD, st));
        if (n > 1) RFN_TRY(rfn_rowgroup_sum(dPd, A, n, dPi, A, (long)T2 * Bc, A, st));
        rfn_gemm_seg sg[2] = {seg_dx(dPi, A, prm[P.dec(6)], R, A), seg_dx(dUd, GD, prm[P.dec(4)], R, GD)};
        RFN_TRY(gemm_segs(T2 * Bc, R, 2, sg, d_comb, R, 0, gx));
    } else {         // the sweep accumulated the attention's share of d thoughts; add the projection's (shared by all steps)
        RFN_TRY(gemm1(T2 * B, R, seg_dx(dPd, A, prm[P.dec(6)], R, A), d_comb, R, 1, gx));
    }
    RFN_TRY(gemm_dw(A, R, grd[P.dec(6)], R, grd[P.dec(7)], dPi, A, comb, R, T2 * Bc, gx));
    if (hoisted) RFN_TRY(gemm_dw(GD, R, grd[P.dec(4)], R, nullptr, dUd, GD, comb, R, T2 * Bc, gx));   // d z2h.weight = dU^T . thoughts
    RFN_TRY(rfn_colsum_f32(W + Lo.dwp, A, S * B, A, grd[P.dec(10)], 0, st));
    RFN_TRY(gemm_dw(A, R, grd[P.dec(8)], R, grd[P.dec(9)], W + Lo.dhpd, A, hd, R, S * B, gx));
    RFN_TRY(gemm_dw(GD, R, grd[P.dec(2)], R, grd[P.dec(3)], gd, GD, hd, R, S * B, gx));
    if (!hoisted) RFN_TRY(gemm_dw(GD, R, grd[P.dec(4)], R, grd[P.dec(5)], gd, GD, W + Lo.zd, R, S * B, gx));
    RFN_TRY(gemm_dw(GD, E, grd[P.dec(0)], E, grd[P.dec(1)], gd, GD, W + Lo.xs, E, S * B, gx));
    if (hoisted) RFN_TRY(mem_batch({{grd[P.dec(5)], grd[P.dec(3)], (long)GD}}, st));
    // embedding: dx = dgates . W_i2h, then the fixed-order scatter
    RFN_TRY(gemm1(S * B, E, seg_dx(gd, GD, prm[P.dec(0)], E, GD), W + Lo.dxs, E, 0, gx));
    return rfn_embed_bwd(W + Lo.dxs, E, ids, B, ld_ids, 1, S * B, E, V1, grd[P.embed()], st);
}
}  // namespace

extern "C" int rfn_decoder_bwd(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb,
                               const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids,
                               const float* log_prob, const float* d_log_prob, float* d_comb, float* d_h0,
                               float* d_c0, float* const* grd, void* ws, size_t ws_bytes, uint64_t seed_arg, void* st) {
    return rfn_decoder_bwd_ex(d, B, S, prm, comb, h0, c0, ids, ld_ids, log_prob, d_log_prob, d_comb, d_h0, d_c0, grd, ws, ws_bytes,
                              seed_arg, 1, st);
}
// The backward pass on a checked call.  d_log_prob == NULL: the logits rows of the workspace already hold d logits, with any n
// (nothing below the log-softmax backward reads log_prob, and every later step takes its row counts from B and n).
static int decoder_bwd_body(const rfn_dims* d, int B, int S, int n, const float* const* prm, const float* comb, const int64_t* ids,
                            int64_t ld_ids, const float* log_prob, const float* d_log_prob, float* d_comb, float* d_h0, float* d_c0,
                            float* const* grd, void* ws, size_t ws_bytes, RfnSeed seed, void* st) {
    const DecoderLayout Lo = decoder_layout(d, B, S, 1, n);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    float* W = (float*)ws;
    DecBwd c{d, PIdx(d), B, n, B / n, S, d->R, d->A, d->E, d->T2, d->V1, gate_width(d->decoder_maxout, d->R), (long)B * d->R, (long)B * d->A,
             prm, comb, ids, ld_ids, d_comb, d_h0, d_c0, grd, W, Lo, seed, st, GemmCtx{},
             W + Lo.hd, W + Lo.cd, W + Lo.gd, W + Lo.dhe, W + Lo.dhrec, W + Lo.dc, W + Lo.dz, W + Lo.dPd};
    RFN_TRY(phase_gemm(d, W, Lo.gws, Lo.tk, true, st, &c.gx));
    const PIdx& P = c.P;
    const int R = d->R, V1 = d->V1;
    float* dlg = W + Lo.logits;
    // log-softmax backward into time-major rows, then the batched logit layer
    // (no log_prob: rfn_xe_logits_bwd already turned the logits rows into d logits)
    if (d_log_prob) RFN_TRY(rfn_log_softmax_bwd(d_log_prob, log_prob, S * B, V1, B, (long)S * V1, V1, dlg, V1, st));
    RFN_TRY(gemm_logits_dw(V1, R, grd[P.logit_w()], grd[P.logit_b()], dlg, c.hd + c.BR, S * B, c.gx));
    RFN_TRY(gemm_logits_dx(S * B, R, V1, dlg, prm[P.logit_w()], c.dhe, c.gx));
    RFN_TRY(dec_hoisted(d) ? c.sweep_hoisted() : c.sweep_unhoisted());
    return c.tail(dec_hoisted(d));
}
extern "C" int rfn_decoder_bwd_ex(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb,
                                  const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids,
                                  const float* log_prob, const float* d_log_prob, float* d_comb, float* d_h0, float* d_c0,
                                  float* const* grd, void* ws, size_t ws_bytes, uint64_t seed_arg, int rows_per_image, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1 || S < 1) return RFN_ERR_SHAPE;
    const int n = rows_per_image;
    RFN_TRY(rows_per_image_ok(d, B, n));
    if (!prm || !comb || !ids || (!log_prob != !d_log_prob) || !d_comb || !d_h0 || !d_c0 || !grd || !ws || (n > 1 && !log_prob))
        return RFN_ERR_ARG;
    (void)h0; (void)c0;
    return decoder_bwd_body(d, B, S, n, prm, comb, ids, ld_ids, log_prob, d_log_prob, d_comb, d_h0, d_c0, grd, ws, ws_bytes, seed, st);
}

// ---- the logits-only pair with n rows per image (rfn.h "policy-gradient loss from the logits") --------------------------------
// rfn_decoder_fwd_ex with log_prob == NULL and rfn_decoder_bwd_ex from the d logits in the workspace, for any rows_per_image:
// the launches of those two calls, nothing else.  rfn_decoder_logits_ex: where the time-major rows lie under that layout.
extern "C" int rfn_decoder_logits_fwd(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb, const float* h0,
                                      const float* c0, const int64_t* ids, int64_t ld_ids, void* ws, size_t ws_bytes, int train,
                                      uint64_t seed_arg, int rows_per_image, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1 || S < 1) return RFN_ERR_SHAPE;
    const int n = rows_per_image;
    RFN_TRY(rows_per_image_ok(d, B, n));
    if (!prm || !comb || !h0 || !c0 || !ids || !ws) return RFN_ERR_ARG;
    const DecoderLayout Lo = decoder_layout(d, B, S, train, n);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    return decoder_fwd_body(d, B, S, n, prm, comb, h0, c0, ids, ld_ids, nullptr, (float*)ws, Lo, seed, st);
}
extern "C" float* rfn_decoder_logits_ex(const rfn_dims* d, int B, int S, int train, int rows_per_image, void* ws) {
    if (check_dims(d) != RFN_OK || B < 1 || S < 1 || rows_per_image < 1 || B % rows_per_image || !ws) return nullptr;
    return (float*)ws + decoder_layout(d, B, S, train, rows_per_image).logits;
}
extern "C" int rfn_decoder_logits_bwd(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb, const int64_t* ids,
                                      int64_t ld_ids, float* d_comb, float* d_h0, float* d_c0, float* const* grd, void* ws,
                                      size_t ws_bytes, uint64_t seed_arg, int rows_per_image, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1 || S < 1) return RFN_ERR_SHAPE;
    const int n = rows_per_image;
    RFN_TRY(rows_per_image_ok(d, B, n));
    if (!prm || !comb || !ids || !d_comb || !d_h0 || !d_c0 || !grd || !ws) return RFN_ERR_ARG;
    if (ws_bytes < decoder_layout(d, B, S, 1, n).total * sizeof(float)) return RFN_ERR_WORKSPACE;
    return decoder_bwd_body(d, B, S, n, prm, comb, ids, ld_ids, nullptr, nullptr, d_comb, d_h0, d_c0, grd, ws, ws_bytes, seed, st);
}
// The same sweep from a given d hidden (rfn.h "mixture of softmaxes"): the output layer's backward ran elsewhere.
extern "C" int rfn_decoder_bwd_hidden(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb,
                                      const float* h0, const float* c0, const int64_t* ids, int64_t ld_ids, const float* d_hidden,
                                      float* d_comb, float* d_h0, float* d_c0, float* const* grd, void* ws, size_t ws_bytes,
                                      uint64_t seed_arg, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1 || S < 1) return RFN_ERR_SHAPE;
    if (!dec_hoisted(d)) return RFN_ERR_UNSUPPORTED;
    if (!prm || !comb || !ids || !d_hidden || !d_comb || !d_h0 || !d_c0 || !grd || !ws) return RFN_ERR_ARG;
    (void)h0; (void)c0;
    const DecoderLayout Lo = decoder_layout(d, B, S, 1, 1);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    float* W = (float*)ws;
    DecBwd c{d, PIdx(d), B, 1, B, S, d->R, d->A, d->E, d->T2, d->V1, gate_width(d->decoder_maxout, d->R), (long)B * d->R, (long)B * d->A,
             prm, comb, ids, ld_ids, d_comb, d_h0, d_c0, grd, W, Lo, seed, st, GemmCtx{},
             W + Lo.hd, W + Lo.cd, W + Lo.gd, W + Lo.dhe, W + Lo.dhrec, W + Lo.dc, W + Lo.dz, W + Lo.dPd};
    RFN_TRY(phase_gemm(d, W, Lo.gws, Lo.tk, true, st, &c.gx));
    const PIdx& P = c.P;
    RFN_TRY(mem_batch({{c.dhe, d_hidden, (long)S * c.BR}, {grd[P.logit_w()], nullptr, (long)d->V1 * d->R}, {grd[P.logit_b()], nullptr, (long)d->V1}}, st));
    RFN_TRY(c.sweep_hoisted());
    return c.tail(true);
}
