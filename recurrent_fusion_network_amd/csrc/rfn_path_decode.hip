// The free-running decoder: one step on caller-held state (sample / beam / one_time_step) and the whole decode loops queued by
// one call.  Every step is the cell of the teacher-forced pass (decoder_cell_core, rfn_path_decoder.hip).
#include "rfn_path.h"
#include "rfn_beam_step.h"   // BEAM_MAX_W / BEAM_MAX_S: the limits of the beam-step kernels

// =============================================================================================
// free-running decoder step (sample / beam / one_time_step)
// =============================================================================================
extern "C" size_t rfn_decoder_step_ws_bytes(const rfn_dims* d, int B) {
    if (check_dims(d) != RFN_OK || B < 1) return 0;
    Bump b;
    b.take((size_t)B * d->E);
    b.take((size_t)B * d->A);
    b.take((size_t)B * d->T2);
    b.take((size_t)B * d->R);
    b.take((size_t)B * gate_width(d->decoder_maxout, d->R));
    b.take((size_t)B * d->V1);
    b.take(STEP_GEMM_WS_FLOATS);
    return b.off * sizeof(float);
}

extern "C" size_t rfn_decoder_cproj_floats(const rfn_dims* d, int B) {
    if (check_dims(d) != RFN_OK || B < 1) return 0;
    return cproj_u_off(d, B) + (size_t)d->T2 * B * gate_width(d->decoder_maxout, d->R);
}

extern "C" int rfn_decoder_prepare(const rfn_dims* d, int B, const float* const* prm, const float* comb, float* cproj,
                                   void* st) {
    RFN_TRY(check_dims(d));
    if (B < 1) return RFN_ERR_SHAPE;
    if (!prm || !comb || !cproj) return RFN_ERR_ARG;
    const PIdx P(d);
    const GemmCtx gx{st, nullptr, 0, d->gemm_flags};
    RFN_TRY(gemm1(d->T2 * B, d->A, seg_lin(comb, d->R, prm[P.dec(6)], d->R, d->R, prm[P.dec(7)]), cproj, d->A, 0, gx));
    if (!dec_hoisted(d)) return RFN_OK;
    const int GD = gate_width(d->decoder_maxout, d->R);   // the same unsplit product as decoder_fwd_begin's
    return gemm1(d->T2 * B, GD, seg_lin(comb, d->R, prm[P.dec(4)], d->R, d->R, nullptr), cproj + cproj_u_off(d, B), GD, 0, gx);
}

// One decoder step computed with exactly the operation sequence of one step of rfn_decoder_fwd (unsplit i2h, then
// h2h + z2h accumulated onto it, same split-K scratch size, same dropout stream (seed, OFF_DECODER + step)), so the
// distribution a host samples from here IS the one the teacher-forced gradient pass differentiates
// (misc/RecurrentFusionModel.py:260-270, 623-631: the reference samples from the dropout-affected outputs themselves).
//
// StepLists: what the step hands to a search that drives it, beyond logits / logp.  The default is "no lists" (rfn_decoder_step).
struct StepLists {
    float* topv = nullptr;                      // the rows' W best log-probs and their tokens, no full rows (rfn_log_softmax_topk*)
    int32_t* topi = nullptr;
    int W = 0;
    int row_div = 1;                            // rows that read one thought vector (comb / cproj hold B / row_div of them)
    const int32_t* blk = nullptr;               // decoding constraints: the rows' block lists mask the lists
    int64_t ld_blk = 0;
    const int32_t* blk_n = nullptr;
    const int32_t* want = nullptr;              // lexical search: the image's n_want required ids, whose log-probs go to wantv
    int n_want = 0;
    float* wantv = nullptr;
    const rfn_beam_stochastic* sbs = nullptr;   // stochastic search: the W best Gumbel-perturbed entries of the live rows,
    uint64_t sbs_offset = 0;                    // with the noise of (sbs->seed, sbs_offset)
};
static int decoder_step_impl(const rfn_dims* d, int B, const float* const* prm, const float* comb, const float* cproj,
                             const int64_t* ids, const float* xt, int64_t ld_xt, float* h, float* c, float* logits,
                             float* logp, int64_t ld_logp, void* ws, size_t ws_bytes, uint64_t seed_arg, int step,
                             void* st, const StepLists& ls = {}) {
    const int row_div = ls.row_div;
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1 || step < 0 || row_div < 1 || B % row_div) return RFN_ERR_SHAPE;
    if (!prm || !comb || !cproj || (!ids && !xt) || !h || !c || !ws) return RFN_ERR_ARG;
    if (xt && ld_xt < d->E) return RFN_ERR_SHAPE;
    if (ws_bytes < rfn_decoder_step_ws_bytes(d, B)) return RFN_ERR_WORKSPACE;
    const PIdx P(d);
    const int R = d->R, A = d->A, E = d->E, T2 = d->T2, V1 = d->V1;
    const int GD = gate_width(d->decoder_maxout, R);
    Bump b;
    float* W = (float*)ws;
    const GemmCtx gx{st, W + b.take(STEP_GEMM_WS_FLOATS), STEP_GEMM_WS_FLOATS * sizeof(float), d->gemm_flags};  // split-K scratch
    const GemmCtx gx_whole{st, nullptr, 0, d->gemm_flags};
    float* x = W + b.take((size_t)B * E);
    float* hp = W + b.take((size_t)B * A);
    float* al = W + b.take((size_t)B * T2);
    float* z = W + b.take((size_t)B * R);
    float* g = W + b.take((size_t)B * GD);
    float* lg = logits ? logits : W + b.take((size_t)B * V1);
    if (!xt) RFN_TRY(rfn_embed_fwd(prm[P.embed()], E, V1, ids, B, 1, 0, B, x, E, st));
    RFN_TRY(gemm1(B, GD, xt ? seg_lin(xt, ld_xt, prm[P.dec(0)], E, E, prm[P.dec(1)]) : seg_lin(x, E, prm[P.dec(0)], E, E, prm[P.dec(1)]),
                  g, GD, 0, gx_whole));
    RFN_TRY(decoder_cell_core(d, B, prm, comb, cproj, cproj + cproj_u_off(d, B / row_div), row_div, h, c, h, c, hp, al, z, g, gx,
                              seed, step, st));
    if (logits || logp || ls.topv) {
        RFN_TRY(gemm_logits(B, V1, h, R, prm[P.logit_w()], prm[P.logit_b()], lg, gx_whole));
        if (logp) {
            if (ld_logp < V1) return RFN_ERR_SHAPE;
            RFN_TRY(rfn_log_softmax_fwd(lg, V1, B, V1, B, ld_logp, 0, logp, st));
        }
        if (ls.topv && ls.sbs)
            RFN_TRY(rfn_log_softmax_topk_gumbel(lg, V1, B, V1, ls.W, ls.blk, ls.ld_blk, ls.blk_n, ls.sbs->live, ls.sbs->seed,
                                                ls.sbs_offset, ls.sbs->topk64, ls.topv, ls.topi, st));
        else if (ls.topv && ls.want)
            RFN_TRY(rfn_log_softmax_topk_want(lg, V1, B, V1, ls.W, row_div, ls.want, ls.n_want, ls.n_want, ls.blk, ls.ld_blk, ls.blk_n,
                                              ls.topv, ls.topi, ls.wantv, st));
        else if (ls.topv)
            RFN_TRY(rfn_log_softmax_topk_masked(lg, V1, B, V1, ls.W, ls.blk, ls.ld_blk, ls.blk_n, ls.topv, ls.topi, st));
    }
    return RFN_OK;
}

extern "C" int rfn_decoder_step(const rfn_dims* d, int B, const float* const* prm, const float* comb,
                                const float* cproj, const int64_t* ids, float* h, float* c, float* logits, float* logp,
                                int64_t ld_logp, void* ws, size_t ws_bytes, uint64_t seed, int step, void* st) {
    if (!ids) return RFN_ERR_ARG;
    return decoder_step_impl(d, B, prm, comb, cproj, ids, nullptr, 0, h, c, logits, logp, ld_logp, ws, ws_bytes, seed,
                             step, st);
}
// the reference's one_time_step signature: the caller has already embedded the token (xt = model.embed(it))
extern "C" int rfn_decoder_step_embedded(const rfn_dims* d, int B, const float* const* prm, const float* comb,
                                         const float* cproj, const float* xt, int64_t ld_xt, float* h, float* c,
                                         float* logits, float* logp, int64_t ld_logp, void* ws, size_t ws_bytes,
                                         uint64_t seed, int step, void* st) {
    if (!xt) return RFN_ERR_ARG;
    return decoder_step_impl(d, B, prm, comb, cproj, nullptr, xt, ld_xt, h, c, logits, logp, ld_logp, ws, ws_bytes,
                             seed, step, st);
}

// =============================================================================================
// whole decode loops queued by one call (no host work between steps)
// =============================================================================================
// sample() free-running decode (misc/RecurrentFusionModel.py:616-653): step t = 0 feeds BOS; step t >= 1 feeds the token
// picked from step t-1's distribution (mode 0: argmax; mode 1: inverse-CDF draw with the caller's uniform u[t-1][b]).
// Every step is rfn_decoder_step (embedding K10, cell a5, logit + log-softmax K11) on the same buffers, so the result is
// bit for bit what the step-by-step host loop gives -- only the host is gone from the loop.  `unf` keeps one row of
// unfinished flags per step so that the caller applies the reference's early exit (:645) with ONE read-back afterwards.
static int check_constraints(const rfn_decode_constraints* cons, int S) {
    if (!cons) return RFN_OK;
    if (S < 1 || S > 64) return RFN_ERR_SHAPE;
    if (cons->block_ngram != 0 && (cons->block_ngram < 2 || cons->block_ngram > 4)) return RFN_ERR_SHAPE;
    if (cons->n_banned < 0 || cons->n_banned > RFN_DECODE_MAX_IDS || cons->n_bad < 0 || cons->n_bad > RFN_DECODE_MAX_IDS)
        return RFN_ERR_SHAPE;
    if (!cons->blk || !cons->blk_n || (cons->n_banned && !cons->banned) || (cons->n_bad && !cons->bad_endings)) return RFN_ERR_ARG;
    return RFN_OK;
}
extern "C" int rfn_decoder_loop_ex2(const rfn_dims* d, int B, int steps, const float* const* prm, const float* comb,
                                    const float* cproj, float* h, float* c, int mode, float inv_temperature, const float* u,
                                    float* logp_all, int64_t ld_b, int64_t ld_t, int64_t* seq, int64_t ld_seq, float* seq_lp,
                                    int64_t ld_lp, int32_t* unf, int64_t* ids, void* ws, size_t ws_bytes, uint64_t seed,
                                    const rfn_decode_constraints* cons, const rfn_decode_sampling* samp, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed_checked;
    RFN_TRY(path_seed(d, seed, &seed_checked));   // the steps below resolve it again
    if (B < 1 || steps < 1 || (mode != 0 && mode != 1)) return RFN_ERR_SHAPE;
    if (!prm || !comb || !cproj || !h || !c || !logp_all || !seq || !seq_lp || !unf || !ids || !ws) return RFN_ERR_ARG;
    if (mode == 1 && !u) return RFN_ERR_ARG;
    const int V1 = d->V1, S = steps - 1;
    if (cons && S >= 1) RFN_TRY(check_constraints(cons, S));
    // samp: truncate the rows before a draw (mode 1; the argmax survives any truncation), n rows per image
    const int n_img = samp && samp->rows_per_image ? samp->rows_per_image : 1;
    const bool trunc = samp && mode == 1 && ((samp->top_k > 0 && samp->top_k < V1) || samp->top_p < 1.f);
    if (n_img < 1 || B % n_img) return RFN_ERR_SHAPE;
    if (n_img > 1 && !dec_hoisted(d)) return RFN_ERR_UNSUPPORTED;   // the three-launch cell reads comb per row
    if (trunc && (!(samp->top_p > 0.f) || !(inv_temperature > 0.f))) return RFN_ERR_SHAPE;
    if (hipMemsetAsync(ids, 0, (size_t)B * sizeof(int64_t), (hipStream_t)st) != hipSuccess) return RFN_ERR_LAUNCH;   // BOS
    StepLists ls;
    ls.row_div = n_img;   // n_img = 1: rfn_decoder_step
    for (int t = 0; t < steps; ++t) {
        if (t >= 1) {
            float* prev = logp_all + (long)(t - 1) * ld_t;
            if (cons) {   // the row's history is what the picks before this one recorded in seq
                RFN_TRY(rfn_decode_blocklist(seq, ld_seq, 1, nullptr, B, S, t, cons->block_ngram, cons->banned, cons->n_banned,
                                             cons->bad_endings, cons->n_bad, V1, cons->blk, cons->blk_n, st));
                RFN_TRY(rfn_logp_mask_rows(prev, ld_b, B, V1, cons->blk, RFN_DECODE_MAX_IDS + S, cons->blk_n, st));
            }
            if (trunc) RFN_TRY(rfn_logp_truncate_rows(prev, ld_b, B, V1, samp->top_k, samp->top_p, inv_temperature, nullptr, st));
            if (mode == 1)   // the draw first: the greedy-pick kernel below then records ITS log-prob and finished flags
                RFN_TRY(rfn_multinomial_pick(prev, ld_b, B, V1, inv_temperature, u + (long)(t - 1) * B, nullptr, 1.f, ids, 1, st));
            RFN_TRY(rfn_pick_record(prev, ld_b, B, V1, t, mode == 1 ? ids : nullptr, ids, seq + (t - 1), ld_seq, seq_lp + (t - 1),
                                    ld_lp, t > 1 ? unf + (long)(t - 1) * B : nullptr, unf + (long)t * B, st));
        }
        RFN_TRY(decoder_step_impl(d, B, prm, comb, cproj, ids, nullptr, 0, h, c, nullptr, logp_all + (long)t * ld_t, ld_b, ws,
                                  ws_bytes, seed, t, st, ls));
    }
    return RFN_OK;
}
extern "C" int rfn_decoder_loop_ex(const rfn_dims* d, int B, int steps, const float* const* prm, const float* comb,
                                   const float* cproj, float* h, float* c, int mode, float inv_temperature, const float* u,
                                   float* logp_all, int64_t ld_b, int64_t ld_t, int64_t* seq, int64_t ld_seq, float* seq_lp,
                                   int64_t ld_lp, int32_t* unf, int64_t* ids, void* ws, size_t ws_bytes, uint64_t seed,
                                   const rfn_decode_constraints* cons, void* st) {
    return rfn_decoder_loop_ex2(d, B, steps, prm, comb, cproj, h, c, mode, inv_temperature, u, logp_all, ld_b, ld_t, seq, ld_seq,
                                seq_lp, ld_lp, unf, ids, ws, ws_bytes, seed, cons, nullptr, st);
}
extern "C" int rfn_decoder_loop(const rfn_dims* d, int B, int steps, const float* const* prm, const float* comb,
                                const float* cproj, float* h, float* c, int mode, float inv_temperature, const float* u,
                                float* logp_all, int64_t ld_b, int64_t ld_t, int64_t* seq, int64_t ld_seq, float* seq_lp,
                                int64_t ld_lp, int32_t* unf, int64_t* ids, void* ws, size_t ws_bytes, uint64_t seed,
                                void* st) {
    return rfn_decoder_loop_ex(d, B, steps, prm, comb, cproj, h, c, mode, inv_temperature, u, logp_all, ld_b, ld_t, seq, ld_seq,
                               seq_lp, ld_lp, unf, ids, ws, ws_bytes, seed, nullptr, st);
}

// The step-wise training decoder with draws between the steps (scheduled sampling :260-270, multinomial sample() with
// grad :623-631), queued by one call: begin, then for every step s >= 1 rows whose coin u_coin[s][b] < ss_prob get a
// token drawn from step s-1's distribution (uniform u_draw[s][b]), then rfn_decoder_fwd_step.  Leaves workspace, ids and
// log_prob exactly as the host loop over rfn_multinomial_pick / rfn_decoder_fwd_step does.
extern "C" int rfn_decoder_fwd_sampled_ex(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb,
                                          const float* h0, const float* c0, int64_t* ids, int64_t ld_ids, float ss_prob,
                                          float inv_temperature, const float* u_draw, const float* u_coin, float* log_prob,
                                          void* ws, size_t ws_bytes, int train, uint64_t seed, int rows_per_image, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed_checked;
    RFN_TRY(path_seed(d, seed, &seed_checked));   // the steps below resolve it again
    if (B < 1 || S < 1) return RFN_ERR_SHAPE;
    if (!prm || !comb || !h0 || !c0 || !ids || !u_draw || !u_coin || !log_prob || !ws) return RFN_ERR_ARG;
    RFN_TRY(decoder_fwd_begin_n(d, B, S, rows_per_image, prm, comb, h0, c0, ws, ws_bytes, train, st));
    const long ld_b = (long)S * d->V1;
    for (int s = 0; s < S; ++s) {
        if (s >= 1)
            RFN_TRY(rfn_multinomial_pick(log_prob + (long)(s - 1) * d->V1, ld_b, B, d->V1, inv_temperature, u_draw + (long)s * B,
                                         u_coin + (long)s * B, ss_prob, ids + s, ld_ids, st));
        RFN_TRY(decoder_fwd_step_n(d, B, S, rows_per_image, s, prm, comb, ids + s, ld_ids, log_prob, ws, ws_bytes, train, seed, st));
    }
    return RFN_OK;
}
extern "C" int rfn_decoder_fwd_sampled(const rfn_dims* d, int B, int S, const float* const* prm, const float* comb,
                                       const float* h0, const float* c0, int64_t* ids, int64_t ld_ids, float ss_prob,
                                       float inv_temperature, const float* u_draw, const float* u_coin, float* log_prob,
                                       void* ws, size_t ws_bytes, int train, uint64_t seed, void* st) {
    return rfn_decoder_fwd_sampled_ex(d, B, S, prm, comb, h0, c0, ids, ld_ids, ss_prob, inv_temperature, u_draw, u_coin, log_prob, ws,
                                      ws_bytes, train, seed, 1, st);
}

// one group is the plain search, with the same launches
static bool beam_diverse(const rfn_beam_diversity* div) { return div && div->groups > 1; }
// rfn_beam_loop_ex4's refusals, in the order tests/test_native_abi.py pins.  ptrs_ok: every buffer all four searches need is there.
static int check_beam_loop(const rfn_dims* d, int NB, int W, int S, bool ptrs_ok, uint64_t seed, const int64_t* beam_seq,
                           const float* beam_lp, const rfn_decode_constraints* cons, const rfn_beam_diversity* div,
                           const rfn_beam_lexical* lex, const rfn_beam_stochastic* sbs) {
    RFN_TRY(check_dims(d));
    RfnSeed seed_checked;
    RFN_TRY(path_seed(d, seed, &seed_checked));   // the steps resolve it again
    if (NB < 1 || W < 1 || S < 1) return RFN_ERR_SHAPE;
    if (!ptrs_ok) return RFN_ERR_ARG;
    if (W > BEAM_MAX_W) return RFN_ERR_SHAPE;
    RFN_TRY(check_constraints(cons, S));
    if (cons && !beam_seq) return RFN_ERR_ARG;
    if (div && (div->groups < 1 || W % div->groups || !(div->lambda >= 0.f))) return RFN_ERR_SHAPE;
    const bool diverse = beam_diverse(div);
    if (diverse && !div->done_group) return RFN_ERR_ARG;
    if (lex) {
        if (diverse) return RFN_ERR_UNSUPPORTED;
        const int C = lex->n_sets, NW = lex->n_want;
        if (C < 1 || C > RFN_LEX_MAX_SETS || W % (1 << C) || NW < 1 || NW > RFN_LEX_MAX_IDS || NW > W - W / (1 << C) || S > BEAM_MAX_S)
            return RFN_ERR_SHAPE;
        if (!lex->want || !lex->want_bits || !lex->init_state || !lex->wantv || !lex->state_n || !lex->done_state || !beam_seq)
            return RFN_ERR_ARG;
    }
    if (sbs) {
        if (diverse || lex) return RFN_ERR_UNSUPPORTED;
        if (S > BEAM_MAX_S) return RFN_ERR_SHAPE;
        if (!sbs->phi || !sbs->gumbel || !sbs->live || !sbs->weight || !sbs->n_live || !sbs->topk64 || !beam_seq || !beam_lp)
            return RFN_ERR_ARG;
    }
    return RFN_OK;
}
// sample_beam's search (misc/RecurrentFusionModel.py:451-531) for all images at once, queued by one call: per step the
// device-side bookkeeping (rfn_beam_step), the re-gather of the recurrent state rows and one decoder step on the
// NB * W beam rows.  h / c are ping-ponged with h_alt / c_alt; on return the live state is in h / c again.
// div: diverse beam search (rfn.h): the step is rfn_beam_step_div on the same top-W lists, everything else is unchanged.
// lex: lexically constrained search (rfn.h): the step is rfn_beam_step_lex, and every decoder step also writes the log-probs of the
// image's required tokens (rfn_log_softmax_topk_want in place of rfn_log_softmax_topk_masked); the launch count is unchanged.
// sbs: stochastic beam search (rfn.h): the step is rfn_beam_step_sbs on the lists rfn_log_softmax_topk_gumbel writes in place of
// rfn_log_softmax_topk_masked, with the noise of (sbs->seed, sbs->offset0 + t) for step t; the launch count is unchanged.
extern "C" int rfn_beam_loop_ex4(const rfn_dims* d, int NB, int W, int S, const float* const* prm, const float* comb,
                                 const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp,
                                 int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids,
                                 int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active, int max_done,
                                 void* ws, size_t ws_bytes, uint64_t seed, const rfn_decode_constraints* cons,
                                 const rfn_beam_diversity* div, const rfn_beam_lexical* lex, const rfn_beam_stochastic* sbs,
                                 void* st) {
    RFN_TRY(check_beam_loop(d, NB, W, S, prm && comb && cproj && h && c && h_alt && c_alt && logp && ids && order && ws, seed, beam_seq,
                            beam_lp, cons, div, lex, sbs));
    const int rows = NB * W, V1 = d->V1, R = d->R;
    const bool diverse = beam_diverse(div);
    // `logp` holds, per beam row, its W best log-probs and their tokens (2 * W values): the search never looks at more
    // (:463-466), so the full (rows, V+1) log-prob matrix is neither written nor read back
    float* topv = logp;
    int32_t* topi = (int32_t*)(logp + (size_t)rows * W);
    StepLists ls;
    ls.topv = topv, ls.topi = topi, ls.W = W;
    ls.row_div = W;   // the W rows of an image share its thought vectors (comb / cproj: NB rows)
    if (cons) ls.blk = cons->blk, ls.ld_blk = RFN_DECODE_MAX_IDS + S, ls.blk_n = cons->blk_n;
    if (lex) ls.want = lex->want, ls.n_want = lex->n_want, ls.wantv = lex->wantv;
    ls.sbs = sbs;
    float *hc = h, *cc = c, *ha = h_alt, *ca = c_alt;
    if (hipMemsetAsync(ids, 0, (size_t)rows * sizeof(int64_t), (hipStream_t)st) != hipSuccess) return RFN_ERR_LAUNCH;
    if (sbs) RFN_TRY(rfn_beam_sbs_begin(NB, W, V1, sbs->seed, sbs->offset0, sbs->phi, sbs->gumbel, sbs->live, st));
    for (int t = 0; t <= S; ++t) {
        if (t >= 1) {
            if (sbs)
                RFN_TRY(rfn_beam_step_sbs(sbs->topk64, topv, topi, V1, W, S, t, NB, beam_seq, beam_lp, sbs->phi, sbs->gumbel, sbs->live,
                                          order, ids, sbs->weight, sbs->n_live, st));
            else if (lex)   // at t == 1 the step takes the occupancy from init_state and writes state_n
                RFN_TRY(rfn_beam_step_lex(topv, topi, lex->wantv, lex->want, lex->want_bits, lex->n_want, lex->n_sets, V1, W, S, t, NB,
                                          max_done, beam_seq, beam_lp, beam_sum, order, ids, done_seq, done_lp, done_p, done_n,
                                          lex->state_n, lex->done_state, lex->init_state, active, st));
            else if (diverse)
                RFN_TRY(rfn_beam_step_div(topv, topi, V1, W, div->groups, div->lambda, S, t, NB, max_done, beam_seq, beam_lp,
                                          beam_sum, order, ids, done_seq, done_lp, done_p, done_n, div->done_group, active, st));
            else
                RFN_TRY(rfn_beam_step_topk(topv, topi, V1, W, S, t, NB, max_done, beam_seq, beam_lp, beam_sum, order, ids, done_seq,
                                           done_lp, done_p, done_n, active, st));
            if (t == S) break;   // the reference still runs one more decoder step whose output is never used
            RFN_TRY(rfn_gather_rows(hc, ha, order, rows, R, st));
            RFN_TRY(rfn_gather_rows(cc, ca, order, rows, R, st));
            float* x = hc; hc = ha; ha = x;
            x = cc; cc = ca; ca = x;
        }
        if (cons)   // the lists for step t + 1, which reads this step's log-probs: rfn_beam_step has forked the beam arrays
            RFN_TRY(rfn_decode_blocklist(beam_seq, 1, rows, nullptr, rows, S, t + 1, cons->block_ngram, cons->banned, cons->n_banned,
                                         cons->bad_endings, cons->n_bad, V1, cons->blk, cons->blk_n, st));
        if (sbs) ls.sbs_offset = sbs->offset0 + (uint64_t)(t + 1);   // this step's lists are read by step t + 1
        RFN_TRY(decoder_step_impl(d, rows, prm, comb, cproj, ids, nullptr, 0, hc, cc, nullptr, nullptr, 0, ws, ws_bytes, seed, t, st, ls));
    }
    if (hc != h) {   // an odd number of swaps: bring the live state home
        RFN_TRY(mem_batch({{h, hc, (long)rows * R}, {c, cc, (long)rows * R}}, st));
    }
    return RFN_OK;
}
extern "C" int rfn_beam_loop_ex3(const rfn_dims* d, int NB, int W, int S, const float* const* prm, const float* comb,
                                 const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp,
                                 int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids,
                                 int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active, int max_done,
                                 void* ws, size_t ws_bytes, uint64_t seed, const rfn_decode_constraints* cons,
                                 const rfn_beam_diversity* div, const rfn_beam_lexical* lex, void* st) {
    return rfn_beam_loop_ex4(d, NB, W, S, prm, comb, cproj, h, c, h_alt, c_alt, logp, beam_seq, beam_lp, beam_sum, order, ids, done_seq,
                             done_lp, done_p, done_n, active, max_done, ws, ws_bytes, seed, cons, div, lex, nullptr, st);
}
extern "C" int rfn_beam_loop_ex2(const rfn_dims* d, int NB, int W, int S, const float* const* prm, const float* comb,
                                 const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp,
                                 int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids,
                                 int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active, int max_done,
                                 void* ws, size_t ws_bytes, uint64_t seed, const rfn_decode_constraints* cons,
                                 const rfn_beam_diversity* div, void* st) {
    return rfn_beam_loop_ex3(d, NB, W, S, prm, comb, cproj, h, c, h_alt, c_alt, logp, beam_seq, beam_lp, beam_sum, order, ids, done_seq,
                             done_lp, done_p, done_n, active, max_done, ws, ws_bytes, seed, cons, div, nullptr, st);
}
extern "C" int rfn_beam_loop_ex(const rfn_dims* d, int NB, int W, int S, const float* const* prm, const float* comb,
                                const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp,
                                int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids,
                                int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active, int max_done,
                                void* ws, size_t ws_bytes, uint64_t seed, const rfn_decode_constraints* cons, void* st) {
    return rfn_beam_loop_ex2(d, NB, W, S, prm, comb, cproj, h, c, h_alt, c_alt, logp, beam_seq, beam_lp, beam_sum, order, ids, done_seq,
                             done_lp, done_p, done_n, active, max_done, ws, ws_bytes, seed, cons, nullptr, st);
}
extern "C" int rfn_beam_loop(const rfn_dims* d, int NB, int W, int S, const float* const* prm, const float* comb,
                             const float* cproj, float* h, float* c, float* h_alt, float* c_alt, float* logp,
                             int64_t* beam_seq, float* beam_lp, float* beam_sum, int32_t* order, int64_t* ids,
                             int64_t* done_seq, float* done_lp, float* done_p, int32_t* done_n, int32_t* active, int max_done,
                             void* ws, size_t ws_bytes, uint64_t seed, void* st) {
    return rfn_beam_loop_ex(d, NB, W, S, prm, comb, cproj, h, c, h_alt, c_alt, logp, beam_seq, beam_lp, beam_sum, order, ids, done_seq,
                            done_lp, done_p, done_n, active, max_done, ws, ws_bytes, seed, nullptr, st);
}
