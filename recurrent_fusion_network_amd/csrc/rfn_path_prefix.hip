// Phase 1: initial state, fusion stage I (T1 steps x M cells), reason heads, state mean, fusion stage II (T2 steps) -- forward,
// backward and the per-encoder stage-I weight gradients.
#include "rfn_path.h"

// =============================================================================================
// phase 1: init state + fusion stages I and II
// =============================================================================================
extern "C" size_t rfn_prefix_ws_bytes(const rfn_dims* d, int B, int train) {
    if (check_dims(d) != RFN_OK || B < 1) return 0;
    return prefix_layout(d, B, train).total * sizeof(float);
}
// rfn.h "attention maps": where a finished forward pass left its attention weights (every form of the pass writes them there)
extern "C" float* rfn_prefix_alpha1(const rfn_dims* d, int B, int train, int enc, void* ws) {
    if (check_dims(d) != RFN_OK || B < 1 || enc < 0 || enc >= d->M || !ws) return nullptr;
    return (float*)ws + prefix_layout(d, B, train).al1[enc];
}
extern "C" float* rfn_prefix_alpha2(const rfn_dims* d, int B, int train, void* ws) {
    if (check_dims(d) != RFN_OK || B < 1 || !ws) return nullptr;
    return (float*)ws + prefix_layout(d, B, train).al2;
}

namespace {
// Stage-I attention of step t, all M encoders: ONE set of operand tables for every form of the forward launch (grouped, het,
// single) and of the backward launch (grouped, grouped-ks, het; the per-encoder fused-ks / fused / split calls index into it).
struct S1Attn {
    float *p[RFN_MAX_ENC], *sc[RFN_MAX_ENC], *al[RFN_MAX_ENC], *z[RFN_MAX_ENC];   // p: the projection slab; backward overwrites it
    float *dz[RFN_MAX_ENC], *dhp[RFN_MAX_ENC], *dw[RFN_MAX_ENC];                  //    in place with its gradient
    const float *hp[RFN_MAX_ENC], *w[RFN_MAX_ENC], *b[RFN_MAX_ENC];
    void* img[RFN_MAX_ENC];         // k-slow plane image of encoder i's dP1 (the _KS forms)
    int L[RFN_MAX_ENC], D[RFN_MAX_ENC];
    const int32_t* len[RFN_MAX_ENC];   // ragged maps: the caller's per-image row counts (NULL: all rows); `ragged`: any set
    bool ragged;
    bool same_ld;                   // M > 1 encoders that share (L, D): the grouped forms
    size_t sc_floats;               // raw scores of the forward launch, laid out in the (idle) split-K scratch
};
// The plain-GEMM fallbacks read their K segments back out of rfn_cell_out.seg[], which cell_lin / cell_dx fill only up to
// RFN_CELL_MAXSEG: one segment per encoder has to fit.
static_assert(RFN_CELL_MAXSEG >= RFN_MAX_ENC, "a cell-GEMM output holds one K segment per encoder");
// Stage-II step t.  Forward: K1 = every h_2_att_h_i(h) and h2h(h) in one launch (they share h); the M attentions over the T1
// thoughts; K3 = sum_i z_2_h_i(z_i) accumulated onto the gates with the LSTM update as its epilogue.  Read by the chain
// (prepared), by the three launches and -- review_maxout, or a step the cell GEMM refuses -- by the plain-GEMM fallback.
struct S2Fwd {
    rfn_cell_out k1[RFN_MAX_ENC + 1], k3;
    const float *p[RFN_MAX_ENC], *hp[RFN_MAX_ENC], *w[RFN_MAX_ENC], *b[RFN_MAX_ENC], *x[RFN_MAX_ENC];
    float *al[RFN_MAX_ENC], *z[RFN_MAX_ENC];
    bool fused;
};
// Backward: Kb1 = dh_rec and every dz_i = dgates . [W_hh | W_z_i] in one launch; the M attention backwards (dP overwrites P in
// place); Kb2 = dh_rec += sum_i dhp_i . W_h_i whose epilogue completes d h of step t-1 (+ its external share dh2e[t-1]) and
// runs that step's LSTM backward.  The same three readers.
struct S2Bwd {
    rfn_cell_out kb1[RFN_MAX_ENC + 1], kb2;
    float *p[RFN_MAX_ENC], *dhp[RFN_MAX_ENC], *dw[RFN_MAX_ENC], *dx[RFN_MAX_ENC];
    const float *hp[RFN_MAX_ENC], *w[RFN_MAX_ENC], *al[RFN_MAX_ENC], *x[RFN_MAX_ENC], *dz[RFN_MAX_ENC];
};

// One call of phase 1, forward or backward: the caller's arrays, the slabs of its workspace (the d* ones exist in a training
// layout only) and the problem tables the stages fill.
struct Prefix {
    const rfn_dims* d;
    const PIdx P;
    const int B, M, R, A, T1, T2, K, G2;
    const long MR, BMR, BR, BA;
    const float* const* prm;
    const float* const* att;
    float* const W;
    const PrefixLayout& Lo;
    const RfnSeed seed;
    void* const st;
    GemmCtx gx;
    float *Hs, *Cs, *h2, *c2, *rmat, *dHs, *dC, *dh2e, *dhrec, *dc2, *dz2, *dal, *dwp;
    int32_t* rarg;
    float* const* grd = nullptr;
    const int32_t* const* att_len = nullptr;   // rfn_prefix_*_ex: per-encoder (B,) row counts of the stage-I maps, or NULL
    rfn_gemm_problem pr[64];
    rfn_gemm_seg segs[64];

    Prefix(const rfn_dims* d_, int B_, const float* const* prm_, const float* const* att_, void* ws, const PrefixLayout& Lo_,
           RfnSeed seed_, void* st_)
        : d(d_), P(d_), B(B_), M(d_->M), R(d_->R), A(d_->A), T1(d_->T1), T2(d_->T2), K(d_->K), G2(gate_width(d_->review_maxout, d_->R)),
          MR((long)M * R), BMR(B * MR), BR((long)B * R), BA((long)B * A), prm(prm_), att(att_), W((float*)ws), Lo(Lo_), seed(seed_),
          st(st_), Hs(W + Lo.Hs), Cs(W + Lo.Cs), h2(W + Lo.h2), c2(W + Lo.c2), rmat(W + Lo.rmat), dHs(W + Lo.dHs), dC(W + Lo.dC),
          dh2e(W + Lo.dh2e), dhrec(W + Lo.dhrec), dc2(W + Lo.dc2), dz2(W + Lo.dz2), dal(W + Lo.dal), dwp(W + Lo.dwp),
          rarg((int32_t*)(W + Lo.rarg)) {}

    // forward
    int init_state(const float* const* fc, const float* const* init_h, const float* const* init_c);
    int s1_projections();
    void s1_attn_of(int t, S1Attn* a) const;
    int s1_fwd_step(int t);
    int s1_heads_and_mean(float* reason_pred);
    int s2_projections();
    void s2_fwd_of(int t, S2Fwd* s) const;
    int s2_fwd_sweep();
    // backward
    int s2_head_bwd(const float* d_comb, const float* d_reason);
    void s2_bwd_of(int t, S2Bwd* s) const;
    int s2_bwd_sweep(const float* d_h, const float* d_c);
    int s2_wgrad();
    int mean_and_s1_heads_bwd(const float* d_reason);
    void s1_dz_of(int t, rfn_cell_out* kz) const;
    void s1x_of(int t, rfn_cell_out* kx) const;
    void s1y_of(int t, bool small, rfn_cell_out* ky) const;
    bool s1_small_steps() const;
    int s1_bwd_step(int t, bool small);
    int s1_bwd_tail(const float* const* fc);
};

// K0: h0_i = fc2h_i(fc_i) written straight into the concatenated H of step 0; c0 = h0 (:202-208)
int Prefix::init_state(const float* const* fc, const float* const* init_h, const float* const* init_c) {
    if (init_h) {   // caller-provided stage-I state (get_thought_vectors(fc, att, state_list), :283)
        for (int i = 0; i < M; ++i) {
            if (!init_h[i] || !init_c[i]) return RFN_ERR_ARG;
            RFN_TRY(rfn_axpby_2d(1.f, init_h[i], R, 0.f, Hs + i * R, MR, B, R, st));
            RFN_TRY(rfn_axpby_2d(1.f, init_c[i], R, 0.f, Cs + i * R, MR, B, R, st));
        }
        return RFN_OK;
    }
    rfn_cell_out k0[RFN_MAX_ENC];
    for (int i = 0; i < M; ++i) {
        if (!fc[i]) return RFN_ERR_ARG;
        k0[i] = cell_out(Hs + i * R, MR, R, 0);
        cell_lin(k0[i], fc[i], d->F[i], prm[P.fc_w(i)], d->F[i], d->F[i], prm[P.fc_b(i)]);
    }
    if (cell_ok(B, M, k0, R)) {   // the M fc2h products in one launch
        RFN_TRY(cell_run(B, M, k0, R, 0.f, RfnSeed{}, st, cell_variant(d)));
    } else {
        for (int i = 0; i < M; ++i) RFN_TRY(gemm1(B, R, k0[i].seg[0], Hs + i * R, MR, 0, gx));
    }
    return copy_f32(Cs, Hs, BMR, st);
}

// hoisted feature projections of stage I, all T1 step weights grouped: step-major slabs P1_i[t][(b,l)][a], so that
// every consumer streams contiguous memory (the attention kernels of step t, the weight-gradient GEMM's k-rows)
int Prefix::s1_projections() {
    for (int i = 0; i < M; ++i) {
        if (T1 > 64) return RFN_ERR_SHAPE;
        if (x3_takes(d, B, i)) {
            // bf16-plane GEMM: the features and the T1 stacked step weights as plane images, one launch for all steps
            const int BL = B * d->L[i], Di = d->D[i];
            char* imgX = (char*)(W + Lo.x3);
            char* imgW = imgX + rfn_x3_image_bytes(BL, Di);
            const float* srcs[64];
            float* outs[64];
            const float* bias[64];
            srcs[0] = att[i];
            RFN_TRY(rfn_x3_split(srcs, 1, Di, BL, Di, 1, imgX, st));
            for (int t = 0; t < T1; ++t) {
                srcs[t] = prm[P.s1(t, i, 0)];
                outs[t] = W + Lo.P1[i] + (long)t * BL * A;
                bias[t] = prm[P.s1(t, i, 1)];
            }
            RFN_TRY(rfn_x3_split(srcs, T1, Di, A, Di, 1, imgW, st));
            RFN_TRY(probe_mark(d, 2 * i, st));
            RFN_TRY(rfn_x3_gemm(BL, T1 * A, Di, imgX, imgW, BL, A, outs, bias, A, 0, 1, nullptr, st));
            RFN_TRY(probe_mark(d, 2 * i + 1, st));
            continue;
        }
        for (int t = 0; t < T1; ++t)
            pr[t] = prob1(W + Lo.P1[i] + (long)t * B * d->L[i] * A, A,
                          seg_lin(att[i], d->D[i], prm[P.s1(t, i, 0)], d->D[i], d->D[i], prm[P.s1(t, i, 1)]));
        RFN_TRY(probe_mark(d, 2 * i, st));
        RFN_TRY(gemm_groups(B * d->L[i], A, T1, pr, 0, gx));
        RFN_TRY(probe_mark(d, 2 * i + 1, st));
    }
    return RFN_OK;
}

void Prefix::s1_attn_of(int t, S1Attn* a) const {
    a->same_ld = M > 1;
    for (int i = 1; i < M; ++i) a->same_ld = a->same_ld && d->L[i] == d->L[0] && d->D[i] == d->D[0];
    a->sc_floats = 0;
    a->ragged = false;
    for (int i = 0; i < M; ++i) {
        a->len[i] = att_len ? att_len[i] : nullptr;
        a->ragged = a->ragged || a->len[i];
        const long Li = d->L[i], Di = d->D[i], ti = (long)t * M + i;
        a->p[i] = W + Lo.P1[i] + (long)t * B * Li * A;
        a->hp[i] = W + Lo.hp1 + ti * BA;
        a->w[i] = prm[P.s1(t, i, 4)];
        a->b[i] = prm[P.s1(t, i, 5)];
        a->sc[i] = W + Lo.gws + a->sc_floats;   // slabs of different sizes (het form) start on 16-byte boundaries
        a->sc_floats += a->same_ld ? (size_t)B * Li : ((size_t)B * Li + 3) & ~(size_t)3;
        a->al[i] = W + Lo.al1[i] + (long)t * B * Li;
        a->z[i] = W + Lo.z1[i] + (long)t * B * Di;
        a->dz[i] = W + Lo.dz1[i] + t * Lo.dz1_st[i];
        a->dhp[i] = W + Lo.dhp1 + ti * BA;
        a->dw[i] = dwp + ti * BA;
        a->img[i] = W + Lo.x3p[i];
        a->L[i] = (int)Li;
        a->D[i] = (int)Di;
    }
}

// ---- stage I, step t: M cells (:213-217, :101-114, :47-74) ---------------------------
int Prefix::s1_fwd_step(int t) {
    float* Hc = Hs + t * BMR;
    float* Hn = Hs + (t + 1) * BMR;
    float* Cc = Cs + t * BMR;
    float* Cn = Cs + (t + 1) * BMR;
    float* hp = W + Lo.hp1 + (long)t * M * B * A;
    float* g = W + Lo.g1 + (long)t * M * B * 4 * R;
    rfn_cell_out k[RFN_MAX_ENC];
    // h_2_att_h of the M cells: one launch, encoder i's own h = column block i of H
    for (int i = 0; i < M; ++i) {
        k[i] = cell_out(hp + (long)i * B * A, A, A, 0);
        cell_lin(k[i], Hc + i * R, MR, prm[P.s1(t, i, 2)], R, R, prm[P.s1(t, i, 3)]);
    }
    if (cell_ok(B, M, k, R)) {
        RFN_TRY(cell_run(B, M, k, R, 0.f, RfnSeed{}, st, cell_variant(d)));
    } else {
        for (int i = 0; i < M; ++i) pr[i] = prob1(k[i].C, A, k[i].seg[0]);
        RFN_TRY(gemm_groups(B, A, M, pr, 0, gx));
    }
    // attention of the M encoders: one grouped pair of launches when they share (L, D), one heterogeneous pair otherwise.
    // Raw scores land in the (idle) split-K scratch; the context kernel normalises them on the fly.
    S1Attn a;
    s1_attn_of(t, &a);
    if (a.sc_floats > GEMM_WS_FLOATS) return RFN_ERR_SHAPE;
    const long L0 = d->L[0], D0 = d->D[0];
    if (a.ragged)   // per-image row counts: the contiguous-layout launch pair takes them for any mix of maps (one encoder included)
        RFN_TRY(rfn_attn_fwd_ragged(M, a.p, a.hp, a.w, a.b, att, B, a.L, A, a.D, a.sc, a.al, a.z, a.len, st));
    else if (a.same_ld)
        RFN_TRY(rfn_attn_fwd_grouped(M, a.p, L0 * A, (long)A, a.hp, a.w, a.b, att, L0 * D0, D0, B, (int)L0, A, (int)D0, a.sc, a.al,
                                     a.z, D0, st));
    else if (M > 1)   // maps of different (L, D): still one pair of launches
        RFN_TRY(rfn_attn_fwd_het(M, a.p, a.hp, a.w, a.b, att, B, a.L, A, a.D, a.sc, a.al, a.z, st));
    else
        RFN_TRY(rfn_attn_fwd(a.p[0], L0 * A, (long)A, a.hp[0], a.w[0], a.b[0], att[0], L0 * D0, D0, B, (int)L0, A, (int)D0, a.sc[0],
                             a.al[0], a.z[0], D0, st));
    // gates_i = H2h_i(H) + z2h_i(z_i), then the LSTM update of cell (t, i): encoder i's state is column block i of the (B, M*R) rows
    for (int i = 0; i < M; ++i) {
        k[i] = cell_out(g + (long)i * B * 4 * R, 4 * R, 4 * R, 0);
        cell_lin(k[i], Hc, MR, prm[P.s1(t, i, 6)], MR, (int)MR, prm[P.s1(t, i, 7)]);
        cell_lin(k[i], a.z[i], a.D[i], prm[P.s1(t, i, 8)], a.D[i], a.D[i], prm[P.s1(t, i, 9)]);
        cell_lstm(k[i], Cc + i * R, MR, Cn + i * R, MR, Hn + i * R, MR, (uint64_t)(t * M + i));
    }
    // Small batches (BASELINE config 2, the shards of a strong-scaled batch): the M gate products in ONE cell-GEMM launch
    // with the LSTM update as its epilogue (no split-K partials, no reduce launch) -- when the launch's 32-row tiles do not
    // outnumber the CUs two to one; beyond that the 128 x 128 split-K kernel below is the faster one (17 GFLOP per step at C3).
    if ((long)rfn_cdiv(B, 32) * M * (4 * R / 32) <= 2L * stage1_cell_cus() && cell_ok(B, M, k, R))
        return cell_run(B, M, k, R, d->drop_fusion, seed, st, cell_variant(d));
    // gate GEMM of the M cells (grouped) with the LSTM update riding on its split-K reduce
    for (int i = 0; i < M; ++i) {
        rfn_gemm_problem& p = pr[i];
        memset(&p, 0, sizeof(p));
        p.C = k[i].C;
        p.ldc = 4 * R;
        p.nseg = 2;
        p.seg[0] = k[i].seg[0];
        p.seg[1] = k[i].seg[1];
    }
    rfn_gemm_lstm lu;
    memset(&lu, 0, sizeof(lu));
    lu.c_prev = Cc; lu.c_next = Cn; lu.h_next = Hn;
    lu.ldcp = lu.ldcn = lu.ldh = MR;
    lu.gs_cprev = lu.gs_cnext = lu.gs_h = R;
    lu.drop_p = d->drop_fusion; lu.seed = seed.val; lu.offset = (uint64_t)(t * M);
    return rfn_gemm_f32_lstm(B, R, M, pr, gx.ws, gx.ws_bytes, gx.flags, &lu, seed.dev, st);
}

int Prefix::s1_heads_and_mean(float* reason_pred) {
    // reason heads of stage I: max over steps of reason_linear_individual (:217, :229)
    for (int i = 0; i < M; ++i)   // all encoders' heads: one grouped GEMM into M slabs, one max-over-steps launch
        pr[i] = prob1(rmat + (long)i * T1 * B * K, K,
                      seg_lin(Hs + BMR + i * R, MR, prm[P.rind_w(i)], R, R, prm[P.rind_b(i)]));
    RFN_TRY(gemm_groups(T1 * B, K, M, pr, 0, gx));
    RFN_TRY(rfn_max_over_steps_fwd_grouped(rmat, T1, B, K, reason_pred, rarg, M, st));
    // state mean over encoders (:233-235): sum first, then divide, as the reference does
    const float* mx[2] = {Hs + T1 * BMR, Cs + T1 * BMR};
    float* my[2] = {h2, c2};
    return rfn_mean_over_groups(2, mx, MR, R, M, my, R, B, R, st);
}

// hoisted thought projections of stage II: rows (t', b) of encoder i's thoughts = Hs[1:]
int Prefix::s2_projections() {
    for (int i = 0; i < M; ++i) {
        if (T2 > 64) return RFN_ERR_SHAPE;
        for (int t = 0; t < T2; ++t)
            pr[t] = prob1(W + Lo.P2[i] + (long)t * A, (long)T2 * A,
                          seg_lin(Hs + BMR + i * R, MR, prm[P.s2(t, i, 2)], R, R, prm[P.s2(t, i, 3)]));
        RFN_TRY(gemm_groups(T1 * B, A, T2, pr, 0, gx));
    }
    return RFN_OK;
}

void Prefix::s2_fwd_of(int t, S2Fwd* s) const {
    float* hc = h2 + t * BR;
    float* z = W + Lo.z2 + (long)t * M * BR;
    float* g = W + Lo.g2 + (long)t * B * G2;
    s->k1[M] = cell_out(g, G2, G2, 0);
    cell_lin(s->k1[M], hc, R, prm[P.s2_hh_w(t)], R, R, prm[P.s2_hh_b(t)]);
    s->k3 = cell_out(g, G2, G2, 1);
    for (int i = 0; i < M; ++i) {
        s->p[i] = W + Lo.P2[i] + (long)t * A;
        s->hp[i] = W + Lo.hp2 + ((long)t * M + i) * BA;
        s->w[i] = prm[P.s2(t, i, 6)];
        s->b[i] = prm[P.s2(t, i, 7)];
        s->x[i] = Hs + BMR + i * R;   // thoughts_i[b, l] = Hs[1 + l][b, iR:]
        s->al[i] = W + Lo.al2 + ((long)t * M + i) * B * T1;
        s->z[i] = z + i * BR;
        s->k1[i] = cell_out(W + Lo.hp2 + ((long)t * M + i) * BA, A, A, 0);
        cell_lin(s->k1[i], hc, R, prm[P.s2(t, i, 4)], R, R, prm[P.s2(t, i, 5)]);
        cell_lin(s->k3, z + i * BR, R, prm[P.s2(t, i, 0)], R, R, prm[P.s2(t, i, 1)]);
    }
    cell_lstm(s->k3, c2 + t * BR, R, c2 + (t + 1) * BR, R, hc + BR, R, OFF_STAGE2 + (uint64_t)t);
    s->fused = !d->review_maxout && cell_ok(B, M + 1, s->k1, R) && cell_ok(B, 1, &s->k3, R);
}

// ---- stage II: T2 steps (:241-244, LSTMSoftMultiAttentionFeatArrayNoInputCore.py:41-73) ---
// When every step takes the fused form the T2 steps run as one chain (inside one persistent launch if asked for, rfn_chain.hip).
int Prefix::s2_fwd_sweep() {
    S2Fwd s;
    {
        std::vector<ChainStep> steps((size_t)T2);
        bool ok = true;
        for (int t = 0; t < T2 && ok; ++t) {
            s2_fwd_of(t, &s);
            ok = s.fused && cell_prepare(B, M + 1, s.k1, R, 0.f, RfnSeed{}, &steps[t].g0, cell_variant(d)) == RFN_OK &&
                 rfn_attn_small_prepare_fwd(M, s.p, (long)T2 * A, (long)B * T2 * A, s.hp, s.w, s.b, s.x, MR, BMR, B, T1, A, R, s.al, s.z,
                                            R, &steps[t].at) == RFN_OK &&
                 cell_prepare(B, 1, &s.k3, R, d->drop_reason, seed, &steps[t].g2, cell_variant(d)) == RFN_OK;
        }
        if (ok) return rfn_chain_run(steps.data(), T2, chain_persist(d, RFN_PATH_OPT_PERSIST_S2_FWD), (uint32_t*)(W + Lo.bar), st);
    }
    for (int t = 0; t < T2; ++t) {
        s2_fwd_of(t, &s);
        if (s.fused) {
            RFN_TRY(cell_run(B, M + 1, s.k1, R, 0.f, RfnSeed{}, st, cell_variant(d)));
        } else {
            for (int i = 0; i < M; ++i) pr[i] = prob1(s.k1[i].C, A, s.k1[i].seg[0]);
            RFN_TRY(gemm_groups(B, A, M, pr, 0, gx));
        }
        RFN_TRY(rfn_attn_small_fwd(M, s.p, (long)T2 * A, (long)B * T2 * A, s.hp, s.w, s.b, s.x, MR, BMR, B, T1, A, R, s.al, s.z, R, st));
        if (s.fused) {
            RFN_TRY(cell_run(B, 1, &s.k3, R, d->drop_reason, seed, st, cell_variant(d)));
        } else {   // gates = h2h(h) + sum_i z_2_h_i(z_i) as one product of M + 1 K segments, then the LSTM update
            float* g = W + Lo.g2 + (long)t * B * G2;
            segs[0] = s.k1[M].seg[0];
            for (int i = 0; i < M; ++i) segs[1 + i] = s.k3.seg[i];
            RFN_TRY(gemm_segs(B, G2, M + 1, segs, g, G2, 0, gx));
            RFN_TRY(rfn_lstm_fwd(g, G2, c2 + t * BR, R, c2 + (t + 1) * BR, R, h2 + (t + 1) * BR, R, B, R, d->review_maxout,
                                 d->drop_reason, seed, OFF_STAGE2 + (uint64_t)t, st));
        }
    }
    return RFN_OK;
}

// ---- reason head of stage II (:244, :253) -------------------------------------------------
int Prefix::s2_head_bwd(const float* d_comb, const float* d_reason) {
    RFN_TRY(rfn_max_over_steps_bwd(d_reason ? d_reason + (long)M * B * K : nullptr, rarg + (long)M * B * K, T2, B, K, rmat, st));
    // d thoughts from the decoder (or zero) into the slab the reason head accumulates onto; d H of stage I zeroed: it
    // collects thoughts (through stage II) + reason heads + mean
    RFN_TRY(mem_batch({{dh2e, d_comb, (long)T2 * BR}, {dHs, nullptr, (long)(T1 + 1) * BMR}}, st));
    RFN_TRY(gemm1(T2 * B, R, seg_dx(rmat, K, prm[P.r_w()], R, K), dh2e, R, 1, gx));
    return gemm_dw(K, R, grd[P.r_w()], R, grd[P.r_b()], rmat, K, h2 + BR, R, T2 * B, gx);
}

void Prefix::s2_bwd_of(int t, S2Bwd* s) const {
    float* g = W + Lo.g2 + (long)t * B * G2;
    s->kb1[0] = cell_out(dhrec, R, R, 0);
    cell_dx(s->kb1[0], g, G2, prm[P.s2_hh_w(t)], R, G2);
    s->kb2 = cell_out(dhrec, R, R, 1);
    for (int i = 0; i < M; ++i) {
        const long ti = (long)t * M + i;
        s->p[i] = W + Lo.P2[i] + (long)t * A;
        s->hp[i] = W + Lo.hp2 + ti * BA;
        s->w[i] = prm[P.s2(t, i, 6)];
        s->al[i] = W + Lo.al2 + ti * B * T1;
        s->x[i] = Hs + BMR + i * R;   // thoughts_i[b, l] = Hs[1 + l][b, iR:]
        s->dz[i] = dz2 + i * BR;
        s->dhp[i] = W + Lo.dhp2 + ti * BA;
        s->dw[i] = dwp + ti * BA;
        s->dx[i] = dHs + BMR + i * R;
        s->kb1[1 + i] = cell_out(dz2 + i * BR, R, R, 0);
        cell_dx(s->kb1[1 + i], g, G2, prm[P.s2(t, i, 0)], R, G2);
        cell_dx(s->kb2, s->dhp[i], A, prm[P.s2(t, i, 4)], R, A);
    }
    if (t > 0)
        cell_lstm_bwd(s->kb2, W + Lo.g2 + (long)(t - 1) * B * G2, G2, c2 + (t - 1) * BR, R, c2 + t * BR, R, dh2e + (t - 1) * BR, R,
                      dc2, R, dc2, R, OFF_STAGE2 + (uint64_t)(t - 1));
}

// ---- stage II backward ------------------------------------------------------------------------
// The operands of EVERY step are validated before the fused form is chosen (each step has its own weights and slabs;
// a step the cell GEMM cannot take must not be discovered mid-sweep, when the gates are already gate gradients).
int Prefix::s2_bwd_sweep(const float* d_h, const float* d_c) {
    S2Bwd s;
    bool fused = !d->review_maxout;
    for (int t = 0; t < T2 && fused; ++t) {
        s2_bwd_of(t, &s);
        fused = cell_ok(B, M + 1, s.kb1, R) && cell_ok(B, 1, &s.kb2, R);
    }
    // LSTM backward of step t as a launch of its own (unfused: every step; fused: the last one, which gets only the external
    // gradients -- thoughts, reason head, decoder state)
    auto lstm_bwd_of = [&](int t) {
        return rfn_lstm_bwd(W + Lo.g2 + (long)t * B * G2, G2, c2 + t * BR, R, c2 + (t + 1) * BR, R, dh2e + t * BR, R,
                            (t == T2 - 1) ? d_c : dc2, R, dc2, R, B, R, d->review_maxout, d->drop_reason, seed, OFF_STAGE2 + (uint64_t)t, st);
    };
    if (fused) {
        if (d_h) RFN_TRY(rfn_axpby_2d(1.f, d_h, R, 1.f, dh2e + (T2 - 1) * BR, R, B, R, st));
        RFN_TRY(lstm_bwd_of(T2 - 1));
    }
    int t_hi = T2 - 1;
    if (fused && T2 >= 3) {
        // steps T2-1 ... 1 in one persistent launch (rfn_chain.hip); step 0, whose Kb2 is a plain accumulate, follows as launches
        std::vector<ChainStep> steps((size_t)(T2 - 1));
        bool ok = true;
        for (int t = T2 - 1; t >= 1 && ok; --t) {
            ChainStep& cs = steps[(size_t)(T2 - 1 - t)];
            s2_bwd_of(t, &s);
            ok = cell_prepare(B, M + 1, s.kb1, R, 0.f, RfnSeed{}, &cs.g0, cell_variant(d)) == RFN_OK &&
                 rfn_attn_small_prepare_bwd(M, s.p, (long)T2 * A, (long)B * T2 * A, s.hp, s.w, s.al, s.x, MR, BMR, s.dz, R, B, T1, A, R,
                                            s.p, (long)T2 * A, (long)B * T2 * A, 0, s.dhp, s.dw, s.dx, &cs.at) == RFN_OK &&
                 cell_prepare(B, 1, &s.kb2, R, d->drop_reason, seed, &cs.g2, cell_variant(d)) == RFN_OK;
        }
        if (ok) {
            RFN_TRY(rfn_chain_run(steps.data(), T2 - 1, chain_persist(d, RFN_PATH_OPT_PERSIST_S2_BWD), (uint32_t*)(W + Lo.bar), st));
            t_hi = 0;
        }
    }
    for (int t = t_hi; t >= 0; --t) {
        s2_bwd_of(t, &s);
        if (!fused) {
            float* dht = dh2e + t * BR;  // total dh of h2[t+1]
            if (t < T2 - 1) RFN_TRY(rfn_axpby_2d(1.f, dhrec, R, 1.f, dht, R, B, R, st));
            else if (d_h) RFN_TRY(rfn_axpby_2d(1.f, d_h, R, 1.f, dht, R, B, R, st));
            RFN_TRY(lstm_bwd_of(t));
            // dh_rec = dgates . W_hh ; dz_i = dgates . W_z_i   (same shape: one grouped launch)
            for (int i = 0; i <= M; ++i) pr[i] = prob1(s.kb1[i].C, R, s.kb1[i].seg[0]);
            RFN_TRY(gemm_groups(B, R, M + 1, pr, 0, gx));
        } else {
            RFN_TRY(cell_run(B, M + 1, s.kb1, R, 0.f, RfnSeed{}, st, cell_variant(d)));
        }
        RFN_TRY(rfn_attn_small_bwd(M, s.p, (long)T2 * A, (long)B * T2 * A, s.hp, s.w, s.al, s.x, MR, BMR, s.dz, R, B, T1, A, R, s.p,
                                   (long)T2 * A, (long)B * T2 * A, 0, s.dhp, s.dw, s.dx, st));
        if (!fused) RFN_TRY(gemm_segs(B, R, M, s.kb2.seg, dhrec, R, 1, gx));
        else RFN_TRY(cell_run(B, 1, &s.kb2, R, d->drop_reason, seed, st, cell_variant(d)));
    }
    return RFN_OK;
}

// weight gradients of stage II, grouped over steps; every bias gradient rides on the GEMM that streams
// the same dY (h2h.b = z_2_h[i].b = colsum(dgates); h_2_att_h.b = att_2_att_h.b = colsum over (b) resp. (l,b))
int Prefix::s2_wgrad() {
    {
        float* outs[64];
        for (int t = 0; t < T2; ++t)
            for (int i = 0; i < M; ++i) outs[t * M + i] = grd[P.s2(t, i, 6)];
        if (T2 * M > 64) return RFN_ERR_SHAPE;
        RFN_TRY(rfn_colsum_grouped_f32(dwp, BA, A, B, A, outs, T2 * M, st));
        // att_h_2_out.bias shifts all scores of a softmax equally: its gradient is exactly 0
        for (int t = 0; t < T2; ++t)
            for (int i = 0; i < M; ++i) outs[t * M + i] = grd[P.s2(t, i, 7)];
        RFN_TRY(rfn_fill_small_f32(outs, T2 * M, 1, 0.f, st));
    }
    for (int t = 0; t < T2; ++t)
        pr[t] = prob_dw(grd[P.s2_hh_w(t)], R, grd[P.s2_hh_b(t)], W + Lo.g2 + (long)t * B * G2, G2, h2 + t * BR, R, B);
    RFN_TRY(gemm_groups(G2, R, T2, pr, 0, gx));
    for (int i = 0; i < M; ++i) {
        for (int t = 0; t < T2; ++t)
            pr[t] = prob_dw(grd[P.s2(t, i, 0)], R, grd[P.s2(t, i, 1)], W + Lo.g2 + (long)t * B * G2, G2,
                            W + Lo.z2 + ((long)t * M + i) * BR, R, B);
        RFN_TRY(gemm_groups(G2, R, T2, pr, 0, gx));
        for (int t = 0; t < T2; ++t)
            pr[t] = prob_dw(grd[P.s2(t, i, 4)], R, grd[P.s2(t, i, 5)], W + Lo.dhp2 + ((long)t * M + i) * BA, A,
                            h2 + t * BR, R, B);
        RFN_TRY(gemm_groups(A, R, T2, pr, 0, gx));
        // d att_2_att_h.weight[t] = dP2_i[:, t]^T . thoughts_i   (K = T1*B rows)
        for (int t = 0; t < T2; ++t)
            pr[t] = prob_dw(grd[P.s2(t, i, 2)], R, grd[P.s2(t, i, 3)], W + Lo.P2[i] + (long)t * A, (long)T2 * A,
                            Hs + BMR + i * R, MR, T1 * B);
        RFN_TRY(gemm_groups(A, R, T2, pr, 0, gx));
        // d thoughts_i += sum_t dP2_i[:, t] . W_a[t]
        for (int t = 0; t < T2; ++t) segs[t] = seg_dx(W + Lo.P2[i] + (long)t * A, (long)T2 * A, prm[P.s2(t, i, 2)], R, A);
        RFN_TRY(gemm_segs(T1 * B, R, T2, segs, dHs + BMR + i * R, MR, 1, gx));
    }
    return RFN_OK;
}

int Prefix::mean_and_s1_heads_bwd(const float* d_reason) {
    // ---- state mean backward (:233-235): every encoder's final (h, c) gets d / M --------------------
    const float invM = 1.0f / (float)M;
    const float* bx[2] = {dhrec, dc2};
    float* by[2] = {dHs + T1 * BMR, dC};
    const float bb[2] = {1.f, 0.f};
    RFN_TRY(rfn_bcast_to_groups(2, invM, bx, R, bb, by, MR, R, M, B, R, st));
    // ---- reason heads of stage I ----------------------------------------------------------------------
    RFN_TRY(rfn_max_over_steps_bwd_grouped(d_reason, rarg, T1, B, K, rmat, M, st));
    for (int i = 0; i < M; ++i)
        pr[i] = prob1(dHs + BMR + i * R, MR, seg_dx(rmat + (long)i * T1 * B * K, K, prm[P.rind_w(i)], R, K));
    RFN_TRY(gemm_groups(T1 * B, R, M, pr, 1, gx));
    for (int i = 0; i < M; ++i)
        pr[i] = prob_dw(grd[P.rind_w(i)], R, grd[P.rind_b(i)], rmat + (long)i * T1 * B * K, K, Hs + BMR + i * R, MR,
                        T1 * B);
    return gemm_groups(K, R, M, pr, 0, gx);
}

// ---- stage I backward --------------------------------------------------------------------------------
// Small batches (BASELINE config 2, the shards of a strong-scaled batch) take three launches per step instead of seven:
//   X  every product of the step's gate gradients in ONE cell-GEMM launch: the M partial slabs d gates_j . W_H[t,j] of
//      d H_t (each cell reads the whole concatenated H, :53) and the M d z_i = d gates_i . W_z[t,i];
//   the attention backward of the M encoders (unchanged);
//   Y  d H_t[:, i] = external + sum_j slab_j[:, i] + d hproj_i . W_h[t,i], whose epilogue runs the LSTM backward of cell
//      (t-1, i) -- the next thing the sweep needs (no split-K partials, no reduce / axpby / lstm launches).
// Taken while the X launch's 32-row tiles do not outnumber the CUs two to one and every product fits the cell GEMM.
void Prefix::s1_dz_of(int t, rfn_cell_out* kz) const {   // dz_i = dgates_i . W_z[t,i], an output each
    for (int i = 0; i < M; ++i) {
        kz[i] = cell_out(W + Lo.dz1[i] + t * Lo.dz1_st[i], d->D[i], d->D[i], 0);
        cell_dx(kz[i], W + Lo.g1 + ((long)t * M + i) * B * 4 * R, 4 * R, prm[P.s1(t, i, 8)], d->D[i], 4 * R);
    }
}
void Prefix::s1x_of(int t, rfn_cell_out* kx) const {
    for (int j = 0; j < M; ++j) {
        kx[j] = cell_out(W + Lo.dHpart + (long)j * BMR, MR, (int)MR, 0);
        cell_dx(kx[j], W + Lo.g1 + ((long)t * M + j) * B * 4 * R, 4 * R, prm[P.s1(t, j, 6)], MR, 4 * R);
    }
    s1_dz_of(t, kx + M);
}
// dH_t[:, i] += d hproj_i . W_h[t,i]; small: + the M slabs of X, with the LSTM backward of cell (t-1, i) as its epilogue
void Prefix::s1y_of(int t, bool small, rfn_cell_out* ky) const {
    for (int i = 0; i < M; ++i) {
        ky[i] = cell_out(dHs + t * BMR + i * R, MR, R, 1);
        cell_dx(ky[i], W + Lo.dhp1 + ((long)t * M + i) * BA, A, prm[P.s1(t, i, 2)], R, A);
        if (!small) continue;
        ky[i].acc_slabs = W + Lo.dHpart + i * R;
        ky[i].acc_parts = M;
        ky[i].acc_stride = BMR;
        if (t > 0)
            cell_lstm_bwd(ky[i], W + Lo.g1 + ((long)(t - 1) * M + i) * B * 4 * R, 4 * R, Cs + (t - 1) * BMR + i * R, MR,
                          Cs + t * BMR + i * R, MR, nullptr, 0, dC + i * R, MR, dC + i * R, MR, (uint64_t)((t - 1) * M + i));
    }
}
bool Prefix::s1_small_steps() const {
    bool small = 2 * M <= RFN_CELL_MAXOUT && M <= 8;
    long cols = (long)M * (MR / 32);
    for (int i = 0; i < M; ++i) cols += d->D[i] / 32;
    small = small && (long)rfn_cdiv(B, 32) * cols <= 2L * stage1_cell_cus();
    for (int t = 0; t < T1 && small; ++t) {
        rfn_cell_out tx[2 * RFN_MAX_ENC], ty[RFN_MAX_ENC];
        s1x_of(t, tx);
        s1y_of(t, true, ty);
        // step 0's Y is a plain accumulate, the others carry the gate-gradient epilogue: one epilogue per launch
        small = cell_ok(B, 2 * M, tx, R) && cell_ok(B, M, ty, R);
    }
    return small;
}
int Prefix::s1_bwd_step(int t, bool small) {
    float* dHn = dHs + (t + 1) * BMR;  // total gradient of Hs[t+1]
    float* dHc = dHs + t * BMR;        // external gradient of Hs[t]; the recurrent part is added here
    float* g = W + Lo.g1 + (long)t * M * B * 4 * R;
    rfn_cell_out k[2 * RFN_MAX_ENC];
    rfn_cell_out* kz = small ? k + M : k;   // the dz products: the second half of X, or a launch of their own
    if (!small || t == T1 - 1)
        RFN_TRY(rfn_lstm_bwd_grouped(g, 4 * R, Cs + t * BMR, MR, Cs + (t + 1) * BMR, MR, dHn, MR, dC, MR, dC, MR, B, R, 0,
                                     d->drop_fusion, seed, (uint64_t)(t * M), M, (long)B * 4 * R, R, R, R, st));
    bool same_d = true;
    for (int i = 1; i < M; ++i) same_d = same_d && d->D[i] == d->D[0];
    bool dz_done = (same_d && M > 1) || small;
    if (small) {
        s1x_of(t, k);
        RFN_TRY(cell_run(B, 2 * M, k, R, 0.f, RfnSeed{}, st, cell_variant(d)));
    } else {
        // dH_t += sum_i dgates_i . W_H[t,i]   (every cell reads the whole concatenated H, :53)
        for (int i = 0; i < M; ++i) segs[i] = seg_dx(g + (long)i * B * 4 * R, 4 * R, prm[P.s1(t, i, 6)], MR, 4 * R);
        RFN_TRY(gemm_segs(B, (int)MR, M, segs, dHc, MR, 1, gx));
        s1_dz_of(t, kz);
        if (same_d && M > 1) {   // one grouped launch when the encoders share a feature width
            for (int i = 0; i < M; ++i) pr[i] = prob1(kz[i].C, d->D[0], kz[i].seg[0]);
            RFN_TRY(gemm_groups(B, d->D[0], M, pr, 0, gx));
        } else if (M > 1 && cell_ok(B, M, kz, R)) {   // heterogeneous feature widths: the M products still share one launch
            RFN_TRY(cell_run(B, M, kz, R, 0.f, RfnSeed{}, st, cell_variant(d)));
            dz_done = true;
        }
    }
    S1Attn a;
    s1_attn_of(t, &a);
    const long L0 = d->L[0], D0 = d->D[0];
    const AttnBwdForm form0 = attn_bwd_form(d, B, 0, dz_done);
    if (a.ragged && (form0 == AB_GROUPED || form0 == AB_HET))   // same launch as either form (contiguous layouts), with row counts
        RFN_TRY(rfn_attn_bwd_ragged(M, a.p, a.hp, a.w, a.al, att, a.dz, B, a.L, A, a.D, a.p, 0, a.dhp, a.dw, a.len, st));
    else if (form0 == AB_GROUPED_KS)   // all encoders' attention backward of this step: one launch; dP1 straight into the k-slow plane images
        RFN_TRY(rfn_attn_bwd_grouped_ks(M, a.p, L0 * A, (long)A, a.hp, a.w, a.al, att, L0 * D0, D0, a.dz, D0, B, (int)L0, A, (int)D0,
                                        a.img, x3_row_pad(T1 * A), t * A, a.dhp, a.dw, st));
    else if (form0 == AB_GROUPED)
        RFN_TRY(rfn_attn_bwd_grouped(M, a.p, L0 * A, (long)A, a.hp, a.w, a.al, att, L0 * D0, D0, a.dz, D0, B, (int)L0, A, (int)D0, a.p,
                                     L0 * A, (long)A, 0, a.dhp, a.dw, st));
    else if (form0 == AB_HET)   // maps of different (L, D): the M attention backwards of this step in one launch
        RFN_TRY(rfn_attn_bwd_het(M, a.p, a.hp, a.w, a.al, att, a.dz, B, a.L, A, a.D, a.p, 0, a.dhp, a.dw, st));
    else
        for (int i = 0; i < M; ++i) {   // encoder by encoder
            const long Li = a.L[i], Di = a.D[i];
            if (!dz_done) RFN_TRY(gemm1(B, (int)Di, kz[i].seg[0], a.dz[i], Di, 0, gx));
            const AttnBwdForm form = attn_bwd_form(d, B, i, dz_done);
            if (a.ragged && form != AB_FUSED_KS) {   // the one-launch form also where the two-kernel pair would run: it has no ragged form
                RFN_TRY(rfn_attn_bwd_ragged(1, a.p + i, a.hp + i, a.w + i, a.al + i, att + i, a.dz + i, B, a.L + i, A, a.D + i, a.p + i,
                                            0, a.dhp + i, a.dw + i, a.len + i, st));
            } else if (form == AB_FUSED_KS) {   // d alpha stays in LDS, dP1 as bf16 planes
                RFN_TRY(rfn_attn_bwd_grouped_ks(1, a.p + i, Li * A, (long)A, a.hp + i, a.w + i, a.al + i, att + i, Li * Di, Di, a.dz + i,
                                                Di, B, (int)Li, A, (int)Di, a.img + i, x3_row_pad(T1 * A), t * A, a.dhp + i, a.dw + i, st));
            } else if (form == AB_FUSED) {   // d alpha stays in LDS, one launch
                RFN_TRY(rfn_attn_bwd(a.p[i], Li * A, (long)A, a.hp[i], a.w[i], a.al[i], att[i], Li * Di, Di, a.dz[i], Di, B, (int)Li, A,
                                     (int)Di, a.p[i], Li * A, (long)A, 0, a.dhp[i], a.dw[i], st));
            } else {
                float* dali = dal + (long)i * B * Li;
                RFN_TRY(rfn_attn_context_bwd_dalpha(att[i], Li * Di, Di, a.dz[i], Di, B, (int)Li, (int)Di, dali, st));
                RFN_TRY(rfn_attn_scores_bwd(a.p[i], Li * A, (long)A, a.hp[i], a.w[i], a.al[i], dali, B, (int)Li, A, a.p[i], Li * A,
                                            (long)A, 0, a.dhp[i], a.dw[i], st));
            }
        }
    s1y_of(t, small, k);
    if (small) return cell_run(B, M, k, R, d->drop_fusion, seed, st, cell_variant(d));
    if (cell_ok(B, M, k, R)) return cell_run(B, M, k, R, 0.f, RfnSeed{}, st, cell_variant(d));
    for (int i = 0; i < M; ++i) pr[i] = prob1(k[i].C, MR, k[i].seg[0]);
    return gemm_groups(B, R, M, pr, 1, gx);
}

// c0 = h0.clone() (:206): dh0 += dc0 ; fc2h gradients; the attention output layers of stage I
int Prefix::s1_bwd_tail(const float* const* fc) {
    RFN_TRY(rfn_axpby_2d(1.f, dC, MR, 1.f, dHs, MR, B, (int)MR, st));
    for (int i = 0; i < M; ++i)
        RFN_TRY(gemm_dw(R, d->F[i], grd[P.fc_w(i)], d->F[i], grd[P.fc_b(i)], dHs + i * R, MR, fc[i], d->F[i], B, gx));
    float* outs[64];
    if (T1 * M > 64) return RFN_ERR_SHAPE;
    for (int t = 0; t < T1; ++t)
        for (int i = 0; i < M; ++i) outs[t * M + i] = grd[P.s1(t, i, 4)];
    RFN_TRY(rfn_colsum_grouped_f32(dwp, BA, A, B, A, outs, T1 * M, st));
    for (int t = 0; t < T1; ++t)
        for (int i = 0; i < M; ++i) outs[t * M + i] = grd[P.s1(t, i, 5)];
    return rfn_fill_small_f32(outs, T1 * M, 1, 0.f, st);
}
}  // namespace

// Per-image row counts of the stage-I maps (rfn.h, rfn_prefix_fwd_ex): the forms that were not taught them are refused
// here, before anything is launched -- never run with the lengths ignored.
static int check_att_len(const rfn_dims* d, int B, const int32_t* const* att_len) {
    bool any = false;
    for (int i = 0; att_len && i < d->M; ++i) any = any || att_len[i];
    if (!any) return RFN_OK;
    if (d->path_flags & (RFN_PATH_OPT_PERSIST_S2_FWD | RFN_PATH_OPT_PERSIST_S2_BWD)) return RFN_ERR_UNSUPPORTED;
    for (int i = 0; i < d->M; ++i)   // dP1 as bf16 planes from the attention backward (rfn_attn_bwd_grouped_ks)
        if (att_len[i] && x3_dp_emitted(d, B, i)) return RFN_ERR_UNSUPPORTED;
    return RFN_OK;
}

static int prefix_fwd_impl(const rfn_dims* d, int B, const float* const* prm, const float* const* fc,
                           const float* const* init_h, const float* const* init_c, const float* const* att,
                           float* comb, float* h_out, float* c_out, float* reason_pred, void* ws, size_t ws_bytes,
                           int train, RfnSeed seed, const int32_t* const* att_len, void* st) {
    RFN_TRY(check_dims(d));
    if (B < 1) return RFN_ERR_SHAPE;
    if (!prm || (!fc && !(init_h && init_c)) || !att || !ws) return RFN_ERR_ARG;
    RFN_TRY(check_att_len(d, B, att_len));
    const PrefixLayout Lo = prefix_layout(d, B, train);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    Prefix c(d, B, prm, att, ws, Lo, seed, st);
    c.att_len = att_len;
    RFN_TRY(phase_gemm(d, c.W, Lo.gws, Lo.tk, true, st, &c.gx));
    RFN_TRY(c.init_state(fc, init_h, init_c));
    RFN_TRY(c.s1_projections());
    for (int t = 0; t < c.T1; ++t) RFN_TRY(c.s1_fwd_step(t));
    RFN_TRY(c.s1_heads_and_mean(reason_pred));
    RFN_TRY(c.s2_projections());
    RFN_TRY(c.s2_fwd_sweep());
    const int M = c.M, T2 = c.T2, K = c.K, R = c.R;
    const long BR = c.BR;
    RFN_TRY(gemm1(T2 * B, K, seg_lin(c.h2 + BR, R, prm[c.P.r_w()], R, R, prm[c.P.r_b()]), c.rmat, K, 0, c.gx));
    RFN_TRY(rfn_max_over_steps_fwd(c.rmat, T2, B, K, reason_pred + (long)M * B * K, c.rarg + (long)M * B * K, st));
    return mem_batch({{comb, c.h2 + BR, (long)T2 * BR}, {h_out, c.h2 + (long)T2 * BR, BR}, {c_out, c.c2 + (long)T2 * BR, BR}}, st);
}

extern "C" int rfn_prefix_fwd_ex(const rfn_dims* d, int B, const float* const* prm, const float* const* fc,
                                 const float* const* att, float* comb, float* h_out, float* c_out, float* reason_pred,
                                 void* ws, size_t ws_bytes, int train, uint64_t seed, const int32_t* const* att_len, void* st) {
    if (!fc) return RFN_ERR_ARG;
    RfnSeed sd;
    RFN_TRY(path_seed(d, seed, &sd));
    return prefix_fwd_impl(d, B, prm, fc, nullptr, nullptr, att, comb, h_out, c_out, reason_pred, ws, ws_bytes, train,
                           sd, att_len, st);
}
extern "C" int rfn_prefix_fwd(const rfn_dims* d, int B, const float* const* prm, const float* const* fc,
                              const float* const* att, float* comb, float* h_out, float* c_out, float* reason_pred,
                              void* ws, size_t ws_bytes, int train, uint64_t seed, void* st) {
    return rfn_prefix_fwd_ex(d, B, prm, fc, att, comb, h_out, c_out, reason_pred, ws, ws_bytes, train, seed, nullptr, st);
}
// get_thought_vectors with a caller-provided state_list (inference only: no backward through the given state)
extern "C" int rfn_prefix_fwd_from_state_ex(const rfn_dims* d, int B, const float* const* prm, const float* const* init_h,
                                            const float* const* init_c, const float* const* att, float* comb,
                                            float* h_out, float* c_out, float* reason_pred, void* ws, size_t ws_bytes,
                                            const int32_t* const* att_len, void* st) {
    if (!init_h || !init_c) return RFN_ERR_ARG;
    return prefix_fwd_impl(d, B, prm, nullptr, init_h, init_c, att, comb, h_out, c_out, reason_pred, ws, ws_bytes, 0,
                           RfnSeed{}, att_len, st);
}
extern "C" int rfn_prefix_fwd_from_state(const rfn_dims* d, int B, const float* const* prm, const float* const* init_h,
                                         const float* const* init_c, const float* const* att, float* comb,
                                         float* h_out, float* c_out, float* reason_pred, void* ws, size_t ws_bytes,
                                         void* st) {
    return rfn_prefix_fwd_from_state_ex(d, B, prm, init_h, init_c, att, comb, h_out, c_out, reason_pred, ws, ws_bytes, nullptr, st);
}

extern "C" int rfn_prefix_bwd_ex(const rfn_dims* d, int B, const float* const* prm, const float* const* fc,
                                 const float* const* att, const float* d_comb, const float* d_h, const float* d_c,
                                 const float* d_reason, float* const* grd, void* ws, size_t ws_bytes, uint64_t seed_arg,
                                 int defer_wgrad, const int32_t* const* att_len, void* st) {
    RFN_TRY(check_dims(d));
    RfnSeed seed;
    RFN_TRY(path_seed(d, seed_arg, &seed));
    if (B < 1) return RFN_ERR_SHAPE;
    if (!prm || !fc || !att || !grd || !ws) return RFN_ERR_ARG;
    RFN_TRY(check_att_len(d, B, att_len));
    const PrefixLayout Lo = prefix_layout(d, B, 1);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    Prefix c(d, B, prm, att, ws, Lo, seed, st);
    c.grd = grd;
    c.att_len = att_len;
    RFN_TRY(phase_gemm(d, c.W, Lo.gws, Lo.tk, true, st, &c.gx));
    if (c.T1 > 64 || c.T2 > 64) return RFN_ERR_SHAPE;
    RFN_TRY(c.s2_head_bwd(d_comb, d_reason));
    RFN_TRY(c.s2_bwd_sweep(d_h, d_c));
    RFN_TRY(c.s2_wgrad());
    RFN_TRY(c.mean_and_s1_heads_bwd(d_reason));
    const bool small = c.s1_small_steps();
    for (int t = c.T1 - 1; t >= 0; --t) RFN_TRY(c.s1_bwd_step(t, small));
    RFN_TRY(c.s1_bwd_tail(fc));
    // weight gradients of stage I (per encoder; see rfn_prefix_bwd_wgrad) unless the caller defers them
    if (!defer_wgrad)   // the short part-A products of every encoder first, then the long att_2_att_h products back to back
        for (int part = 1; part <= 2; ++part)
            for (int i = 0; i < c.M; ++i) RFN_TRY(rfn_prefix_bwd_wgrad(d, B, att, grd, ws, ws_bytes, i, part, st));
    return RFN_OK;
}
extern "C" int rfn_prefix_bwd(const rfn_dims* d, int B, const float* const* prm, const float* const* fc,
                              const float* const* att, const float* d_comb, const float* d_h, const float* d_c,
                              const float* d_reason, float* const* grd, void* ws, size_t ws_bytes, uint64_t seed_arg,
                              int defer_wgrad, void* st) {
    return rfn_prefix_bwd_ex(d, B, prm, fc, att, d_comb, d_h, d_c, d_reason, grd, ws, ws_bytes, seed_arg, defer_wgrad, nullptr, st);
}

// Stage-I weight gradients of ONE encoder, grouped over the T1 steps (bias gradients ride along):
// H2h, z2h, h_2_att_h and the dominant d att_2_att_h.weight[t,i] = dP1_i[:, t]^T . att_i (K = B*L_i).
// Reads only the workspace rfn_prefix_bwd left behind, so a data-parallel host can all-reduce encoder i's
// gradient bucket while encoder i+1's GEMMs run.
extern "C" int rfn_prefix_bwd_wgrad(const rfn_dims* d, int B, const float* const* att, float* const* grd, void* ws,
                                    size_t ws_bytes, int enc, int parts, void* st) {
    RFN_TRY(check_dims(d));
    if (B < 1 || enc < 0 || enc >= d->M || (parts & ~3) || !parts) return RFN_ERR_SHAPE;
    if (!att || !grd || !ws) return RFN_ERR_ARG;
    const PrefixLayout Lo = prefix_layout(d, B, 1);
    if (ws_bytes < Lo.total * sizeof(float)) return RFN_ERR_WORKSPACE;
    const PIdx P(d);
    const int M = d->M, R = d->R, A = d->A, T1 = d->T1, i = enc;
    if (T1 > 64) return RFN_ERR_SHAPE;
    const long MR = (long)M * R, BMR = (long)B * MR, BA = (long)B * A;
    float* W = (float*)ws;
    GemmCtx gx;
    RFN_TRY(phase_gemm(d, W, Lo.gws, Lo.tk, false, st, &gx));   // the tickets are zero: rfn_prefix_bwd left them so
    const float* Hs = W + Lo.Hs;
    rfn_gemm_problem pr[64];
    const long Li = d->L[i], Di = d->D[i];
    // att_2_att_h.bias and h_2_att_h.bias enter the same pre-activation (AttentionModelCore.py:36-38), so their
    // gradients are the same vector: the column-sum launch of part A writes it to both; the long att_2_att_h GEMM
    // carries no bias-gradient rider.
    auto part_b = [&]() -> int {   // the dominant att_2_att_h gradient (small bucket, long GEMM)
        if (x3_takes(d, B, i)) {
            // bf16-plane GEMM: dW[t] = dP1[t]^T . att.  Both operands are reduction-index-major in memory ((b,l) rows), so
            // they are kept that way as k-slow plane images and rfn_x3_gemm_ks transposes while reading LDS: no
            // transposing pass.  dP1's image was written by the attention backward itself when B >= 96 (fused kernel);
            // for small batches it is split from the f32 slabs here.
            const int BL = (int)(B * Li), TA = T1 * A;
            char* ksX = (char*)(W + Lo.x3);
            float* part = (float*)(ksX + rfn_x3_image_bytes((int)Di, BL));
            char* ksP = (char*)(W + Lo.x3p[i]);
            const int sk = rfn_x3_splitk_for(TA, (int)Di, BL);
            const float* srcs[64];
            float* outs[64];
            srcs[0] = att[i];
            RFN_TRY(rfn_x3_split_ks(srcs, 1, Di, BL, (int)Di, ksX, st));
            for (int t = 0; t < T1; ++t) {
                srcs[t] = W + Lo.P1[i] + (long)t * BL * A;
                outs[t] = grd[P.s1(t, i, 0)];
            }
            if (!x3_dp_emitted(d, B, i)) {
                RFN_TRY(rfn_x3_split_ks(srcs, T1, A, BL, A, ksP, st));
            } else if (BL % 32) {   // the attention kernels wrote the B*L real rows; the GEMM also reads the pad rows
                const long row_bytes = 3L * x3_row_pad(TA) * 2;
                if (hipMemsetAsync(ksP + BL * row_bytes, 0, (size_t)((BL + 31) / 32 * 32 - BL) * row_bytes, (hipStream_t)st) !=
                    hipSuccess)
                    return RFN_ERR_LAUNCH;
            }
            RFN_TRY(probe_mark(d, 2 * M + 2 * i, st));
            RFN_TRY(rfn_x3_gemm_ks(TA, (int)Di, BL, ksP, ksX, A, (int)Di, outs, nullptr, Di, 0, sk, part, st));
            return probe_mark(d, 2 * M + 2 * i + 1, st);
        }
        for (int t = 0; t < T1; ++t)
            pr[t] = prob_dw(grd[P.s1(t, i, 0)], Di, nullptr, W + Lo.P1[i] + (long)t * B * Li * A, A, att[i], Di,
                            (int)(B * Li));
        RFN_TRY(probe_mark(d, 2 * M + 2 * i, st));
        RFN_TRY(gemm_groups_split_cols(A, (int)Di, T1, pr, 0, gx));
        return probe_mark(d, 2 * M + 2 * i + 1, st);
    };
    if ((parts & 2) && !(parts & 1)) return part_b();
    // part A: H2h, z2h, h_2_att_h (large bucket, short GEMMs: K = B rows per step).  Their bias gradients are column
    // sums of tensors that are tiny next to the weight gradients (dgates: T1*B*4R floats per encoder), so they come from
    // one grouped column-sum launch each instead of riding on the GEMMs -- which keeps the two big products
    // (2 x T1 x 4R x {M*R, D}) on the LDS-DMA kernel.  H2h.bias and z2h.bias enter the same pre-activation and share
    // one gradient, like h_2_att_h.bias and att_2_att_h.bias.
    float* outs[64];
    const float* g1i = W + Lo.g1 + (long)i * B * 4 * R;           // (t, i) slab = g1i + t * M*B*4R
    float* outs2[64];
    for (int t = 0; t < T1; ++t) {
        outs[t] = grd[P.s1(t, i, 7)];
        outs2[t] = grd[P.s1(t, i, 9)];     // z2h.bias = H2h.bias gradient
    }
    RFN_TRY(rfn_colsum_grouped2_f32(g1i, (long)M * B * 4 * R, 4 * R, B, 4 * R, outs, outs2, T1, st));
    for (int t = 0; t < T1; ++t) {
        outs[t] = grd[P.s1(t, i, 3)];
        outs2[t] = grd[P.s1(t, i, 1)];     // att_2_att_h.bias = h_2_att_h.bias gradient
    }
    RFN_TRY(rfn_colsum_grouped2_f32(W + Lo.dhp1 + (long)i * BA, (long)M * BA, A, B, A, outs, outs2, T1, st));
    for (int t = 0; t < T1; ++t)
        pr[t] = prob_dw(grd[P.s1(t, i, 6)], MR, nullptr, g1i + (long)t * M * B * 4 * R, 4 * R, Hs + t * BMR, MR, B);
    RFN_TRY(gemm_groups(4 * R, (int)MR, T1, pr, 0, gx));
    for (int t = 0; t < T1; ++t)
        pr[t] = prob_dw(grd[P.s1(t, i, 8)], Di, nullptr, g1i + (long)t * M * B * 4 * R, 4 * R,
                        W + Lo.z1[i] + (long)t * B * Di, Di, B);
    RFN_TRY(gemm_groups_split_cols(4 * R, (int)Di, T1, pr, 0, gx));
    for (int t = 0; t < T1; ++t)
        pr[t] = prob_dw(grd[P.s1(t, i, 2)], R, nullptr, W + Lo.dhp1 + ((long)t * M + i) * BA, A, Hs + t * BMR + i * R, MR, B);
    RFN_TRY(gemm_groups(A, R, T1, pr, 0, gx));
    if (parts & 2) RFN_TRY(part_b());
    return RFN_OK;
}

// Gradients of the inputs (rfn.h): reads what rfn_prefix_bwd left in a workspace laid out with RFN_PATH_OPT_INPUT_GRADS.
extern "C" int rfn_prefix_bwd_inputs(const rfn_dims* d, int B, const float* const* prm, float* const* d_fc, float* const* d_att,
                                     void* ws, size_t ws_bytes, const int32_t* const* att_len, void* st) {
    RFN_TRY(check_dims(d));
    if (B < 1) return RFN_ERR_SHAPE;
    if (!prm || !ws) return RFN_ERR_ARG;
    if (!(d->path_flags & RFN_PATH_OPT_INPUT_GRADS)) return RFN_ERR_UNSUPPORTED;   // one d z buffer, overwritten by every step
    const int M = d->M, R = d->R, A = d->A, T1 = d->T1;
    for (int i = 0; i < M; ++i)   // dP1 exists as bf16 planes only (rfn_attn_bwd_grouped_ks): product (A) has no operand
        if (d_att && d_att[i] && x3_dp_emitted(d, B, i)) return RFN_ERR_UNSUPPORTED;
    const PrefixLayout Lo = prefix_layout(d, B, 1);
    if (ws_bytes < Lo.total * sizeof(float))
        return ws_bytes >= prefix_layout(d, B, 0).total * sizeof(float) ? RFN_ERR_UNSUPPORTED : RFN_ERR_WORKSPACE;
    const PIdx P(d);
    const long MR = (long)M * R;
    float* W = (float*)ws;
    GemmCtx gx;
    RFN_TRY(phase_gemm(d, W, Lo.gws, Lo.tk, false, st, &gx));   // the tickets are zero: rfn_prefix_bwd left them so
    // (C) dHs[0] holds d h0 + d c0 (s1_bwd_tail)
    for (int i = 0; d_fc && i < M; ++i)
        if (d_fc[i])
            RFN_TRY(gemm1(B, d->F[i], seg_dx(W + Lo.dHs + (long)i * R, MR, prm[P.fc_w(i)], d->F[i], R), d_fc[i], d->F[i], 0, gx));
    rfn_gemm_seg segs[64];
    for (int i = 0; d_att && i < M; ++i) {
        if (!d_att[i]) continue;
        const int Li = d->L[i], Di = d->D[i];
        const long BL = (long)B * Li;
        // The streaming kernel OVERWRITES and the GEMM accumulates: the map is then written once by (B) and read once and
        // written once by the GEMM epilogue.  The other order costs the same bytes only on full maps; this one also gives the
        // padded rows of a ragged map their exact zeros for free (the kernel writes them, the GEMM adds dP1's zero rows), and
        // the kernel never has to read a map whose every byte it replaces.
        // (B): T1 is cut so that a call's dz rows fit the kernel's LDS tile; later calls continue the same fmaf chain.
        const int tmax = rfn_attn_dseq_steps_max_t(Di);
        for (int t0 = 0; t0 < T1; t0 += tmax)
            RFN_TRY(rfn_attn_context_bwd_dseq_steps(T1 - t0 < tmax ? T1 - t0 : tmax, W + Lo.al1[i] + t0 * BL, BL,
                                                    W + Lo.dz1[i] + t0 * Lo.dz1_st[i], (long)Lo.dz1_st[i], Di, B, Li, Di, d_att[i],
                                                    (long)Li * Di, Di, t0 > 0, att_len ? att_len[i] : nullptr, st));
        // (A): T1 K-segments dP1_i[t] (B * L_i, A) . W_att2att[t, i] (A, D_i)
        for (int t = 0; t < T1; ++t) segs[t] = seg_dx(W + Lo.P1[i] + t * BL * A, A, prm[P.s1(t, i, 0)], Di, A);
        RFN_TRY(gemm_segs((int)BL, Di, T1, segs, d_att[i], Di, 1, gx));
    }
    return RFN_OK;
}
