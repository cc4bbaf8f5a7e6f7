// Definitions behind rfn_path.h (helpers shared by the phases) and the parameter table of the C ABI.
#include "rfn_path.h"

// outside rfn_path, in the file's own anonymous namespace: the kernel keeps the name it has always had in traces
namespace {
struct MemOps { MemOp op[MEM_BATCH]; };
__global__ __launch_bounds__(256) void mem_batch_k(const MemOps o) {
    const MemOp m = o.op[blockIdx.y];
    const long stride = (long)gridDim.x * 256, i0 = (long)blockIdx.x * 256 + threadIdx.x;
    const bool v4 = (((uintptr_t)m.dst | (uintptr_t)m.src) & 15) == 0;
    const long n4 = v4 ? m.n >> 2 : 0;
    typedef float f4 __attribute__((ext_vector_type(4)));
    if (m.src) {
        for (long i = i0; i < n4; i += stride) reinterpret_cast<f4*>(m.dst)[i] = reinterpret_cast<const f4*>(m.src)[i];
        for (long i = 4 * n4 + i0; i < m.n; i += stride) m.dst[i] = m.src[i];
    } else {
        for (long i = i0; i < n4; i += stride) reinterpret_cast<f4*>(m.dst)[i] = f4{0.f, 0.f, 0.f, 0.f};
        for (long i = 4 * n4 + i0; i < m.n; i += stride) m.dst[i] = 0.f;
    }
}
}  // namespace

namespace rfn_path __attribute__((visibility("hidden"))) {

int path_seed(const rfn_dims* d, uint64_t seed_arg, RfnSeed* out) {
    if (!d) return RFN_ERR_ARG;
    *out = RfnSeed{nullptr, seed_arg};
    if (d->path_flags & RFN_PATH_OPT_SEED_DEV) {
        if (!seed_arg || (seed_arg & 7u)) return RFN_ERR_ARG;
        *out = RfnSeed{reinterpret_cast<const uint64_t*>((uintptr_t)seed_arg), 0};
    }
    return RFN_OK;
}

int check_dims(const rfn_dims* d) {
    if (!d) return RFN_ERR_ARG;
    if (d->M < 1 || d->M > RFN_MAX_ENC || d->R < 1 || d->A < 1 || d->E < 1 || d->T1 < 1 || d->T2 < 1 || d->K < 1 ||
        d->V1 < 2)
        return RFN_ERR_SHAPE;
    for (int i = 0; i < d->M; ++i)
        if (d->L[i] < 1 || d->D[i] < 1 || d->F[i] < 1) return RFN_ERR_SHAPE;
    // the per-phase grouped launches carry at most 64 (step, encoder) pointer slots (rfn.h, rfn_dims)
    if (d->T1 * d->M > 64 || d->T2 * d->M > 64) return RFN_ERR_SHAPE;
    if (d->drop_fusion < 0 || d->drop_fusion >= 1 || d->drop_reason < 0 || d->drop_reason >= 1 || d->drop_lm < 0 ||
        d->drop_lm >= 1)
        return RFN_ERR_SHAPE;
    return RFN_OK;
}

int gemm_logits(int rows, int V1, const float* h, int R, const float* Wl, const float* bl, float* C, const GemmCtx& gx) {
    // both operands are [row][k]: the LDS-DMA kernel takes the ragged vocabulary in one launch (edge tiles clamp their
    // source rows); only a hidden size that is not a whole K step keeps the main + remainder split
    const int Va = aligned_part(V1);
    if (Va == V1 || Va == 0 || R % 32 == 0) return gemm1(rows, V1, seg_lin(h, R, Wl, R, R, bl), C, V1, 0, gx);
    RFN_TRY(gemm1(rows, Va, seg_lin(h, R, Wl, R, R, bl), C, V1, 0, gx));
    return gemm1(rows, V1 - Va, seg_lin(h, R, Wl + (long)Va * R, R, R, bl + Va), C + Va, V1, 0, gx);
}
int gemm_logits_dw(int V1, int R, float* dW, float* db, const float* dlg, const float* h, int rows, const GemmCtx& gx) {
    // The bias gradient (column sums of the 165 MB dlogits) comes from its own streaming pass (~35 us) instead of riding
    // on the GEMM: without the rider the 42-GFLOP weight gradient takes the LDS-DMA kernel (0.55 -> 0.33 ms at C3).
    const bool big = (double)rows * V1 * R >= 2e9 && db;
    if (big) {
        RFN_TRY(rfn_colsum_f32(dlg, V1, rows, V1, db, 0, gx.st));
        db = nullptr;
    }
    const int Va = aligned_part(V1);
    if (Va == V1 || Va == 0) return gemm_dw(V1, R, dW, R, db, dlg, V1, h, R, rows, gx);
    RFN_TRY(gemm_dw(Va, R, dW, R, db, dlg, V1, h, R, rows, gx));
    return gemm_dw(V1 - Va, R, dW + (long)Va * R, R, db ? db + Va : nullptr, dlg + Va, V1, h, R, rows, gx);
}
int gemm_logits_dx(int rows, int R, int V1, const float* dlg, const float* Wl, float* dh, const GemmCtx& gx) {
    const int Va = aligned_part(V1);
    if (Va == V1 || Va == 0) return gemm1(rows, R, seg_dx(dlg, V1, Wl, R, V1), dh, R, 0, gx);
    RFN_TRY(gemm1(rows, R, seg_dx(dlg, V1, Wl, R, Va), dh, R, 0, gx));
    return gemm1(rows, R, seg_dx(dlg + Va, V1, Wl + (long)Va * R, R, V1 - Va), dh, R, 1, gx);
}
// any number of K segments into one C (chunks of RFN_GEMM_MAXSEG, later chunks accumulate)
int gemm_segs(int M, int N, int nseg, const rfn_gemm_seg* segs, float* C, long ldc, int acc, const GemmCtx& gx) {
    for (int s0 = 0; s0 < nseg; s0 += RFN_GEMM_MAXSEG) {
        rfn_gemm_problem p;
        memset(&p, 0, sizeof(p));
        p.C = C; p.ldc = ldc;
        p.nseg = (nseg - s0 < RFN_GEMM_MAXSEG) ? nseg - s0 : RFN_GEMM_MAXSEG;
        for (int s = 0; s < p.nseg; ++s) p.seg[s] = segs[s0 + s];
        RFN_TRY(rfn_gemm_f32_tk(M, N, 1, &p, (s0 > 0) ? 1 : acc, gx.ws, gx.ws_bytes, gx.flags, gx.tickets, gx.n_tickets, gx.st));
    }
    return RFN_OK;
}
// any number of same-shape problems (chunks of RFN_GEMM_MAXGROUP)
int gemm_groups(int M, int N, int n, const rfn_gemm_problem* p, int acc, const GemmCtx& gx) {
    for (int g0 = 0; g0 < n; g0 += RFN_GEMM_MAXGROUP) {
        const int ng = (n - g0 < RFN_GEMM_MAXGROUP) ? n - g0 : RFN_GEMM_MAXGROUP;
        RFN_TRY(rfn_gemm_f32_tk(M, N, ng, p + g0, acc, gx.ws, gx.ws_bytes, gx.flags, gx.tickets, gx.n_tickets, gx.st));
    }
    return RFN_OK;
}
// The same for big problems whose column count is not a multiple of the 128-wide tile (a 2208-wide DenseNet feature
// map, feat_array.py:147-150): the aligned main part takes the interior fast path (LDS-DMA kernel), a thin remainder
// (< 128 columns) the bounds-checked one -- as the logit layer does for the vocabulary.  Same sums, same k order per
// output element.  A bias-gradient rider (row sums of the A operand) rides on the main part only.
int gemm_groups_split_cols(int M, int N, int n, const rfn_gemm_problem* p, int acc, const GemmCtx& gx) {
    const int Na = aligned_part(N);
    if (Na == N || Na == 0 || M % 128 != 0) return gemm_groups(M, N, n, p, acc, gx);
    RFN_TRY(gemm_groups(M, Na, n, p, acc, gx));
    rfn_gemm_problem rest[64];
    if (n > 64) return RFN_ERR_SHAPE;
    for (int g = 0; g < n; ++g) {
        rest[g] = p[g];
        rest[g].C = p[g].C + Na;
        rest[g].a_colsum = nullptr;
        for (int s = 0; s < p[g].nseg; ++s) {
            rfn_gemm_seg& sg = rest[g].seg[s];
            sg.B = sg.b_kfast ? sg.B + (long)Na * sg.ldb : sg.B + Na;
            if (sg.bias) sg.bias += Na;
        }
    }
    return gemm_groups(M, N - Na, n, rest, acc, gx);
}

int phase_gemm(const rfn_dims* d, float* W, size_t gws, size_t tk, bool zero_tickets, void* st, GemmCtx* gx) {
    const bool tk_on = (d->gemm_flags & RFN_GEMM_OPT_SPLITK_IN_KERNEL) != 0;
    *gx = GemmCtx{st, W + gws, GEMM_WS_FLOATS * sizeof(float), d->gemm_flags, tk_on ? (int32_t*)(W + tk) : nullptr,
                  tk_on ? GEMM_TICKETS : 0};
    return tk_on && zero_tickets ? zero_f32(W + tk, GEMM_TICKETS, st) : RFN_OK;
}

int mem_batch(std::initializer_list<MemOp> ops, void* st) {
    MemOps o;
    int n = 0;
    long big = 0;
    for (const MemOp& m : ops) {
        if (!m.dst || m.n <= 0) continue;
        if (n == MEM_BATCH) return RFN_ERR_SHAPE;
        o.op[n++] = m;
        big = m.n > big ? m.n : big;
    }
    if (!n) return RFN_OK;
    for (int i = n; i < MEM_BATCH; ++i) o.op[i] = MemOp{nullptr, nullptr, 0};
    long blocks = (big / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(mem_batch_k, dim3((unsigned)blocks, n), dim3(256), 0, (hipStream_t)st, o);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

bool x3_takes(const rfn_dims* d, int B, int i) {
    if (!(d->gemm_flags & RFN_GEMM_OPT_BF16X3)) return false;
    if (d->A % 256 || d->D[i] % 4 || d->T1 > 64) return false;
    if (d->gemm_flags & RFN_GEMM_OPT_BF16X3_ANY_SIZE) return true;
    return 2.0 * B * d->L[i] * d->D[i] * d->A * d->T1 >= 2e10;
}
static bool attn_bwd_small_map(const rfn_dims* d, int B, int i) {
    return !x3_takes(d, B, i) && (long)d->L[i] * d->D[i] <= FUSED_ATTN_BWD_SMALL_MAP;
}
AttnBwdForm attn_bwd_form(const rfn_dims* d, int B, int i, bool dz_in_one_launch) {
    const int M = d->M;
    bool same_ld = M > 1;
    for (int j = 1; j < M; ++j) same_ld = same_ld && d->D[j] == d->D[0] && d->L[j] == d->L[0];
    if (same_ld && ((long)B * M >= FUSED_ATTN_BWD_MIN_B || attn_bwd_small_map(d, B, 0)))
        return x3_takes(d, B, 0) ? AB_GROUPED_KS : AB_GROUPED;
    if (!same_ld && M > 1 && dz_in_one_launch) {   // every encoder must qualify for the exact-f32 fused form in the shared launch
        bool het = true;
        for (int j = 0; j < M && het; ++j)
            het = !x3_takes(d, B, j) && ((long)B * M >= FUSED_ATTN_BWD_MIN_B || attn_bwd_small_map(d, B, j));
        if (het) return AB_HET;
    }
    if (B >= FUSED_ATTN_BWD_MIN_B && x3_takes(d, B, i)) return AB_FUSED_KS;
    if (B >= FUSED_ATTN_BWD_MIN_B || attn_bwd_small_map(d, B, i)) return AB_FUSED;
    return AB_SPLIT;
}
bool x3_dp_emitted(const rfn_dims* d, int B, int i) {   // dP1 of encoder i reaches its k-slow plane image from the attention launches
    const AttnBwdForm f = attn_bwd_form(d, B, i, false);       // (the HET form never takes plane products)
    return f == AB_GROUPED_KS || f == AB_FUSED_KS;
}
static size_t x3_scratch_floats(const rfn_dims* d, int B, int train) {
    size_t most = 0;
    for (int i = 0; i < d->M; ++i) {
        if (!x3_takes(d, B, i)) continue;
        const int BL = B * d->L[i], TA = d->T1 * d->A, Di = d->D[i];
        size_t fwd = rfn_x3_image_bytes(BL, Di) + rfn_x3_image_bytes(TA, Di);
        size_t bwd = 0;
        if (train) bwd = rfn_x3_image_bytes(Di, BL) + 4 * rfn_x3_part_floats(TA, Di, rfn_x3_splitk_for(TA, Di, BL));
        const size_t need = (fwd > bwd ? fwd : bwd) / 4 + 256;
        if (need > most) most = need;
    }
    return most;
}
PrefixLayout prefix_layout(const rfn_dims* d, int B, int train) {
    const size_t G2 = (size_t)gate_width(d->review_maxout, d->R);
    PrefixLayout L;
    memset(&L, 0, sizeof(L));
    Bump b;
    const size_t M = d->M, R = d->R, A = d->A, T1 = d->T1, T2 = d->T2, K = d->K, Bz = B;
    size_t maxL = T1;
    for (int i = 0; i < d->M; ++i) {
        L.P1[i] = b.take(Bz * d->L[i] * T1 * A);
        L.al1[i] = b.take(T1 * Bz * d->L[i]);
        L.z1[i] = b.take(T1 * Bz * d->D[i]);
        L.P2[i] = b.take(T1 * Bz * T2 * A);
        if ((size_t)d->L[i] > maxL) maxL = d->L[i];
    }
    L.Hs = b.take((T1 + 1) * Bz * M * R);
    L.Cs = b.take((T1 + 1) * Bz * M * R);
    L.hp1 = b.take(T1 * M * Bz * A);
    L.g1 = b.take(T1 * M * Bz * 4 * R);
    L.rmat = b.take((T1 * M > T2 ? T1 * M : T2) * Bz * K);   // M slabs (T1,B,K) of the stage-I heads / one (T2,B,K)
    L.rarg = b.take((M + 1) * Bz * K);  // int32, same width
    L.h2 = b.take((T2 + 1) * Bz * R);
    L.c2 = b.take((T2 + 1) * Bz * R);
    L.hp2 = b.take(T2 * M * Bz * A);
    L.al2 = b.take(T2 * M * Bz * T1);
    L.z2 = b.take(T2 * M * Bz * R);
    L.g2 = b.take(T2 * Bz * G2);
    L.gws = b.take(GEMM_WS_FLOATS);
    L.tk = b.take(GEMM_TICKETS);
    L.bar = b.take(RFN_CHAIN_BAR_WORDS);
    L.x3 = b.take(x3_scratch_floats(d, B, train));
    if (train)
        for (int i = 0; i < d->M; ++i)
            if (x3_takes(d, B, i)) L.x3p[i] = b.take(rfn_x3_image_bytes(d->T1 * d->A, B * d->L[i]) / 4 + 64);
    if (train) {
        // RFN_PATH_OPT_INPUT_GRADS: every step's d z is kept (slice t at dz1 + t * dz1_st, each 256-B aligned like the single
        // buffer, so that the launches that write and read it decide their alignment cases as without the bit)
        const bool keep_dz = (d->path_flags & RFN_PATH_OPT_INPUT_GRADS) != 0;
        for (int i = 0; i < d->M; ++i) {
            L.dz1_st[i] = keep_dz ? (Bz * d->D[i] + 63) & ~(size_t)63 : 0;
            L.dz1[i] = b.take(keep_dz ? T1 * L.dz1_st[i] : Bz * d->D[i]);
        }
        L.dHs = b.take((T1 + 1) * Bz * M * R);
        L.dHpart = b.take(M * Bz * M * R);       // small batches: the M partial products d gates_j . W_H_j of a stage-I step
        L.dC = b.take(Bz * M * R);
        L.dal = b.take(M * Bz * maxL);
        L.dwp = b.take((T1 > T2 ? T1 : T2) * M * Bz * A);
        L.dhp1 = b.take(T1 * M * Bz * A);
        L.dh2e = b.take(T2 * Bz * R);
        L.dhrec = b.take(Bz * R);
        L.dc2 = b.take(Bz * R);
        L.dz2 = b.take(M * Bz * R);
        L.dhp2 = b.take(T2 * M * Bz * A);
    }
    L.total = b.off;
    return L;
}

DecoderLayout decoder_layout(const rfn_dims* d, int B, int S, int train, int n) {
    const size_t GD = (size_t)gate_width(d->decoder_maxout, d->R);
    DecoderLayout L;
    memset(&L, 0, sizeof(L));
    Bump b;
    const size_t R = d->R, A = d->A, E = d->E, T2 = d->T2, V1 = d->V1, Bz = B, Sz = S;
    const size_t Bi = B / n;          // images: what is computed from the thought vectors alone is kept once per image
    L.Pd = b.take(T2 * Bi * A);
    L.Ud = b.take(T2 * Bi * GD);      // U = thought vectors . W_z^T (z2h hoisted through the attention, rfn_deccell.hip)
    L.xs = b.take(Sz * Bz * E);
    L.gd = b.take(Sz * Bz * GD);
    L.hd = b.take((Sz + 1) * Bz * R);
    L.cd = b.take((Sz + 1) * Bz * R);
    L.hpd = b.take(Sz * Bz * A);
    L.ald = b.take(Sz * Bz * T2);
    L.zd = b.take(Sz * Bz * R);
    L.logits = b.take(Sz * Bz * V1);  // logits in forward, dlogits in backward
    L.gws = b.take(GEMM_WS_FLOATS);
    L.tk = b.take(GEMM_TICKETS);
    L.bar = b.take(RFN_CHAIN_BAR_WORDS);
    if (train) {
        L.dhe = b.take(Sz * Bz * R);
        L.dhrec = b.take(DEC_KSPLIT * Bz * R);   // the recurrent d h; hoisted form: + the K-split partial slabs of d gates . W_hh
        L.dc = b.take(Bz * R);
        L.dz = b.take(Bz * R);
        L.dal = b.take(Bz * T2);
        L.dwp = b.take(Sz * Bz * A);
        L.dhpd = b.take(Sz * Bz * A);
        L.dPd = b.take(T2 * Bz * A);      // per ROW: no two rows of an image accumulate into one address
        if (n > 1) L.dPi = b.take(T2 * Bi * A);   // ... and summed onto the image after the sweep
        L.dUd = b.take(T2 * Bi * GD);
        L.dxs = b.take(Sz * Bz * E);
    }
    L.total = b.off;
    return L;
}

int stage1_cell_cus() {   // CU count of the current device (cached); 256 when it cannot be read
    static int cus[16] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int& c = cus[dev & 15];
    if (c == 0 && hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) c = 256;
    return c > 0 ? c : 256;
}

}  // namespace rfn_path

// =============================================================================================
// parameter table
// =============================================================================================
extern "C" int rfn_abi_version(void) { return RFN_ABI_VERSION; }

extern "C" const char* rfn_error_string(int code) {
    switch (code) {
        case RFN_OK: return "ok";
        case RFN_ERR_SHAPE: return "unsupported or inconsistent dimensions";
        case RFN_ERR_UNSUPPORTED: return "configuration not implemented by the HIP path (maxout)";
        case RFN_ERR_LAUNCH: return "HIP launch / runtime failure";
        case RFN_ERR_WORKSPACE: return "workspace too small";
        case RFN_ERR_ARG: return "null or misaligned pointer";
        default: return "unknown error";
    }
}

extern "C" int rfn_param_count(const rfn_dims* d) {
    const int rc = check_dims(d);
    if (rc != RFN_OK) return rc;
    return PIdx(d).count();
}

static const char* const kAtt[6] = {"att_2_att_h.weight", "att_2_att_h.bias", "h_2_att_h.weight",
                                    "h_2_att_h.bias",     "att_h_2_out.weight", "att_h_2_out.bias"};

extern "C" int rfn_param_name(const rfn_dims* d, int idx, char* buf, size_t n) {
    const int rc = check_dims(d);
    if (rc != RFN_OK) return rc;
    if (!buf || n == 0) return RFN_ERR_ARG;
    const PIdx P(d);
    const int M = d->M;
    if (idx < 0 || idx >= P.count()) return RFN_ERR_SHAPE;
    if (idx < 2 * M) {
        snprintf(buf, n, "fc2h.%d.%s", idx / 2, (idx & 1) ? "bias" : "weight");
    } else if (idx == P.embed()) {
        snprintf(buf, n, "embed.weight");
    } else if (idx == P.logit_w()) {
        snprintf(buf, n, "logit.weight");
    } else if (idx == P.logit_b()) {
        snprintf(buf, n, "logit.bias");
    } else if (idx < P.rind_w(0)) {
        const int r = idx - P.s1(0, 0, 0), cell = r / 10, k = r % 10, t = cell / M, i = cell % M;
        if (k < 6)
            snprintf(buf, n, "review_steps_individual.%d.lstm.%d.att_model.%s", t, i, kAtt[k]);
        else
            snprintf(buf, n, "review_steps_individual.%d.lstm.%d.%s.%s", t, i, (k < 8) ? "H2h" : "z2h",
                     (k & 1) ? "bias" : "weight");
    } else if (idx < P.s2base(0)) {
        const int r = idx - P.rind_w(0);
        snprintf(buf, n, "reason_linear_individual.%d.%s", r / 2, (r & 1) ? "bias" : "weight");
    } else if (idx < P.r_w()) {
        const int per = 2 + 8 * M, r = idx - P.s2base(0), t = r / per, k = r % per;
        if (k < 2) {
            snprintf(buf, n, "review_steps.%d.h2h.%s", t, k ? "bias" : "weight");
        } else {
            const int i = (k - 2) / 8, kk = (k - 2) % 8;
            if (kk < 2)
                snprintf(buf, n, "review_steps.%d.z_2_h.%d.%s", t, i, kk ? "bias" : "weight");
            else
                snprintf(buf, n, "review_steps.%d.att_model.%d.%s", t, i, kAtt[kk - 2]);
        }
    } else if (idx == P.r_w()) {
        snprintf(buf, n, "reason_linear.weight");
    } else if (idx == P.r_b()) {
        snprintf(buf, n, "reason_linear.bias");
    } else {
        const int k = idx - P.dec(0);
        static const char* const names[3] = {"i2h", "h2h", "z2h"};
        if (k < 6)
            snprintf(buf, n, "decoder.%s.%s", names[k / 2], (k & 1) ? "bias" : "weight");
        else
            snprintf(buf, n, "decoder.%s", kAtt[k - 6]);
    }
    return RFN_OK;
}

extern "C" int rfn_param_shape(const rfn_dims* d, int idx, int64_t* rows, int64_t* cols) {
    const int rc = check_dims(d);
    if (rc != RFN_OK) return rc;
    if (!rows || !cols) return RFN_ERR_ARG;
    const PIdx P(d);
    const int M = d->M, R = d->R, A = d->A;
    const int G2 = gate_width(d->review_maxout, R), GD = gate_width(d->decoder_maxout, R);
    if (idx < 0 || idx >= P.count()) return RFN_ERR_SHAPE;
    auto att_shape = [&](int k, int feat, int64_t* r, int64_t* c) {
        const int64_t rr[6] = {A, A, A, A, 1, 1};
        const int64_t cc[6] = {feat, 1, R, 1, A, 1};
        *r = rr[k];
        *c = cc[k];
    };
    if (idx < 2 * M) {
        *rows = R;
        *cols = (idx & 1) ? 1 : d->F[idx / 2];
    } else if (idx == P.embed()) {
        *rows = d->V1; *cols = d->E;
    } else if (idx == P.logit_w()) {
        *rows = d->V1; *cols = R;
    } else if (idx == P.logit_b()) {
        *rows = d->V1; *cols = 1;
    } else if (idx < P.rind_w(0)) {
        const int r = idx - P.s1(0, 0, 0), cell = r / 10, k = r % 10, i = cell % M;
        if (k < 6) att_shape(k, d->D[i], rows, cols);
        else { *rows = 4 * R; *cols = (k & 1) ? 1 : (k < 8 ? M * R : d->D[i]); }
    } else if (idx < P.s2base(0)) {
        *rows = d->K; *cols = ((idx - P.rind_w(0)) & 1) ? 1 : R;
    } else if (idx < P.r_w()) {
        const int per = 2 + 8 * M, k = (idx - P.s2base(0)) % per;
        if (k < 2) { *rows = G2; *cols = k ? 1 : R; }
        else {
            const int kk = (k - 2) % 8;
            if (kk < 2) { *rows = G2; *cols = kk ? 1 : R; }
            else att_shape(kk - 2, R, rows, cols);
        }
    } else if (idx == P.r_w()) {
        *rows = d->K; *cols = R;
    } else if (idx == P.r_b()) {
        *rows = d->K; *cols = 1;
    } else {
        const int k = idx - P.dec(0);
        if (k < 6) { *rows = GD; *cols = (k & 1) ? 1 : (k < 2 ? d->E : R); }
        else att_shape(k - 6, R, rows, cols);
    }
    return RFN_OK;
}
