// Per-row kernels of the free-running decode, everything between a step's log-probs and its token: the blocked tokens of
// every row (n-gram blocking, banned ids, bad endings) and their mask, top-k / top-p truncation, the multinomial pick, and the
// greedy pick / record.  A result is a function of the row and the caller's uniforms alone.
#include "rfn_common.h"

// ---- decoding constraints: the blocked tokens of every row at step t, and their mask (rfn.h) ---------------------------------
// One wave per row.  Lane j holds token j of the row's history (at most 63 tokens: t <= S <= 64); it matches the n-gram that
// starts at j against the history's last n - 1 tokens through LDS, and a ballot packs the blocked continuations behind the
// banned ids.  Ids outside [0, V1) are dropped here, so every consumer may index a row with what it reads.
#define DEC_BLK_WAVES 4
__global__ __launch_bounds__(64 * DEC_BLK_WAVES) void decode_blocklist_k(
    const int64_t* __restrict__ hist, long s_row, long s_tok, const int* __restrict__ order, int rows, int S, int t, int n,
    const int* __restrict__ banned, int n_banned, const int* __restrict__ bad, int n_bad, int V1, int* __restrict__ blk,
    int* __restrict__ blk_n) {
    __shared__ int hs[DEC_BLK_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * DEC_BLK_WAVES + wave;
    const bool live = r < rows;
    const int len = t - 1, width = RFN_DECODE_MAX_IDS + S;
    int tok = -1;
    if (live && lane < len) {
        const long src = order ? order[r] : r;
        tok = (int)hist[src * s_row + lane * s_tok];
    }
    hs[wave][lane] = tok;
    __syncthreads();
    if (!live) return;
    int* out = blk + (long)r * width;
    const int last = len > 0 ? hs[wave][len - 1] : -1;
    int count = 0;
    if (!(len > 0 && last == 0)) {               // a finished row is left alone
        const int b = lane < n_banned ? banned[lane] : -1;
        const bool bok = b > 0 && b < V1;
        unsigned long long m = __ballot(bok);
        if (bok) out[__popcll(m & ((1ull << lane) - 1ull))] = b;
        count = __popcll(m);
        bool hit = false;
        int nxt = 0;
        if (n >= 2 && t >= n && lane + n - 1 < len) {
            hit = true;
            for (int i = 0; i < n - 1; ++i) hit = hit && hs[wave][lane + i] == hs[wave][len - (n - 1) + i];
            nxt = hs[wave][lane + n - 1];
            hit = hit && nxt > 0 && nxt < V1;      // END is never blocked by a repeated n-gram
        }
        m = __ballot(hit);
        if (hit) out[count + __popcll(m & ((1ull << lane) - 1ull))] = nxt;
        count += __popcll(m);
        const bool ends_badly = len > 0 && lane < n_bad && bad[lane] == last;
        if (__ballot(ends_badly)) {
            if (lane == 0) out[count] = 0;
            ++count;
        }
    }
    for (int i = count + lane; i < width; i += 64) out[i] = -1;
    if (lane == 0) blk_n[r] = count;
}
extern "C" int rfn_decode_blocklist(const int64_t* hist, int64_t s_row, int64_t s_tok, const int32_t* order, int rows, int S, int t,
                                    int block_ngram, const int32_t* banned, int n_banned, const int32_t* bad_endings, int n_bad,
                                    int V1, int32_t* blk, int32_t* blk_n, void* stream) {
    if (rows < 1 || S < 1 || S > 64 || t < 1 || t > S || V1 < 1) return RFN_ERR_SHAPE;
    if (block_ngram != 0 && (block_ngram < 2 || block_ngram > 4)) return RFN_ERR_SHAPE;
    if (n_banned < 0 || n_banned > RFN_DECODE_MAX_IDS || n_bad < 0 || n_bad > RFN_DECODE_MAX_IDS) return RFN_ERR_SHAPE;
    if (!hist || !blk || !blk_n || (n_banned && !banned) || (n_bad && !bad_endings)) return RFN_ERR_ARG;
    hipLaunchKernelGGL(decode_blocklist_k, dim3(rfn_cdiv(rows, DEC_BLK_WAVES)), dim3(64 * DEC_BLK_WAVES), 0, (hipStream_t)stream,
                       hist, (long)s_row, (long)s_tok, order, rows, S, t, block_ngram, banned, n_banned, bad_endings, n_bad, V1, blk,
                       blk_n);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
// logp[r, blk[r, i]] = -inf for i < blk_n[r]: one wave per row, plain stores (duplicates store the same value twice)
__global__ __launch_bounds__(64 * DEC_BLK_WAVES) void logp_mask_rows_k(float* __restrict__ logp, long ldl, int rows, int V1,
                                                                       const int* __restrict__ blk, long ld_blk,
                                                                       const int* __restrict__ blk_n) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * DEC_BLK_WAVES + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int nb = blk_n[r];
    for (int i = lane; i < nb && i < ld_blk; i += 64) {
        const int id = blk[r * ld_blk + i];
        if (id >= 0 && id < V1) logp[r * ldl + id] = -INFINITY;
    }
}
extern "C" int rfn_logp_mask_rows(float* logp, int64_t ldl, int rows, int V1, const int32_t* blk, int64_t ld_blk,
                                  const int32_t* blk_n, void* stream) {
    if (rows < 1 || V1 < 1 || ldl < V1 || ld_blk < 1) return RFN_ERR_SHAPE;
    if (!logp || !blk || !blk_n) return RFN_ERR_ARG;
    hipLaunchKernelGGL(logp_mask_rows_k, dim3(rfn_cdiv(rows, DEC_BLK_WAVES)), dim3(64 * DEC_BLK_WAVES), 0, (hipStream_t)stream, logp,
                       (long)ldl, rows, V1, blk, (long)ld_blk, blk_n);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
// ---- multinomial pick of sample() / scheduled sampling (misc/RecurrentFusionModel.py:623-631, 260-270) --------
// One block per row: inverse-CDF draw from p[v] ~ exp(logp[v] * inv_temperature) with the caller's uniform u[b].
// Thread t owns the contiguous index range [t*C, (t+1)*C); the 256 range sums are scanned in LDS in index order, the
// thread whose range contains u * total walks it.  The reference draws on the host with torch.multinomial; RNG streams
// are not portable anyway, the DISTRIBUTION is the same and the draw is a deterministic function of (logp, u).
__global__ __launch_bounds__(256) void multinomial_pick_k(const float* __restrict__ logp, long ldl, int V1,
                                                          float inv_temp, const float* __restrict__ u,
                                                          const float* __restrict__ coin, float keep_prob,
                                                          int64_t* __restrict__ ids, long ld_ids) {
    __shared__ float part[256];
    __shared__ int pick;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (coin && !(coin[b] < keep_prob)) return;   // block-uniform: this row keeps the token it already has
    const float* x = logp + b * ldl;
    const int C = (V1 + 255) / 256, v0 = tid * C, v1 = min(V1, v0 + C);
    float sum = 0.f;
    for (int v = v0; v < v1; ++v) sum += __expf(x[v] * inv_temp);
    part[tid] = sum;
    if (tid == 0) pick = -1;
    __syncthreads();
    float before = 0.f, total = 0.f;
    for (int k = 0; k < 256; ++k) {   // 256 LDS broadcasts per thread: same order for everyone
        const float pk = part[k];
        if (k < tid) before += pk;
        total += pk;
    }
    const float target = u[b] * total;
    // the owner is the first range with before <= target < before + sum; target == total (u -> 1) goes to the last
    // non-empty range
    const bool owner = sum > 0.f && target >= before && (target < before + sum);
    if (owner) atomicMax(&pick, tid);
    __syncthreads();
    if (pick < 0) {   // rounding put target at / past the total: last range with mass
        if (sum > 0.f) atomicMax(&pick, tid);
        __syncthreads();
    }
    if (tid == pick) {
        float acc = before;
        int chosen = v0;   // rounding corner (target at / past the range's end): the last index WITH mass
        for (int v = v0; v < v1; ++v) {
            const float e = __expf(x[v] * inv_temp);
            acc += e;
            if (e > 0.f) chosen = v;
            if (target < acc) break;
        }
        ids[b * ld_ids] = chosen;
    }
}
extern "C" int rfn_multinomial_pick(const float* logp, int64_t ldl, int B, int V1, float inv_temperature, const float* u,
                                    const float* coin, float keep_prob, int64_t* ids, int64_t ld_ids, void* stream) {
    if (B <= 0 || V1 <= 0 || ldl < V1 || !(inv_temperature > 0.f)) return RFN_ERR_SHAPE;
    if (!logp || !u || !ids) return RFN_ERR_ARG;
    hipLaunchKernelGGL(multinomial_pick_k, dim3(B), dim3(256), 0, (hipStream_t)stream, logp, (long)ldl, V1,
                       inv_temperature, u, coin, keep_prob, ids, (long)ld_ids);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- truncated sampling: top-k, then nucleus (top-p), of every row, in place (rfn.h "truncated sampling") -----------------
// One block per row, no sort: the kept set is {key > K} plus the m lowest ids with key == K, where key is the order-preserving
// integer image of the float (-0 counted as +0, so the order is rfn_rows.h's row_before).  (K, m) come from a radix select by
// 8-bit digits, top digit first, one histogram bin per thread:
//   top-k   bins count entries; target = k;
//   top-p   bins hold MASS over the survivors of top-k; target = ceil(p * total).
// Mass is exact integer arithmetic: w = exp((x - max) * inv_temp) in fp64 (the common factor exp(max * inv_temp) cancels in
// c_j >= p * c_n) is rounded DOWN to a multiple of 2^-47, and every sum is a 64-bit integer sum (V1 <= 65536 keeps the total
// at or below 2^63).  Integer adds commute, so LDS atomics and any thread count give the same bins: the result is a function of
// the row alone.  The tie group at K is cut by the same integers: m = ceil((target - mass above K) / w(K)).
// Against exact arithmetic a mass is off by less than V1 * 2^-47 of the total from the rounding down (a weight below 2^-47 of
// the largest counts as 0) plus fp64 rounding: below 5e-10 of the total.  fp32 weights would be off by about 1e-5 of it, which
// is the mass of ONE entry near a top_p = 0.9 cut of a 10k-word row: fp64 is what makes the cut the definition's, and at 37
// entries per thread its cost is small.
// Rows of up to TRUNC_STAGE_MAX entries keep their keys in LDS between the passes (9488 entries: 38 KB, four blocks per CU);
// longer rows re-read the log-probs, which the log-softmax before them left in L2.
#define TRUNC_STAGE_MAX 15360     /* 60 KB of keys + the static arrays below stay inside the 64 KB a block gets by default */
#define TRUNC_V1_MAX 65536
#define TRUNC_KEY_NINF 0x007fffffu
typedef unsigned long long trunc_u64;
__device__ __forceinline__ unsigned trunc_key(float x) {
    if (x == 0.f) x = 0.f;   // -0 and +0 are one value in the order
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float trunc_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
__device__ __forceinline__ trunc_u64 trunc_weight(unsigned key, float mx, float inv_temp) {
    const double e = exp(((double)trunc_unkey(key) - (double)mx) * (double)inv_temp) * 140737488355328.0;   // * 2^47: exact
    return e >= 1.0 ? (trunc_u64)e : 0ull;                                            // NaN (a row holding +inf) -> 0
}
// exclusive prefix sum over the 256 threads in thread order, and the total; scr: 4 words of LDS
__device__ __forceinline__ trunc_u64 trunc_scan(trunc_u64 v, trunc_u64* scr, trunc_u64* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    trunc_u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const trunc_u64 y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    __syncthreads();   // scr may still be read from the call before
    if (lane == 63) scr[wave] = inc;
    __syncthreads();
    trunc_u64 before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const trunc_u64 s = scr[w];
        if (w < wave) before += s;
        tot += s;
    }
    *total = tot;
    return before + inc - v;
}
struct TruncSel {
    unsigned key;        // K
    trunc_u64 above;     // count / mass of the participants with key > K
    trunc_u64 target;
};
template <bool STAGE>
__device__ __forceinline__ unsigned trunc_load(const unsigned* keys, const float* x, int v) {
    if constexpr (STAGE) return keys[v];
    else return trunc_key(x[v]);
}
// Participants: entries with key > lo, each worth 1 (MASS = false) or its weight, plus `tie_val` more at key == lo (top-k's
// admitted part of its tie group; 0: none).  target: k, or top_p (then ceil(top_p * total) is taken).  A total of 0 returns
// target 0: nothing to select.
template <bool STAGE, bool MASS>
__device__ TruncSel trunc_select(const unsigned* keys, const float* x, int V1, unsigned lo, trunc_u64 tie_val, float mx,
                                 float inv_temp, trunc_u64 k, float top_p, trunc_u64* bins, trunc_u64* scr, unsigned* found) {
    const int tid = threadIdx.x;
    unsigned prefix = 0;
    trunc_u64 above = 0, target = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        __syncthreads();     // the pass before has read bins / found
        bins[tid] = 0;
        __syncthreads();
        const unsigned hi_mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        int cur = -1;        // runs of one digit (the top digits of log-probs hardly differ) go to LDS as one add
        trunc_u64 acc = 0;
        for (int v = tid; v < V1; v += 256) {
            const unsigned key = trunc_load<STAGE>(keys, x, v);
            if (key <= lo || ((key ^ prefix) & hi_mask)) continue;
            const int bin = (int)((key >> shift) & 255u);
            const trunc_u64 val = MASS ? trunc_weight(key, mx, inv_temp) : 1ull;
            if (bin != cur) {
                if (acc) atomicAdd(&bins[cur], acc);
                cur = bin;
                acc = 0;
            }
            acc += val;
        }
        if (acc) atomicAdd(&bins[cur], acc);
        if (tid == 0 && tie_val && !((lo ^ prefix) & hi_mask)) atomicAdd(&bins[(lo >> shift) & 255u], tie_val);
        __syncthreads();
        // thread t looks at digit 255 - t: the scan in thread order is the sum over the higher digits
        const int digit = 255 - tid;
        const trunc_u64 mine = bins[digit];
        trunc_u64 total;
        const trunc_u64 higher = trunc_scan(mine, scr, &total);
        if (shift == 24) {
            if (total == 0) return TruncSel{lo, 0, 0};
            if (MASS) {
                const double want = ceil((double)top_p * (double)total);
                target = want >= (double)total ? total : (trunc_u64)want;
                if (target < 1) target = 1;
            }
        }
        if (above + higher < target && above + higher + mine >= target) {   // exactly one thread
            found[0] = (unsigned)digit;
            bins[digit] = above + higher;      // its own bin: nobody else reads it any more
        }
        __syncthreads();
        const unsigned dg = found[0] & 255u;
        above = bins[dg];
        prefix |= dg << shift;
    }
    return TruncSel{prefix, above, target};
}
template <bool STAGE>
__global__ __launch_bounds__(256) void logp_truncate_rows_k(float* __restrict__ logp, long ldl, int V1, int top_k, float top_p,
                                                            float inv_temp, int* __restrict__ kept_n) {
    extern __shared__ unsigned trunc_keys[];     // STAGE: V1 keys
    __shared__ trunc_u64 bins[256];
    __shared__ trunc_u64 scr[4];
    __shared__ float wmax[4];
    __shared__ unsigned found[2];
    __shared__ int flags[2];                     // a NaN seen; kept entries
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* x = logp + r * ldl;
    if (tid == 0) flags[0] = flags[1] = 0, found[0] = found[1] = 0;
    __syncthreads();
    // pass 0: keys to LDS, the maximum, the finite count, NaN
    float mx = -INFINITY;
    int nfin = 0;
    bool nan = false;
    for (int v = tid; v < V1; v += 256) {
        const float xv = x[v];
        if constexpr (STAGE) trunc_keys[v] = trunc_key(xv);
        nan = nan || xv != xv;
        nfin += xv > -INFINITY;
        mx = fmaxf(mx, xv);
    }
    if (nan) flags[0] = 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) wmax[wave] = mx;
    trunc_u64 nfinite;
    trunc_scan((trunc_u64)nfin, scr, &nfinite);   // its barriers also publish the keys, wmax and flags
    mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (flags[0] || nfinite == 0) {               // left untouched: the pick's own rules apply
        if (tid == 0 && kept_n) kept_n[r] = flags[0] ? -1 : 0;
        return;
    }
    unsigned K = TRUNC_KEY_NINF;     // kept: key > K, and the m lowest ids with key == K
    trunc_u64 m = 0;
    if (top_k > 0 && (trunc_u64)top_k < nfinite) {
        const TruncSel s = trunc_select<STAGE, false>(trunc_keys, x, V1, TRUNC_KEY_NINF, 0, mx, inv_temp, (trunc_u64)top_k, 1.f,
                                                      bins, scr, found);
        K = s.key;
        m = s.target - s.above;
    }
    if (top_p < 1.f) {
        const trunc_u64 wK = m ? trunc_weight(K, mx, inv_temp) : 0ull;
        const TruncSel s = trunc_select<STAGE, true>(trunc_keys, x, V1, K, m * wK, mx, inv_temp, 0, top_p, bins, scr, found);
        if (s.target) {
            const trunc_u64 w = trunc_weight(s.key, mx, inv_temp), need = s.target - s.above;
            trunc_u64 mp = w ? (need + w - 1) / w : 1;
            if (s.key == K && mp > m) mp = m;     // cannot happen: the admitted part of top-k's tie group reaches the target
            K = s.key;
            m = mp;
        }
    }
    // the id of the m-th entry with key == K: thread t owns the contiguous ids [t * C, (t + 1) * C), as the multinomial pick
    int cut = -1;
    if (m) {
        const int C = (V1 + 255) / 256, v0 = min(V1, tid * C), v1 = min(V1, v0 + C);
        int ties = 0;
        for (int v = v0; v < v1; ++v) ties += trunc_load<STAGE>(trunc_keys, x, v) == K;
        trunc_u64 total;
        const trunc_u64 before = trunc_scan((trunc_u64)ties, scr, &total);
        if (tid == 0) found[1] = (unsigned)(V1 - 1);     // m >= the group's size (cannot happen): all of it
        __syncthreads();
        if (before < m && m <= before + (trunc_u64)ties) {
            int left = (int)(m - before);
            for (int v = v0; v < v1; ++v)
                if (trunc_load<STAGE>(trunc_keys, x, v) == K && --left == 0) {
                    found[1] = (unsigned)v;
                    break;
                }
        }
        __syncthreads();
        cut = (int)found[1];
    }
    int kept = 0;
    for (int v = tid; v < V1; v += 256) {
        const unsigned key = trunc_load<STAGE>(trunc_keys, x, v);
        const bool keep = key > K || (key == K && v <= cut);
        kept += keep;
        if (!keep && key != TRUNC_KEY_NINF) x[v] = -INFINITY;
    }
    if (kept_n) {
        if (kept) atomicAdd(&flags[1], kept);
        __syncthreads();
        if (tid == 0) kept_n[r] = flags[1];
    }
}
extern "C" int rfn_logp_truncate_rows(float* logp, int64_t ldl, int rows, int V1, int top_k, float top_p, float inv_temperature,
                                      int32_t* kept_n, void* stream) {
    if (rows <= 0 || V1 <= 0 || ldl < V1 || !(inv_temperature > 0.f) || !(top_p > 0.f && top_p < INFINITY))
        return RFN_ERR_SHAPE;
    if (!logp) return RFN_ERR_ARG;
    if ((top_k <= 0 || top_k >= V1) && top_p >= 1.f) return RFN_OK;     // both off: nothing is launched
    if (V1 > TRUNC_V1_MAX) return RFN_ERR_UNSUPPORTED;
    if (V1 <= TRUNC_STAGE_MAX)
        hipLaunchKernelGGL(logp_truncate_rows_k<true>, dim3(rows), dim3(256), (size_t)V1 * sizeof(unsigned), (hipStream_t)stream,
                           logp, (long)ldl, V1, top_k, top_p, inv_temperature, kept_n);
    else
        hipLaunchKernelGGL(logp_truncate_rows_k<false>, dim3(rows), dim3(256), 0, (hipStream_t)stream, logp, (long)ldl, V1, top_k,
                           top_p, inv_temperature, kept_n);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- greedy pick of sample() (misc/RecurrentFusionModel.py:619-649) -----------------------------------
// Order of the arg-max, as torch.max has it: NaN ranks above every number, equals (two NaNs included) go to the lower index.
// Every thread that owns an element starts from it, so a row of all -inf yields token 0 and a row with NaN its first NaN:
// the picked id is always in [0, V1).  On rows of ordinary numbers the comparisons are the ones `>` / `==` made.
__device__ __forceinline__ bool pick_gt(float x, float y) { return x > y || (x != x && y == y); }
__device__ __forceinline__ bool pick_before(float x, int i, float y, int j) {
    return pick_gt(x, y) || (!pick_gt(y, x) && i < j);
}
__global__ __launch_bounds__(256) void greedy_pick_k(const float* __restrict__ logp, long ldl, int V1, int t,
                                                     int64_t* __restrict__ next_ids, int64_t* __restrict__ seq_out,
                                                     long ld_seq, float* __restrict__ lp_out, long ld_lp,
                                                     const int32_t* unf_prev, int32_t* unf_out,
                                                     const int64_t* given /* may alias next_ids */) {
    __shared__ float vs[4];
    __shared__ int is[4];
    const int b = blockIdx.x;
    const float* x = logp + b * ldl;
    if (given) {   // the token was drawn elsewhere (multinomial): record its log-prob and the finished flags only
        if (threadIdx.x == 0) {
            long it = given[b];
            if (it < 0 || it >= V1) it = 0;
            int unf = (t == 1) ? 1 : unf_prev[b];
            unf = unf && (it > 0);
            unf_out[b] = unf;
            next_ids[b] = it;
            seq_out[b * ld_seq] = unf ? it : 0;
            lp_out[b * ld_lp] = x[it];
        }
        return;
    }
    float m = -INFINITY;
    int mi = 0x7fffffff;   // a thread past the row's end: loses to every real entry, -inf included
    if (threadIdx.x < V1) {
        m = x[threadIdx.x];
        mi = threadIdx.x;
    }
    for (int v = threadIdx.x + 256; v < V1; v += 256) {
        const float xv = x[v];
        if (pick_gt(xv, m)) {  // strided ascending scan keeps the first maximum per thread
            m = xv;
            mi = v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(mi, o, 64);
        if (pick_before(om, oi, m, mi)) {
            m = om;
            mi = oi;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        vs[wave] = m;
        is[wave] = mi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w)
            if (pick_before(vs[w], is[w], m, mi)) {
                m = vs[w];
                mi = is[w];
            }
        int unf = (t == 1) ? 1 : unf_prev[b];
        unf = unf && (mi > 0);
        unf_out[b] = unf;
        next_ids[b] = mi;
        seq_out[b * ld_seq] = unf ? mi : 0;
        lp_out[b * ld_lp] = m;
    }
}
extern "C" int rfn_pick_record(const float* logp, int64_t ldl, int B, int V1, int t, const int64_t* given,
                               int64_t* next_ids, int64_t* seq_out, int64_t ld_seq, float* lp_out, int64_t ld_lp,
                               const int32_t* unf_prev, int32_t* unf_out, void* stream) {
    if (B <= 0 || V1 <= 0 || t < 1) return RFN_ERR_SHAPE;
    if (!logp || !next_ids || !seq_out || !lp_out || !unf_out || (t > 1 && !unf_prev)) return RFN_ERR_ARG;
    hipLaunchKernelGGL(greedy_pick_k, dim3(B), dim3(given ? 64 : 256), 0, (hipStream_t)stream, logp, (long)ldl, V1, t, next_ids,
                       seq_out, (long)ld_seq, lp_out, (long)ld_lp, unf_prev, unf_out, given);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
extern "C" int rfn_greedy_pick(const float* logp, int64_t ldl, int B, int V1, int t, int64_t* next_ids,
                               int64_t* seq_out, int64_t ld_seq, float* lp_out, int64_t ld_lp,
                               const int32_t* unf_prev, int32_t* unf_out, void* stream) {
    return rfn_pick_record(logp, ldl, B, V1, t, nullptr, next_ids, seq_out, ld_seq, lp_out, ld_lp, unf_prev, unf_out, stream);
}
