// The self-critical reward on the GPU (get_rewards.py:39-112): CIDEr-D (cider/pyciderevalcap/ciderD, CiderD(n=4,
// sigma=6.0)) and BLEU-D (cider/pyciderevalcap/bleuD, BleuD(4) with option 'closest') of token-id captions, and
// compute_reward's mix of the two.
//
// Shared by both scorers (rw_): a caption is the ids of its row up to and including the first 0 (all T ids when there
// is none), as array_to_str builds it.  An n-gram (n = 1..4) packs into one uint64: four 15-bit ids and n in bits
// 60-62, so no valid key is 0 and equal keys are equal n-grams (no hash collision can change a result).  rw_cook turns
// a caption into first-occurrence keys, term counts and a word count; rw_refs_k stores that for every reference (one
// workgroup per image); a hypothesis kernel cooks its score row (one workgroup per row) and walks the references of
// its image through LDS with rw_lookup.  rw_reward_k forms the reward from the scores.  The _ex entry points take flags:
// with RFN_CAPTION_END_EXCLUDED a caption is the ids strictly before the first 0 (eval_utils.decode_sequence: what validation
// scores), which rw_cook honours for every scorer; an image with an empty reference is then bad (its rows score NaN).
//
// CIDEr-D (cd_): document frequencies live in an open-addressing, linear-probe table:
//   - corpus mode: the workspace table is cleared and filled every call; one integer atomicAdd per unique
//     n-gram of an image adds the number of score rows that point at that image (compute_reward's crefs);
//   - table mode: rfn_ciderd_table_build inserts a precomputed df once and stores log(max(1, df)).
// Launches of one call: [clear], refs (with the df insert in corpus mode), ref_vec (tf-idf values and per-n norms of
// every reference), hyp (the row's vector, the clipped similarity against every reference of its image, the score).
// Everything after the df counts is fp64 in fixed summation orders, so scores are bitwise reproducible; the only
// atomics are the integer df counts.
//
// Consensus reranking (cs_, cd_pair_k; rfn.h "consensus reranking"): an image's n candidates are cooked once as its references;
// cd_pair_k (one workgroup per (image, candidate)) fills a row of the pairwise utility with cd_pair_term, the device function
// cd_hyp_k's reference loop runs too, and forms the leave-one-out consensus score; cs_pick_k picks and gathers.
//
// Caption-set diversity (cs_div_k, cs_loo_bleu_k, cs_bleu_corpus_k, cs_eig_k; rfn.h "caption-set diversity"): the same cooked
// candidates and the same U, read for Div-m (distinct n-grams over the set), mBLEU (each candidate against the others) and
// Self-CIDEr (the spectrum of the symmetrised U).  rw_group_stats_k: best / argmax / mean of a score column per image.
//
// BLEU-D (bd_): launches of one call: refs, hyp (clip every distinct n-gram of the row against the maximum count over
// the image's references, reduce correct[4], pick the closest reference length, write the row's four scores and its
// integer components) and, when asked for, corpus (the same formula over the sums of the components).  Everything
// before the formula is integer counting, the formula is fp64 in one thread: bitwise reproducible, no atomics on
// global memory.
#include <math.h>

#include <algorithm>

#include "rfn_common.h"

#define RW_N 4
#define RW_MAX_T 64
#define RW_MAX_REFS 32
#define RW_MAX_ID 32767
#define RW_THREADS 256   // >= RW_N * RW_MAX_T: one thread per n-gram slot (n, position)

__device__ __forceinline__ uint64_t cd_hash(uint64_t k) {   // splitmix64 finaliser
    k ^= k >> 30;
    k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 27;
    k *= 0x94D049BB133111EBull;
    k ^= k >> 31;
    return k;
}

// slot of `key` in a table of `slots` (a power of two) entries, -1 when absent
__device__ __forceinline__ long cd_find(const uint64_t* keys, long slots, uint64_t key) {
    long h = (long)(cd_hash(key) & (uint64_t)(slots - 1));
    for (long probe = 0; probe < slots; ++probe) {
        const uint64_t k = keys[h];
        if (k == key) return h;
        if (k == 0) return -1;
        h = (h + 1) & (slots - 1);
    }
    return -1;
}

// slot that holds `key` after inserting it (-1 when the table is full)
__device__ __forceinline__ long cd_insert(uint64_t* keys, long slots, uint64_t key) {
    long h = (long)(cd_hash(key) & (uint64_t)(slots - 1));
    for (long probe = 0; probe < slots; ++probe) {
        const unsigned long long prev = atomicCAS((unsigned long long*)(keys + h), 0ull, (unsigned long long)key);
        if (prev == 0ull || prev == (unsigned long long)key) return h;
        h = (h + 1) & (slots - 1);
    }
    return -1;
}

// log(max(1, df)) of `key`: corpus mode counts integer df in cnt[], table mode stores the log itself
struct CdDf {
    const uint64_t* keys;
    const uint32_t* cnt;      // corpus mode
    const double* logdf;      // table mode
    long slots;
};
__device__ __forceinline__ double cd_logdf(const CdDf& df, uint64_t key) {
    const long h = cd_find(df.keys, df.slots, key);
    if (df.logdf) return h < 0 ? 0.0 : df.logdf[h];
    return log(fmax(1.0, h < 0 ? 0.0 : (double)df.cnt[h]));
}

// Cook one caption of T ids (block-wide; blockDim.x = RW_THREADS).  Thread t < 4T owns n-gram slot (n = t / T,
// p = t % T); it returns the key when its slot holds the FIRST occurrence of an n-gram in the caption (0 otherwise) and
// the n-gram's term count in *tf.  *words: the caption's word count; the return of *bad: an id outside [0, vocab].
// excl: the caption ends before its first 0 (and may be empty) instead of after it.
// skey: RW_THREADS keys of LDS; sw / sbad: LDS ints.  All threads must call it.
__device__ uint64_t rw_cook(const int64_t* __restrict__ ids, int T, int vocab, int excl, uint64_t* skey, int* sw, int* sbad,
                            int* tf, int* words, int* bad) {
    const int t = threadIdx.x;
    if (t == 0) {
        *sw = T;
        *sbad = 0;
    }
    __syncthreads();
    int64_t id = -1;
    if (t < T) {
        id = ids[t];
        if (id == 0) atomicMin(sw, excl ? t : t + 1);
    }
    __syncthreads();
    const int W = *sw;
    if (t < W && (id < 0 || id > vocab)) atomicOr(sbad, 1);
    __syncthreads();
    const int b = *sbad;
    uint64_t key = 0;
    int n = 0, p = 0;
    if (t < RW_N * T) {
        n = t / T;
        p = t - n * T;
        if (!b && p + n < W) {
            key = (uint64_t)(n + 1) << 60;
            for (int k = 0; k <= n; ++k) key |= (uint64_t)ids[p + k] << (15 * k);
        }
    }
    skey[t] = key;
    __syncthreads();
    int cnt = 0;
    if (key) {
        bool first = true;
        for (int q = n * T; q < n * T + T; ++q) {
            if (skey[q] == key) {
                ++cnt;
                if (q < t) first = false;
            }
        }
        if (!first) key = 0;
    }
    __syncthreads();   // the caller may overwrite skey next
    *tf = cnt;
    *words = W;
    *bad = b;
    return key;
}

// ---- corpus mode: clear the df table ----------------------------------------------------------------
__global__ void cd_clear_k(uint64_t* __restrict__ keys, uint32_t* __restrict__ cnt, long slots) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long)gridDim.x * blockDim.x) {
        keys[i] = 0;
        cnt[i] = 0;
    }
}

// ---- references: one workgroup per image ----------------------------------------------------------------
// Writes, per (image, ref) slot: rkey[4*Tg] (first occurrences), rcnt[4*Tg] (term counts), rwords (the word count); per
// image img_bad.  CORPUS_DF (CIDEr-D's corpus mode) then adds the image's row count to the df of every n-gram its
// references hold (once per image); only that instantiation uses dynamic LDS: max_refs * 4 * Tg keys.  excl: rw_cook's; an
// empty reference then makes the image bad.
template <bool CORPUS_DF>
__global__ __launch_bounds__(RW_THREADS) void rw_refs_k(const int64_t* __restrict__ gts, const int32_t* __restrict__ n_refs,
                                                        int max_refs, int Tg, int vocab, int excl, uint64_t* __restrict__ rkey,
                                                        int32_t* __restrict__ rcnt, int32_t* __restrict__ rwords,
                                                        int32_t* __restrict__ img_bad, const int32_t* __restrict__ row_img,
                                                        int n_rows, uint64_t* dkeys, uint32_t* dcnt, long dslots) {
    extern __shared__ uint64_t all[];
    __shared__ uint64_t skey[RW_THREADS];
    __shared__ int sw, sbad, srows;
    const int i = blockIdx.x, t = threadIdx.x, S = RW_N * Tg;
    const int nr = n_refs[i];
    int bad_img = (nr < 1 || nr > max_refs);
    const int nrc = bad_img ? 0 : nr;
    for (int j = 0; j < nrc; ++j) {
        int tf, words, bad;
        const uint64_t key = rw_cook(gts + ((long)i * max_refs + j) * Tg, Tg, vocab, excl, skey, &sw, &sbad, &tf, &words, &bad);
        const long o = ((long)i * max_refs + j) * S;
        if (t < S) {
            rkey[o + t] = key;
            rcnt[o + t] = tf;
            if (CORPUS_DF) all[j * S + t] = key;
        }
        if (t == 0) rwords[(long)i * max_refs + j] = words;
        bad_img |= bad | (words == 0);   // words == 0: under excl only
    }
    if (t == 0) img_bad[i] = bad_img;
    if (!CORPUS_DF || bad_img) return;   // bad_img is block-uniform
    if (t == 0) srows = 0;
    __syncthreads();
    int mine = 0;
    for (int r = t; r < n_rows; r += RW_THREADS) mine += (row_img[r] == i);
    if (mine) atomicAdd(&srows, mine);
    __syncthreads();
    const int rows = srows;
    if (rows == 0) return;
    for (int x = t; x < nrc * S; x += RW_THREADS) {
        const uint64_t key = all[x];
        if (!key) continue;
        const int j = x / S, s = x - j * S, n = s / Tg;
        bool seen = false;
        for (int jj = 0; jj < j && !seen; ++jj)
            for (int q = 0; q < Tg; ++q)
                if (all[jj * S + n * Tg + q] == key) {
                    seen = true;
                    break;
                }
        if (seen) continue;
        const long h = cd_insert(dkeys, dslots, key);
        if (h >= 0) atomicAdd(dcnt + h, (uint32_t)rows);
    }
}

// The value one reference holds for `key`, an n-gram of order n + 1 of the caller's caption (0 when key is 0 or absent).
// Block-wide: stages the reference's 4*Tg keys and values into rk / rv (RW_THREADS entries of LDS each), then every thread
// scans the n-segment for its own key.  All threads must call it, and pass a barrier before the next call.
template <typename V>
__device__ __forceinline__ V rw_lookup(const uint64_t* __restrict__ ref_key, const V* __restrict__ ref_val, int Tg, uint64_t key,
                                       int n, uint64_t* rk, V* rv) {
    const int t = threadIdx.x;
    if (t < RW_N * Tg) {
        rk[t] = ref_key[t];
        rv[t] = ref_val[t];
    }
    __syncthreads();
    if (key)
        for (int q = n * Tg; q < n * Tg + Tg; ++q)
            if (rk[q] == key) return rv[q];
    return 0;
}

// ---- CIDEr-D reference vectors: one thread per (image, ref, n) -------------------------------------------
__global__ void cd_ref_vec_k(const int32_t* __restrict__ n_refs, const int32_t* __restrict__ img_bad, int n_img, int max_refs,
                             int Tg, const uint64_t* __restrict__ rkey, const int32_t* __restrict__ rcnt,
                             double* __restrict__ rval, double* __restrict__ rnorm, CdDf df, double ref_docs,
                             const double* __restrict__ ref_docs_dev /* NULL, or where the count lives (consensus, corpus mode) */) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long)n_img * max_refs * RW_N) return;
    if (ref_docs_dev) ref_docs = *ref_docs_dev;
    const int n = (int)(g % RW_N);
    const long ij = g / RW_N;
    const int i = (int)(ij / max_refs), j = (int)(ij % max_refs);
    if (img_bad[i] || j >= n_refs[i]) return;
    const double ref_len = log(ref_docs);
    const long o = ij * RW_N * Tg + (long)n * Tg;
    double nrm = 0.0;
    for (int p = 0; p < Tg; ++p) {
        const uint64_t key = rkey[o + p];
        if (!key) continue;
        const double v = (double)rcnt[o + p] * (ref_len - cd_logdf(df, key));
        rval[o + p] = v;   // only under a key: cd_hyp_k reads a value only where the key matches
        nrm += v * v;
    }
    rnorm[g] = sqrt(nrm);
}

// ---- CIDEr-D, one (hypothesis, reference) pair: what cd_hyp_k's reference loop and cd_pair_k's candidate loop both run ----
// Block-wide.  key: the caller's n-gram (thread t owns slot t of the hypothesis, T ids wide); hk / hv: the hypothesis' keys and
// tf-idf values (LDS), hnorm its four norms, hlen its bigram count; ref_*: the cooked reference (Tg ids wide).  Thread t < RW_N
// returns the order-(t + 1) term: the clipped similarity, divided by both norms when both are non-zero, times the Gaussian length
// penalty, added to `a` (cd_hyp_k's running sum over references; 0.0 gives the term itself); the others return `a`.  All threads
// must call it, and pass a barrier before the next call.
__device__ __forceinline__ double cd_pair_term(double a, uint64_t key, int T, const uint64_t* hk, const double* hv, const double* hnorm, int hlen,
                                               const uint64_t* __restrict__ ref_key, const double* __restrict__ ref_val,
                                               const double* __restrict__ ref_norm, int ref_words, int Tg, double sigma, uint64_t* rk,
                                               double* rv, double* contrib) {
    const int t = threadIdx.x;
    const double vr = rw_lookup(ref_key, ref_val, Tg, key, t / T, rk, rv);
    if (key) {
        const double vh = hv[t];
        contrib[t] = (vr < vh ? vr : vh) * vr;
    }
    __syncthreads();
    if (t < RW_N) {   // the reference's order: n-grams of one n in first-occurrence order
        double s = 0.0;
        for (int p = 0; p < T; ++p)
            if (hk[t * T + p]) s += contrib[t * T + p];
        const double nh = hnorm[t], nrf = ref_norm[t];
        if (nh != 0.0 && nrf != 0.0) s /= nh * nrf;
        const double delta = (double)(hlen - (ref_words > 1 ? ref_words - 1 : 0));
        s *= exp(-(delta * delta) / (2.0 * sigma * sigma));
        a += s;
    }
    return a;
}

// ---- CIDEr-D hypotheses: one workgroup per score row ---------------------------------------------------
__global__ __launch_bounds__(RW_THREADS) void cd_hyp_k(const int64_t* __restrict__ res, int T, const int32_t* __restrict__ row_img,
                                                       int n_img, const int32_t* __restrict__ n_refs, const int32_t* __restrict__ img_bad,
                                                       int max_refs, int Tg, const uint64_t* __restrict__ rkey,
                                                       const double* __restrict__ rval, const double* __restrict__ rnorm,
                                                       const int32_t* __restrict__ rwords, int vocab, int excl, CdDf df,
                                                       double ref_docs, double sigma, double* __restrict__ scores) {
    __shared__ uint64_t skey[RW_THREADS], hk[RW_THREADS], rk[RW_THREADS];
    __shared__ double hv[RW_THREADS], rv[RW_THREADS], contrib[RW_THREADS];
    __shared__ double hnorm[RW_N], acc[RW_N];
    __shared__ int sw, sbad;
    const int r = blockIdx.x, t = threadIdx.x, Sg = RW_N * Tg;
    const int i = row_img[r];
    if (i < 0 || i >= n_img || img_bad[i]) {   // block-uniform
        if (t == 0) scores[r] = __builtin_nan("");
        return;
    }
    const int nr = n_refs[i];
    int tf, words, bad;
    const uint64_t key = rw_cook(res + (long)r * T, T, vocab, excl, skey, &sw, &sbad, &tf, &words, &bad);
    if (bad) {
        if (t == 0) scores[r] = __builtin_nan("");
        return;
    }
    const double ref_len = log(ref_docs);
    hk[t] = key;
    hv[t] = key ? (double)tf * (ref_len - cd_logdf(df, key)) : 0.0;
    __syncthreads();
    double a = 0.0;
    if (t < RW_N) {   // the reference's order: n-grams of one n in first-occurrence order
        double s = 0.0;
        for (int p = 0; p < T; ++p)
            if (hk[t * T + p]) s += hv[t * T + p] * hv[t * T + p];
        hnorm[t] = sqrt(s);
    }
    const int hlen = words > 1 ? words - 1 : 0;
    for (int j = 0; j < nr; ++j) {
        const long ij = (long)i * max_refs + j;
        a = cd_pair_term(a, key, T, hk, hv, hnorm, hlen, rkey + ij * Sg, rval + ij * Sg, rnorm + ij * RW_N, rwords[ij], Tg, sigma, rk,
                         rv, contrib);
        __syncthreads();
    }
    if (t < RW_N) acc[t] = a;
    __syncthreads();
    if (t == 0) {
        double m = (((0.0 + acc[0]) + acc[1]) + acc[2]) + acc[3];
        m /= (double)RW_N;
        m /= (double)nr;
        scores[r] = m * 10.0;
    }
}

// ---- CIDEr-D table mode: build ------------------------------------------------------------------------
__global__ void cd_table_clear_k(uint64_t* __restrict__ keys, double* __restrict__ logdf, long slots) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (long)gridDim.x * blockDim.x) {
        keys[i] = 0;
        logdf[i] = 0.0;
    }
}
__global__ void cd_table_insert_k(const int32_t* __restrict__ ids, const double* __restrict__ counts, long n_entries, int vocab,
                                  uint64_t* __restrict__ keys, double* __restrict__ logdf, long slots) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_entries) return;
    int len = 0;
    while (len < RW_N && ids[e * RW_N + len] >= 0) ++len;
    if (len == 0) return;
    uint64_t key = (uint64_t)len << 60;
    for (int k = 0; k < RW_N; ++k) {
        const int id = ids[e * RW_N + k];
        if (k < len) {
            if (id > vocab) return;   // can never match a caption of this vocabulary
            key |= (uint64_t)id << (15 * k);
        } else if (id >= 0) {
            return;                   // ids after the padding: not an n-gram
        }
    }
    const long h = cd_insert(keys, slots, key);
    if (h >= 0) logdf[h] = log(fmax(1.0, counts[e]));
}

// ---- BLEU-D ---------------------------------------------------------------------------------------------------
#define BD_COMPS 10   // testlen, reflen, guess[4], correct[4]

__device__ void bd_formula(const double* correct, const double* guess, double testlen, double reflen, double* bleu) {
    const double small = 1e-9, tiny = 1e-15;
    double p = 1.0;
    for (int k = 0; k < RW_N; ++k) {
        p *= (correct[k] + tiny) / (guess[k] + small);
        bleu[k] = pow(p, 1.0 / (double)(k + 1));
    }
    const double ratio = (testlen + tiny) / (reflen + small);
    if (ratio < 1.0) {
        const double bp = exp(1.0 - 1.0 / ratio);
        for (int k = 0; k < RW_N; ++k) bleu[k] *= bp;
    }
}

// one workgroup per score row.  comps: n_rows x BD_COMPS (testlen = -1 marks a row that scores NaN); ucomps: NULL or the
// caller's copy of it (zeros for a NaN row).
__global__ __launch_bounds__(RW_THREADS) void bd_hyp_k(const int64_t* __restrict__ res, int T, const int32_t* __restrict__ row_img,
                                                       int n_img, const int32_t* __restrict__ n_refs, const int32_t* __restrict__ img_bad,
                                                       int max_refs, int Tg, const uint64_t* __restrict__ rkey,
                                                       const int32_t* __restrict__ rcnt, const int32_t* __restrict__ rwords, int vocab,
                                                       int excl, double* __restrict__ scores, int32_t* __restrict__ comps,
                                                       int32_t* __restrict__ ucomps) {
    __shared__ uint64_t skey[RW_THREADS], rk[RW_THREADS];
    __shared__ int rc[RW_THREADS], clip[RW_THREADS];
    __shared__ int correct[RW_N];
    __shared__ int sw, sbad;
    const int r = blockIdx.x, t = threadIdx.x, Sg = RW_N * Tg;
    const int i = row_img[r];
    int tf = 0, words = 0, bad = (i < 0 || i >= n_img || img_bad[i]);   // block-uniform
    uint64_t key = 0;
    if (!bad) key = rw_cook(res + (long)r * T, T, vocab, excl, skey, &sw, &sbad, &tf, &words, &bad);
    if (bad) {
        if (t < RW_N) scores[(long)r * RW_N + t] = __builtin_nan("");
        if (t < BD_COMPS) {
            comps[(long)r * BD_COMPS + t] = t == 0 ? -1 : 0;
            if (ucomps) ucomps[(long)r * BD_COMPS + t] = 0;
        }
        return;
    }
    const int nr = n_refs[i];
    const int n = t / T;
    int maxc = 0;
    for (int j = 0; j < nr; ++j) {
        const long ij = (long)i * max_refs + j;
        maxc = max(maxc, rw_lookup(rkey + ij * Sg, rcnt + ij * Sg, Tg, key, n, rk, rc));
        __syncthreads();
    }
    clip[t] = key ? min(tf, maxc) : 0;
    __syncthreads();
    if (t < RW_N) {
        int s = 0;
        for (int p = 0; p < T; ++p) s += clip[t * T + p];
        correct[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        int reflen = rwords[(long)i * max_refs], best = abs(reflen - words);   // min((|l - testlen|, l)): a tie takes the shorter
        for (int j = 1; j < nr; ++j) {
            const int l = rwords[(long)i * max_refs + j], d = abs(l - words);
            if (d < best || (d == best && l < reflen)) {
                best = d;
                reflen = l;
            }
        }
        int c[BD_COMPS];
        c[0] = words;
        c[1] = reflen;
        double cor[RW_N], gue[RW_N], bleu[RW_N];
        for (int k = 0; k < RW_N; ++k) {
            c[2 + k] = words - k > 0 ? words - k : 0;
            c[2 + RW_N + k] = correct[k];
            gue[k] = (double)c[2 + k];
            cor[k] = (double)correct[k];
        }
        bd_formula(cor, gue, (double)words, (double)reflen, bleu);
        for (int k = 0; k < RW_N; ++k) scores[(long)r * RW_N + k] = bleu[k];
        for (int k = 0; k < BD_COMPS; ++k) {
            comps[(long)r * BD_COMPS + k] = c[k];
            if (ucomps) ucomps[(long)r * BD_COMPS + k] = c[k];
        }
    }
}

// one workgroup: the corpus-level four from the integer sums of the rows' components (NaN rows left out)
__global__ __launch_bounds__(RW_THREADS) void bd_corpus_k(const int32_t* __restrict__ comps, int n_rows, double* __restrict__ corpus) {
    __shared__ long long part[RW_THREADS];
    __shared__ long long tot[BD_COMPS];
    const int t = threadIdx.x;
    for (int k = 0; k < BD_COMPS; ++k) {
        long long s = 0;
        for (int r = t; r < n_rows; r += RW_THREADS)
            if (comps[(long)r * BD_COMPS] >= 0) s += comps[(long)r * BD_COMPS + k];
        part[t] = s;
        __syncthreads();
        for (int w = RW_THREADS / 2; w > 0; w >>= 1) {
            if (t < w) part[t] += part[t + w];
            __syncthreads();
        }
        if (t == 0) tot[k] = part[0];
        __syncthreads();
    }
    if (t == 0) {
        double cor[RW_N], gue[RW_N], bleu[RW_N];
        for (int k = 0; k < RW_N; ++k) {
            gue[k] = (double)tot[2 + k];
            cor[k] = (double)tot[2 + RW_N + k];
        }
        bd_formula(cor, gue, (double)tot[0], (double)tot[1], bleu);
        for (int k = 0; k < RW_N; ++k) corpus[k] = bleu[k];
    }
}

// ---- ROUGE-L (coco-caption/pycocoevalcap/rouge) ---------------------------------------------------------------------------
// One workgroup per score row, one launch.  Wave w takes the references j = w, w + 4, ... of the row's image: lane q holds the
// reference's id q, so a ballot of (id == hyp[p]) is the 64-bit match mask of hypothesis word p and the LCS length is the
// bit-vector recurrence V = (V + (V & M)) | (V - (V & M)) over the hypothesis words (Hyyro 2004; V starts all ones, the LCS is the
// number of zero bits).  The masks are wave-uniform, so the recurrence runs on the scalar unit.  Integer throughout; thread 0 then
// forms the row's one fp64 formula from max(lcs) / len(hyp) and max over references of lcs / len(ref).
__global__ __launch_bounds__(RW_THREADS) void rl_score_k(const int64_t* __restrict__ res, int T, const int32_t* __restrict__ row_img,
                                                         int n_img, const int64_t* __restrict__ gts, const int32_t* __restrict__ n_refs,
                                                         int max_refs, int Tg, int vocab, int excl, double beta,
                                                         double* __restrict__ scores, int32_t* __restrict__ lcs_out /* or NULL */) {
    __shared__ int hyp[RW_MAX_T];
    __shared__ int slcs[RW_MAX_REFS], slen[RW_MAX_REFS];
    __shared__ int shl, sbad;
    const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = row_img[r];
    int nr = 0;
    bool bad = (i < 0 || i >= n_img);   // block-uniform
    if (!bad) {
        nr = n_refs[i];
        bad = (nr < 1 || nr > max_refs);
    }
    if (lcs_out && t < max_refs) lcs_out[(long)r * max_refs + t] = 0;
    if (bad) {
        if (t == 0) scores[r] = __builtin_nan("");
        return;
    }
    if (t == 0) sbad = 0;
    __syncthreads();
    if (wave == 0) {   // the hypothesis: its length and its range check
        const int64_t id = lane < T ? res[(long)r * T + lane] : -1;
        const unsigned long long zero = __ballot(lane < T && id == 0);
        int hl = T;
        if (zero) hl = __ffsll(zero) - 1 + (excl ? 0 : 1);
        if (lane < hl && (id < 0 || id > vocab)) sbad = 1;
        hyp[lane] = (int)id;
        if (lane == 0) shl = hl;
    }
    __syncthreads();
    const int hl = shl;
    for (int j = wave; j < nr; j += RW_THREADS / 64) {
        const int64_t id = lane < Tg ? gts[((long)i * max_refs + j) * Tg + lane] : -1;
        const unsigned long long zero = __ballot(lane < Tg && id == 0);
        int rl = Tg;
        if (zero) rl = __ffsll(zero) - 1 + (excl ? 0 : 1);
        if ((lane < rl && (id < 0 || id > vocab)) || rl == 0) sbad = 1;   // an empty reference (excl only) is bad too
        const int tok = (int)id;
        unsigned long long V = ~0ull;
        for (int p = 0; p < hl; ++p) {
            const unsigned long long U = V & __ballot(lane < rl && tok == hyp[p]);
            V = (V + U) | (V - U);
        }
        if (lane == 0) {
            slcs[j] = __popcll(~V);
            slen[j] = rl;
        }
    }
    __syncthreads();
    if (sbad) {   // block-uniform
        if (t == 0) scores[r] = __builtin_nan("");
        return;
    }
    if (lcs_out && t < nr) lcs_out[(long)r * max_refs + t] = slcs[t];
    if (t == 0) {
        double score = 0.0;
        if (hl > 0) {   // an empty hypothesis is the reference's one empty token, which matches nothing
            double pmax = 0.0, rmax = 0.0;
            for (int j = 0; j < nr; ++j) {
                pmax = fmax(pmax, (double)slcs[j] / (double)hl);
                rmax = fmax(rmax, (double)slcs[j] / (double)slen[j]);
            }
            const double b2 = beta * beta;
            if (pmax != 0.0 && rmax != 0.0) score = ((1.0 + b2) * pmax * rmax) / (rmax + b2 * pmax);
        }
        scores[r] = score;
    }
}

// ---- the corpus mean of a score column: one workgroup, fp64 in a fixed order (thread t sums x[t], x[t + 256], ..., then a
// binary tree over LDS), NaN rows skipped and counted.  No atomics: bitwise reproducible.
__global__ __launch_bounds__(RW_THREADS) void rw_mean_k(const double* __restrict__ x, long n, long stride, double* __restrict__ mean,
                                                        int64_t* __restrict__ skipped) {
#pragma clang fp contract(off)
    __shared__ double part[RW_THREADS];
    __shared__ long long nan_part[RW_THREADS];
    const int t = threadIdx.x;
    double s = 0.0;
    long long k = 0;
    for (long r = t; r < n; r += RW_THREADS) {
        const double v = x[r * stride];
        if (v != v)
            ++k;
        else
            s += v;
    }
    part[t] = s;
    nan_part[t] = k;
    __syncthreads();
    for (int w = RW_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            part[t] += part[t + w];
            nan_part[t] += nan_part[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        const long kept = n - (long)nan_part[0];
        *mean = kept > 0 ? part[0] / (double)kept : __builtin_nan("");
        if (skipped) *skipped = (int64_t)nan_part[0];
    }
}

// ---- the reward: compute_reward's mix ((bleu4 * w_b) + (cider * w_c)) + spice * 0, each product and sum rounded on its own;
// a NULL scorer is the 0 * weight the reference adds (which also turns a -0 into +0)
__global__ void rw_reward_k(const double* __restrict__ cider, double cider_weight, const double* __restrict__ bleu,
                            double bleu4_weight, int B, int T, int use_baseline, float* __restrict__ out, double* __restrict__ out64) {
#pragma clang fp contract(off)
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long)B * T) return;
    const int b = (int)(g / T);
    double sb = 0.0, sc = 0.0;
    if (bleu) {
        sb = bleu[(long)b * RW_N + 3];
        if (use_baseline) sb = sb - bleu[(long)(B + b) * RW_N + 3];
    }
    if (cider) {
        sc = cider[b];
        if (use_baseline) sc = sc - cider[B + b];
    }
    const double tb = sb * bleu4_weight, tc = sc * cider_weight;
    const double v = (tb + tc) + 0.0;
    if (out) out[g] = (float)v;
    if (out64) out64[g] = v;
}

// ---- the grouped reward (rfn.h "multi-sample self-critical"): row r = k * n + j is draw j of image k; the baseline of a draw is
// the mean of the image's other n - 1 scores, summed from 0.0 in ascending order and divided once; then rw_reward_k's mix
__device__ __forceinline__ double rw_loo_diff(const double* __restrict__ s, long stride, int r, int n, int baseline) {
#pragma clang fp contract(off)
    const double mine = s[(long)r * stride];
    if (!baseline) return mine;
    const int k0 = r - r % n;
    double sum = 0.0;
    for (int i = 0; i < n; ++i)
        if (k0 + i != r) sum = sum + s[(long)(k0 + i) * stride];
    const double base = sum / (double)(n - 1);
    return mine - base;
}
__global__ void rw_reward_group_k(const double* __restrict__ cider, double cider_weight, const double* __restrict__ bleu,
                                  double bleu4_weight, int B, int n, int T, int baseline, float* __restrict__ out,
                                  double* __restrict__ out64) {
#pragma clang fp contract(off)
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long)B * T) return;
    const int r = (int)(g / T);
    const double sb = bleu ? rw_loo_diff(bleu + 3, RW_N, r, n, baseline) : 0.0;
    const double sc = cider ? rw_loo_diff(cider, 1, r, n, baseline) : 0.0;
    const double tb = sb * bleu4_weight, tc = sc * cider_weight;
    const double v = (tb + tc) + 0.0;
    if (out) out[g] = (float)v;
    if (out64) out64[g] = v;
}

// ---- the reward of a distinct-sample set (rfn.h rfn_scst_reward_distinct) -----------------------------------------------------------
// The n rows of an image are a sample WITHOUT replacement (stochastic beam search, rfn_beam_step_sbs) with importance weights w_j:
// the normalised importance-weighted policy-gradient estimator with its built-in baseline of Kool, van Hoof and Welling,
// "Stochastic Beams and Where to Find Them" (ICML 2019), section 4.2 / appendix: q_j = w_j / sum_i w_i over the rows with w > 0,
// base = sum_j q_j * s_j, coefficient q_j * (s_j - base), times n so that the criterion's 1 / (images * n) leaves sum_j q_j in the
// place of the group step's (1 / n) sum_j.  Rows with w <= 0 (dead rows, the threshold row) or a NaN weight enter no sum and get 0.0.
__device__ __forceinline__ double rw_mixed_score(const double* __restrict__ cider, double cider_weight, const double* __restrict__ bleu,
                                                 double bleu4_weight, int r) {
#pragma clang fp contract(off)
    const double sb = bleu ? bleu[(long)r * RW_N + 3] : 0.0;
    const double sc = cider ? cider[r] : 0.0;
    const double tb = sb * bleu4_weight, tc = sc * cider_weight;
    return (tb + tc) + 0.0;
}
__global__ void rw_reward_distinct_k(const double* __restrict__ cider, double cider_weight, const double* __restrict__ bleu,
                                     double bleu4_weight, const double* __restrict__ weight, int B, int n, int T, int baseline,
                                     float* __restrict__ out, double* __restrict__ out64) {
#pragma clang fp contract(off)
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long)B * T) return;
    const int r = (int)(g / T), k0 = r - r % n;
    double v = 0.0;
    const double w = weight[r];
    if (w > 0.0) {
        double wsum = 0.0;
        for (int i = 0; i < n; ++i) {
            const double wi = weight[k0 + i];
            if (wi > 0.0) wsum = wsum + wi;
        }
        if (wsum - wsum == 0.0) {                 // finite (w > 0 rows exist: this one)
            double base = 0.0;
            if (baseline)
                for (int i = 0; i < n; ++i) {
                    const double wi = weight[k0 + i];
                    if (wi > 0.0) {
                        const double qi = wi / wsum;
                        const double term = qi * rw_mixed_score(cider, cider_weight, bleu, bleu4_weight, k0 + i);
                        base = base + term;
                    }
                }
            const double q = w / wsum;
            const double diff = rw_mixed_score(cider, cider_weight, bleu, bleu4_weight, r) - base;
            const double c = q * diff;
            v = c * (double)n;
        }
    }
    if (out) out[g] = (float)v;
    if (out64) out64[g] = v;
}

// ---- consensus (minimum-Bayes-risk) reranking (rfn.h "consensus reranking") ---------------------------------------------------
// The n candidates of an image are cooked ONCE as that image's "references" (rw_refs_k, cd_ref_vec_k); cd_pair_k then walks
// candidate i against every candidate j with cd_pair_term, the loop body of cd_hyp_k, so a pair is cd_hyp_k's bits.
//
// cs_prep_k (one workgroup): the per-image candidate counts the cooking reads (n where the caller passed none), the score rows of
// the corpus df (entry k * n + j points at image k when candidate j is valid, at -1 otherwise, so rw_refs_k<true> adds n_cand[k]
// per image) and their number, the corpus document count.  Integer counting only.
__global__ __launch_bounds__(RW_THREADS) void cs_prep_k(const int32_t* __restrict__ n_cand, int n_img, int n, int32_t* __restrict__ nc_eff,
                                                        int32_t* __restrict__ row_img, double* __restrict__ ref_docs) {
    __shared__ int total;
    const int t = threadIdx.x;
    if (t == 0) total = 0;
    __syncthreads();
    for (long x = t; x < (long)n_img * n; x += RW_THREADS) {
        const int k = (int)(x / n), j = (int)(x - (long)k * n);
        const int nc = n_cand ? n_cand[k] : n;
        const bool ok = nc >= 1 && nc <= n;
        row_img[x] = (ok && j < nc) ? k : -1;
        if (j == 0) {
            nc_eff[k] = nc;
            if (ok) atomicAdd(&total, nc);
        }
    }
    __syncthreads();
    if (t == 0) *ref_docs = (double)total;
}

// c[i] = (sum_{j != i} w_j U[i][j]) / (sum_{j != i} w_j), j ascending, every product, sum and the quotient rounded on its own
__device__ __forceinline__ double cs_leave_one_out(const double* u, const double* __restrict__ w, int nc, int i) {
#pragma clang fp contract(off)
    double num = 0.0, den = 0.0;
    for (int j = 0; j < nc; ++j) {
        if (j == i) continue;
        const double wj = w ? w[j] : 1.0;
        const double prod = wj * u[j];
        num = num + prod;
        den = den + wj;
    }
    return den == 0.0 ? 0.0 : num / den;
}

// One workgroup per (image k, candidate i): row i of U[k] and c[k][i].  Grid choice: DESIGN.md section 9.
__global__ __launch_bounds__(RW_THREADS) void cd_pair_k(const int32_t* __restrict__ n_cand, const int32_t* __restrict__ img_bad, int n,
                                                        int T, const uint64_t* __restrict__ rkey, const double* __restrict__ rval,
                                                        const double* __restrict__ rnorm, const int32_t* __restrict__ rwords,
                                                        const double* __restrict__ weights, double sigma, double* __restrict__ U,
                                                        double* __restrict__ c) {
    __shared__ uint64_t hk[RW_THREADS], rk[RW_THREADS];
    __shared__ double hv[RW_THREADS], rv[RW_THREADS], contrib[RW_THREADS];
    __shared__ double sn[RW_N], su[RW_MAX_REFS];
    __shared__ int swbad;
    const int k = blockIdx.x / n, i = blockIdx.x - k * n, t = threadIdx.x, S = RW_N * T;
    const long ki = (long)k * n + i;
    const double nan = __builtin_nan("");
    const int nc = n_cand[k];
    int bad = img_bad[k];   // block-uniform; covers n_cand outside [1, n]
    if (!bad && weights) {
        if (t == 0) swbad = 0;
        __syncthreads();
        if (t < nc && !(weights[(long)k * n + t] >= 0.0)) swbad = 1;   // negative or NaN
        __syncthreads();
        bad = swbad;
    }
    if (bad || i >= nc) {
        if (U)
            for (int j = t; j < n; j += RW_THREADS) U[ki * n + j] = nan;
        if (t == 0) c[ki] = nan;
        return;
    }
    uint64_t key = 0;
    if (t < S) key = rkey[ki * S + t];
    hk[t] = key;
    hv[t] = key ? rval[ki * S + t] : 0.0;   // a value exists only under a key
    __syncthreads();
    const int words = rwords[ki];
    const int hlen = words > 1 ? words - 1 : 0;
    for (int j = 0; j < nc; ++j) {
        const long kj = (long)k * n + j;
        const double s = cd_pair_term(0.0, key, T, hk, hv, rnorm + ki * RW_N, hlen, rkey + kj * S, rval + kj * S, rnorm + kj * RW_N,
                                      rwords[kj], T, sigma, rk, rv, contrib);
        if (t < RW_N) sn[t] = s;
        __syncthreads();
        if (t == 0) {   // cd_hyp_k's closing formula with one reference
            double m = (((0.0 + sn[0]) + sn[1]) + sn[2]) + sn[3];
            m /= (double)RW_N;
            su[j] = m * 10.0;
        }
    }
    __syncthreads();
    if (U)
        for (int j = t; j < n; j += RW_THREADS) U[ki * n + j] = j < nc ? su[j] : nan;
    if (t == 0) c[ki] = cs_leave_one_out(su, weights ? weights + (long)k * n : nullptr, nc, i);
}

// One wave per image.  c != NULL: best[k] = the lowest i < n_cand[k] whose c[k][i] is the maximum (-1 when one of them is NaN:
// a bad image).  Then, for every array pair given, row best[k] of the image's n rows goes to row k of the output (zeros for -1).
__global__ __launch_bounds__(64) void cs_pick_k(const double* __restrict__ c, const int32_t* __restrict__ n_cand, int n,
                                                int64_t* __restrict__ best, int S, const int64_t* __restrict__ seq_in,
                                                int64_t* __restrict__ seq_out, const float* __restrict__ lp_in, float* __restrict__ lp_out,
                                                const float* __restrict__ p_in, float* __restrict__ p_out) {
    __shared__ long long sb;
    const int k = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) {
        long long b = -1;
        if (c) {
            const int nc = min(max(n_cand[k], 0), n);
            double m = 0.0;
            for (int i = 0; i < nc; ++i) {
                const double v = c[(long)k * n + i];
                if (v != v) {
                    b = -1;
                    break;
                }
                if (b < 0 || v > m) {
                    m = v;
                    b = i;
                }
            }
            best[k] = b;
        } else {
            b = best[k];
            if (b < 0 || b >= n) b = -1;
        }
        sb = b;
    }
    __syncthreads();
    const long long b = sb;
    const long src = ((long)k * n + (b < 0 ? 0 : b));
    if (seq_in)
        for (int s = lane; s < S; s += 64) seq_out[(long)k * S + s] = b < 0 ? 0 : seq_in[src * S + s];
    if (lp_in)
        for (int s = lane; s < S; s += 64) lp_out[(long)k * S + s] = b < 0 ? 0.0f : lp_in[src * S + s];
    if (p_in && lane == 0) p_out[k] = b < 0 ? 0.0f : p_in[src];
}

// ---- caption-set diversity (rfn.h "caption-set diversity") ---------------------------------------------------------------------
// Every kernel below reads what the consensus cooking left in the workspace: rkey / rcnt / rwords per (image, candidate), img_bad
// per image (which covers n_cand outside [1, n]) and cs_prep_k's candidate counts.
//
// Div-m.  One workgroup per image.  The image's n_cand * 4 * T first-occurrence keys are staged in dynamic LDS (the layout
// rw_refs_k<true> stages: 64 KiB at n = 32, T = 64, inside the 160 KiB of a CU); a key counts when no EARLIER candidate holds it in
// the same order's segment.  Staging and scanning was chosen over an LDS hash set: keys are already unique within a candidate, the
// scan needs no 64-bit LDS compare-and-swap and no probe bound, its result does not depend on insertion order, and rw_refs_k<true>
// has run the very same loop at the same limits since the corpus df exists.  Integer counting; one fp64 add and one division.
__global__ __launch_bounds__(RW_THREADS) void cs_div_k(const int32_t* __restrict__ n_cand, const int32_t* __restrict__ img_bad, int n,
                                                       int T, const uint64_t* __restrict__ rkey, const int32_t* __restrict__ rwords,
                                                       int32_t* __restrict__ distinct, int32_t* __restrict__ words,
                                                       double* __restrict__ div) {
    extern __shared__ uint64_t all[];
    __shared__ int cnt[RW_N];
    const int k = blockIdx.x, t = threadIdx.x, S = RW_N * T;
    if (img_bad[k]) {   // block-uniform
        if (t < RW_N) {
            if (distinct) distinct[(long)k * RW_N + t] = 0;
            if (div) div[(long)k * RW_N + t] = __builtin_nan("");
        }
        if (t == 0 && words) words[k] = 0;
        return;
    }
    const int nc = n_cand[k];
    if (t < RW_N) cnt[t] = 0;
    for (int x = t; x < nc * S; x += RW_THREADS) all[x] = rkey[(long)k * n * S + x];
    __syncthreads();
    int mine[RW_N] = {0, 0, 0, 0};
    for (int x = t; x < nc * S; x += RW_THREADS) {
        const uint64_t key = all[x];
        if (!key) continue;
        const int j = x / S, s = x - j * S, m = s / T;
        bool seen = false;
        for (int jj = 0; jj < j && !seen; ++jj)
            for (int q = 0; q < T; ++q)
                if (all[jj * S + m * T + q] == key) {
                    seen = true;
                    break;
                }
        if (!seen)
            for (int o = 0; o < RW_N; ++o) mine[o] += (o == m);
    }
    for (int o = 0; o < RW_N; ++o)
        if (mine[o]) atomicAdd(&cnt[o], mine[o]);
    __syncthreads();
    if (t < RW_N) {
        int w = 0;
        for (int j = 0; j < nc; ++j) w += rwords[(long)k * n + j];
        if (distinct) distinct[(long)k * RW_N + t] = cnt[t];
        if (div) div[(long)k * RW_N + t] = (double)cnt[t] / (1e-6 + (double)w);
        if (t == 0 && words) words[k] = w;
    }
}

// mBLEU.  One workgroup per (image k, candidate i), like cd_pair_k: BLEU-D of candidate i against the image's other valid
// candidates, by bd_hyp_k's rules (clip against the largest count in any one reference, the closest reference length, the shorter
// on a tie, bd_formula).  The hypothesis is the cooked keys and counts.  comps: the workspace copy (testlen = -1 marks a NaN row, a
// slot behind n_cand included); scores / ucomps: NULL or the caller's (n_img, n, 4) and (n_img, n, 10).
__global__ __launch_bounds__(RW_THREADS) void cs_loo_bleu_k(const int32_t* __restrict__ n_cand, const int32_t* __restrict__ img_bad,
                                                            int n, int T, const uint64_t* __restrict__ rkey,
                                                            const int32_t* __restrict__ rcnt, const int32_t* __restrict__ rwords,
                                                            double* __restrict__ scores, int32_t* __restrict__ comps,
                                                            int32_t* __restrict__ ucomps) {
    __shared__ uint64_t rk[RW_THREADS];
    __shared__ int rc[RW_THREADS], clip[RW_THREADS];
    __shared__ int correct[RW_N];
    const int k = blockIdx.x / n, i = blockIdx.x - k * n, t = threadIdx.x, S = RW_N * T;
    const long ki = (long)k * n + i;
    const int nc = img_bad[k] ? 0 : n_cand[k];   // block-uniform
    if (i >= nc || nc < 2) {                     // a bad image, a slot behind n_cand, or nothing to compare with
        if (scores && t < RW_N) scores[ki * RW_N + t] = __builtin_nan("");
        if (t < BD_COMPS) {
            comps[ki * BD_COMPS + t] = t == 0 ? -1 : 0;
            if (ucomps) ucomps[ki * BD_COMPS + t] = 0;
        }
        return;
    }
    uint64_t key = 0;
    int tf = 0;
    if (t < S) {
        key = rkey[ki * S + t];
        tf = rcnt[ki * S + t];
    }
    const int m = t / T;
    int maxc = 0;
    for (int j = 0; j < nc; ++j) {
        if (j == i) continue;
        const long kj = (long)k * n + j;
        maxc = max(maxc, rw_lookup(rkey + kj * S, rcnt + kj * S, T, key, m, rk, rc));
        __syncthreads();
    }
    clip[t] = key ? min(tf, maxc) : 0;
    __syncthreads();
    if (t < RW_N) {
        int s = 0;
        for (int p = 0; p < T; ++p) s += clip[t * T + p];
        correct[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        const int words = rwords[ki];
        int reflen = 0, best = 0;
        bool have = false;
        for (int j = 0; j < nc; ++j) {
            if (j == i) continue;
            const int l = rwords[(long)k * n + j], d = abs(l - words);
            if (!have || d < best || (d == best && l < reflen)) {
                best = d;
                reflen = l;
                have = true;
            }
        }
        int c[BD_COMPS];
        c[0] = words;
        c[1] = reflen;
        double cor[RW_N], gue[RW_N], bleu[RW_N];
        for (int o = 0; o < RW_N; ++o) {
            c[2 + o] = words - o > 0 ? words - o : 0;
            c[2 + RW_N + o] = correct[o];
            gue[o] = (double)c[2 + o];
            cor[o] = (double)correct[o];
        }
        bd_formula(cor, gue, (double)words, (double)reflen, bleu);
        for (int o = 0; o < BD_COMPS; ++o) {
            comps[ki * BD_COMPS + o] = c[o];
            if (ucomps) ucomps[ki * BD_COMPS + o] = c[o];
        }
        if (scores)
            for (int o = 0; o < RW_N; ++o) scores[ki * RW_N + o] = bleu[o];
    }
}

// One workgroup per candidate slot i, in bd_corpus_k's shape: bd_formula over the integer sums of slot i's components across the
// images whose row is not NaN; a slot no image scored is NaN.
__global__ __launch_bounds__(RW_THREADS) void cs_bleu_corpus_k(const int32_t* __restrict__ comps, int n_img, int n,
                                                               double* __restrict__ corpus) {
    __shared__ long long part[RW_THREADS];
    __shared__ long long tot[BD_COMPS + 1];
    const int i = blockIdx.x, t = threadIdx.x;
    for (int c = 0; c <= BD_COMPS; ++c) {   // c == BD_COMPS: the number of rows summed
        long long s = 0;
        for (int k = t; k < n_img; k += RW_THREADS) {
            const long o = ((long)k * n + i) * BD_COMPS;
            if (comps[o] >= 0) s += c < BD_COMPS ? comps[o + c] : 1;
        }
        part[t] = s;
        __syncthreads();
        for (int w = RW_THREADS / 2; w > 0; w >>= 1) {
            if (t < w) part[t] += part[t + w];
            __syncthreads();
        }
        if (t == 0) tot[c] = part[0];
        __syncthreads();
    }
    if (t == 0) {
        double cor[RW_N], gue[RW_N], bleu[RW_N];
        for (int o = 0; o < RW_N; ++o) {
            gue[o] = (double)tot[2 + o];
            cor[o] = (double)tot[2 + RW_N + o];
        }
        bd_formula(cor, gue, (double)tot[0], (double)tot[1], bleu);
        for (int o = 0; o < RW_N; ++o) corpus[(long)i * RW_N + o] = tot[BD_COMPS] > 0 ? bleu[o] : __builtin_nan("");
    }
}

// Self-CIDEr.  One wave per image; K = (U + U^T) / 2 / 10 over the valid candidates lives in LDS (8 KiB at n = 32).  fp64 cyclic
// Jacobi in one fixed order: sweeps over (p, q), p < q, row by row; a rotation is skipped when |K_pq| <= 2^-60 ||K||_F (the norm of
// the matrix before the first sweep); the loop ends after the first sweep that rotated nothing, or after CS_EIG_SWEEPS.  Lane r
// updates K_rp, K_rq and their mirror images, lane 0 the two diagonal entries; every lane computes the same c, s, t from the same
// LDS words.  Nothing depends on another image or on the grid, so an image's bits are its own.  Then lane 0 sorts the diagonal,
// drops what lies below 1e-12 lambda_max and forms -log(max sqrt / sum sqrt) / log(n_cand).
#define CS_EIG_SWEEPS 30
__global__ __launch_bounds__(64) void cs_eig_k(const int32_t* __restrict__ n_cand, const int32_t* __restrict__ img_bad, int n,
                                               const double* __restrict__ U, double* __restrict__ eig,
                                               double* __restrict__ self_cider) {
#pragma clang fp contract(off)
    __shared__ double K[RW_MAX_REFS * RW_MAX_REFS];
    __shared__ double lam[RW_MAX_REFS];
    const int k = blockIdx.x, lane = threadIdx.x;
    const double nan = __builtin_nan("");
    if (img_bad[k]) {   // block-uniform
        if (eig)
            for (int j = lane; j < n; j += 64) eig[(long)k * n + j] = nan;
        if (lane == 0 && self_cider) self_cider[k] = nan;
        return;
    }
    const int nc = n_cand[k];
    const double* u = U + (long)k * n * n;
    for (int x = lane; x < nc * nc; x += 64) {
        const int i = x / nc, j = x - i * nc;
        K[i * RW_MAX_REFS + j] = ((u[i * n + j] + u[j * n + i]) / 2.0) / 10.0;
    }
    __syncthreads();
    double f2 = 0.0;
    for (int i = 0; i < nc; ++i)
        for (int j = 0; j < nc; ++j) f2 = f2 + K[i * RW_MAX_REFS + j] * K[i * RW_MAX_REFS + j];
    const double thr = sqrt(f2) * 0x1p-60;
    for (int sweep = 0; sweep < CS_EIG_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < nc - 1; ++p)
            for (int q = p + 1; q < nc; ++q) {
                const double apq = K[p * RW_MAX_REFS + q];
                if (!(fabs(apq) > thr)) continue;   // wave-uniform: every lane read the same word
                ++rotated;
                const double app = K[p * RW_MAX_REFS + p], aqq = K[q * RW_MAX_REFS + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double tt = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                double arp = 0.0, arq = 0.0;
                const bool mine = lane < nc && lane != p && lane != q;
                if (mine) {
                    arp = K[lane * RW_MAX_REFS + p];
                    arq = K[lane * RW_MAX_REFS + q];
                }
                __syncthreads();   // every read of this rotation is done
                if (mine) {
                    const double np_ = c * arp - s * arq, nq_ = s * arp + c * arq;
                    K[lane * RW_MAX_REFS + p] = np_;
                    K[p * RW_MAX_REFS + lane] = np_;
                    K[lane * RW_MAX_REFS + q] = nq_;
                    K[q * RW_MAX_REFS + lane] = nq_;
                }
                if (lane == 0) {
                    K[p * RW_MAX_REFS + p] = app - tt * apq;
                    K[q * RW_MAX_REFS + q] = aqq + tt * apq;
                    K[p * RW_MAX_REFS + q] = 0.0;
                    K[q * RW_MAX_REFS + p] = 0.0;
                }
                __syncthreads();
            }
        if (!rotated) break;
    }
    if (lane == 0) {
        for (int i = 0; i < nc; ++i) {   // insertion sort, ascending
            const double v = K[i * RW_MAX_REFS + i];
            int j = i;
            while (j > 0 && lam[j - 1] > v) {
                lam[j] = lam[j - 1];
                --j;
            }
            lam[j] = v;
        }
        if (self_cider) {
            const double top = lam[nc - 1];
            double r = nan;
            if (nc > 1 && top > 0.0) {
                const double cut = 1e-12 * top;
                double sum = 0.0, big = 0.0;
                for (int i = 0; i < nc; ++i) {
                    if (lam[i] < cut) continue;
                    big = sqrt(lam[i]);
                    sum = sum + big;
                }
                r = -log(big / sum) / log((double)nc);
            }
            self_cider[k] = r;
        }
    }
    __syncthreads();
    if (eig)
        for (int j = lane; j < n; j += 64) eig[(long)k * n + j] = j < nc ? lam[j] : nan;
}

// ---- best-of-n, its lowest index and mean-of-n of a score column: one thread per image.  scores[(k * n + j) * stride], j <
// n_cand[k] (NULL: n); the sum runs ascending from 0.0 and is divided once.  One NaN among the valid entries, or a count outside
// [1, n], gives NaN, -1, NaN.
__global__ void rw_group_stats_k(const double* __restrict__ scores, long stride, int n_img, int n, const int32_t* __restrict__ n_cand,
                                 double* __restrict__ best, int64_t* __restrict__ arg, double* __restrict__ mean) {
#pragma clang fp contract(off)
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_img) return;
    const int nc = n_cand ? n_cand[k] : n;
    double m = __builtin_nan(""), sum = 0.0;
    long long b = -1;
    if (nc >= 1 && nc <= n)
        for (int j = 0; j < nc; ++j) {
            const double v = scores[(k * n + j) * stride];
            if (v != v) {
                b = -1;
                break;
            }
            sum = sum + v;
            if (b < 0 || v > m) {
                m = v;
                b = j;
            }
        }
    if (best) best[k] = b < 0 ? __builtin_nan("") : m;
    if (arg) arg[k] = b;
    if (mean) mean[k] = b < 0 ? __builtin_nan("") : sum / (double)nc;
}

// ---- host side --------------------------------------------------------------------------------------------
namespace {
const size_t kAlign = 256;
size_t up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

long corpus_slots(int n_img, int max_refs, int T_gt) {
    const long distinct = (long)n_img * max_refs * RW_N * T_gt;   // an upper bound of the distinct reference n-grams
    long s = 1024;
    while (s < 2 * distinct) s <<= 1;
    return s;
}

bool dims_ok(int n_rows, int T_res, int n_img, int max_refs, int T_gt) {
    return n_rows >= 1 && n_img >= 1 && T_res >= 1 && T_res <= RW_MAX_T && T_gt >= 1 && T_gt <= RW_MAX_T && max_refs >= 1 &&
           max_refs <= RW_MAX_REFS;
}

// The workspace of one call: the cooked references (what rw_refs_k writes), then what the scorer adds.
enum Scorer { CIDER_TABLE, CIDER_CORPUS, BLEU, ROUGE };
struct Layout {
    size_t rkey, rcnt, rwords, bad;      // shared
    size_t dkeys, dcnt, rval, rnorm;     // CIDEr-D (the df table in corpus mode only)
    size_t comps;                        // BLEU-D
    size_t total;
    long dslots;
};
Layout layout(Scorer scorer, int n_rows, int n_img, int max_refs, int T_gt) {
    Layout L{};
    const size_t nref = (size_t)n_img * max_refs;
    size_t o = 0;
    if (scorer == ROUGE) {   // one launch that cooks nothing and stores nothing between kernels: a token block
        L.total = kAlign;
        return L;
    }
    L.rkey = o;   o = up(o + nref * RW_N * T_gt * 8);
    L.rcnt = o;   o = up(o + nref * RW_N * T_gt * 4);
    L.rwords = o; o = up(o + nref * 4);
    L.bad = o;    o = up(o + (size_t)n_img * 4);
    if (scorer == BLEU) {
        L.comps = o; o = up(o + (size_t)n_rows * BD_COMPS * 4);
    } else {
        L.dslots = scorer == CIDER_CORPUS ? corpus_slots(n_img, max_refs, T_gt) : 0;
        L.dkeys = o; o = up(o + (size_t)L.dslots * 8);
        L.dcnt = o;  o = up(o + (size_t)L.dslots * 4);
        L.rval = o;  o = up(o + nref * RW_N * T_gt * 8);
        L.rnorm = o; o = up(o + nref * RW_N * 8);
    }
    L.total = o;
    return L;
}

// The checks the score calls share, in their precedence; fills *L when it returns RFN_OK.
// extra_shape_ok: the caller's own shape conditions.
int check_score_args(Scorer scorer, const void* res, int n_rows, int T_res, const void* row_img, const void* gts, const void* n_refs,
                     int n_img, int max_refs, int T_gt, int vocab, unsigned flags, bool extra_shape_ok, const void* scores,
                     const void* ws, size_t ws_bytes, Layout* L) {
    if (!dims_ok(n_rows, T_res, n_img, max_refs, T_gt) || vocab < 0 || vocab > RW_MAX_ID || !extra_shape_ok) return RFN_ERR_SHAPE;
    if (flags & ~RFN_CAPTION_END_EXCLUDED) return RFN_ERR_ARG;
    if (!res || !row_img || !gts || !n_refs || !scores || !ws || !rfn_aligned16(ws)) return RFN_ERR_ARG;
    *L = layout(scorer, n_rows, n_img, max_refs, T_gt);
    return ws_bytes < L->total ? RFN_ERR_WORKSPACE : RFN_OK;
}
}  // namespace

extern "C" size_t rfn_ciderd_ws_bytes(int n_rows, int T_res, int n_img, int max_refs, int T_gt, int corpus) {
    if (!dims_ok(n_rows, T_res, n_img, max_refs, T_gt)) return 0;
    return layout(corpus ? CIDER_CORPUS : CIDER_TABLE, n_rows, n_img, max_refs, T_gt).total;
}

extern "C" size_t rfn_bleud_ws_bytes(int n_rows, int T_res, int n_img, int max_refs, int T_gt) {
    if (!dims_ok(n_rows, T_res, n_img, max_refs, T_gt)) return 0;
    return layout(BLEU, n_rows, n_img, max_refs, T_gt).total;
}

extern "C" size_t rfn_ciderd_table_bytes(int64_t slots) {
    if (slots < 2 || (slots & (slots - 1))) return 0;
    return (size_t)slots * 16;
}

extern "C" int rfn_ciderd_table_build(const int32_t* ngram_ids, const double* counts, int64_t n_entries, int vocab, void* table,
                                      int64_t slots, void* stream) {
    if (n_entries < 0 || slots < 2 || (slots & (slots - 1)) || n_entries > slots / 2 || vocab < 0 || vocab > RW_MAX_ID)
        return RFN_ERR_SHAPE;
    if (!table || (n_entries > 0 && (!ngram_ids || !counts)) || !rfn_aligned16(table)) return RFN_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    uint64_t* keys = (uint64_t*)table;
    double* logdf = (double*)(keys + slots);
    cd_table_clear_k<<<(int)std::min<long>(rfn_cdiv(slots, 256), 4096), 256, 0, st>>>(keys, logdf, slots);
    RFN_CHECK_LAUNCH();
    if (n_entries > 0) {
        cd_table_insert_k<<<rfn_cdiv(n_entries, 256), 256, 0, st>>>(ngram_ids, counts, n_entries, vocab, keys, logdf, slots);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}

extern "C" int rfn_ciderd_score_ex(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                                   const int32_t* n_refs, int n_img, int max_refs, int T_gt, const void* table, int64_t slots,
                                   double ref_docs, int vocab, double sigma, unsigned flags, double* scores, void* ws,
                                   size_t ws_bytes, void* stream) {
    const int excl = (flags & RFN_CAPTION_END_EXCLUDED) != 0;
    const bool corpus = table == nullptr;
    const bool table_ok = corpus || (slots >= 2 && !(slots & (slots - 1)) && ref_docs > 0.0);
    Layout L;
    const int rc = check_score_args(corpus ? CIDER_CORPUS : CIDER_TABLE, res, n_rows, T_res, row_img, gts, n_refs, n_img, max_refs,
                                    T_gt, vocab, flags, table_ok, scores, ws, ws_bytes, &L);
    if (rc != RFN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    uint64_t* rkey = (uint64_t*)(w + L.rkey);
    int32_t* rcnt = (int32_t*)(w + L.rcnt);
    int32_t* rwords = (int32_t*)(w + L.rwords);
    int32_t* bad = (int32_t*)(w + L.bad);
    double* rval = (double*)(w + L.rval);
    double* rnorm = (double*)(w + L.rnorm);
    CdDf df;
    if (corpus) {
        uint64_t* dkeys = (uint64_t*)(w + L.dkeys);
        uint32_t* dcnt = (uint32_t*)(w + L.dcnt);
        df = CdDf{dkeys, dcnt, nullptr, L.dslots};
        ref_docs = (double)n_rows;   // compute_reward: ref_len = log(len(crefs)), one entry per score row
        cd_clear_k<<<(int)std::min<long>(rfn_cdiv(L.dslots, 256), 4096), 256, 0, st>>>(dkeys, dcnt, L.dslots);
        RFN_CHECK_LAUNCH();
        const size_t lds = (size_t)max_refs * RW_N * T_gt * 8;   // <= 64 KiB
        if (lds > 48 * 1024)
            hipFuncSetAttribute((const void*)rw_refs_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        rw_refs_k<true><<<n_img, RW_THREADS, lds, st>>>(gts, n_refs, max_refs, T_gt, vocab, excl, rkey, rcnt, rwords, bad, row_img,
                                                        n_rows, dkeys, dcnt, L.dslots);
    } else {
        df = CdDf{(const uint64_t*)table, nullptr, (const double*)((const uint64_t*)table + slots), slots};
        rw_refs_k<false><<<n_img, RW_THREADS, 0, st>>>(gts, n_refs, max_refs, T_gt, vocab, excl, rkey, rcnt, rwords, bad, nullptr, 0,
                                                       nullptr, nullptr, 0);
    }
    RFN_CHECK_LAUNCH();
    const long nvec = (long)n_img * max_refs * RW_N;
    cd_ref_vec_k<<<rfn_cdiv(nvec, 256), 256, 0, st>>>(n_refs, bad, n_img, max_refs, T_gt, rkey, rcnt, rval, rnorm, df, ref_docs,
                                                      nullptr);
    RFN_CHECK_LAUNCH();
    cd_hyp_k<<<n_rows, RW_THREADS, 0, st>>>(res, T_res, row_img, n_img, n_refs, bad, max_refs, T_gt, rkey, rval, rnorm, rwords, vocab,
                                            excl, df, ref_docs, sigma, scores);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_ciderd_score(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                                const int32_t* n_refs, int n_img, int max_refs, int T_gt, const void* table, int64_t slots,
                                double ref_docs, int vocab, double sigma, double* scores, void* ws, size_t ws_bytes,
                                void* stream) {
    return rfn_ciderd_score_ex(res, n_rows, T_res, row_img, gts, n_refs, n_img, max_refs, T_gt, table, slots, ref_docs, vocab, sigma,
                               0u, scores, ws, ws_bytes, stream);
}

extern "C" int rfn_bleud_score_ex(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                                  const int32_t* n_refs, int n_img, int max_refs, int T_gt, int vocab, unsigned flags, double* scores,
                                  int32_t* comps, double* corpus, void* ws, size_t ws_bytes, void* stream) {
    const int excl = (flags & RFN_CAPTION_END_EXCLUDED) != 0;
    Layout L;
    const int rc = check_score_args(BLEU, res, n_rows, T_res, row_img, gts, n_refs, n_img, max_refs, T_gt, vocab, flags, true, scores,
                                    ws, ws_bytes, &L);
    if (rc != RFN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    uint64_t* rkey = (uint64_t*)(w + L.rkey);
    int32_t* rcnt = (int32_t*)(w + L.rcnt);
    int32_t* rwords = (int32_t*)(w + L.rwords);
    int32_t* bad = (int32_t*)(w + L.bad);
    int32_t* wcomps = (int32_t*)(w + L.comps);
    rw_refs_k<false><<<n_img, RW_THREADS, 0, st>>>(gts, n_refs, max_refs, T_gt, vocab, excl, rkey, rcnt, rwords, bad, nullptr, 0,
                                                   nullptr, nullptr, 0);
    RFN_CHECK_LAUNCH();
    bd_hyp_k<<<n_rows, RW_THREADS, 0, st>>>(res, T_res, row_img, n_img, n_refs, bad, max_refs, T_gt, rkey, rcnt, rwords, vocab, excl,
                                            scores, wcomps, comps);
    RFN_CHECK_LAUNCH();
    if (corpus) {
        bd_corpus_k<<<1, RW_THREADS, 0, st>>>(wcomps, n_rows, corpus);
        RFN_CHECK_LAUNCH();
    }
    return RFN_OK;
}

extern "C" int rfn_bleud_score(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                               const int32_t* n_refs, int n_img, int max_refs, int T_gt, int vocab, double* scores, int32_t* comps,
                               double* corpus, void* ws, size_t ws_bytes, void* stream) {
    return rfn_bleud_score_ex(res, n_rows, T_res, row_img, gts, n_refs, n_img, max_refs, T_gt, vocab, 0u, scores, comps, corpus, ws,
                              ws_bytes, stream);
}

extern "C" size_t rfn_rougel_ws_bytes(int n_rows, int T_res, int n_img, int max_refs, int T_gt) {
    if (!dims_ok(n_rows, T_res, n_img, max_refs, T_gt)) return 0;
    return layout(ROUGE, n_rows, n_img, max_refs, T_gt).total;
}

extern "C" int rfn_rougel_score(const int64_t* res, int n_rows, int T_res, const int32_t* row_img, const int64_t* gts,
                                const int32_t* n_refs, int n_img, int max_refs, int T_gt, int vocab, unsigned flags, double beta,
                                double* scores, int32_t* lcs, void* ws, size_t ws_bytes, void* stream) {
    Layout L;
    const int rc = check_score_args(ROUGE, res, n_rows, T_res, row_img, gts, n_refs, n_img, max_refs, T_gt, vocab, flags,
                                    beta > 0.0, scores, ws, ws_bytes, &L);
    if (rc != RFN_OK) return rc;
    rl_score_k<<<n_rows, RW_THREADS, 0, (hipStream_t)stream>>>(res, T_res, row_img, n_img, gts, n_refs, max_refs, T_gt, vocab,
                                                               (flags & RFN_CAPTION_END_EXCLUDED) != 0, beta, scores, lcs);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_score_mean(const double* scores, int64_t n, int64_t stride, double* mean, int64_t* n_skipped, void* stream) {
    if (n < 1 || stride < 1) return RFN_ERR_SHAPE;
    if (!scores || !mean) return RFN_ERR_ARG;
    rw_mean_k<<<1, RW_THREADS, 0, (hipStream_t)stream>>>(scores, (long)n, (long)stride, mean, n_skipped);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_scst_reward_mix(const double* cider, double cider_weight, const double* bleu, double bleu4_weight, int B, int T,
                                   int use_baseline, float* out, double* out64, void* stream) {
    if (B < 1 || T < 1) return RFN_ERR_SHAPE;
    if ((!cider && !bleu) || (!out && !out64)) return RFN_ERR_ARG;
    const long n = (long)B * T;
    rw_reward_k<<<rfn_cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(cider, cider_weight, bleu, bleu4_weight, B, T, use_baseline, out,
                                                                   out64);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_scst_reward_group(const double* cider, double cider_weight, const double* bleu, double bleu4_weight, int B, int n,
                                     int T, int baseline, float* out, double* out64, void* stream) {
    if (B < 1 || T < 1 || n < 1 || B % n || (baseline != 0 && baseline != 1) || (baseline == 1 && n == 1)) return RFN_ERR_SHAPE;
    if ((!cider && !bleu) || (!out && !out64)) return RFN_ERR_ARG;
    const long cnt = (long)B * T;
    rw_reward_group_k<<<rfn_cdiv(cnt, 256), 256, 0, (hipStream_t)stream>>>(cider, cider_weight, bleu, bleu4_weight, B, n, T, baseline,
                                                                          out, out64);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_scst_reward_distinct(const double* cider, double cider_weight, const double* bleu, double bleu4_weight,
                                        const double* weight, int B, int n, int T, int baseline, float* out, double* out64,
                                        void* stream) {
    if (B < 1 || T < 1 || n < 1 || B % n || (baseline != 0 && baseline != 1) || (baseline == 1 && n < 3)) return RFN_ERR_SHAPE;
    if ((!cider && !bleu) || !weight || (!out && !out64)) return RFN_ERR_ARG;
    const long cnt = (long)B * T;
    rw_reward_distinct_k<<<rfn_cdiv(cnt, 256), 256, 0, (hipStream_t)stream>>>(cider, cider_weight, bleu, bleu4_weight, weight, B, n, T,
                                                                             baseline, out, out64);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- consensus reranking -----------------------------------------------------------------------------------------------------
namespace {
// The candidates cooked as references (the scorer's layout with one score row per candidate), then cs_prep_k's three outputs.
struct ConsensusLayout {
    Layout L;
    size_t ncand, row_img, ref_docs, total;
};
ConsensusLayout consensus_layout(int n_img, int n, int T, bool corpus) {
    ConsensusLayout C{};
    C.L = layout(corpus ? CIDER_CORPUS : CIDER_TABLE, n_img * n, n_img, n, T);
    size_t o = C.L.total;
    C.ncand = o;    o = up(o + (size_t)n_img * 4);
    C.row_img = o;  o = up(o + (size_t)n_img * n * 4);
    C.ref_docs = o; o = up(o + 8);
    C.total = o;
    return C;
}
bool consensus_dims_ok(int n_img, int n, int T) {
    return n_img >= 1 && n >= 1 && n <= RW_MAX_REFS && T >= 1 && T <= RW_MAX_T && (long)n_img * n <= 0x7fffffffL;
}
// The workspace of a consensus-shaped call as pointers, and the launches that fill it: cs_prep_k, then the candidates cooked as
// their image's references ([clear], refs, and -- want_vec -- the tf-idf vectors).  Without want_vec nothing reads a df, so the
// plain rw_refs_k runs in both df modes.
struct Cooked {
    uint64_t* rkey;
    int32_t *rcnt, *rwords, *bad, *nc, *row_img;
    double *rval, *rnorm, *docs;
};
Cooked cooked_of(const ConsensusLayout& CL, void* ws) {
    char* w = (char*)ws;
    const Layout& L = CL.L;
    return Cooked{(uint64_t*)(w + L.rkey), (int32_t*)(w + L.rcnt),     (int32_t*)(w + L.rwords),
                  (int32_t*)(w + L.bad),   (int32_t*)(w + CL.ncand),   (int32_t*)(w + CL.row_img),
                  (double*)(w + L.rval),   (double*)(w + L.rnorm),     (double*)(w + CL.ref_docs)};
}
int consensus_cook(const int64_t* cands, int n_img, int n, int T, const int32_t* n_cand, const void* table, int64_t slots,
                   double ref_docs, int vocab, int excl, bool want_vec, const ConsensusLayout& CL, const Cooked& K, hipStream_t st) {
    const Layout& L = CL.L;
    const bool corpus = table == nullptr;
    char* w = (char*)K.rkey - L.rkey;
    cs_prep_k<<<1, RW_THREADS, 0, st>>>(n_cand, n_img, n, K.nc, K.row_img, K.docs);
    RFN_CHECK_LAUNCH();
    CdDf df;
    if (corpus && want_vec) {
        uint64_t* dkeys = (uint64_t*)(w + L.dkeys);
        uint32_t* dcnt = (uint32_t*)(w + L.dcnt);
        df = CdDf{dkeys, dcnt, nullptr, L.dslots};
        cd_clear_k<<<(int)std::min<long>(rfn_cdiv(L.dslots, 256), 4096), 256, 0, st>>>(dkeys, dcnt, L.dslots);
        RFN_CHECK_LAUNCH();
        const size_t lds = (size_t)n * RW_N * T * 8;   // <= 64 KiB
        if (lds > 48 * 1024)
            hipFuncSetAttribute((const void*)rw_refs_k<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        rw_refs_k<true><<<n_img, RW_THREADS, lds, st>>>(cands, K.nc, n, T, vocab, excl, K.rkey, K.rcnt, K.rwords, K.bad, K.row_img,
                                                        n_img * n, dkeys, dcnt, L.dslots);
    } else {
        df = CdDf{(const uint64_t*)table, nullptr, corpus ? nullptr : (const double*)((const uint64_t*)table + slots), slots};
        rw_refs_k<false><<<n_img, RW_THREADS, 0, st>>>(cands, K.nc, n, T, vocab, excl, K.rkey, K.rcnt, K.rwords, K.bad, nullptr, 0,
                                                       nullptr, nullptr, 0);
    }
    RFN_CHECK_LAUNCH();
    if (!want_vec) return RFN_OK;
    const long nvec = (long)n_img * n * RW_N;
    cd_ref_vec_k<<<rfn_cdiv(nvec, 256), 256, 0, st>>>(K.nc, K.bad, n_img, n, T, K.rkey, K.rcnt, K.rval, K.rnorm, df, ref_docs,
                                                      corpus ? K.docs : nullptr);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}
}  // namespace

extern "C" size_t rfn_consensus_ws_bytes(int n_img, int n, int T, int corpus) {
    if (!consensus_dims_ok(n_img, n, T)) return 0;
    return consensus_layout(n_img, n, T, corpus != 0).total;
}

extern "C" int rfn_consensus_ciderd(const int64_t* cands, int n_img, int n, int T, const int32_t* n_cand, const double* weights,
                                    const void* table, int64_t slots, double ref_docs, int vocab, double sigma, unsigned flags,
                                    double* U, double* c, int64_t* best, void* ws, size_t ws_bytes, void* stream) {
    const int excl = (flags & RFN_CAPTION_END_EXCLUDED) != 0;
    const bool corpus = table == nullptr;
    const bool table_ok = corpus || (slots >= 2 && !(slots & (slots - 1)) && ref_docs > 0.0);
    if (!consensus_dims_ok(n_img, n, T) || vocab < 0 || vocab > RW_MAX_ID || !table_ok) return RFN_ERR_SHAPE;
    if (flags & ~RFN_CAPTION_END_EXCLUDED) return RFN_ERR_ARG;
    if (!cands || !c || !best || !ws || !rfn_aligned16(ws)) return RFN_ERR_ARG;
    const ConsensusLayout CL = consensus_layout(n_img, n, T, corpus);
    if (ws_bytes < CL.total) return RFN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Cooked K = cooked_of(CL, ws);
    const int rc = consensus_cook(cands, n_img, n, T, n_cand, table, slots, ref_docs, vocab, excl, true, CL, K, st);
    if (rc != RFN_OK) return rc;
    const int32_t *nc = K.nc, *bad = K.bad, *rwords = K.rwords;
    const uint64_t* rkey = K.rkey;
    const double *rval = K.rval, *rnorm = K.rnorm;
    cd_pair_k<<<n_img * n, RW_THREADS, 0, st>>>(nc, bad, n, T, rkey, rval, rnorm, rwords, weights, sigma, U, c);
    RFN_CHECK_LAUNCH();
    cs_pick_k<<<n_img, 64, 0, st>>>(c, nc, n, best, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_consensus_gather(const int64_t* best, int n_img, int n, int S, const int64_t* seq_in, int64_t* seq_out,
                                    const float* lp_in, float* lp_out, const float* p_in, float* p_out, void* stream) {
    if (n_img < 1 || n < 1 || S < 1) return RFN_ERR_SHAPE;
    if (!best || (!seq_in && !lp_in && !p_in) || !seq_in != !seq_out || !lp_in != !lp_out || !p_in != !p_out) return RFN_ERR_ARG;
    cs_pick_k<<<n_img, 64, 0, (hipStream_t)stream>>>(nullptr, nullptr, n, const_cast<int64_t*>(best), S, seq_in, seq_out, lp_in,
                                                     lp_out, p_in, p_out);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

// ---- caption-set diversity ------------------------------------------------------------------------------------------------------
namespace {
// The consensus workspace, then U and cd_pair_k's scores (read by the eigen kernel when the caller keeps neither) and the BLEU
// components of every (image, slot).
struct CapsetLayout {
    ConsensusLayout C;
    size_t U, c, comps, total;
};
CapsetLayout capset_layout(int n_img, int n, int T, bool corpus) {
    CapsetLayout P{};
    P.C = consensus_layout(n_img, n, T, corpus);
    size_t o = P.C.total;
    const size_t rows = (size_t)n_img * n;
    P.U = o;     o = up(o + rows * n * 8);
    P.c = o;     o = up(o + rows * 8);
    P.comps = o; o = up(o + rows * BD_COMPS * 4);
    P.total = o;
    return P;
}
}  // namespace

extern "C" size_t rfn_capset_ws_bytes(int n_img, int n, int T, int corpus) {
    if (!consensus_dims_ok(n_img, n, T)) return 0;
    return capset_layout(n_img, n, T, corpus != 0).total;
}

extern "C" int rfn_capset_diversity(const int64_t* cands, int n_img, int n, int T, const int32_t* n_cand, const void* table,
                                    int64_t slots, double ref_docs, int vocab, double sigma, unsigned flags, int32_t* distinct,
                                    int32_t* words, double* div, double* mbleu, int32_t* mbleu_comps, double* mbleu_corpus, double* U,
                                    double* eig, double* self_cider, void* ws, size_t ws_bytes, void* stream) {
    const int excl = (flags & RFN_CAPTION_END_EXCLUDED) != 0;
    const bool corpus = table == nullptr;
    const bool table_ok = corpus || (slots >= 2 && !(slots & (slots - 1)) && ref_docs > 0.0);
    if (!consensus_dims_ok(n_img, n, T) || vocab < 0 || vocab > RW_MAX_ID || !table_ok) return RFN_ERR_SHAPE;
    if (flags & ~RFN_CAPTION_END_EXCLUDED) return RFN_ERR_ARG;
    if (!cands || !ws || !rfn_aligned16(ws)) return RFN_ERR_ARG;
    const CapsetLayout P = capset_layout(n_img, n, T, corpus);
    if (ws_bytes < P.total) return RFN_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const bool want_div = distinct || words || div, want_bleu = mbleu || mbleu_comps || mbleu_corpus;
    const bool want_eig = eig || self_cider, want_u = U || want_eig;
    if (!want_div && !want_bleu && !want_u) return RFN_OK;
    const Cooked K = cooked_of(P.C, ws);
    const int rc = consensus_cook(cands, n_img, n, T, n_cand, table, slots, ref_docs, vocab, excl, want_u, P.C, K, st);
    if (rc != RFN_OK) return rc;
    char* w = (char*)ws;
    if (want_div) {
        const size_t lds = (size_t)n * RW_N * T * 8;   // <= 64 KiB
        if (lds > 48 * 1024) hipFuncSetAttribute((const void*)cs_div_k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        cs_div_k<<<n_img, RW_THREADS, lds, st>>>(K.nc, K.bad, n, T, K.rkey, K.rwords, distinct, words, div);
        RFN_CHECK_LAUNCH();
    }
    if (want_bleu) {
        int32_t* comps = (int32_t*)(w + P.comps);
        cs_loo_bleu_k<<<n_img * n, RW_THREADS, 0, st>>>(K.nc, K.bad, n, T, K.rkey, K.rcnt, K.rwords, mbleu, comps, mbleu_comps);
        RFN_CHECK_LAUNCH();
        if (mbleu_corpus) {
            cs_bleu_corpus_k<<<n, RW_THREADS, 0, st>>>(comps, n_img, n, mbleu_corpus);
            RFN_CHECK_LAUNCH();
        }
    }
    if (want_u) {
        double* u = U ? U : (double*)(w + P.U);
        cd_pair_k<<<n_img * n, RW_THREADS, 0, st>>>(K.nc, K.bad, n, T, K.rkey, K.rval, K.rnorm, K.rwords, nullptr, sigma, u,
                                                    (double*)(w + P.c));
        RFN_CHECK_LAUNCH();
        if (want_eig) {
            cs_eig_k<<<n_img, 64, 0, st>>>(K.nc, K.bad, n, u, eig, self_cider);
            RFN_CHECK_LAUNCH();
        }
    }
    return RFN_OK;
}

extern "C" int rfn_score_group_stats(const double* scores, int64_t stride, int n_img, int n, const int32_t* n_cand, double* best,
                                     int64_t* arg, double* mean, void* stream) {
    if (n_img < 1 || n < 1 || stride < 1) return RFN_ERR_SHAPE;
    if (!scores || (!best && !arg && !mean)) return RFN_ERR_ARG;
    rw_group_stats_k<<<rfn_cdiv(n_img, 256), 256, 0, (hipStream_t)stream>>>(scores, (long)stride, n_img, n, n_cand, best, arg, mean);
    RFN_CHECK_LAUNCH();
    return RFN_OK;
}

extern "C" int rfn_scst_reward(const double* scores, int B, int T, double weight, int use_baseline, float* out, double* out64,
                               void* stream) {
    return rfn_scst_reward_mix(scores, weight, nullptr, 0.0, B, T, use_baseline, out, out64, stream);
}
