// jf_logprobs.hip — per-token log-probabilities (jf_logprobs_rows): for every row the log-probability and rank of a chosen id
// and the row's top N ids with their log-probabilities.  The definition is in include/jacobiforcing.h: logprob(id) =
// (xs[id] - max xs) - ln sum exp(xs - max xs), the log of the UNROUNDED softmax of the scaled row at the request's temperature
// (top_k / top_p are not applied); order = descending xs, equal xs by ascending id.
//
// Two launches whatever R is, no atomics, no workgroup waits for another:
//   lp_partial_kernel   one workgroup per (row, chunk of LP_TPB * LP_NV vectors).  The chunk is loaded ONCE into registers (16-byte
//                       loads; an element-wise path for rows that are not 16-byte aligned and for the ragged end of a row),
//                       then walked twice there: the raw maximum first (the scaling is monotone, so the largest scaled value
//                       belongs to the largest raw one), then sum exp(xs - chunk max), the count of ids in front of the chosen id
//                       and — TOPN only — the chunk's first top_n ids of the order.
//   lp_finish_kernel    one workgroup per row: chunk maxima and sums merged in float64, the counts added into the rank, the
//                       chunks' candidates merged into the row's top N, the outputs written.
// An id's order key is one 64-bit word, packed the way jf_argmax_dev.h packs its keys: the monotone image of the xs bits
// (order_key: -0.0 == +0.0) in the high word, the complemented id in the low word — "in front of" is one 64-bit compare, and
// every valid id's key is non-zero (0 marks an empty slot).
//
// Top N of a chunk without N reductions over the chunk: every thread keeps the largest key of its own elements; the top_n-th
// largest of those 256 maxima (one wavefront, top_n shuffle rounds) is a threshold at least top_n elements reach and that only
// elements of top_n threads can reach, so at most top_n * 64 elements pass it (typically top_n plus a few).  Those are pushed
// into an LDS list by ballot compaction (every wavefront into a region of its own, sized by the number of its threads that hold
// a passing element), and ranked there by counting.
#include "jf_common.h"

constexpr int LP_TPB = 256;                        // threads of a workgroup (both kernels)
constexpr int LP_NV = 8;                           // 16-byte vectors per thread: a chunk is 8 192 float32 / 16 384 bf16 elements
constexpr int LP_LIST = 64 * JF_LOGPROBS_MAX_TOP;  // candidates a chunk can push (64 >= LP_NV * EPV elements of each of <= top_n threads)
constexpr float LP_LOG2E = 1.44269504088896340736f;
template <int DT> struct LpChunk { static constexpr int ELEMS = LP_TPB * LP_NV * Elem<DT>::EPV; };
static_assert(LP_NV * Elem<JF_BF16>::EPV <= 64 && LP_NV * Elem<JF_F32>::EPV <= 64, "a thread's elements fit its share of the list");

struct LpPart { float m, s; int32_t cnt, rsv; };   // per (row, chunk): max xs (NaN: the row is invalid), sum exp(xs - m), ids in front

__device__ __forceinline__ float lp_bf16_rne(float x) {        // nearest bfloat16 (ties to even), as a float
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return x;
    u = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
    return __uint_as_float(u);
}
// The scaled logit.  SCALE 0: T == 1.  1: the true division (float32; bf16: rounded once more to bf16).  2 (bf16 only): the host
// has checked that bf16(x * fl(1/T)) equals bf16(fl32(x / T)) for every bf16 mantissa (lp_scale_is_exact: the same test, and the
// same product form, as the jf_rs_* kernels use for their rows).
template <int DT, int SCALE>
__device__ __forceinline__ float lp_scale(float x, float t, float inv_t) {
    if constexpr (SCALE == 0) return x;
    else if constexpr (DT == JF_F32) return __fdiv_rn(x, t);
    else if constexpr (SCALE == 2) return lp_bf16_rne(x * inv_t);
    else return lp_bf16_rne(__fdiv_rn(x, t));
}
__device__ __forceinline__ float lp_key_to_float(uint32_t k) {   // inverse of order_key for non-NaN payloads
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ bool lp_bad_max(float m) {            // NaN or +inf: the row has no log-probabilities
    return order_key(__float_as_uint(m)) >= 0xFF800000u;
}

// the EPV raw values starting at element e0 (a multiple of EPV) as one 16-byte vector; slots at or beyond `end` hold -inf
template <int DT, bool VEC>
__device__ __forceinline__ u32x4 lp_load(const typename Elem<DT>::T *p, int64_t e0, int64_t end) {
    constexpr int EPV = Elem<DT>::EPV;
    if (VEC && e0 + EPV <= end) return __builtin_nontemporal_load((const u32x4 *)(p + e0));
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (DT == JF_F32) {
            w[j] = (e0 + j < end) ? p[e0 + j] : 0xFF800000u;
        } else {
            const uint32_t a = (e0 + 2 * j < end) ? p[e0 + 2 * j] : 0xFF80u;
            const uint32_t b = (e0 + 2 * j + 1 < end) ? p[e0 + 2 * j + 1] : 0xFF80u;
            w[j] = a | (b << 16);
        }
    }
    const u32x4 v = {w[0], w[1], w[2], w[3]};
    return v;
}
template <int DT>
__device__ __forceinline__ void lp_unpack(const u32x4 v, uint32_t (&b)[Elem<DT>::EPV]) {   // float32 bit patterns of the elements
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (DT == JF_F32) b[j] = w[j];
        else { b[2 * j] = w[j] << 16; b[2 * j + 1] = w[j] & 0xFFFF0000u; }
    }
}
__device__ __forceinline__ float lp_wave_sum_f32(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct LpShared {                                   // TOPN only
    uint64_t tmax[LP_TPB];                          // every thread's largest key
    uint64_t list[LP_LIST];                         // the elements that reach the threshold, wavefront by wavefront
    uint64_t t0;
    int nthr[LP_TPB / 64], ncand[LP_TPB / 64];
};

template <int DT, bool VEC, int SCALE, bool TOPN>
__global__ __launch_bounds__(LP_TPB) void lp_partial_kernel(const void *logits, int64_t V, int64_t row_stride, float t, float inv_t,
                                                            const int64_t *__restrict__ chosen, int cpr, int top_n,
                                                            LpPart *__restrict__ part, unsigned long long *__restrict__ cand) {
    using E = Elem<DT>;
    constexpr int EPV = E::EPV, NW = LP_TPB / 64;
    const int64_t item = blockIdx.x;
    const int64_t row = item / cpr;
    const int c = (int)(item - row * cpr);
    const int64_t begin = (int64_t)c * LpChunk<DT>::ELEMS;
    int64_t end = begin + LpChunk<DT>::ELEMS;
    if (end > V) end = V;
    const typename E::T *p = (const typename E::T *)logits + row * row_stride;
    const int tid = threadIdx.x, wv = tid >> 6;

    u32x4 v[LP_NV];
#pragma unroll
    for (int u = 0; u < LP_NV; ++u) v[u] = lp_load<DT, VEC>(p, begin + (int64_t)(u * LP_TPB + tid) * EPV, end);
    // the chosen id's key: one load per workgroup.  An id outside [0, V) is never dereferenced and has nothing in front of it.
    const int64_t cid = chosen[row];
    uint32_t ck = 0xFFFFFFFFu, cidx = 0u;
    if (cid >= 0 && cid < V) {
        ck = order_key(__float_as_uint(lp_scale<DT, SCALE>(load_f<DT>(p, cid), t, inv_t)));
        cidx = (uint32_t)cid;
    }

    // ---- walk 1: the chunk's raw maximum
    uint32_t mk = 0u;
#pragma unroll
    for (int u = 0; u < LP_NV; ++u) {
        uint32_t b[EPV];
        lp_unpack<DT>(v[u], b);
#pragma unroll
        for (int j = 0; j < EPV; ++j) { const uint32_t k = order_key(b[j]); mk = k > mk ? k : mk; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(mk, off, 64); mk = o > mk ? o : mk; }
    __shared__ uint32_t s_mk[NW];
    __shared__ float s_sum[NW];
    __shared__ int s_cnt[NW];
    if ((tid & 63) == 0) s_mk[wv] = mk;
    __syncthreads();
    mk = s_mk[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) mk = s_mk[w] > mk ? s_mk[w] : mk;
    const float m = mk == 0xFFFFFFFFu ? __uint_as_float(0x7FC00000u) : lp_scale<DT, SCALE>(lp_key_to_float(mk), t, inv_t);
    if (lp_bad_max(m)) {                             // NaN or +inf in the chunk (workgroup-uniform): the finish kernel reads nothing else
        if (tid == 0) part[item] = LpPart{__uint_as_float(0x7FC00000u), 0.f, 0, 0};
        return;
    }
    const float mm = m == -INFINITY ? 0.f : m;       // an all -inf chunk: every term is exp(-inf) = 0

    // ---- walk 2: sum exp(xs - m), ids in front of the chosen one, every thread's largest key
    float s = 0.f;
    int cnt = 0;
    uint64_t best = 0ull;
#pragma unroll
    for (int u = 0; u < LP_NV; ++u) {
        uint32_t b[EPV];
        lp_unpack<DT>(v[u], b);
        const uint32_t id0 = (uint32_t)begin + (uint32_t)(u * LP_TPB + tid) * EPV;      // V < 2^31: ids and the padding behind them fit
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
            const float xs = lp_scale<DT, SCALE>(__uint_as_float(b[j]), t, inv_t);
            s += __builtin_amdgcn_exp2f((xs - mm) * LP_LOG2E);
            const uint32_t k = order_key(__float_as_uint(xs)), id = id0 + j;
            const bool valid = id < (uint32_t)end;
            cnt += (valid && (k > ck || (k == ck && id < cidx))) ? 1 : 0;
            if constexpr (TOPN) {
                const uint64_t k64 = valid ? (((uint64_t)k << 32) | (uint64_t)(~id)) : 0ull;
                best = k64 > best ? k64 : best;
            }
        }
    }
    s = lp_wave_sum_f32(s);
    cnt = wave_sum_i32(cnt);
    if ((tid & 63) == 0) { s_sum[wv] = s; s_cnt[wv] = cnt; }
    __syncthreads();
    if (tid == 0) {
        float ss = 0.f;
        int cc = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { ss += s_sum[w]; cc += s_cnt[w]; }
        part[item] = LpPart{m, ss, cc, 0};
    }

    if constexpr (TOPN) {
        __shared__ LpShared sh;
        sh.tmax[tid] = best;
        __syncthreads();
        if (tid < 64) {                              // the top_n-th largest of the 256 maxima (0: fewer than top_n threads hold an element)
            const uint64_t a[4] = {sh.tmax[tid], sh.tmax[tid + 64], sh.tmax[tid + 128], sh.tmax[tid + 192]};
            uint64_t bound = ~0ull, cur = 0ull;
            for (int r = 0; r < top_n; ++r) {
                uint64_t m4 = 0ull;
#pragma unroll
                for (int q = 0; q < 4; ++q) m4 = (a[q] < bound && a[q] > m4) ? a[q] : m4;
                cur = wave_max_u64(m4);
                if (cur == 0ull) break;
                bound = cur;
            }
            if (tid == 0) sh.t0 = cur;
        }
        __syncthreads();
        const uint64_t t0 = sh.t0;
        const bool mine = best != 0ull && best >= t0;                    // this thread holds at least one element of the list
        const unsigned long long holders = __ballot(mine);
        if ((tid & 63) == 0) sh.nthr[wv] = __popcll(holders);
        __syncthreads();
        int off = 0;                                                     // this wavefront's region: 64 slots per holder in front of it
        for (int w = 0; w < wv; ++w) off += sh.nthr[w] * 64;
        const int base = off;
        if (holders != 0ull) {
#pragma unroll
            for (int u = 0; u < LP_NV; ++u) {
                uint32_t b[EPV];
                lp_unpack<DT>(v[u], b);
                const uint32_t id0 = (uint32_t)begin + (uint32_t)(u * LP_TPB + tid) * EPV;
#pragma unroll
                for (int j = 0; j < EPV; ++j) {
                    const uint32_t k = order_key(__float_as_uint(lp_scale<DT, SCALE>(__uint_as_float(b[j]), t, inv_t))), id = id0 + j;
                    const uint64_t k64 = ((uint64_t)k << 32) | (uint64_t)(~id);
                    const bool pass = mine && id < (uint32_t)end && k64 >= t0;
                    const unsigned long long bal = __ballot(pass);
                    if (bal != 0ull) {
                        const int pos = off + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
                        if (pass && pos < LP_LIST) sh.list[pos] = k64;
                        off += __popcll(bal);
                    }
                }
            }
        }
        if ((tid & 63) == 0) sh.ncand[wv] = off - base;
        __syncthreads();
        // rank the candidates by counting (their keys are distinct); the first top_n of them are the chunk's
        int wbase[NW], wn[NW], total = 0;
        {
            int b0 = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) { wbase[w] = b0; wn[w] = sh.ncand[w]; b0 += sh.nthr[w] * 64; total += wn[w]; }
        }
        unsigned long long *out = cand + item * (int64_t)top_n;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            for (int i = tid; i < wn[w]; i += LP_TPB) {
                const uint64_t key = sh.list[wbase[w] + i];
                int r = 0;
#pragma unroll
                for (int w2 = 0; w2 < NW; ++w2)
                    for (int i2 = 0; i2 < wn[w2]; ++i2) r += sh.list[wbase[w2] + i2] > key ? 1 : 0;
                if (r < top_n) out[r] = key;
            }
        }
        if (tid < top_n && tid >= total) out[tid] = 0ull;                // fewer elements than top_n: empty slots
    }
}

template <int DT, int SCALE>
__global__ __launch_bounds__(LP_TPB) void lp_finish_kernel(const void *logits, int64_t V, int64_t row_stride, float t, float inv_t,
                                                           const int64_t *__restrict__ chosen, int cpr, int top_n,
                                                           const LpPart *__restrict__ part, const unsigned long long *__restrict__ cand,
                                                           float *__restrict__ logprob, int32_t *__restrict__ rank,
                                                           int64_t *__restrict__ top_ids, float *__restrict__ top_logprobs) {
    using E = Elem<DT>;
    constexpr int NW = LP_TPB / 64;
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x, wv = tid >> 6;
    const typename E::T *p = (const typename E::T *)logits + row * row_stride;
    const LpPart *pr = part + row * cpr;
    __shared__ float s_m[NW];
    __shared__ int s_bad[NW], s_cnt[NW];
    __shared__ double s_s[NW];
    __shared__ uint64_t s_key[NW], s_top[JF_LOGPROBS_MAX_TOP];

    // the row's maximum; a NaN chunk maximum marks the row
    float m = -INFINITY;
    int bad = 0;
    for (int c = tid; c < cpr; c += LP_TPB) {
        const float mc = pr[c].m;
        bad |= (mc != mc) ? 1 : 0;
        m = fmaxf(m, mc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { m = fmaxf(m, __shfl_xor(m, off, 64)); bad |= __shfl_xor(bad, off, 64); }
    if ((tid & 63) == 0) { s_m[wv] = m; s_bad[wv] = bad; }
    __syncthreads();
    m = s_m[0]; bad = s_bad[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) { m = fmaxf(m, s_m[w]); bad |= s_bad[w]; }
    const bool invalid = bad != 0 || m == -INFINITY;                     // workgroup-uniform
    const float qnan = __uint_as_float(0x7FC00000u);
    if (invalid) {
        if (tid == 0) { logprob[row] = qnan; rank[row] = -1; }
        if (tid < top_n) { top_ids[row * top_n + tid] = -1; top_logprobs[row * top_n + tid] = qnan; }
        return;
    }
    // sums relative to the row's maximum, in float64; the counts
    double S = 0.0;
    int cnt = 0;
    for (int c = tid; c < cpr; c += LP_TPB) {
        const LpPart q = pr[c];
        if (q.m != -INFINITY) S += (double)q.s * exp((double)q.m - (double)m);
        cnt += q.cnt;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) S += __shfl_xor(S, off, 64);
    cnt = wave_sum_i32(cnt);
    if ((tid & 63) == 0) { s_s[wv] = S; s_cnt[wv] = cnt; }
    __syncthreads();
    S = s_s[0]; cnt = s_cnt[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) { S += s_s[w]; cnt += s_cnt[w]; }
    const double lnS = log(S);
    if (tid == 0) {
        const int64_t cid = chosen[row];
        if (cid >= 0 && cid < V) {
            const float xs = lp_scale<DT, SCALE>(load_f<DT>(p, cid), t, inv_t);
            logprob[row] = (float)(((double)xs - (double)m) - lnS);
            rank[row] = 1 + cnt;
        } else {
            logprob[row] = qnan;
            rank[row] = -1;
        }
    }
    if (top_n <= 0) return;
    // the row's top N: top_n rounds of "largest candidate below the last one" over the chunks' lists
    const unsigned long long *cr = cand + row * (int64_t)cpr * top_n;
    const int64_t ncand = (int64_t)cpr * top_n;
    uint64_t bound = ~0ull;
    for (int r = 0; r < top_n; ++r) {
        uint64_t best = 0ull;
        for (int64_t i = tid; i < ncand; i += LP_TPB) {
            const uint64_t k = cr[i];
            best = (k < bound && k > best) ? k : best;
        }
        best = wave_max_u64(best);
        if ((tid & 63) == 0) s_key[wv] = best;
        __syncthreads();
        best = s_key[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) best = s_key[w] > best ? s_key[w] : best;
        if (tid == 0) s_top[r] = best;
        __syncthreads();
        if (best != 0ull) bound = best;
    }
    if (tid < top_n) {
        const uint64_t k = s_top[tid];
        const int64_t id = (int64_t)(uint32_t)(~(uint32_t)k);
        int64_t oid = -1;
        float lp = -INFINITY;                                            // V < top_n: id -1, log-probability -inf
        if (k != 0ull && id < V) {
            const float xs = lp_scale<DT, SCALE>(load_f<DT>(p, id), t, inv_t);
            oid = id;
            lp = (float)(((double)xs - (double)m) - lnS);
        }
        top_ids[row * top_n + tid] = oid;
        top_logprobs[row * top_n + tid] = lp;
    }
}

// ---- host -----------------------------------------------------------------------------------------
// Does bf16(x * fl(1/T)) equal bf16(fl32(x / T)) for every normal bf16 x?  Both roundings commute with powers of two, so the
// 128 mantissas decide (the test jf_rs_probs applies to its rows).
static bool lp_scale_is_exact(float t) {
    const float inv_t = 1.f / t;
    auto rne = [](float v) { uint32_t u; memcpy(&u, &v, 4); u = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u; return u; };
    for (int m = 128; m < 256; ++m) {
        const volatile float x = (float)m;
        const volatile float q = x * inv_t, r = x / t;
        if (rne(q) != rne(r)) return false;
    }
    return true;
}
static int64_t lp_cpr(int dtype, int64_t V) {
    const int64_t ch = dtype == JF_F32 ? LpChunk<JF_F32>::ELEMS : LpChunk<JF_BF16>::ELEMS;
    return (V + ch - 1) / ch;
}
static size_t lp_ws_bytes(int64_t items, int32_t top_n) { return (size_t)items * (sizeof(LpPart) + (size_t)top_n * 8); }

extern "C" size_t jf_logprobs_workspace_bytes(int64_t R, int64_t V, int32_t top_n) {
    if (R <= 0 || V <= 0) return 0;
    if (top_n < 0) top_n = 0;
    if (top_n > JF_LOGPROBS_MAX_TOP) top_n = JF_LOGPROBS_MAX_TOP;
    return lp_ws_bytes(R * lp_cpr(JF_F32, V), top_n);                     // float32 rows have the most chunks: enough for either dtype
}

extern "C" int jf_logprobs_rows(const void *logits, int dtype, int64_t R, int64_t V, int64_t row_stride, float temperature,
                                const int64_t *chosen, int32_t top_n, float *logprob, int32_t *rank, int64_t *top_ids,
                                float *top_logprobs, void *workspace, size_t workspace_bytes, void *stream) {
    if (R <= 0) return JF_OK;
    if (!logits || !chosen || !logprob || !rank || !workspace) return fail(JF_E_INVALID, "jf_logprobs_rows: null pointer");
    if (dtype != JF_F32 && dtype != JF_BF16) return fail(JF_E_INVALID, "jf_logprobs_rows: dtype %d", dtype);
    if (V <= 0 || V > 0x7FFFFFFFll || row_stride < V)
        return fail(JF_E_INVALID, "jf_logprobs_rows: bad shape V=%lld stride=%lld", (long long)V, (long long)row_stride);
    if (top_n < 0 || top_n > JF_LOGPROBS_MAX_TOP) return fail(JF_E_INVALID, "jf_logprobs_rows: top_n=%d (0..%d)", (int)top_n, JF_LOGPROBS_MAX_TOP);
    if (top_n > 0 && (!top_ids || !top_logprobs)) return fail(JF_E_INVALID, "jf_logprobs_rows: null top_ids / top_logprobs with top_n=%d", (int)top_n);
    const int64_t cpr = lp_cpr(dtype, V);
    if (R > 0x7FFFFFFFll || R * cpr > 0x7FFFFFFFll) return fail(JF_E_INVALID, "jf_logprobs_rows: R=%lld (R * chunks per row must fit a grid)", (long long)R);
    if (workspace_bytes < jf_logprobs_workspace_bytes(R, V, top_n) || ((uintptr_t)workspace % 16) != 0)
        return fail(JF_E_INVALID, "jf_logprobs_rows: workspace too small or not 16-byte aligned");
    const float t = (temperature <= 0.f) ? 1.f : temperature;
    const float inv_t = 1.f / t;
    const int esz = dtype == JF_F32 ? 4 : 2;
    const bool vec = (((uintptr_t)logits) % 16 == 0) && ((row_stride * esz) % 16 == 0);
    const bool unit = t == 1.f;
    LpPart *part = (LpPart *)workspace;
    unsigned long long *cand = (unsigned long long *)(part + R * cpr);    // (16-byte records in front: 8-byte aligned)
    hipStream_t s = (hipStream_t)stream;
    const dim3 pgrid((unsigned)(R * cpr)), fgrid((unsigned)R), block(LP_TPB);
#define JF_LP_P(DT, VECF, SC)                                                                                                        \
    do {                                                                                                                             \
        if (top_n > 0) lp_partial_kernel<DT, VECF, SC, true><<<pgrid, block, 0, s>>>(logits, V, row_stride, t, inv_t, chosen, (int)cpr, top_n, part, cand); \
        else lp_partial_kernel<DT, VECF, SC, false><<<pgrid, block, 0, s>>>(logits, V, row_stride, t, inv_t, chosen, (int)cpr, 0, part, cand);              \
    } while (0)
#define JF_LP_V(DT, SC)                                                                                                              \
    do {                                                                                                                             \
        if (vec) JF_LP_P(DT, true, SC); else JF_LP_P(DT, false, SC);                                                                 \
        lp_finish_kernel<DT, SC><<<fgrid, block, 0, s>>>(logits, V, row_stride, t, inv_t, chosen, (int)cpr, top_n, part, cand, logprob, rank,  \
                                                         top_ids, top_logprobs);                                                     \
    } while (0)
    if (dtype == JF_F32) {
        if (unit) JF_LP_V(JF_F32, 0); else JF_LP_V(JF_F32, 1);
    } else {
        if (unit) JF_LP_V(JF_BF16, 0); else if (lp_scale_is_exact(t)) JF_LP_V(JF_BF16, 2); else JF_LP_V(JF_BF16, 1);
    }
#undef JF_LP_V
#undef JF_LP_P
    return check_launch("logprobs kernels");
}
