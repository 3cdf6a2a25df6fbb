// Per-token log-probabilities of given ids from a block of logits rows in ONE pass over the rows - the tail of the reference's loss
// (chatglm_q/model.py:384-390: logits .float(), then F.cross_entropy) and of its perplexity run (examples/evaluations/ppl.py) without
// the fp32 copy of the logits and without a second and third walk over them:
//
//     lse[r]     = log(sum_j exp(float(x[r, j])))          fp32, max-subtracted
//     logprob[r] = float(x[r, target[r]]) - lse[r]         0 when target[r] == ignore_index, NaN when it is outside [0, N)
//     argmax[r]  = lowest index of the row maximum         optional
//
// One workgroup per row.  Every lane keeps a running (max, sum, index of the max) over the 16-byte chunks it owns: a chunk whose
// maximum exceeds the lane's rescales the sum once (rare after the first few chunks), then its values are added as
// exp2((v - max) * log2 e) - v_exp_f32, the sum is relative to the exact maximum, so the result has log_softmax's error and not that
// of a sum of large exponentials.  Lanes are merged by DPP wave reductions and one LDS step; the target logit is one extra load by
// thread 0, requested before the walk.  A row is read with 16-byte loads from its first 16-byte aligned element on; the elements in
// front of it and behind the last whole chunk are read one by one, so no load touches bytes outside [row, row + N).
//
// -inf entries: a lane that has seen nothing but -inf subtracts 0 instead of its maximum (exp2(-inf) = 0, never (-inf) - (-inf)).  A row
// of nothing but -inf has lse = -inf and a NaN log-prob, as log_softmax gives it.  A NaN logit reaches the row's sum and so its lse and
// log-prob; the maximum search skips it (argmax then indexes the largest number of the row).
//
// The same walk serves qlinear_step_logprobs (further down): the record of a generation step - the chosen id's log-prob and the most
// likely alternatives - bit for bit what this file's scoring kernel returns for the same row.
#include <limits.h>

#include "launch.h"
#include "ql_common.h"

namespace ql {
namespace {

constexpr float LP_LOG2E = 1.44269504088896340736f;
constexpr int LP_U = 4;                  // 16-byte chunks a thread requests before it uses the first

struct LpRun {
    float m, s;                          // running maximum, sum of exp(v - m)
    int i;                               // lowest index holding m
};

__device__ __forceinline__ float lp_exp(float d) { return __builtin_amdgcn_exp2f(d * LP_LOG2E); }
// factor that carries a sum relative to `from` over to the larger maximum `to`
__device__ __forceinline__ float lp_carry(float from, float to) { return from == -INFINITY ? 0.f : lp_exp(from - to); }

template <int CH>
__device__ __forceinline__ void lp_absorb(LpRun& r, const float (&v)[CH], int base) {
    float cm = v[0];
#pragma unroll
    for (int e = 1; e < CH; ++e) cm = fmaxf(cm, v[e]);
    if (cm > r.m) {                      // a lane's chunks come in ascending order: strict > keeps the lowest index
        int k = CH - 1;
#pragma unroll
        for (int e = CH - 2; e >= 0; --e) k = v[e] == cm ? e : k;
        r.s *= lp_exp(r.m - cm);         // r.m == -inf: the sum is still 0
        r.m = cm;
        r.i = base + k;
    }
    const float mr = r.m == -INFINITY ? 0.f : r.m;
#pragma unroll
    for (int e = 0; e < CH; ++e) r.s += lp_exp(v[e] - mr);
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// Every element of a row exactly once, in the chunk ownership all kernels of this file share: lane `tid` of TB gets the unaligned
// head's element tid, the aligned 16-byte chunks tid, tid + TB, ... (LP_U requests in flight) and the ragged tail's element tid.
// f(v, base): v = the elements as floats (1 or CH of them), base = the index of v[0].  No load touches bytes outside [row, row + N).
template <typename T, int TB, typename F>
__device__ __forceinline__ void lp_for_each_chunk(const T* __restrict__ row, int N, int tid, F&& f) {
    constexpr int CH = 16 / (int)sizeof(T);
    // [0, head): in front of the first 16-byte boundary; [head, head + nvec * CH): whole aligned chunks; the rest: the ragged tail
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / (unsigned)sizeof(T));
    head = head < N ? head : N;
    const int nvec = (N - head) / CH, tail0 = head + nvec * CH;
    if (tid < head) {
        const float v[1] = {Act<T>::load(row + tid)};
        f(v, tid);
    }
    const T* body = row + head;
    for (int c0 = tid; c0 < nvec; c0 += LP_U * TB) {
        u32x4 raw[LP_U];
#pragma unroll
        for (int u = 0; u < LP_U; ++u) {                     // every request before the first use; clamped to a chunk of the row, not predicated
            const int c = c0 + u * TB;
            raw[u] = *reinterpret_cast<const u32x4*>(body + (size_t)(c < nvec ? c : c0) * CH);
        }
#pragma unroll
        for (int u = 0; u < LP_U; ++u) {
            const int c = c0 + u * TB;
            if (c < nvec) {
                float v[CH];
                if constexpr (sizeof(T) == 2) {
                    unpack8<T>(raw[u], v);
                } else {
#pragma unroll
                    for (int e = 0; e < CH; ++e) v[e] = u32_as_f32(raw[u][e]);
                }
                f(v, head + c * CH);
            }
        }
    }
    if (tail0 + tid < N) {                                   // fewer than CH elements
        const float v[1] = {Act<T>::load(row + tail0 + tid)};
        f(v, tail0 + tid);
    }
}

// the walk: a lane's running (max, sum, index) over the elements it owns
template <typename T, int TB>
__device__ __forceinline__ LpRun lp_walk(const T* __restrict__ row, int N, int tid) {
    LpRun r = {-INFINITY, 0.f, INT_MAX};
    lp_for_each_chunk<T, TB>(row, N, tid, [&](const auto& v, int base) { lp_absorb(r, v, base); });
    return r;
}

// lanes -> wave (DPP) -> one LDS slot per wave; the caller synchronises, then ONE thread runs lp_merge_waves
template <int NW>
__device__ __forceinline__ void lp_merge_lanes(const LpRun& r, int tid, float (&wm)[NW], float (&ws)[NW], int (&wi)[NW]) {
    const float M = wave_max_dpp(r.m);
    const float S = wave_sum(r.s * lp_carry(r.m, M));
    const int I = wave_min_i(r.m == M ? r.i : INT_MAX);
    if ((tid & 63) == 0) {
        wm[tid >> 6] = M;
        ws[tid >> 6] = S;
        wi[tid >> 6] = I;
    }
}

// the row's (maximum, sum of exp(v - maximum), lowest index of the maximum or INT_MAX) from the waves' slots
template <int NW>
__device__ __forceinline__ LpRun lp_merge_waves(const float (&wm)[NW], const float (&ws)[NW], const int (&wi)[NW]) {
    float m = wm[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, wm[w]);
    float s = 0.f;
    int i = INT_MAX;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        s += ws[w] * lp_carry(wm[w], m);
        if (wm[w] == m) i = wi[w] < i ? wi[w] : i;
    }
    return {m, s, i};
}

template <typename T, int TB>
__global__ __launch_bounds__(TB) void token_logprob_kernel(const T* __restrict__ logits, int N, int64_t ldl,
                                                           const int64_t* __restrict__ targets, int64_t ignore_index,
                                                           float* __restrict__ logprob_out, float* __restrict__ lse_out,
                                                           int64_t* __restrict__ argmax_out) {
    constexpr int NW = TB / 64;
    __shared__ float wm[NW], ws[NW];
    __shared__ int wi[NW];
    const int tid = threadIdx.x;
    const T* row = logits + (int64_t)blockIdx.x * ldl;

    // the target's logit: requested now, used after the walk
    float xt = 0.f;
    bool ignored = false;
    if (tid == 0) {
        const int64_t t = targets[blockIdx.x];
        ignored = t == ignore_index;
        xt = (!ignored && t >= 0 && t < (int64_t)N) ? Act<T>::load(row + t) : __builtin_nanf("");
    }

    const LpRun r = lp_walk<T, TB>(row, N, tid);
    lp_merge_lanes<NW>(r, tid, wm, ws, wi);
    __syncthreads();
    if (tid == 0) {
        const LpRun g = lp_merge_waves<NW>(wm, ws, wi);
        const float m = g.m, ls = logf(g.s);
        const int i = g.i;
        logprob_out[blockIdx.x] = ignored ? 0.f : (xt - m) - ls;
        if (lse_out) lse_out[blockIdx.x] = m + ls;
        if (argmax_out) argmax_out[blockIdx.x] = i == INT_MAX ? 0 : i;     // nothing but -inf / NaN: index 0
    }
}

// ---- one generation step's record: the chosen token's log-prob and the n_top most likely alternatives (qlinear_step_logprobs) ----------
// One workgroup of 1024 threads per row, launched behind the step's selection.  The log-sum-exp is the walk above, so every value
// written is bit for bit what token_logprob_kernel<T, 1024> returns for the same row and id.  Selection of the n_top <= 20 best under
// the total order (value descending, index ascending; a NaN ranks as -inf):
//   1. the walk leaves every lane's own maximum; the maxima of the 64 groups of 16 lanes go to LDS, and t0 = the K-th largest of
//      them (K = min(n_top, N)) - K different groups hold an element >= t0, so at least K positions do;
//   2. a second walk - only lanes whose own maximum reaches t0 take it, their chunks come from L2 - appends every (value, index)
//      with value >= t0 to a list in LDS (random rows of 65 024: ~25 entries);
//   3. every entry is ranked by counting the entries in front of it; rank j < K writes slot j.
// A list that would overflow (LP_CAND entries: a sorted row, a row of mostly -inf, a tie group that large) takes the exact slow
// path: K rounds of a workgroup arg-max over the elements behind the one the previous round took.
constexpr int LP_CAND = 1024;            // candidate list: one entry per thread in the ranking

__device__ __forceinline__ float lp_order_value(float x) { return x != x ? -INFINITY : x; }
// (v, i) stands in front of (w, j) in the total order
__device__ __forceinline__ bool lp_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

template <typename T>
__global__ __launch_bounds__(1024) void step_logprobs_kernel(const T* __restrict__ logits, int N, int64_t ldl,
                                                             const int64_t* __restrict__ tok, const int32_t* __restrict__ row_state,
                                                             int32_t* __restrict__ count, float* __restrict__ chosen,
                                                             int32_t* __restrict__ top_ids, float* __restrict__ top_lp, int64_t cap,
                                                             int n_top) {
    constexpr int TB = 1024, NW = TB / 64, NG = TB / 16;
    __shared__ float wm[NW], ws[NW], gm[NG], cv[LP_CAND], sh[3];
    __shared__ int wi[NW], ci[LP_CAND], cnt;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int c = count[b];
    if (row_state && row_state[2 * b] <= c) return;          // the row recorded no token in this step (finished / out of budget)
    if ((int64_t)c >= cap) return;                           // the record is full
    const T* row = logits + (int64_t)b * ldl;
    const int K = n_top < N ? n_top : N;

    float xt = 0.f;
    if (tid == 0) {
        const int64_t t = tok[b];
        xt = (t >= 0 && t < (int64_t)N) ? Act<T>::load(row + t) : __builtin_nanf("");
        cnt = 0;
    }

    const LpRun r = lp_walk<T, TB>(row, N, tid);
    lp_merge_lanes<NW>(r, tid, wm, ws, wi);
    if (K > 0) {                                             // maxima of the groups of 16 lanes (r.m is never NaN)
        float g = r.m;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) g = fmaxf(g, __shfl_xor(g, off, 64));
        if ((tid & 15) == 0) gm[tid >> 4] = g;
    }
    __syncthreads();
    const int64_t slot = (int64_t)b * cap + c;
    if (tid == 0) {
        const LpRun g = lp_merge_waves<NW>(wm, ws, wi);
        const float m = g.m, ls = logf(g.s);
        chosen[slot] = (xt - m) - ls;
        sh[0] = m;
        sh[1] = ls;
        count[b] = c + 1;                                    // every thread read count[b] in front of the barrier above
    }
    if (n_top <= 0) return;
    int32_t* ids_out = top_ids + slot * n_top;
    float* lp_out = top_lp + slot * n_top;
    if (tid >= K && tid < n_top) {                           // fewer than n_top entries in the row
        ids_out[tid] = -1;
        lp_out[tid] = -INFINITY;
    }
    if (tid >= 64 && tid < 64 + NG) {                        // wave 1: t0 = the K-th largest group maximum, by counting
        const int l = tid - 64;
        const float v = gm[l];
        int rank = 0;
        for (int j = 0; j < NG; ++j) rank += lp_before(gm[j], j, v, l) ? 1 : 0;
        if (rank == K - 1) sh[2] = v;
    }
    __syncthreads();
    const float m = sh[0], ls = sh[1], t0 = sh[2];
    if (r.m >= t0) {                                         // a lane whose maximum is below t0 owns no candidate
        lp_for_each_chunk<T, TB>(row, N, tid, [&](const auto& v, int base) {
            constexpr int n = (int)(sizeof(v) / sizeof(float));
#pragma unroll
            for (int e = 0; e < n; ++e) {
                const float x = lp_order_value(v[e]);
                if (x >= t0) {
                    const int at = atomicAdd(&cnt, 1);       // LDS; the ranking below does not depend on the order of arrival
                    if (at < LP_CAND) {
                        cv[at] = x;
                        ci[at] = base + e;
                    }
                }
            }
        });
    }
    __syncthreads();
    const int C = cnt;
    if (C <= LP_CAND) {
        if (tid < C) {
            const float v = cv[tid];
            const int i = ci[tid];
            int rank = 0;
            for (int j = 0; j < C; ++j) rank += lp_before(cv[j], ci[j], v, i) ? 1 : 0;
            if (rank < K) {
                ids_out[rank] = i;
                lp_out[rank] = (Act<T>::load(row + i) - m) - ls;
            }
        }
        return;
    }
    // exact slow path: round j takes the first element, in the total order, behind the one round j - 1 took
    float* sv = cv;                                          // the list is not used on this path
    int* si = ci;
    float pv = INFINITY;
    int pi = -1;
    for (int j = 0; j < K; ++j) {
        float bv = -INFINITY;
        int bi = INT_MAX;
        for (int e = tid; e < N; e += TB) {
            const float x = lp_order_value(Act<T>::load(row + e));
            if (lp_before(pv, pi, x, e) && lp_before(x, e, bv, bi)) {
                bv = x;
                bi = e;
            }
        }
        const float M = wave_max_dpp(bv);
        const int I = wave_min_i(bv == M ? bi : INT_MAX);
        __syncthreads();                                     // the previous round's slots have been read
        if ((tid & 63) == 0) {
            sv[tid >> 6] = M;
            si[tid >> 6] = I;
        }
        __syncthreads();
        pv = sv[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) pv = fmaxf(pv, sv[w]);
        pi = INT_MAX;
#pragma unroll
        for (int w = 0; w < NW; ++w) pi = (sv[w] == pv && si[w] < pi) ? si[w] : pi;
        if (tid == 0 && pi != INT_MAX) {                       // (K <= N: a round always finds an element)
            ids_out[j] = pi;
            lp_out[j] = (Act<T>::load(row + pi) - m) - ls;
        }
    }
}

}  // namespace

int token_logprob(int dtype, const void* logits, int64_t R, int64_t N, int64_t ldl, const int64_t* targets, int64_t ignore_index,
                  float* logprob_out, float* lse_out, int64_t* argmax_out, hipStream_t st) {
    // Few rows: 1024 threads per row (a row's bytes are requested by as many lanes as a workgroup holds; two such workgroups fit a
    // CU, so below ~1024 rows the chip is not full either way).  Many rows: 256 threads per row, 8 rows in flight per CU.
#define QL_LOGPROB(TT)                                                                                                             \
    if (R < 1024)                                                                                                                  \
        token_logprob_kernel<TT, 1024><<<(unsigned)R, 1024, 0, st>>>((const TT*)logits, (int)N, ldl, targets, ignore_index,        \
                                                                     logprob_out, lse_out, argmax_out);                            \
    else                                                                                                                           \
        token_logprob_kernel<TT, 256><<<(unsigned)R, 256, 0, st>>>((const TT*)logits, (int)N, ldl, targets, ignore_index,          \
                                                                   logprob_out, lse_out, argmax_out)
    switch (dtype) {
    case QL_DTYPE_F32: QL_LOGPROB(float); break;
    case QL_DTYPE_F16: QL_LOGPROB(f16); break;
    case QL_DTYPE_BF16: QL_LOGPROB(__bf16); break;
    default: return QL_ERR_BAD_DTYPE;
    }
#undef QL_LOGPROB
    return finish_launch();
}

int step_logprobs(int dtype, const void* logits, int64_t B, int64_t N, int64_t ldl, const int64_t* tok, const int32_t* row_state,
                  int32_t* count, float* chosen, int32_t* top_ids, float* top_lp, int64_t cap, int64_t n_top, hipStream_t st) {
#define QL_STEP_LOGPROBS(TT)                                                                                                       \
    step_logprobs_kernel<TT><<<(unsigned)B, 1024, 0, st>>>((const TT*)logits, (int)N, ldl, tok, row_state, count, chosen, top_ids, \
                                                           top_lp, cap, (int)n_top)
    switch (dtype) {
    case QL_DTYPE_F32: QL_STEP_LOGPROBS(float); break;
    case QL_DTYPE_F16: QL_STEP_LOGPROBS(f16); break;
    case QL_DTYPE_BF16: QL_STEP_LOGPROBS(__bf16); break;
    default: return QL_ERR_BAD_DTYPE;
    }
#undef QL_STEP_LOGPROBS
    return finish_launch();
}

}  // namespace ql
