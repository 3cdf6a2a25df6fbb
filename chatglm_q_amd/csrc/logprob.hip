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

template <typename T, int TB>
__global__ __launch_bounds__(TB) void token_logprob_kernel(const T* __restrict__ logits, int N, int64_t ldl,
                                                           const int64_t* __restrict__ targets, int64_t ignore_index,
                                                           float* __restrict__ logprob_out, float* __restrict__ lse_out,
                                                           int64_t* __restrict__ argmax_out) {
    constexpr int CH = 16 / (int)sizeof(T), NW = TB / 64;
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

    // [0, head): in front of the first 16-byte boundary; [head, head + nvec * CH): whole aligned chunks; the rest: the ragged tail
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) / (unsigned)sizeof(T));
    head = head < N ? head : N;
    const int nvec = (N - head) / CH, tail0 = head + nvec * CH;

    LpRun r = {-INFINITY, 0.f, INT_MAX};
    if (tid < head) {
        const float v[1] = {Act<T>::load(row + tid)};
        lp_absorb<1>(r, v, tid);
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
                lp_absorb<CH>(r, v, head + c * CH);
            }
        }
    }
    if (tail0 + tid < N) {                                   // fewer than CH elements
        const float v[1] = {Act<T>::load(row + tail0 + tid)};
        lp_absorb<1>(r, v, tail0 + tid);
    }

    // lanes -> wave (DPP) -> workgroup (one LDS step)
    const float M = wave_max_dpp(r.m);
    const float S = wave_sum(r.s * lp_carry(r.m, M));
    const int I = wave_min_i(r.m == M ? r.i : INT_MAX);
    if ((tid & 63) == 0) {
        wm[tid >> 6] = M;
        ws[tid >> 6] = S;
        wi[tid >> 6] = I;
    }
    __syncthreads();
    if (tid == 0) {
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
        const float ls = logf(s);
        logprob_out[blockIdx.x] = ignored ? 0.f : (xt - m) - ls;
        if (lse_out) lse_out[blockIdx.x] = m + ls;
        if (argmax_out) argmax_out[blockIdx.x] = i == INT_MAX ? 0 : i;     // nothing but -inf / NaN: index 0
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

}  // namespace ql
