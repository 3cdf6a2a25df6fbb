// Repetition / presence / frequency penalties and a sparse logit bias, applied in place to a step's logits between lm_head and the
// selection kernel (qlinear_logit_penalties), with the token history they need kept in device memory so that the launch can sit
// inside a captured decode step.
//
// State: one int32 per (row, vocabulary entry) - bit 31 = the entry is one of the row's prompt ids (P), bits 0..30 = how often the
// row has generated it (G).  A word is 0 for everything the row has never seen, so "P || G > 0" is "word != 0".
//
// Per entry, x = float(logit), every line ONE fp32 operation rounded to nearest (contraction is switched off for the function: the
// build contracts by default and x - f * G must not become a fused multiply-add):
//     word != 0 :  x = x > 0 ? x / r : x * r          (a NaN takes the multiply and stays NaN)
//     G > 0     :  m = f * float(G);  x = x - m;  x = x - p
//     biased    :  x = x + bias
// and one rounding to the logits dtype.  An entry no rule touches keeps its bits (a 16-byte chunk none of whose entries is touched
// is not written at all).
//
// Ownership: a workgroup serves one tile of PEN_TB chunks of one row, a thread one chunk (16 bytes of logits: 8 / 4 entries) - every
// entry belongs to exactly one thread of the launch.  The history advances in the same launch without atomics: the thread that owns
// entry tok[b] adds 1 to the word it has just loaded, before the rules, and stores it.  The bias list of the row (at most
// QL_LOGIT_BIAS_MAX entries) is scattered by the tile's first threads into a one-byte-per-entry LDS map of the tile, so an entry
// finds its bias with the LDS read of its chunk; rows without a list skip the map and both barriers.
//
// A chunk goes through 16-byte loads / stores when it lies whole inside the row and both the logits row and the state row are
// 16-byte aligned; the ragged last chunk of a row, and every chunk of a row that is not aligned (odd N or ldl, a sliced tensor), go
// entry by entry.  Nothing outside [row, row + N) is read or written.
//
// Bound: a streaming pass over B x N x (logit + 4) bytes read, plus the touched chunks written back (a history of a few hundred
// tokens touches a few hundred chunks per row).
#include "launch.h"
#include "ql_common.h"

namespace ql {
namespace {

constexpr int PEN_TB = 256;
constexpr int PEN_BIAS_MAX = 64;         // QL_LOGIT_BIAS_MAX (include/qlinear_hip.h)
constexpr u32 PEN_PROMPT = 0x80000000u;

// the three rules for one entry; returns whether any of them applied.  `word` is the state AFTER this step's count.
__device__ __forceinline__ bool pen_entry(float& x, u32 word, float r, float p, float f, bool biased, float bias) {
#pragma clang fp contract(off)
    bool touched = false;
    if (word != 0u) {
        x = x > 0.f ? x / r : x * r;
        touched = true;
    }
    const u32 g = word & ~PEN_PROMPT;
    if (g != 0u) {
        const float m = f * (float)g;
        x = x - m;
        x = x - p;
    }
    if (biased) {
        x = x + bias;
        touched = true;
    }
    return touched;
}

template <typename T>
__global__ __launch_bounds__(PEN_TB) void logit_penalties_kernel(T* __restrict__ logits, int N, int64_t ldl,
                                                                 const float* __restrict__ settings,
                                                                 const int32_t* __restrict__ bias_ids,
                                                                 const float* __restrict__ bias_vals,
                                                                 const int32_t* __restrict__ bias_len, int bias_cap,
                                                                 u32* __restrict__ state, int64_t lds,
                                                                 const int64_t* __restrict__ tok,
                                                                 const int32_t* __restrict__ row_state) {
    constexpr int CH = 16 / (int)sizeof(T), TILE = PEN_TB * CH;
    __shared__ __attribute__((aligned(16))) uint8_t slot[TILE];          // 1 + index into the row's bias list, 0 = no bias
    const int b = blockIdx.y, tid = threadIdx.x;
    if (row_state && (row_state[2 * b + 1] & 1)) return;                  // a finished row: no count, no write (uniform per block)

    const int tile0 = blockIdx.x * TILE, v0 = tile0 + tid * CH;
    T* row = logits + (int64_t)b * ldl;
    u32* srow = state + (int64_t)b * lds;
    const float r = settings[3 * b], p = settings[3 * b + 1], f = settings[3 * b + 2];
    int nb = (bias_len && bias_cap > 0) ? bias_len[b] : 0;
    nb = nb < 0 ? 0 : (nb > bias_cap ? bias_cap : nb);
    const int64_t t = tok ? tok[b] : -1;                                  // the id fed into this step (null: the first token)

    uint8_t sl[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) sl[e] = 0;
    if (nb > 0) {                                                         // uniform per block
#pragma unroll
        for (int e = 0; e < CH; ++e) slot[tid * CH + e] = 0;
        __syncthreads();
        if (tid < nb) {
            const int id = bias_ids[(int64_t)b * bias_cap + tid];
            if (id >= tile0 && id < tile0 + TILE && id < N) slot[id - tile0] = (uint8_t)(tid + 1);
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < CH; ++e) sl[e] = slot[tid * CH + e];
    }
    if (v0 >= N) return;

    const float* bv = bias_vals + (int64_t)b * bias_cap;
    const bool counts_here = t >= (int64_t)v0 && t < (int64_t)v0 + CH && t < (int64_t)N;
    const bool vec = v0 + CH <= N && ((reinterpret_cast<uintptr_t>(row) | reinterpret_cast<uintptr_t>(srow)) & 15u) == 0;
    if (vec) {
        u32 w[CH];
        const u32x4* sp = reinterpret_cast<const u32x4*>(srow + v0);
        const u32x4 raw = *reinterpret_cast<const u32x4*>(row + v0);
#pragma unroll
        for (int q = 0; q < CH / 4; ++q) {
            const u32x4 s4 = sp[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) w[4 * q + e] = s4[e];
        }
        if (counts_here) {
#pragma unroll
            for (int e = 0; e < CH; ++e)
                if (v0 + e == (int)t) {
                    w[e] += 1u;
                    srow[v0 + e] = w[e];
                }
        }
        float x[CH];
        if constexpr (sizeof(T) == 2) {
            unpack8<T>(raw, x);
        } else {
#pragma unroll
            for (int e = 0; e < CH; ++e) x[e] = u32_as_f32(raw[e]);
        }
        bool any = false, hit[CH];
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const bool biased = sl[e] != 0;
            const float bias = biased ? bv[sl[e] - 1] : 0.f;
            hit[e] = pen_entry(x[e], w[e], r, p, f, biased, bias);
            any |= hit[e];
        }
        if (any) {
            u32x4 out;
            if constexpr (sizeof(T) == 2) {
                const u32x4 packed = pack8<T>(x);                         // one rounding to T per entry
#pragma unroll
                for (int q = 0; q < 4; ++q) {                             // untouched entries keep their bits
                    const u32 keep = (hit[2 * q] ? 0u : 0x0000FFFFu) | (hit[2 * q + 1] ? 0u : 0xFFFF0000u);
                    out[q] = (raw[q] & keep) | (packed[q] & ~keep);
                }
            } else {
#pragma unroll
                for (int e = 0; e < CH; ++e) out[e] = hit[e] ? f32_as_u32(x[e]) : raw[e];
            }
            *reinterpret_cast<u32x4*>(row + v0) = out;
        }
        return;
    }
    // entry by entry: the ragged end of a row, rows that are not 16-byte aligned
    const int n_here = N - v0 < CH ? N - v0 : CH;
    for (int e = 0; e < n_here; ++e) {
        const int v = v0 + e;
        u32 w = srow[v];
        if (counts_here && v == (int)t) {
            w += 1u;
            srow[v] = w;
        }
        const bool biased = sl[e] != 0;
        const float bias = biased ? bv[sl[e] - 1] : 0.f;
        float x = Act<T>::load(row + v);
        if (pen_entry(x, w, r, p, f, biased, bias)) Act<T>::store(row + v, x);
    }
}

}  // namespace

int logit_penalties(int dtype, void* logits, int64_t B, int64_t N, int64_t ldl, const float* settings, const int32_t* bias_ids,
                    const float* bias_vals, const int32_t* bias_len, int64_t bias_cap, int32_t* state, int64_t lds, const int64_t* tok,
                    const int32_t* row_state, hipStream_t st) {
    static_assert(PEN_BIAS_MAX == QL_LOGIT_BIAS_MAX && PEN_BIAS_MAX <= PEN_TB && PEN_BIAS_MAX < 255, "bias list: one thread and one byte per entry");
#define QL_PENALTIES(TT)                                                                                                           \
    {                                                                                                                              \
        constexpr int64_t tile = PEN_TB * (16 / (int64_t)sizeof(TT));                                                              \
        logit_penalties_kernel<TT><<<dim3((unsigned)((N + tile - 1) / tile), (unsigned)B), PEN_TB, 0, st>>>(                       \
            (TT*)logits, (int)N, ldl, settings, bias_ids, bias_vals, bias_len, (int)bias_cap, (u32*)state, lds, tok, row_state);   \
    }
    switch (dtype) {
    case QL_DTYPE_F32: QL_PENALTIES(float); break;
    case QL_DTYPE_F16: QL_PENALTIES(f16); break;
    case QL_DTYPE_BF16: QL_PENALTIES(__bf16); break;
    default: return QL_ERR_BAD_DTYPE;
    }
#undef QL_PENALTIES
    return finish_launch();
}

}  // namespace ql
