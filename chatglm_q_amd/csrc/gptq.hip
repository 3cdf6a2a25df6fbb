// GPTQ: the column walk of one block of at most 128 input columns as ONE launch (qlinear_gptq_block).
//
// The reference's quantize_weight (chatglm_q/int4/quantizer.py:151-167, int8/quantizer.py:126-137) walks a block's columns one at
// a time, every column about a dozen tiny launches over all weight rows.  The dependency runs along the columns only: a weight
// row never reads another row.  So a lane owns a row and walks its columns alone; nothing is shared, there is no barrier and
// every output element has one owner.
//
// Per row, for j = 0 .. bc-1, every line ONE fp32 operation rounded to nearest (no fused multiply-add: contraction is off for
// this file), w[] the row's current block values, d = Hinv[j][j], qmax = 7 / 127:
//     int4, j % 32 == 0:  m = max_{t<32} |w[j+t]|;  s = max(m / 7, 1e-10);  scale[(c0+j)/32][r] = s
//     int8:               s = scale[r]
//     x = w[j] / s;  c = min(max(rint(x), -qmax), qmax);  q = s * c                      Q[r][j] = q
//     e = w[j] - q;  Loss[r][j] = ((e * e) / (d * d)) * 0.5;  err = e / d                Err[r][j] = err
//     for t in j+1 .. bc-1:  p = err * Hinv[j][t];  w[t] = w[t] - p
// What fixes the bits of w[t] is the ORDER in which the columns j < t are subtracted from it, nothing else.  A lane therefore
// holds GQ_CH = 32 columns in registers at a time: first it subtracts every earlier column j from the 32 (a rolled loop over j,
// 32 multiply / subtract pairs with fixed register numbers, err_j from the lane's LDS slot), then it walks the triangle inside
// the 32 fully unrolled (496 pairs + 32 quantisation steps - about a tenth of the 8 128 pairs of a 128-column triangle, which
// would not fit the instruction cache).  Row j of the Hinv block is the same for every lane: its address is wave-uniform, the
// loads are scalar loads and the multiplies take it from scalar registers.
//
// LDS: err of the block's columns, [column][lane] (no bank conflicts, lane-private: no barrier) - 32 KB per workgroup of one wave.
// Grid: ceil(n_rows / 64) workgroups of 64 lanes, so that even 4 096 rows spread over 64 compute units.
#include "launch.h"
#include "ql_common.h"

namespace ql {
namespace {

constexpr int GQ_TB = 64;      // rows per workgroup: one wave, one row per lane
constexpr int GQ_CH = 32;      // columns a lane holds in registers at a time (= the int4 group)
constexpr int GQ_BC = 128;     // widest block

// One column step of a row: quantise w, store the three outputs, return err.
template <int BITS>
__device__ __forceinline__ float gptq_step(float w, float s, float d, float* __restrict__ q_out, float* __restrict__ err_out,
                                           float* __restrict__ loss_out) {
#pragma clang fp contract(off)
    constexpr float QMAX = BITS == 4 ? 7.f : 127.f;
    const float x = __fdiv_rn(w, s);
    const float c = fminf(fmaxf(rintf(x), -QMAX), QMAX);
    const float q = __fmul_rn(s, c);
    const float e = __fsub_rn(w, q);
    const float err = __fdiv_rn(e, d);
    *q_out = q;
    *loss_out = __fmul_rn(__fdiv_rn(__fmul_rn(e, e), __fmul_rn(d, d)), 0.5f);
    *err_out = err;
    return err;
}

// Columns [T0, T0 + 32) of the block, the lane's 32 values in registers.
template <int BITS>
__device__ __forceinline__ void gptq_chunk(const float* __restrict__ wrow, const float* __restrict__ H, int64_t ldh, int T0,
                                           float* __restrict__ qrow, float* __restrict__ erow, float* __restrict__ lrow,
                                           float* __restrict__ scale_out, float s, float* errs) {
#pragma clang fp contract(off)
    float w[GQ_CH];
#pragma unroll
    for (int k = 0; k < GQ_CH; ++k) w[k] = wrow[T0 + k];
    // the columns before this chunk, in their order
    for (int j = 0; j < T0; ++j) {
        const float err = errs[j * GQ_TB];
        const float* hr = H + (int64_t)j * ldh + T0;
#pragma unroll
        for (int k = 0; k < GQ_CH; ++k) w[k] = __fsub_rn(w[k], __fmul_rn(err, hr[k]));
    }
    // the triangle inside the chunk
#pragma unroll
    for (int jj = 0; jj < GQ_CH; ++jj) {
        const int j = T0 + jj;
        const float* hr = H + (int64_t)j * ldh + T0;
        __builtin_amdgcn_sched_barrier(0);          // a step's scalar loads stay in the step: hoisted, 496 of them spill
        if (BITS == 4 && jj == 0) {
            float m = 0.f;
#pragma unroll
            for (int k = 0; k < GQ_CH; ++k) m = fmaxf(m, fabsf(w[k]));
            s = fmaxf(__fdiv_rn(m, 7.f), 1e-10f);
            *scale_out = s;
        }
        const float err = gptq_step<BITS>(w[jj], s, hr[jj], qrow + j, erow + j, lrow + j);
        errs[j * GQ_TB] = err;
#pragma unroll
        for (int k = jj + 1; k < GQ_CH; ++k) w[k] = __fsub_rn(w[k], __fmul_rn(err, hr[k]));
    }
}

// The ragged end of an int8 block, columns [T0, T0 + nk) with nk < 32: the same walk as rolled loops, the lane's values in its LDS
// slots wl[k * GQ_TB] - the err slots of these very columns, which nothing reads any more (column counts that are no multiple of
// 32: rare, and small code instead of a second unrolled triangle).
__device__ __forceinline__ void gptq_tail8(const float* __restrict__ wrow, const float* __restrict__ H, int64_t ldh, int T0, int nk,
                                           float* __restrict__ qrow, float* __restrict__ erow, float* __restrict__ lrow, float s,
                                           float* errs, float* wl) {
#pragma clang fp contract(off)
    for (int k = 0; k < nk; ++k) wl[k * GQ_TB] = wrow[T0 + k];
    for (int j = 0; j < T0 + nk; ++j) {
        const float* hr = H + (int64_t)j * ldh + T0;
        float err;
        if (j < T0) {
            err = errs[j * GQ_TB];
        } else {
            err = gptq_step<8>(wl[(j - T0) * GQ_TB], s, hr[j - T0], qrow + j, erow + j, lrow + j);
        }
        for (int k = j < T0 ? 0 : j - T0 + 1; k < nk; ++k) wl[k * GQ_TB] = __fsub_rn(wl[k * GQ_TB], __fmul_rn(err, hr[k]));
    }
}

template <int BITS>
__global__ __launch_bounds__(GQ_TB) void gptq_block_kernel(const float* __restrict__ W, int64_t ldw, int n_rows, int c0, int bc,
                                                           const float* __restrict__ H, int64_t ldh, float* __restrict__ Q,
                                                           float* __restrict__ Err, float* __restrict__ Loss,
                                                           float* __restrict__ scale_w, const float* __restrict__ scale_r,
                                                           int64_t lds) {
    __shared__ float errs_all[GQ_BC * GQ_TB];
    const int lane = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * GQ_TB + lane;
    if (r >= n_rows) return;                       // no barrier anywhere: a lane's LDS slots are its own
    const float* wrow = W + r * ldw + c0;
    float* qrow = Q + r * bc;
    float* erow = Err + r * bc;
    float* lrow = Loss + r * bc;
    float* errs = errs_all + lane;
    const float s8 = BITS == 8 ? scale_r[r] : 0.f;
    int T0 = 0;
    for (; T0 + GQ_CH <= bc; T0 += GQ_CH) {
        float* so = BITS == 4 ? scale_w + (int64_t)((c0 + T0) / GQ_CH) * lds + r : nullptr;
        gptq_chunk<BITS>(wrow, H, ldh, T0, qrow, erow, lrow, so, s8, errs);
    }
    if constexpr (BITS == 8) {
        if (T0 < bc) gptq_tail8(wrow, H, ldh, T0, bc - T0, qrow, erow, lrow, s8, errs, errs + T0 * GQ_TB);
    }
}

}  // namespace

int gptq_block(int bits, const float* W, int64_t n_rows, int64_t ldw, int64_t c0, int64_t bc, const float* H, int64_t ldh, float* Q,
               float* Err, float* Loss, float* scale, int64_t lds, hipStream_t st) {
    const unsigned grid = (unsigned)((n_rows + GQ_TB - 1) / GQ_TB);
    if (bits == 4)
        gptq_block_kernel<4><<<grid, GQ_TB, 0, st>>>(W, ldw, (int)n_rows, (int)c0, (int)bc, H, ldh, Q, Err, Loss, scale, nullptr, lds);
    else
        gptq_block_kernel<8><<<grid, GQ_TB, 0, st>>>(W, ldw, (int)n_rows, (int)c0, (int)bc, H, ldh, Q, Err, Loss, nullptr, scale, lds);
    return finish_launch();
}

}  // namespace ql
