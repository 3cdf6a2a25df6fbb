// Beam search inside the decode step: the cross-beam selection with its hypothesis bookkeeping (qlinear_beam_advance) and the reorder of
// the key/value cache by parent beam, in place (qlinear_beam_gather).  P prompts x B beams = R batch rows; rows g*B .. g*B+B-1 are group g.
//
// A beam step is the model step's launches plus three:
//   1. qlinear_step_logprobs on a one-slot record per row (cap = 1, n_top = 2B): every row's 2B best ids and their log-probs - the walk
//      and the selection are logprob.hip's, there is no second walk in this file;
//   2. beam_advance_kernel, one workgroup per group: the merge of the group's B x 2B <= 200 candidates (score = beam score + lp, one
//      fp32 add; ranked by counting, as step_logprobs_kernel ranks its list), the walk of the first 2B, the finished heap, done / live,
//      the trellis append, the next tok / parent / beam score, the reset of the candidate records' counts and - with write_index /
//      pos / mask - the decode step's bookkeeping (greedy_advance_kernel's);
//   3. beam_gather_kernel: buf[r, p] <- buf[parent[r], p] for every buffer of a device table of base addresses, every position p in
//      [first, end) and every row r.  A thread owns one chunk of a position across all B rows of a group: it loads all B, then stores
//      those that change - no other thread touches these addresses, so cycles and duplicates in parent need no ordering between
//      threads.  The source is picked by a compare-select chain over statically indexed registers (no dynamically indexed array: that
//      would live in scratch).  A group whose parents are the identity exits behind the B loads of parent.
// The rules (tests/_beam_oracle.py holds them in Python) are stated with the entry points in include/qlinear_hip.h.  Every score is one
// correctly rounded fp32 add or divide: this file is built without multiply-add contraction.
#include "launch.h"
#include "ql_common.h"

namespace ql {
namespace {

constexpr int BEAMS_MAX = 10;
constexpr int BEAM_CAND_MAX = BEAMS_MAX * 2 * BEAMS_MAX;     // candidates of one group
constexpr int BEAM_TB = 256;                                 // one candidate per thread in the ranking
constexpr int BEAM_GATHER_ROUNDS = 8;                        // chunks a gather thread moves when the range is the whole capacity

__device__ __forceinline__ float beam_order_value(float x) { return x != x ? -INFINITY : x; }

__global__ __launch_bounds__(BEAM_TB) void beam_advance_kernel(int B, const int32_t* __restrict__ cand_ids, const float* __restrict__ cand_lp,
                                                               int32_t* __restrict__ cand_count, float* __restrict__ beam_score,
                                                               int64_t* __restrict__ tok, int32_t* __restrict__ parent,
                                                               int32_t* __restrict__ trellis, int cap, int32_t* __restrict__ steps,
                                                               float* __restrict__ fin_score, float* __restrict__ fin_sum,
                                                               int32_t* __restrict__ fin_len, int32_t* __restrict__ fin_row,
                                                               int32_t* __restrict__ fin_count, int32_t* __restrict__ done,
                                                               int32_t* __restrict__ live, const float* __restrict__ norm,
                                                               const int32_t* __restrict__ cfg, int64_t* __restrict__ write_index,
                                                               int64_t* __restrict__ pos, float* __restrict__ mask, int capacity) {
    __shared__ float c_s[BEAM_CAND_MAX], s_s[2 * BEAMS_MAX], n_s[BEAMS_MAX], h_s[BEAMS_MAX];
    __shared__ int s_i[2 * BEAMS_MAX], s_r[2 * BEAMS_MAX], n_i[BEAMS_MAX], n_r[BEAMS_MAX];
    const int tid = threadIdx.x, g = blockIdx.x, r0 = g * B, W = 2 * B, n = B * W;
    const int R = (int)gridDim.x * B;

    // the decode step's bookkeeping for every row, done or not (greedy_advance_kernel's)
    if (pos && tid < B) pos[r0 + tid] += 1;
    if (write_index && g == 0) {                             // the shared write index and every row's mask: one workgroup
        const int64_t nw = write_index[0] + 1;
        __syncthreads();                                     // every thread has read the index
        if (tid == 0) write_index[0] = nw;
        if (nw >= 0 && nw < capacity)
            for (int r = tid; r < R; r += BEAM_TB) mask[(int64_t)r * capacity + nw] = 0.f;
    }

    const int st = steps[g], eos = cfg[0], early = cfg[1];
    const bool idle = done[g] != 0 || st >= cap || st < 0;
    int cnt = fin_count[g];
    cnt = cnt < 0 ? 0 : (cnt > B ? B : cnt);
    if (tid < B) {
        cand_count[r0 + tid] = 0;                            // the one-slot candidate record is free for the next step
        h_s[tid] = fin_score[r0 + tid];
    }
    if (idle) {                                              // a done group (or a full trellis) rides along
        if (tid < B) {
            tok[r0 + tid] = eos >= 0 ? eos : 0;
            parent[r0 + tid] = r0 + tid;
        }
        return;
    }
    float s = 0.f;
    int id = 0;
    if (tid < n) {
        const int r = r0 + tid / W;
        s = beam_score[r] + cand_lp[(int64_t)r0 * W + tid];  // row r's entry k sits at r * W + k = r0 * W + tid
        id = cand_ids[(int64_t)r0 * W + tid];
        c_s[tid] = beam_order_value(s);
    }
    __syncthreads();
    if (tid < n) {                                           // rank by counting: score descending, then (row, in-row rank) = tid ascending
        const float key = c_s[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float o = c_s[j];
            rank += (o > key || (o == key && j < tid)) ? 1 : 0;
        }
        if (rank < W) {
            s_s[rank] = s;
            s_i[rank] = id;
            s_r[rank] = r0 + tid / W;
        }
    }
    __syncthreads();
    if (tid == 0) {                                          // the walk of the first 2B, in order
        const int t = st + 1;                                // tokens the running beams will have generated after this step
        const float nrm = norm[t];
        int filled = 0;
        for (int j = 0; j < W && filled < B; ++j) {
            const float sc = s_s[j];
            const int i = s_i[j], r = s_r[j];
            if (eos >= 0 && i == eos) {
                if (j < B) {                                 // a finished hypothesis; behind rank B it is skipped
                    const float hs = sc / nrm;
                    int slot = -1;
                    if (cnt < B) {
                        slot = cnt++;
                    } else {
                        int worst = 0;
                        for (int q = 1; q < B; ++q) worst = h_s[q] <= h_s[worst] ? q : worst;   // ties: the highest slot
                        if (hs > h_s[worst]) slot = worst;
                    }
                    if (slot >= 0) {
                        h_s[slot] = hs;
                        fin_score[r0 + slot] = hs;
                        fin_sum[r0 + slot] = sc;
                        fin_len[r0 + slot] = t;
                        fin_row[r0 + slot] = r;
                    }
                }
                continue;
            }
            n_i[filled] = i;
            n_r[filled] = r;
            n_s[filled] = sc;
            ++filled;
        }
        for (; filled < B; ++filled) {                       // cannot happen with 2B candidates per row; keeps every output defined
            n_i[filled] = eos >= 0 ? eos : 0;
            n_r[filled] = r0 + filled;
            n_s[filled] = -INFINITY;
        }
        fin_count[g] = cnt;
        bool fin = cnt == B;
        if (fin && !early) {
            int worst = 0;
            for (int q = 1; q < B; ++q) worst = h_s[q] <= h_s[worst] ? q : worst;
            fin = h_s[worst] >= n_s[0] / nrm;
        }
        steps[g] = t;
        if (fin) {
            done[g] = 1;
            atomicSub(live, 1);
        }
    }
    __syncthreads();
    if (tid < B) {
        const int r = r0 + tid;
        tok[r] = n_i[tid];
        parent[r] = n_r[tid];
        beam_score[r] = n_s[tid];
        int32_t* rec = trellis + ((int64_t)st * R + r) * 2;  // st < cap
        rec[0] = n_i[tid];
        rec[1] = n_r[tid];
    }
}

// CT: the chunk a thread moves (16, 4 or 2 bytes); chunks = chunks per position
template <int B, typename CT>
__global__ __launch_bounds__(256) void beam_gather_kernel(const int64_t* __restrict__ table, const int32_t* __restrict__ parent,
                                                          const int32_t* __restrict__ first, const int64_t* __restrict__ end,
                                                          int capacity, int chunks) {
    const int r0 = (int)blockIdx.y * B;
    int pi[B];
    bool ident = true;
#pragma unroll
    for (int i = 0; i < B; ++i) {
        int p = parent[r0 + i] - r0;                         // clamped to the row's own group: a garbage table stays inside the buffers
        p = p < 0 ? 0 : (p > B - 1 ? B - 1 : p);
        pi[i] = p;
        ident = ident && p == i;
    }
    if (ident) return;                                       // the common case late in a search, and every done group
    int64_t lo = first[0], hi = end[0];
    lo = lo < 0 ? 0 : lo;
    hi = hi > capacity ? capacity : hi;
    if (lo >= hi) return;
    const int64_t total = (hi - lo) * chunks, stride = (int64_t)gridDim.x * 256;
    CT* base = reinterpret_cast<CT*>(table[blockIdx.z]);
    const int64_t row_stride = (int64_t)capacity * chunks;
    // the grid covers the capacity in BEAM_GATHER_ROUNDS grid-strided rounds: a short range is served by the first workgroups' first
    // round, workgroups past the range exit
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        CT* at = base + (int64_t)r0 * row_stride + lo * chunks + e;          // position lo + e / chunks, chunk e % chunks
        CT v[B];
#pragma unroll
        for (int i = 0; i < B; ++i) v[i] = at[(int64_t)i * row_stride];
#pragma unroll
        for (int i = 0; i < B; ++i) {
            CT o = v[0];
#pragma unroll
            for (int j = 1; j < B; ++j) o = pi[i] == j ? v[j] : o;
            if (pi[i] != i) at[(int64_t)i * row_stride] = o;
        }
    }
}

template <typename CT>
void launch_gather(int B, dim3 grid, const int64_t* table, const int32_t* parent, const int32_t* first, const int64_t* end, int capacity,
                   int chunks, hipStream_t st) {
#define QL_BEAM_GATHER(BB) \
    case BB: beam_gather_kernel<BB, CT><<<grid, 256, 0, st>>>(table, parent, first, end, capacity, chunks); break
    switch (B) {
        QL_BEAM_GATHER(1); QL_BEAM_GATHER(2); QL_BEAM_GATHER(3); QL_BEAM_GATHER(4); QL_BEAM_GATHER(5);
        QL_BEAM_GATHER(6); QL_BEAM_GATHER(7); QL_BEAM_GATHER(8); QL_BEAM_GATHER(9); QL_BEAM_GATHER(10);
    }
#undef QL_BEAM_GATHER
}

}  // namespace

int beam_advance(int64_t P, int64_t B, const int32_t* cand_ids, const float* cand_lp, int32_t* cand_count, float* beam_score, int64_t* tok,
                 int32_t* parent, int32_t* trellis, int64_t cap, int32_t* steps, float* fin_score, float* fin_sum, int32_t* fin_len,
                 int32_t* fin_row, int32_t* fin_count, int32_t* done, int32_t* live, const float* norm, const int32_t* cfg,
                 int64_t* write_index, int64_t* pos, float* mask, int64_t capacity, hipStream_t st) {
    static_assert(BEAM_CAND_MAX <= BEAM_TB, "one candidate per thread");
    beam_advance_kernel<<<(unsigned)P, BEAM_TB, 0, st>>>((int)B, cand_ids, cand_lp, cand_count, beam_score, tok, parent, trellis, (int)cap,
                                                         steps, fin_score, fin_sum, fin_len, fin_row, fin_count, done, live, norm, cfg,
                                                         write_index, pos, mask, (int)capacity);
    return finish_launch();
}

int beam_gather(const int64_t* table, int64_t n_buf, int64_t P, int64_t B, int64_t capacity, int64_t pos_bytes, const int32_t* parent,
                const int32_t* first, const int64_t* end, hipStream_t st) {
    const int64_t chunk = pos_bytes % 16 == 0 ? 16 : (pos_bytes % 4 == 0 ? 4 : 2);
    const int64_t chunks = pos_bytes / chunk;
    const int64_t per_group = 256 * BEAM_GATHER_ROUNDS;
    const dim3 grid((unsigned)((capacity * chunks + per_group - 1) / per_group), (unsigned)P, (unsigned)n_buf);   // fixed by the capacity: capturable
    if (chunk == 16) launch_gather<u32x4>((int)B, grid, table, parent, first, end, (int)capacity, (int)chunks, st);
    else if (chunk == 4) launch_gather<uint32_t>((int)B, grid, table, parent, first, end, (int)capacity, (int)chunks, st);
    else launch_gather<uint16_t>((int)B, grid, table, parent, first, end, (int)capacity, (int)chunks, st);
    return finish_launch();
}

}  // namespace ql
