// The controls that depend on the ORDER of a row's tokens, applied in place to a step's logits between lm_head (behind
// qlinear_logit_penalties when that is armed) and the selection kernel (qlinear_history_constraints): no-repeat n-grams, banned
// multi-token sequences, stop sequences and a minimum length.  The row's history - its real prompt ids, then its generated ids - is
// kept in device memory and advanced by the same launch, so the launch can sit inside a captured decode step.
//
// Per row (include/qlinear_hip.h holds the rules in full), L = history length, P = prompt length, g = L - P:
//     0. row_state given and the finished bit set: nothing is read past that bit, nothing is written
//     1. append tok[b] at hist[L] (tok null or L == hist_ld: no append)
//     2. row_state given: a STOP sequence of length m <= g equal to hist[L-m : L] sets the finished bit, takes one off `live`; done
//     3. -inf into logits[id] for every id in [0, N) that
//          the n-gram rule names: hist[i+n-1] for every i in [0, L-n] with hist[i : i+n-1] == hist[L-n+1 : L]
//          a BAN sequence names:  its last id, when the m-1 ids in front of it are the last m-1 of the history
//          a MIN entry names:     its id, while g < min_new
//
// One workgroup per row.  The last HC_TAIL ids of the history (every rule compares against a suffix of them) go to LDS once; the
// sequence table is served by the first threads, one sequence each; the n-gram scan strides the threads over the history positions
// with coalesced int32 loads and compares the window's first id before anything else, which rejects almost every position.  The
// append: every thread reads hist_len[b] and tok[b] itself and substitutes the id for position L (hist_at) - no thread reads the
// appended id from memory - and thread 0 stores the id and the new length only BEHIND the kernel's first barrier, which every thread
// crosses after its own load of the length: a wave that starts late cannot see the length already moved.  Several lanes may store the
// same -inf to one address; no logit is read.  Every logits index
// is range-checked in the thread that stores (ban), every history index is below the clamped L.
//
// Bound: one dependent launch; the scan reads 4 x L bytes of L2-resident history per row (32 KB at 8 128 positions): 32 loads per
// thread at that length, HC_SCAN of them in flight at a time - rounds of L2 latency in one workgroup, not traffic.
#include "launch.h"
#include "ql_common.h"

#include <cmath>

namespace ql {
namespace {

constexpr int HC_TB = 256;
constexpr int HC_SCAN = 4;              // history positions a thread has in flight in the n-gram scan
constexpr int HC_SEQS = 32;              // QL_CONSTRAINT_SEQS_MAX (include/qlinear_hip.h)
constexpr int HC_TAIL = 16;              // QL_CONSTRAINT_SEQ_LEN_MAX: the longest sequence, the largest n
constexpr int HC_BAN = 0, HC_STOP = 1, HC_MIN = 2;

template <typename T>
__device__ __forceinline__ void ban(T* __restrict__ row, int N, int id) {
    if (id >= 0 && id < N) Act<T>::store(row + id, -INFINITY);
}

template <typename T>
__global__ __launch_bounds__(HC_TB) void history_constraints_kernel(T* __restrict__ logits, int N, int64_t ldl, int32_t* __restrict__ hist,
                                                                    int hist_ld, int32_t* __restrict__ hist_len,
                                                                    const int32_t* __restrict__ prompt_len, const int32_t* __restrict__ cfg,
                                                                    const int32_t* __restrict__ seq_tok, const int32_t* __restrict__ seq_len,
                                                                    const int32_t* __restrict__ seq_kind, const int32_t* __restrict__ seq_count,
                                                                    const int64_t* __restrict__ tok, int32_t* __restrict__ row_state,
                                                                    int32_t* __restrict__ live) {
    __shared__ int32_t tail[HC_TAIL];                                     // tail[j] = hist[L - HC_TAIL + j] (j with a position >= 0)
    const int b = blockIdx.x, tid = threadIdx.x;
    if (row_state && (row_state[2 * b + 1] & 1)) return;                  // 0. a finished row (uniform per block)

    int32_t* hrow = hist + (int64_t)b * hist_ld;
    int L = hist_len[b];
    L = L < 0 ? 0 : (L > hist_ld ? hist_ld : L);
    // 1. append: every thread knows the id and where it goes; thread 0 stores both behind the barrier below.  An id that no int32
    // holds is stored as -1
    int app = -1;                                                         // the position whose value is `fed`, not yet in memory
    int32_t fed = 0;
    if (tok && L < hist_ld) {
        const int64_t t = tok[b];
        fed = (t < (int64_t)INT32_MIN || t > (int64_t)INT32_MAX) ? -1 : (int32_t)t;
        app = L;
        L += 1;
    }
    auto hist_at = [&](int i) -> int32_t { return i == app ? fed : hrow[i]; };   // i in [0, L)

    int n = cfg[2 * b], n_seq = seq_count[b];
    const int min_new = cfg[2 * b + 1];
    n = n < 0 ? 0 : (n > HC_TAIL ? HC_TAIL : n);
    n_seq = n_seq < 0 ? 0 : (n_seq > HC_SEQS ? HC_SEQS : n_seq);
    const bool armed = n != 0 || n_seq != 0;                              // (uniform per block)
    if (armed && tid < HC_TAIL) {
        const int i = L - HC_TAIL + tid;
        tail[tid] = i >= 0 ? hist_at(i) : -1;                             // (a slot in front of the history is never compared)
    }
    // every thread has its own copy of the length by now: only behind this barrier may the length in memory move
    __syncthreads();
    if (app >= 0 && tid == 0) {
        hrow[app] = fed;
        hist_len[b] = L;
    }
    if (!armed) return;                                                   // nothing armed: the row appends and is done

    int P = prompt_len[b];
    P = P < 0 ? 0 : (P > L ? L : P);
    const int g = L - P;

    // this thread's sequence (threads 0 .. n_seq-1): does the history end with all of it, or with all but its last id?
    int kind = -1, m = 0, first_id = -1, last_id = -1;
    bool ends_with_head = false, ends_with_all = false;
    if (tid < n_seq) {
        const int s = b * HC_SEQS + tid;
        m = seq_len[s];
        m = m < 0 ? 0 : (m > HC_TAIL ? HC_TAIL : m);
        kind = seq_kind[s];
        if (m > 0) {
            const int32_t* sq = seq_tok + (int64_t)s * HC_TAIL;
            first_id = sq[0];
            last_id = sq[m - 1];
            if (L >= m - 1) {                                             // hist[L-m+1 : L] == seq[: m-1]
                bool eq = true;
                for (int j = 0; j < m - 1; ++j) eq &= tail[HC_TAIL - (m - 1) + j] == sq[j];
                ends_with_head = eq;
            }
            if (g >= m) {                                                 // hist[L-m : L] == seq, all of it generated
                bool eq = true;
                for (int j = 0; j < m; ++j) eq &= tail[HC_TAIL - m + j] == sq[j];
                ends_with_all = eq;
            }
        }
    }
    // 2. stop
    if (row_state) {
        if (__syncthreads_or(kind == HC_STOP && ends_with_all)) {
            if (tid == 0) {
                row_state[2 * b + 1] |= 1;                                // this launch owns the row's flags word: one thread per row
                atomicSub(live, 1);
            }
            return;
        }
    }
    // 3. bans
    T* row = logits + (int64_t)b * ldl;
    if (m > 0) {
        if (kind == HC_BAN && ends_with_head) ban(row, N, last_id);       // (m == 1: an empty head always matches)
        if (kind == HC_MIN && g < min_new) ban(row, N, first_id);
    }
    if (n == 0 || L < n) return;                                          // L < n: the range [0, L - n] is empty
    const int w = n - 1;                                                  // the window: hist[i : i+w] against the last w ids
    const int32_t key0 = w > 0 ? tail[HC_TAIL - w] : 0;
    const int last = L - n;                                               // i <= last: i + n - 1 <= L - 1
    for (int i0 = tid; i0 <= last; i0 += HC_SCAN * HC_TB) {
        int32_t first[HC_SCAN];                                           // HC_SCAN positions in flight: a round's loads are issued together
#pragma unroll
        for (int u = 0; u < HC_SCAN; ++u) {
            const int i = i0 + u * HC_TB;
            first[u] = i <= last ? hist_at(i) : 0;
        }
#pragma unroll
        for (int u = 0; u < HC_SCAN; ++u) {
            const int i = i0 + u * HC_TB;
            if (i > last) continue;
            if (w == 0) {                                                 // n = 1: every id of the history
                ban(row, N, first[u]);
                continue;
            }
            if (first[u] != key0) continue;
            bool eq = true;
            for (int j = 1; j < w; ++j) eq &= hist_at(i + j) == tail[HC_TAIL - w + j];
            if (eq) ban(row, N, hist_at(i + w));
        }
    }
}

}  // namespace

int history_constraints(int dtype, void* logits, int64_t B, int64_t N, int64_t ldl, int32_t* hist, int64_t hist_ld, int32_t* hist_len,
                        const int32_t* prompt_len, const int32_t* cfg, const int32_t* seq_tok, const int32_t* seq_len,
                        const int32_t* seq_kind, const int32_t* seq_count, const int64_t* tok, int32_t* row_state, int32_t* live,
                        hipStream_t st) {
    static_assert(HC_SEQS == QL_CONSTRAINT_SEQS_MAX && HC_TAIL == QL_CONSTRAINT_SEQ_LEN_MAX && HC_SEQS <= HC_TB && HC_TAIL <= HC_TB,
                  "sequence table: one thread per sequence, one per tail slot");
    static_assert(HC_BAN == QL_CONSTRAINT_BAN && HC_STOP == QL_CONSTRAINT_STOP && HC_MIN == QL_CONSTRAINT_MIN, "sequence kinds");
#define QL_CONSTRAINTS(TT)                                                                                                         \
    history_constraints_kernel<TT><<<dim3((unsigned)B), HC_TB, 0, st>>>((TT*)logits, (int)N, ldl, hist, (int)hist_ld, hist_len,     \
                                                                        prompt_len, cfg, seq_tok, seq_len, seq_kind, seq_count, tok, \
                                                                        row_state, live);
    switch (dtype) {
    case QL_DTYPE_F32: QL_CONSTRAINTS(float); break;
    case QL_DTYPE_F16: QL_CONSTRAINTS(f16); break;
    case QL_DTYPE_BF16: QL_CONSTRAINTS(__bf16); break;
    default: return QL_ERR_BAD_DTYPE;
    }
#undef QL_CONSTRAINTS
    return finish_launch();
}

}  // namespace ql
