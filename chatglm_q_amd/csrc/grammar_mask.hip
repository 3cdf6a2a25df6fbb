// Regex-constrained generation: the mask of a byte-level DFA over the vocabulary, applied in place to a step's logits between the history
// constraints' launch (or the penalties', or lm_head) and the selection kernel (qlinear_grammar_mask).  A row's automaton (chatglm_q_amd/
// grammar.py: byte classes, transition table, accept flags) and its current state live in device memory, the vocabulary is a byte table
// (tok_off, tok_bytes) shared by all rows, and the launch advances the state by the id the step was fed - so it can sit inside a
// captured decode step and one graph serves every pattern.
//
// Per row (include/qlinear_hip.h holds the rules in full), s = state[b], -1 = dead:
//     0. row_state given and the finished bit set, or n_states == 0: nothing is read past that, nothing is written
//     1. advance: s' = walk(s, bytes(tok[b])); tok null, an id outside the table or an empty byte string: s' = s; dead stays dead
//     2. mask: -inf into logits[id] for every id in [0, N) other than eos_id whose bytes are empty or die from s';
//              -inf into logits[eos_id] unless s' is live and accepting (a dead s' leaves it alone: such a row ends)
//     3. state[b] = s', stored exactly once per launch
//
// Geometry: grid ceil(N / GR_CHUNK) x B - batch 1 is the main case, and one workgroup per row would put 65 024 walks on one CU.  Every
// workgroup copies the row's class map and the LIVE part of its table (n_states * n_classes entries, 16 bytes per thread and round)
// into LDS, computes s' itself from the state and the fed id IT read, then walks its own GR_CHUNK tokens: coalesced offset loads, the
// token's bytes GR_ROUND at a time (independent byte loads, one round of L2 latency for almost every token), two dependent LDS reads per
// byte (class, transition), out at the first dead transition.  n_classes is not stored anywhere: it is 1 + the largest entry of the
// row's class map (a wave reduction behind the copy), so a class can never index past the table's live part.
//
// Rule 3 across workgroups: no workgroup reads in this launch anything another workgroup of this launch wrote.  Every workgroup reads
// the OLD state[b]; behind its last logit store, a workgroup barrier and an agent-scope release, one thread draws a ticket (one agent-
// scope atomic add on ticket[b]); the workgroup whose ticket is the last stores ITS s' (all computed the same one) and puts the ticket
// back to 0.  By then every workgroup of the row has read the old state - its read is in front of its own ticket - so none can see
// the new one.  Nothing spins, nothing waits on another workgroup; the next launch's reads are ordered by the kernel boundary.
//
// Every index is clamped: n_states to [0, QL_GRAMMAR_STATES_MAX] and to what fits the table with the row's n_classes, a state or a table
// entry outside [0, n_states) is dead, offsets must satisfy 0 <= off[id] <= off[id + 1] <= n_bytes or the id is masked (the fed id:
// the state dies).  A corrupt table masks too much; it never reads out of range.  No logit is read; nothing is stored into an allowed
// id nor past column N.
//
// Bound: one dependent launch.  Per row it reads 4 (N + 1) bytes of offsets plus the token bytes from L2 (about 0.6 MB for the real
// 65 024-token vocabulary), the DFA copy once per workgroup (at most 32.25 KB, typically under 1 KB), then N short dependent LDS
// chains, one per token, GR_TB of them in flight per workgroup.
// Measured (tools/grammar_bench.py, profiles/grammar_ab.txt; MI355X, fp16 x 65 024, graph replay, a synthetic vocabulary of 65 024
// tokens / 375 KB, batch 1 / 8 / 32): [A-D] 8.2 / 35.4 / 116.9 us, a flat JSON object inside a string value (64 282 ids survive to their
// last byte) 9.4 / 35.4 / 111.2, a counted run of 3 001 states 9.8 / 38.9 / 133.4, a table at the limit (32 KB per workgroup) 9.0 / 38.8 /
// 132.0; the empty launch 1.7, the streaming read of the same bytes 2.0 / 2.6 / 4.2, the arg-max launch 6.2 / 6.5 / 6.9, the sampler's
// 17.2 / 17.4 / 17.7.  At batch 1 the launch is below the sampler's and 1.3 - 1.6 x the arg-max; it does NOT stay there: the time
// grows with the row count, about 4 us per row whatever the pattern - neither the walks (the pattern that kills every token at its
// first byte costs the same) nor the table copy (8 bytes or 32 KB: within 15 %) - so what bounds it at batch 8 and 32 is a cost per
// WORKGROUP (254 per row, 8 128 at batch 32): the suspects are the agent-scope release in front of every ticket and the tickets
// themselves; not attributed (no variant without them, no larger GR_CHUNK measured).  20 VGPRs, no scratch, 33 040 bytes of LDS.
#include "launch.h"
#include "ql_common.h"

#include <cmath>

namespace ql {
namespace {

constexpr int GR_TB = 256;
constexpr int GR_CHUNK = QL_GRAMMAR_CHUNK;          // tokens of one workgroup
constexpr int GR_PER = GR_CHUNK / GR_TB;            // ... of one thread
constexpr int GR_TABLE = QL_GRAMMAR_TABLE_MAX;      // uint16 entries of a row's table: 32 KB of LDS
constexpr int GR_STATES = QL_GRAMMAR_STATES_MAX;
constexpr int GR_ACCEPT_LD = QL_GRAMMAR_STATES_MAX + 1;
constexpr int GR_ROUND = 8;                         // bytes of a token loaded together

// the state after bytes [o0, o1) of the table from state s in [0, ns); -1 at the first dead transition.  0 <= o0 <= o1 <= n_bytes
__device__ __forceinline__ int walk(const uint16_t* tbl, const uint8_t* cls, int ns, int nc, int s, const uint8_t* __restrict__ bytes,
                                    int o0, int o1) {
    for (int o = o0; o < o1 && s >= 0; o += GR_ROUND) {
        uint8_t v[GR_ROUND];
#pragma unroll
        for (int j = 0; j < GR_ROUND; ++j) v[j] = o + j < o1 ? bytes[o + j] : 0;
#pragma unroll
        for (int j = 0; j < GR_ROUND; ++j) {
            if (o + j < o1 && s >= 0) {
                const int t = tbl[s * nc + cls[v[j]]];             // s < ns, class < nc: below ns * nc <= GR_TABLE
                s = t < ns ? t : -1;                                // DEAD (0xFFFF) and anything else past the row's states
            }
        }
    }
    return s;
}

template <typename T>
__global__ __launch_bounds__(GR_TB) void grammar_mask_kernel(T* __restrict__ logits, int N, int64_t ldl, const int32_t* __restrict__ tok_off,
                                                             const uint8_t* __restrict__ tok_bytes, int n_tok, int n_bytes,
                                                             const uint8_t* __restrict__ class_of, const uint16_t* __restrict__ table,
                                                             const uint8_t* __restrict__ accept, const int32_t* __restrict__ cfg,
                                                             int32_t* state, int32_t* ticket, const int64_t* __restrict__ tok,
                                                             const int32_t* __restrict__ row_state) {
    __shared__ __align__(16) uint16_t tbl[GR_TABLE];
    __shared__ uint8_t cls[256];
    __shared__ int wave_max[GR_TB / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (row_state && (row_state[2 * b + 1] & 1)) return;                  // 0. a finished row (uniform per row: no workgroup draws a ticket)
    int ns = cfg[2 * b];
    const int eos = cfg[2 * b + 1];
    if (ns <= 0) return;                                                  // 0. no grammar on this row (uniform per row)
    ns = ns > GR_STATES ? GR_STATES : ns;

    // the class map (one byte per thread) and n_classes = 1 + its largest entry
    const int c = class_of[(int64_t)b * 256 + tid];
    cls[tid] = (uint8_t)c;
    int m = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    if ((tid & 63) == 0) wave_max[tid >> 6] = m;
    // the old state and the fed id's offsets: read by every thread itself, in front of the barrier (the loads overlap the copy)
    int s = state[b];
    int f0 = 0, f1 = 0;
    if (tok) {
        const int64_t t = tok[b];
        if (t >= 0 && t < (int64_t)N && t < (int64_t)n_tok) {            // outside the table: s' = s
            f0 = tok_off[t];
            f1 = tok_off[t + 1];
        }
    }
    __syncthreads();
    int nc = 1;
#pragma unroll
    for (int w = 0; w < GR_TB / 64; ++w) nc = wave_max[w] + 1 > nc ? wave_max[w] + 1 : nc;
    if (ns * nc > GR_TABLE) ns = GR_TABLE / nc;                           // (nc <= 256: at least 64 states stay)
    const int live = ns * nc;
    {
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(table + (int64_t)b * GR_TABLE);
        uint4* dst = reinterpret_cast<uint4*>(tbl);
        for (int i = tid; i < (live + 7) / 8; i += GR_TB) dst[i] = src[i];     // (GR_TABLE % 8 == 0: inside the row's table)
    }
    __syncthreads();

    // 1. advance
    s = (s < 0 || s >= ns) ? -1 : s;
    if (f1 != f0) {                                                       // (an empty byte string: s' = s)
        if (f0 < 0 || f1 < f0 || f1 > n_bytes) s = -1;                    // corrupt offsets: the state dies
        else if (s >= 0) s = walk(tbl, cls, ns, nc, s, tok_bytes, f0, f1);
    }

    // 2. mask
    T* row = logits + (int64_t)b * ldl;
    const int base = blockIdx.x * GR_CHUNK + tid;
    int o0[GR_PER], o1[GR_PER];
#pragma unroll
    for (int u = 0; u < GR_PER; ++u) {
        const int id = base + u * GR_TB;
        const bool in = id < N && id < n_tok;
        o0[u] = in ? tok_off[id] : 0;
        o1[u] = in ? tok_off[id + 1] : 0;
    }
#pragma unroll
    for (int u = 0; u < GR_PER; ++u) {
        const int id = base + u * GR_TB;
        if (id >= N) continue;
        bool allowed = false;
        if (id == eos) {
            allowed = s < 0 || accept[(int64_t)b * GR_ACCEPT_LD + s] != 0;
        } else if (s >= 0 && o0[u] >= 0 && o1[u] > o0[u] && o1[u] <= n_bytes) {
            allowed = walk(tbl, cls, ns, nc, s, tok_bytes, o0[u], o1[u]) >= 0;
        }
        if (!allowed) Act<T>::store(row + id, -INFINITY);
    }

    // 3. the ticket: behind this workgroup's last logit store and its read of the old state
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int drawn = __hip_atomic_fetch_add(ticket + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (drawn == (int)gridDim.x - 1) {                                // the last of the row's workgroups: every one has read the old state
            __hip_atomic_store(state + b, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

int grammar_mask(int dtype, void* logits, int64_t B, int64_t N, int64_t ldl, const int32_t* tok_off, const uint8_t* tok_bytes, int64_t n_tok,
                 int64_t n_bytes, const uint8_t* class_of, const uint16_t* table, const uint8_t* accept, const int32_t* cfg, int32_t* state,
                 int32_t* ticket, const int64_t* tok, const int32_t* row_state, hipStream_t st) {
    static_assert(GR_TB == 256, "one thread per entry of the class map");
    static_assert(GR_CHUNK % GR_TB == 0 && GR_PER >= 1, "whole tokens per thread");
    static_assert(GR_TABLE % 8 == 0 && GR_TABLE * 2 + 256 + 64 <= 65536, "the table copy: 16-byte words, LDS under the default limit");
    const dim3 grid((unsigned)((N + GR_CHUNK - 1) / GR_CHUNK), (unsigned)B);
#define QL_GRAMMAR(TT)                                                                                                              \
    grammar_mask_kernel<TT><<<grid, GR_TB, 0, st>>>((TT*)logits, (int)N, ldl, tok_off, tok_bytes, (int)n_tok, (int)n_bytes, class_of, \
                                                    table, accept, cfg, state, ticket, tok, row_state);
    switch (dtype) {
    case QL_DTYPE_F32: QL_GRAMMAR(float); break;
    case QL_DTYPE_F16: QL_GRAMMAR(f16); break;
    case QL_DTYPE_BF16: QL_GRAMMAR(__bf16); break;
    default: return QL_ERR_BAD_DTYPE;
    }
#undef QL_GRAMMAR
    return finish_launch();
}

}  // namespace ql
