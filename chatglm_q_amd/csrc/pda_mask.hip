// JSON-constrained generation: the mask of a byte-level PUSHDOWN automaton over the vocabulary, applied in place to a step's logits in
// the place qlinear_grammar_mask has (behind the history constraints' launch, in front of the selection kernel): qlinear_pda_mask.
// What grammar_mask.hip keeps per row - byte classes, transition table, accept flags, the current state - plus one bounded stack of
// symbols 1..n_syms: depth comes from the stack, not from the table (chatglm_q_amd/grammar.py: BytePDA, json_grammar).  The automaton is
// deterministic and real-time - one move per byte, no empty moves - so a token's walk is the DFA walk with a stack beside the state.
//
// Per row (include/qlinear_hip.h holds the rules in full), configuration = (s, stack), s = state[b], -1 = dead:
//     0. row_state given and the finished bit set, or n_states <= 0: nothing is read past that, nothing is written
//     1. advance: (s', stack') = walk((s, stack), bytes(tok[b])); tok null, an id outside the table, no bytes: nothing moves; dead stays dead
//     2. one move on byte x: e = table[(s * (n_syms + 1) + top) * n_classes + class_of[x]], top = 0 for an empty stack; bits 0 - 11 the next
//        state (>= n_states: dead), bits 12 - 13 the op (0 none, 1 pop, 2 push, 3 dead), bits 14 - 15 the pushed symbol; a pop at depth 0,
//        a push of symbol 0 or of one > n_syms, a push at depth == max_depth: dead
//     3. the window rule: a walk that holds more than QL_PDA_LOCAL_MAX symbols above the lowest depth it has reached is dead
//     4. mask: -inf into every id other than eos_id whose bytes are empty or die from (s', stack'); -inf into eos_id unless s' is accepting
//        and depth' == 0 (a dead s' leaves it alone)
//     5. state[b], depth[b] and stack[b][low .. depth') - the part the advance changed - stored exactly once per launch
//     6. clamps: n_states, n_syms, max_depth to their caps and to what fits the table; a depth outside [0, max_depth] or a stack symbol
//        outside 1..n_syms read as top: dead
//
// Geometry and the table copy are grammar_mask.hip's: grid ceil(N / PD_CHUNK) x B, every workgroup copies the row's class map, its
// stack (64 bytes) and the LIVE part of the table (n_states * (n_syms + 1) * n_classes entries) into LDS and computes (s', stack')
// itself.  Rule 3 is what keeps a walk in registers: a thread's own pushes sit in ONE 64-bit register, 2 bits per symbol, the top cached in
// another; the row's stack - the LDS copy, rewritten to stack' behind the advance - is read only when a pop goes below the thread's own
// pushes (then the new top comes from it).  No per-thread array, no scratch.  Per byte: two dependent LDS reads (class, transition)
// as in the DFA walk, then the op's integer work on registers - a third dependent LDS read only on a pop into the row's stack.
//
// Rule 5 across workgroups is the DFA kernel's protocol unchanged: every workgroup reads the OLD state, depth and stack in front of
// its own ticket; behind its last logit store, a workgroup barrier and an agent-scope release one thread draws a ticket; the workgroup
// whose ticket is the last stores ITS s', depth' and the changed symbols (all computed the same) and puts the ticket back to 0.  No
// workgroup reads in this launch anything another workgroup of this launch wrote; nothing spins.  Ordinary vector stores.
//
// Every index is clamped (rule 6): s < n_states, top <= n_syms, class < n_classes keep a table index below n_states * (n_syms + 1) *
// n_classes <= QL_GRAMMAR_TABLE_MAX; the row's stack is read at [0, max_depth) with max_depth <= QL_PDA_DEPTH_MAX and written at
// [low, low + own) with low + own <= max_depth; offsets are checked as in the DFA kernel.  A corrupt row masks too much; it never
// indexes out of range.  No logit is read; nothing is stored into an allowed id nor past column N.
//
// Compiler's resource report (gfx950, all three dtypes): 25 VGPRs, no scratch, 33 104 bytes of LDS (4 workgroups per CU).
// Measured (tools/pda_bench.py, profiles/grammar_pda_ab.txt; MI355X, fp16 x 65 024, graph replay, the synthetic vocabulary of
// tools/grammar_bench.py, every launch fed an empty token, all legs alternated in one run; batch 1 / 8 / 32): json_grammar() at its start
// 8.7 / 38.3 / 124.8 us, inside a string value at depth 3 (64 250 ids survive to their last byte) 11.4 / 39.4 / 128.3.  The price of the
// stack machinery on equal work - a lifted DFA through this kernel over the SAME DFA through qlinear_grammar_mask: [A-D] 8.44 against
// 8.11 us (1.04 / 1.04 / 1.00 x at batch 1 / 8 / 32), the flat-JSON pattern at its start 8.36 against 8.17 (1.02 / 1.02 / 0.98 x), inside a
// string value 11.06 against 9.46 (1.17 / 1.07 / 1.09 x); the empty launch 1.75, arg-max 6.1 / 6.4 / 6.6, sampler 17.1 / 17.2 / 17.5.  So the
// fixed part (the stack copy, the clamps, two more barriers) is 0.2 - 0.3 us and the rest grows with the bytes walked: +1.6 us where almost
// every token survives to its last byte - the per-byte work behind the transition read (decoding the op, the compares and selects of
// a move that in these runs never pushes or pops).  Which of those instructions: not attributed.  The growth with the row count is the
// DFA launch's own (a cost per workgroup, grammar_mask.hip), not this kernel's.
#include "launch.h"
#include "ql_common.h"

#include <cmath>

namespace ql {
namespace {

constexpr int PD_TB = 256;
constexpr int PD_CHUNK = QL_GRAMMAR_CHUNK;          // tokens of one workgroup
constexpr int PD_PER = PD_CHUNK / PD_TB;            // ... of one thread
constexpr int PD_TABLE = QL_GRAMMAR_TABLE_MAX;      // uint16 entries of a row's table: 32 KB of LDS
constexpr int PD_STATES = QL_GRAMMAR_STATES_MAX;
constexpr int PD_ACCEPT_LD = QL_GRAMMAR_STATES_MAX + 1;
constexpr int PD_DEPTH = QL_PDA_DEPTH_MAX;
constexpr int PD_LOCAL = QL_PDA_LOCAL_MAX;
constexpr int PD_SYMS = QL_PDA_SYMS_MAX;
constexpr int PD_ROUND = 8;                         // bytes of a token loaded together

// the row's constants behind the clamps
struct Row {
    int ns, nsy, nc, maxd;
};

// a walk's configuration: the state (-1 = dead); `low` symbols of the row's stack (the LDS copy) still beneath the walk's own pushes -
// the lowest depth the walk has reached; `own` pushes of its own, the newest in the low bits of `reg`, 2 bits each; the symbol on top
struct Config {
    int s, low, own, top;
    uint64_t reg;
};

// bytes [o0, o1) of the table from configuration c (c.s in [0, ns), c.top the top of c's stack); c.s = -1 at the first dead move,
// and the rest of c means nothing then.  0 <= o0 <= o1 <= n_bytes.  stk: the row's stack, PD_DEPTH bytes, read below c.low only
__device__ __forceinline__ void walk(const uint16_t* tbl, const uint8_t* cls, const uint8_t* stk, const Row r, Config& c,
                                     const uint8_t* __restrict__ bytes, int o0, int o1) {
    const int per_state = (r.nsy + 1) * r.nc;
    for (int o = o0; o < o1 && c.s >= 0; o += PD_ROUND) {
        uint8_t v[PD_ROUND];
#pragma unroll
        for (int j = 0; j < PD_ROUND; ++j) v[j] = o + j < o1 ? bytes[o + j] : 0;
#pragma unroll
        for (int j = 0; j < PD_ROUND; ++j) {
            if (o + j < o1 && c.s >= 0) {
                // s < ns, top <= nsy, class < nc: below ns * (nsy + 1) * nc <= PD_TABLE
                const int e = tbl[c.s * per_state + c.top * r.nc + cls[v[j]]];
                const int t = e & 0xFFF, op = (e >> 12) & 3, sym = e >> 14;
                bool dead = t >= r.ns || op == 3;
                if (op == 2) {
                    dead |= sym == 0 || sym > r.nsy || c.low + c.own >= r.maxd || c.own >= PD_LOCAL;   // ... the window rule
                    c.reg = (c.reg << 2) | (uint64_t)sym;
                    c.own += 1;
                    c.top = sym;
                } else if (op == 1) {
                    if (c.own > 0) {
                        c.reg >>= 2;
                        c.own -= 1;
                    } else if (c.low > 0) {
                        c.low -= 1;
                    } else {
                        dead = true;
                    }
                    if (c.own > 0) {
                        c.top = (int)(c.reg & 3);
                    } else if (c.low > 0) {                          // the one read of the row's stack: 0 <= low - 1 < maxd <= PD_DEPTH
                        const int y = stk[c.low - 1];
                        dead |= y < 1 || y > r.nsy;
                        c.top = y;
                    } else {
                        c.top = 0;
                    }
                }
                c.s = dead ? -1 : t;
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(PD_TB) void pda_mask_kernel(T* __restrict__ logits, int N, int64_t ldl, const int32_t* __restrict__ tok_off,
                                                         const uint8_t* __restrict__ tok_bytes, int n_tok, int n_bytes,
                                                         const uint8_t* __restrict__ class_of, const uint16_t* __restrict__ table,
                                                         const uint8_t* __restrict__ accept, const int32_t* __restrict__ cfg, int32_t* state,
                                                         int32_t* depth, uint8_t* stack, int32_t* ticket, const int64_t* __restrict__ tok,
                                                         const int32_t* __restrict__ row_state) {
    __shared__ __align__(16) uint16_t tbl[PD_TABLE];
    __shared__ uint8_t cls[256];
    __shared__ uint8_t stk[PD_DEPTH];
    __shared__ int wave_max[PD_TB / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (row_state && (row_state[2 * b + 1] & 1)) return;                  // 0. a finished row (uniform per row: no workgroup draws a ticket)
    Row r;
    r.ns = cfg[4 * b];
    const int eos = cfg[4 * b + 1];
    if (r.ns <= 0) return;                                                // 0. no grammar on this row (uniform per row)
    r.ns = r.ns > PD_STATES ? PD_STATES : r.ns;
    r.nsy = cfg[4 * b + 2];
    r.nsy = r.nsy < 0 ? 0 : (r.nsy > PD_SYMS ? PD_SYMS : r.nsy);
    r.maxd = cfg[4 * b + 3];
    r.maxd = r.maxd < 0 ? 0 : (r.maxd > PD_DEPTH ? PD_DEPTH : r.maxd);

    // the class map (one byte per thread), n_classes = 1 + its largest entry, and the OLD stack
    const int cl = class_of[(int64_t)b * 256 + tid];
    cls[tid] = (uint8_t)cl;
    if (tid < PD_DEPTH) stk[tid] = stack[(int64_t)b * PD_DEPTH + tid];
    int m = cl;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(m, o, 64);
        m = other > m ? other : m;
    }
    if ((tid & 63) == 0) wave_max[tid >> 6] = m;
    // the old state and depth and the fed id's offsets: read by every thread itself, in front of the barrier
    Config c;
    c.s = state[b];
    c.low = depth[b];
    int f0 = 0, f1 = 0;
    if (tok) {
        const int64_t t = tok[b];
        if (t >= 0 && t < (int64_t)N && t < (int64_t)n_tok) {            // outside the table: nothing moves
            f0 = tok_off[t];
            f1 = tok_off[t + 1];
        }
    }
    __syncthreads();
    r.nc = 1;
#pragma unroll
    for (int w = 0; w < PD_TB / 64; ++w) r.nc = wave_max[w] + 1 > r.nc ? wave_max[w] + 1 : r.nc;
    if (r.ns * (r.nsy + 1) * r.nc > PD_TABLE) r.ns = PD_TABLE / ((r.nsy + 1) * r.nc);     // (nc <= 256, 4 tops: at least 16 states stay)
    const int live = r.ns * (r.nsy + 1) * r.nc;
    {
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(table + (int64_t)b * PD_TABLE);
        uint4* dst = reinterpret_cast<uint4*>(tbl);
        for (int i = tid; i < (live + 7) / 8; i += PD_TB) dst[i] = src[i];     // (PD_TABLE % 8 == 0: inside the row's table)
    }

    // 6. the configuration the row holds: a state, a depth or a top symbol out of range is dead
    c.own = 0;
    c.reg = 0;
    c.top = 0;
    if (c.s < 0 || c.s >= r.ns || c.low < 0 || c.low > r.maxd) {
        c.s = -1;
        c.low = 0;
    } else if (c.low > 0) {
        c.top = stk[c.low - 1];                                           // (low - 1 < maxd <= PD_DEPTH)
        if (c.top < 1 || c.top > r.nsy) c.s = -1;
    }
    __syncthreads();

    // 1. advance: every thread walks the fed id itself, all to the same (s', stack')
    if (f1 != f0) {                                                       // (an empty byte string: nothing moves)
        if (f0 < 0 || f1 < f0 || f1 > n_bytes) c.s = -1;                  // corrupt offsets: the row dies
        else if (c.s >= 0) walk(tbl, cls, stk, r, c, tok_bytes, f0, f1);
    }
    // stack' = the old stack's lowest `low` symbols and the advance's own pushes on top: into the LDS copy, behind everyone's reads of it
    const int s1 = c.s, low1 = c.low, own1 = s1 >= 0 ? c.own : 0, d1 = low1 + own1, top1 = c.top;
    __syncthreads();
    if (tid < own1) stk[low1 + tid] = (uint8_t)((c.reg >> (2 * (own1 - 1 - tid))) & 3);   // (low1 + own1 <= maxd <= PD_DEPTH)
    __syncthreads();

    // 4. mask
    T* row = logits + (int64_t)b * ldl;
    const int base = blockIdx.x * PD_CHUNK + tid;
    int o0[PD_PER], o1[PD_PER];
#pragma unroll
    for (int u = 0; u < PD_PER; ++u) {
        const int id = base + u * PD_TB;
        const bool in = id < N && id < n_tok;
        o0[u] = in ? tok_off[id] : 0;
        o1[u] = in ? tok_off[id + 1] : 0;
    }
#pragma unroll
    for (int u = 0; u < PD_PER; ++u) {
        const int id = base + u * PD_TB;
        if (id >= N) continue;
        bool allowed = false;
        if (id == eos) {
            allowed = s1 < 0 || (accept[(int64_t)b * PD_ACCEPT_LD + s1] != 0 && d1 == 0);
        } else if (s1 >= 0 && o0[u] >= 0 && o1[u] > o0[u] && o1[u] <= n_bytes) {
            Config w;
            w.s = s1;
            w.low = d1;
            w.own = 0;
            w.top = top1;
            w.reg = 0;
            walk(tbl, cls, stk, r, w, tok_bytes, o0[u], o1[u]);
            allowed = w.s >= 0;
        }
        if (!allowed) Act<T>::store(row + id, -INFINITY);
    }

    // 5. the ticket: behind this workgroup's last logit store and its reads of the old state, depth and stack
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int drawn = __hip_atomic_fetch_add(ticket + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (drawn == (int)gridDim.x - 1) {                                // the last of the row's workgroups: every one has read the old row
            if (s1 >= 0) {                                                // (a dead row keeps its depth and stack)
                for (int i = 0; i < own1; ++i) stack[(int64_t)b * PD_DEPTH + low1 + i] = stk[low1 + i];
                __hip_atomic_store(depth + b, d1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __hip_atomic_store(state + b, s1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

int pda_mask(int dtype, void* logits, int64_t B, int64_t N, int64_t ldl, const int32_t* tok_off, const uint8_t* tok_bytes, int64_t n_tok,
             int64_t n_bytes, const uint8_t* class_of, const uint16_t* table, const uint8_t* accept, const int32_t* cfg, int32_t* state,
             int32_t* depth, uint8_t* stack, int32_t* ticket, const int64_t* tok, const int32_t* row_state, hipStream_t st) {
    static_assert(PD_TB == 256, "one thread per entry of the class map");
    static_assert(PD_CHUNK % PD_TB == 0 && PD_PER >= 1, "whole tokens per thread");
    static_assert(PD_TABLE % 8 == 0 && PD_TABLE * 2 + 256 + PD_DEPTH + 64 <= 65536, "the table copy: 16-byte words, LDS under the default limit");
    static_assert(PD_LOCAL * 2 <= 64 && PD_SYMS <= 3 && PD_DEPTH <= PD_TB && PD_LOCAL <= PD_TB, "a walk's own pushes: one 64-bit register, 2 bits each");
    static_assert(PD_STATES <= 0xFFF, "a next state is 12 bits, 0xFFF is dead");
    const dim3 grid((unsigned)((N + PD_CHUNK - 1) / PD_CHUNK), (unsigned)B);
#define QL_PDA(TT)                                                                                                                  \
    pda_mask_kernel<TT><<<grid, PD_TB, 0, st>>>((TT*)logits, (int)N, ldl, tok_off, tok_bytes, (int)n_tok, (int)n_bytes, class_of, table, \
                                                accept, cfg, state, depth, stack, ticket, tok, row_state);
    switch (dtype) {
    case QL_DTYPE_F32: QL_PDA(float); break;
    case QL_DTYPE_F16: QL_PDA(f16); break;
    case QL_DTYPE_BF16: QL_PDA(__bf16); break;
    default: return QL_ERR_BAD_DTYPE;
    }
#undef QL_PDA
    return finish_launch();
}

}  // namespace ql
