/* qlinear_hip.h - C ABI of libqlinear_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the quantized-linear forward path of K024/chatglm-q.  Each entry point
 * replaces one host->device launch site of the reference (paths relative to the reference
 * checkout):
 *
 *   qlinear_w4g32_fwd / _fwd_packed  <- dynamic_quant_matmul_s4      chatglm_q/int4/triton_ops.py:90-139
 *                                       (kernel _dynamic_quant_matmul_s4_kernel, :18-87)
 *   qlinear_w8_fwd                   <- dynamic_quant_matmul         chatglm_q/int8/triton_ops.py:87-127
 *                                       (kernel _dynamic_quant_matmul_kernel, :13-84)
 *   qlinear_act_quant_i8_rowwise,
 *   qlinear_w8a8_fwd                 <- the int8-activation semantic that exists only in
 *                                       DynamicQuantizeMatMul.symbolic chatglm_q/int8/qlinear.py:56-70
 *                                       and quantize_int8           chatglm_q/int8/quantizer.py:11-19
 *   qlinear_qembedding_*             <- QEmbedding.forward           chatglm_q/int4/qlinear.py:122-131,
 *                                                                    chatglm_q/int8/qlinear.py:118-120
 *
 * Conventions
 *   - plain C types only; all pointers are DEVICE pointers unless stated; the library never
 *     allocates, frees or retains them; the caller owns outputs and workspaces.
 *   - every launch goes to the hipStream_t passed in (as void*); no hidden synchronisation,
 *     no use of the default stream, no mutable global state apart from an idempotent
 *     per-process device-property cache.  Thread-safe.
 *   - return value: 0 = OK; < 0 = argument error (QL_ERR_*); > 0 = hipError_t of the launch.
 *     Nothing is thrown across the ABI, nothing aborts.
 *   - dtype: activation / scale / bias / output element type (QL_DTYPE_*); scales, bias and the
 *     output always have the activation dtype, as the reference asserts
 *     (chatglm_q/int4/triton_ops.py:108).
 *   - rounding: every dequantised weight is rounded to the activation dtype before it is
 *     multiplied, products accumulate in fp32, the sum is rounded once to the activation dtype,
 *     and the optional bias is added after that rounding (a second rounding) - the reference's
 *     exact sequence (chatglm_q/int4/triton_ops.py:72-80, chatglm_q/int4/qlinear.py:92-93).
 */
#ifndef QLINEAR_HIP_H
#define QLINEAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): qlinear_w4g32_fwd_packed_residual gained `flags` in front of `stream` (round 3); qlinear_last_dispatch /
 * qlinear_dispatch_reset / qlinear_dispatch_reload / qlinear_gemm256_serves / qlinear_tiled_dispatch added; the experimental entry points (one-launch MLP pair / persistent MLP
 * engine / W4A8) moved to include/qlinear_hip_dev.h and libqlinear_hip_dev.so. */
/* 3 (round 6): qlinear_top_p_sample added; round 5's additions (qlinear_w4g32_unpack_gemv, qlinear_dispatch_flags,
 * qlinear_w4g32_packed_dispatch, QL_K code 19 = ROWS16, qlinear_gated_serves weight_bits 88 = int8 x int8) had gone out under 2.
 * Still 3: qlinear_token_logprob added - purely additive, no existing entry point changed its signature or its meaning.
 * Still 3: qlinear_batch_sample_advance added - purely additive as well.
 * Still 3: qlinear_logit_penalties (and the constant QL_LOGIT_BIAS_MAX) added - purely additive; the selection entry points
 * (qlinear_greedy_advance, qlinear_top_p_sample, qlinear_batch_sample_advance) are unchanged, they read the adjusted logits.
 * Still 3: qlinear_gptq_block added - purely additive.
 * Still 3: qlinear_step_logprobs (and the constant QL_TOP_LOGPROBS_MAX) added - purely additive; qlinear_token_logprob and the
 * selection entry points are unchanged.
 * Still 3: qlinear_w4g32_onetile_launches and the QLINEAR_DISPATCH family `noonetile` (flag bit 8) added - purely additive.
 * Still 3: qlinear_history_constraints (and the constants QL_CONSTRAINT_SEQS_MAX, QL_CONSTRAINT_SEQ_LEN_MAX, QL_CONSTRAINT_BAN / _STOP /
 * _MIN) added - purely additive; qlinear_logit_penalties and the selection entry points are unchanged.
 * Still 3: qlinear_w4g32_onetile_kc_launches added - purely additive.
 * Still 3: qlinear_beam_advance and qlinear_beam_gather (and the constant QL_BEAMS_MAX) added - purely additive; qlinear_step_logprobs, which
 * supplies their candidates, is unchanged.
 * Still 3: qlinear_grammar_mask (and the constants QL_GRAMMAR_TABLE_MAX, QL_GRAMMAR_STATES_MAX, QL_GRAMMAR_CHUNK) added - purely additive;
 * qlinear_history_constraints and the selection entry points are unchanged, they read the masked logits.
 * Still 3: qlinear_pda_mask (and the constants QL_PDA_DEPTH_MAX, QL_PDA_LOCAL_MAX, QL_PDA_SYMS_MAX) added - purely additive;
 * qlinear_grammar_mask is unchanged, a call takes the one or the other launch. */
#define QLINEAR_ABI_VERSION 3

/* activation dtypes */
#define QL_DTYPE_F32 0
#define QL_DTYPE_F16 1
#define QL_DTYPE_BF16 2

/* status codes */
#define QL_OK 0
#define QL_ERR_NULL_POINTER (-1)
#define QL_ERR_BAD_SHAPE (-2)      /* M/N/K <= 0, K odd, K % group != 0, ld* too small */
#define QL_ERR_BAD_DTYPE (-3)
#define QL_ERR_BAD_GROUP (-4)      /* group size unsupported by this entry point */
#define QL_ERR_MISALIGNED (-5)     /* pointer / leading dimension breaks the alignment contract */
#define QL_ERR_WORKSPACE (-6)      /* workspace missing or too small (see qlinear_workspace_bytes) */
#define QL_ERR_UNSUPPORTED (-7)

/* flags (bit set) accepted by the forward entry points that take a `flags` argument */
#define QL_FLAG_STRICT_ROUNDING 1  /* round every dequantised weight to the activation dtype before the
                                      multiply, bit-for-bit the reference's sequence.  Default (0) feeds
                                      the exactly dequantised weight to the dot product instead, which is
                                      closer to real arithmetic and differs from the reference only by that
                                      per-weight rounding (~2e-4 relative in fp16; within the 1e-3 bar). */

#define QL_FLAG_ACT_PER_TENSOR 2    /* activation quantisation: ONE scale max|A| / 127 for the whole (M, K) tensor - the per-tensor
                                      symmetric variant of DynamicQuantizeMatMul.symbolic's second branch
                                      (chatglm_q/int8/qlinear.py:64-70: ReduceMax(Abs(A)) / 127, QuantizeLinear with zero
                                      point 0) - instead of one scale per row (quantize_int8, chatglm_q/int8/quantizer.py:
                                      11-19).  a_scale still has M entries (all equal), so the GEMM epilogue is unchanged. */

/* operations, for qlinear_workspace_bytes */
#define QL_OP_W4G32_FWD 1
#define QL_OP_W4G32_FWD_PACKED 2
#define QL_OP_W8_FWD 3
#define QL_OP_W8A8_FWD 4
#define QL_OP_W8_FWD_TILED 5
#define QL_OP_W8A8_LINEAR_TILED 6  /* REQUIRED by qlinear_w8a8_linear_tiled: the int8 activations and their scales */
#define QL_OP_W4A8_LINEAR 7        /* REQUIRED by qlinear_w4a8_linear: the same */

int qlinear_abi_version(void);
const char* qlinear_status_string(int status);

/* Number of kernel launches this process has issued through the library (monotonic, relaxed).
 * Lets a caller prove that a result came from the HIP path and not from any fallback. */
uint64_t qlinear_launch_count(void);

/* Debug query: WHICH kernel families the calling thread's library calls launched since qlinear_dispatch_reset(): one byte per
 * launch, newest in the low byte, up to 8 launches (older ones fall off).  tests/test_dispatch_sweep_gpu.py asserts with it that
 * the kernel really changes where the dispatch tables say it does.  Thread-local, no synchronisation, no effect on results. */
#define QL_K_OTHER 1            /* repacks, norms, attention, embeddings, quantisers, ... */
#define QL_K_W4_GEMV 2          /* w4_packed.hip: 1..2 rows (4 per pass), part 1 */
#define QL_K_W4_ROWS4 3         /* w4_rows4.hip: 2..4 rows on v_mfma_f32_4x4x4, part 1 */
#define QL_K_W4_FEWROW 4        /* w4_fewrow.hip: 3..32 rows not served by QL_K_W4_ROWS16, part 2 */
#define QL_K_W4_GEMM128 5       /* w4_gemm.hip: 32..128-row tiles, part 2 (+ QL_K_SPLITK_REDUCE for few rows) */
#define QL_K_W4_GEMM256 6       /* w4_gemm256.hip: 256 x 256 tiles, part 2 */
#define QL_K_W4_CANON 7         /* w4_kernels.hip: canonical layout, split-K */
#define QL_K_W4_GENERIC 8       /* w4_kernels.hip: any group size / alignment */
#define QL_K_SPLITK_REDUCE 9
#define QL_K_W8_GEMV 10         /* w8_kernels.hip: up to 4 rows per pass on the (N, K) buffer */
#define QL_K_W8_FEWROW 11       /* w8_gemm.hip: 3..32 rows, tile-major copy */
#define QL_K_W8_GEMM128 12      /* w8_gemm.hip: 32..128-row tiles (row-major or tile-major weights) */
#define QL_K_W8_GEMM256 13      /* w4_gemm256.hip<W8>: 256 x 256 tiles, tile-major copy */
#define QL_K_W8_GENERIC 14
#define QL_K_W8A8_ROWMAJOR 15   /* w8_kernels.hip: round 1's i8 x i8 kernel on the (N, K) buffer */
#define QL_K_W8A8_TILED 16      /* w8a8.hip: 64 / 128-row tiles, tile-major copy */
#define QL_K_W8A8_GEMM256 17    /* w8a8_gemm256.hip */
#define QL_K_ACT_QUANT 18
#define QL_K_W4_ROWS16 19       /* w4_rows16.hip: 3..16 rows on v_mfma_f32_16x16x32, part 1, one launch */
uint64_t qlinear_last_dispatch(void);
/* Launches of the one-tile one-row int4g32 GEMV (QL_K_W4_GEMV's straight-line kernel) since the library was loaded: which of the two
 * GEMV kernels served a call is not visible in its family code. */
uint64_t qlinear_w4g32_onetile_launches(void);
/* ... of them, launches of its K-complete geometry (two K slices, every wave owns whole columns and stores them itself). */
uint64_t qlinear_w4g32_onetile_kc_launches(void);
void qlinear_dispatch_reset(void);
void qlinear_dispatch_reload(void);   /* parse QLINEAR_DISPATCH again (it is read once, at the first dispatch decision) */
/* The parsed QLINEAR_DISPATCH switches as the library holds them (bit 0 no256, 1 nopeel, 2 nofewrow, 3 norows4, 4 nogroupattn,
 * 5 nohalf, 6 nof32mfma, 7 norows16, 8 noonetile): a host that sizes a workspace or picks an entry point by one of them asks here instead of parsing the variable again. */
unsigned qlinear_dispatch_flags(void);

/* Environment variables read by THIS library (chatglm_q_amd/csrc/tune.h): exactly one,
 *   QLINEAR_DISPATCH = comma list of kernel families the dispatch must not use: no256, nopeel, nofewrow, norows4, nogroupattn,
 *   nohalf (the half-tile last round inside the int4g32 256-tile GEMM's launch: whole tiles only, the older peel where it applies),
 *   nof32mfma (the fp32 matrix-instruction kernel that serves fp32 activations from 128 rows on: the VALU kernels instead),
 *   norows16 (the one-launch 3..16-row kernel on part 1: the few-row kernel on part 2 instead),
 *   noonetile (the straight-line one-row int4g32 GEMV that serves K slices of one 64-group tile: the tile-loop kernel instead, bit-equal)
 * (every family has a slower fallback computing the same function; for A/B measurements and triage).  The host package reads
 * QLINEAR_LIB_PATH (another build of this library) and QLINEAR_STRICT (0 / 1 / auto: the per-weight rounding policy, see
 * QL_FLAG_STRICT_ROUNDING) - chatglm_q_amd/_lib.py.  Every other tuning value is a compile-time constant with its measurement
 * cited at its use; the developer build (make dev, -DQL_DEV_TUNING) turns them back into environment variables. */

/* Bytes of scratch the op wants for this shape (0 = none).  The caller allocates it (e.g. from
 * torch's caching allocator so stream semantics hold) and passes it to the op.  It is REQUIRED by
 * QL_OP_W4G32_FWD (QL_ERR_WORKSPACE otherwise) and OPTIONAL for QL_OP_W4G32_FWD_PACKED / QL_OP_W8_FWD[_TILED] / QL_OP_W8A8_FWD,
 * where it lets a few-row (5 <= M < ~256) MFMA GEMM split K over workgroups into fp32 slabs that a
 * second launch sums; without it (NULL / too small / not 16-byte aligned) those shapes run unsplit -
 * same rounding sequence, several times slower. */
size_t qlinear_workspace_bytes(int op, int64_t M, int64_t N, int64_t K, int64_t group);

/* ---- int4 group-quantised weights, canonical (reference) layout ---------------------------
 * A   (M, K) activations, row stride lda elements, unit inner stride
 * Wq  (K/2, N) uint8, contiguous; byte [k/2, n] = row 2*(k/2) low nibble, row 2*(k/2)+1 high
 *     nibble; stored nibble = q + 8 (chatglm_q/int4/quantizer.py:24-28)
 * S   (K/group, N) scales, contiguous, activation dtype
 * bias (N) or NULL;  C (M, N) row stride ldc
 * Any group size dividing K is accepted; group == 32 with N % 8 == 0 takes the fast kernels. */
int qlinear_w4g32_fwd(const void* A, const uint8_t* Wq, const void* S, const void* bias, void* C,
                      int64_t M, int64_t N, int64_t K, int64_t group, int64_t lda, int64_t ldc,
                      int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the int4g32 product w.r.t. the activations (the weights are frozen integers):
 *   dA (M, K) = Gout (M, N) . dequant(Wq, S)^T      canonical layout, group 32, fp16 / bf16, N % 16 == 0
 * Same arithmetic as the reference's transposed kernel (every weight rounded to the activation dtype, fp32
 * accumulation, one output rounding).  Replaces dynamic_quant_matmul_transposed_s4
 * (chatglm_q/int4/triton_ops.py:142-264) behind DynamicQuantizeMatMul.backward (chatglm_q/int4/qlinear.py:53-64);
 * unlike the reference's kernel it does not need power-of-two sizes (triton_ops.py:246). */
int qlinear_w4g32_bwd_input(const void* Gout, const uint8_t* Wq, const void* S, void* dA, int64_t M, int64_t N, int64_t K,
                            int64_t group, int64_t ldg, int64_t ldda, int dtype, void* stream);

/* ---- int4 g32, derived layout ---------------------------------------------------------------
 * A lazily built, non-persistent re-arrangement of the SAME weights, two copies in one buffer:
 *   part 1, column-major (rows <= 2, GEMV): the 32 nibbles of one (column, group) in one 16-byte unit,
 *           units K-contiguous per column, scales regrouped per 4 columns - one wave owns whole output
 *           columns and no cross-workgroup reduction is needed;
 *   part 2, tile-major (rows >= 3, MFMA kernels): the same units ordered [column / 32][64-deep K step][lane],
 *           i.e. in the order the lanes of a wave feed their MFMA fragments (1 KB contiguous per load).
 * Built once per weight by qlinear_w4g32_repack from the canonical buffers, which remain the source of truth
 * (state_dict).  group must be 32.  Exact offsets: chatglm_q_amd/csrc/launch.h (W4Layout). */
size_t qlinear_w4g32_packed_bytes(int64_t N, int64_t K, int64_t group, int dtype);
int qlinear_w4g32_repack(const uint8_t* Wq, const void* S, void* packed, int64_t N, int64_t K,
                         int64_t group, int dtype, void* stream);
int qlinear_w4g32_fwd_packed(const void* A, const void* packed, const void* bias, void* C,
                             int64_t M, int64_t N, int64_t K, int64_t group, int64_t lda,
                             int64_t ldc, int dtype, int flags, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The two parts as two allocations, so that a weight which never sees three or more rows (decode-only sessions, fp32)
 * never pays for part 2: part 1 ("gemv", qlinear_w4g32_gemv_bytes) is what qlinear_w4g32_fwd_packed reads for M <= 2
 * and every one-row fused / residual entry point reads; part 2 ("tiled", qlinear_w4g32_tiled_bytes; 0 for fp32, which
 * has no MFMA path) is built FROM part 1 by qlinear_w4g32_tile and serves any row count through
 * qlinear_w4g32_fwd_tiled (the few-row and MFMA GEMM kernels; workspace: qlinear_workspace_bytes(QL_OP_W4G32_FWD_PACKED)).
 * gemv_bytes + tiled_bytes == packed_bytes, and a buffer of qlinear_w4g32_repack is exactly gemv followed by tiled.
 * The host module (chatglm_q_amd/int4/qlinear.py) builds part 2 on the first forward with >= 3 rows. */
/* 1 when qlinear_w4g32_fwd_packed serves this call from part 2 (a caller that keeps the parts apart then calls
 * qlinear_w4g32_fwd_tiled), 0 when part 1 does: one or two rows (GEMV), 2..4 rows in the default arithmetic on the 4x4x4
 * matrix instruction while the staged rows stay within 64 KB (w4_rows4.hip), 3..16 rows of the narrow layer shapes on the
 * 16x16x32 matrix instruction in one launch (w4_rows16.hip: the rule is at rows16_cfg there), fp32 at any row count. */
int qlinear_w4g32_rows_on_tiled(int64_t M, int64_t N, int64_t K, int dtype, int flags);
/* The QL_K_* family that serves such a call from part 1 (QL_K_W4_GEMV / QL_K_W4_ROWS4 / QL_K_W4_ROWS16), 0 when part 2 serves it. */
int qlinear_w4g32_packed_dispatch(int64_t M, int64_t N, int64_t K, int dtype, int flags);
/* 1 when qlinear_w4g32_fwd_tiled_gated (weight_bits 4) / qlinear_w8_fwd_tiled_gated (weight_bits 8) / qlinear_w8a8_fwd_tiled_gated
 * (weight_bits 88: int8 activations x int8 weights, the ring kernel's own rule) serves M rows of a first MLP
 * projection (N = 2 * hidden outputs) with SiLU * gate in its epilogue, 0 when it would return QL_ERR_UNSUPPORTED for the shape:
 * lets a host ask BEFORE it builds the gate-interleaved tile-major copy (~120 MB per ChatGLM2-6B layer). */
int qlinear_gated_serves(int64_t M, int64_t N, int64_t K, int dtype, int weight_bits);
size_t qlinear_w4g32_gemv_bytes(int64_t N, int64_t K, int64_t group, int dtype);
size_t qlinear_w4g32_tiled_bytes(int64_t N, int64_t K, int64_t group, int dtype);
int qlinear_w4g32_repack_gemv(const uint8_t* Wq, const void* S, void* gemv, int64_t N, int64_t K, int64_t group, int dtype,
                              void* stream);
/* The inverse of qlinear_w4g32_repack_gemv (round 5): part 1 -> the canonical buffers Wq (K / 2, N) uint8 and S (K / 32, N), byte for
 * byte.  A host that keeps only derived layouts resident (chatglm_q_amd: DynamicQuantizeLinear.drop_canonical) serves state_dict()
 * and checkpoints - the reference's buffer contract, chatglm_q/loader.py:90-104 - through it. */
int qlinear_w4g32_unpack_gemv(const void* gemv, uint8_t* Wq, void* S, int64_t N, int64_t K, int64_t group, int dtype, void* stream);
int qlinear_w4g32_tile(const void* gemv, void* tiled, int64_t N, int64_t K, int64_t group, int dtype, void* stream);
int qlinear_w4g32_fwd_tiled(const void* A, const void* tiled, const void* bias, void* C, int64_t M, int64_t N, int64_t K,
                            int64_t group, int64_t lda, int64_t ldc, int dtype, void* workspace, size_t workspace_bytes,
                            void* stream);
/* The many-row kernel of qlinear_w4g32_fwd_tiled alone (round 3, w4_gemm256.hip: 256 x 256 output tiles, the weights of a K tile
 * dequantised once per block into LDS, A by LDS-DMA; same arithmetic: every weight (n - 8) * s rounded to the activation dtype,
 * chatglm_q/int4/triton_ops.py:72-73, fp32 accumulation).  qlinear_w4g32_fwd_tiled picks it by itself when the grid fills the
 * chip in whole rounds (prefill row counts); this entry runs it for any M.  QL_ERR_UNSUPPORTED unless K % 64 == 0, K >= 128,
 * 16-byte aligned rows of A and M * lda * 2 < 2^31.  fp16 / bf16. */
int qlinear_w4g32_fwd_tiled256(const void* A, const void* tiled, const void* bias, void* C, int64_t M, int64_t N, int64_t K,
                               int64_t group, int64_t lda, int64_t ldc, int dtype, void* stream);
/* 1 when the dispatch of qlinear_w4g32_fwd_tiled / qlinear_w8_fwd_tiled (and the _gated / _residual entry points, which exist on
 * that kernel only) takes the 256 x 256-tile kernel for M contiguous, 16-byte aligned rows of K 16-bit activations: K % 64 == 0,
 * K >= 128 and a grid that fills the chip in whole rounds (at least one block per CU, last round >= 70 % full).  Lets a caller
 * decide BEFORE it builds a gate-interleaved tile-major copy whether the gated entry point will serve the row count. */
int qlinear_gemm256_serves(int64_t M, int64_t N, int64_t K);
/* Host-only: what qlinear_w4g32_fwd_tiled (weight_bits = 4) / qlinear_w8_fwd_tiled (8) launches for M contiguous 16-bit rows:
 * returns the QL_K_* family of the first launch; *rows_first (nullable) = the rows it serves - fewer than M only for
 * QL_K_W4_GEMM256, when the rows of a thinly filled last round go to QL_K_W4_GEMM128 as a second launch ("peel").  The dispatch
 * table as a function, for tests and tools; 0 for bad arguments. */
int qlinear_tiled_dispatch(int weight_bits, int64_t M, int64_t N, int64_t K, int64_t* rows_first);

/* One-row (decode) forward on the derived layout with an activation PROLOGUE fused into the staging of the
 * activation row, so that the small op in front of the QLinear call costs no launch of its own (SURVEY.md 8f
 * N1).  fp16 / bf16, group 32; exact-dequant arithmetic unless QL_FUSED_STRICT is OR-ed into `prologue` (then every
 * dequantised weight is rounded to the activation dtype first, as QL_FLAG_STRICT_ROUNDING does for qlinear_w4g32_fwd_packed:
 * what the host module asks for with bf16 activations).  Rounding sequence as the model graph's:
 *   QL_PRO_SILU     A is (h | gate), 2K values: row = round(round(silu(h)) * gate)            chatglm_q/model.py:200-201
 *   QL_PRO_ADDNORM  hnew = round(A + delta) (delta nullable), written to hout (nullable);
 *                   row = round(round(hnew * rsqrt(mean(hnew^2) + eps)) * ln_weight)          chatglm_q/model.py:62-73,243-245
 * and optionally the gated-activation EPILOGUE of the MLP's first projection (OR the flag into `prologue`):
 *   QL_EPI_SILU_GATE  the N packed columns come in quads (h_2t, h_2t+1, gate_2t, gate_2t+1) - i.e. the module's
 *                   (K, 2H) weight was column-permuted before qlinear_w4g32_repack (bias likewise) - and C
 *                   receives N / 2 values: C[2t + i] = round(round(silu(y_i)) * y_{i+2}), y = round(sum) (+ bias,
 *                   rounded): the (.., 2H) intermediate of chatglm_q/model.py:200-201 never exists. */
#define QL_PRO_SILU 1
#define QL_PRO_ADDNORM 2
#define QL_EPI_SILU_GATE 0x100
#define QL_FUSED_STRICT 0x200
int qlinear_w4g32_fwd_packed_fused(int prologue, const void* A, const void* packed, const void* bias, void* C,
                                   int64_t N, int64_t K, const void* delta, const void* ln_weight, void* hout,
                                   float eps, int dtype, void* stream);

/* ---- int8 per-output-channel weights -------------------------------------------------------
 * W  int8, logical (K, N) with element strides (ldw_k, ldw_n) - exactly what the reference
 *    wrapper receives: the module passes weight.t() of its (N, K) row-major buffer, i.e.
 *    (ldw_k, ldw_n) = (1, K) (chatglm_q/int8/qlinear.py:90); the reference test passes a
 *    contiguous (K, N), i.e. (N, 1) (tests/test_triton_ops.py:11).
 * S  (N) scales, activation dtype. */
int qlinear_w8_fwd(const void* A, const int8_t* W, const void* S, const void* bias, void* C,
                   int64_t M, int64_t N, int64_t K, int64_t ldw_k, int64_t ldw_n, int64_t lda,
                   int64_t ldc, int dtype, int flags, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- int8 weights, derived tile-major copy (rows >= 3: MFMA kernels) ------------------------
 * tiled[N / 32][64-deep K step][half h][lane][16 bytes]: lane = 32 kb + j, half h holds bytes k = 64 kt + 32 kb + 16 h .. + 15
 * of output channel 32 (n / 32) + j, zero padded - the order in which the lanes of a wave feed their MFMA fragments: every
 * wave load instruction reads 1 KB contiguous (from the (N, K) buffer it is 16 bytes from each of 32 rows).  A lazily
 * built, non-persistent copy like the int4 one; the (N, K) buffer stays the source of truth.  fp16 / bf16,
 * K % 16 == 0.  qlinear_w8_fwd_tiled: few-row kernel (independent K-slice waves) up to 32 rows, tiled GEMM above;
 * workspace as for qlinear_w8_fwd (QL_OP_W8_FWD_TILED, optional). */
size_t qlinear_w8_tiled_bytes(int64_t N, int64_t K);
int qlinear_w8_tile(const int8_t* W, void* tiled, int64_t N, int64_t K, int64_t ldw_n, void* stream);
int qlinear_w8_fwd_tiled(const void* A, const void* tiled, const void* S, const void* bias, void* C, int64_t M, int64_t N,
                         int64_t K, int64_t lda, int64_t ldc, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* The many-row kernel of qlinear_w8_fwd_tiled alone (round 3: the 256 x 256-tile kernel of w4_gemm256.hip fed from the tile-major
 * int8 copy; every weight b * s rounded to the activation dtype, chatglm_q/int8/triton_ops.py:62-73, fp32 accumulation).  Picked
 * automatically at prefill row counts; this entry runs it for any M.  QL_ERR_UNSUPPORTED unless K % 64 == 0, K >= 128, 16-byte
 * aligned rows of A and M * lda * 2 < 2^31. */
int qlinear_w8_fwd_tiled256(const void* A, const void* tiled, const void* S, const void* bias, void* C, int64_t M, int64_t N,
                            int64_t K, int64_t lda, int64_t ldc, int dtype, void* stream);
/* The int4 kernel's prefill epilogues for int8 weight-only (round 3): `tiled` = qlinear_w8_tile of the weights (for _gated: of the
 * gate-interleaved row order (h_2t, h_2t+1, gate_2t, gate_2t+1), S and bias permuted alike; C is (M, N / 2), see
 * qlinear_w4g32_fwd_tiled_gated); _residual: C = round(round(y) + residual), see qlinear_w4g32_fwd_tiled_residual.  Bit-equal to
 * qlinear_w8_fwd_tiled followed by qlinear_silu_mul / an elementwise add.  QL_ERR_UNSUPPORTED unless the 256 x 256-tile kernel serves
 * the row count. */
int qlinear_w8_fwd_tiled_gated(const void* A, const void* tiled, const void* S, const void* bias, void* C, int64_t M, int64_t N,
                               int64_t K, int64_t lda, int64_t ldc, int dtype, void* stream);
int qlinear_w8_fwd_tiled_residual(const void* A, const void* tiled, const void* S, const void* bias, const void* residual, void* C,
                                  int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldc, int64_t ldr, int dtype, void* stream);

/* Few rows (batched decode: 2..32) through a first MLP projection with the SiLU * gate EPILOGUE: `packed` holds the
 * gate-interleaved column order (h_2t, h_2t+1, gate_2t, gate_2t+1), C gets N / 2 columns,
 * C[m, 2t+i] = round(round(silu(y_i)) * y_{i+2}), y = rounded sum (+ bias, rounded) - chatglm_q/model.py:200-201.
 * QL_ERR_UNSUPPORTED when the shape is not served by the few-row kernel without K slabs (N % 32 != 0, narrow
 * matrices, other row counts): run qlinear_w4g32_fwd_packed + qlinear_silu_mul instead.  fp16 / bf16. */
int qlinear_w4g32_fwd_packed_gated(const void* A, const void* packed, const void* bias, void* C, int64_t M, int64_t N, int64_t K,
                                   int64_t lda, int64_t ldc, int dtype, void* stream);
/* Row counts for which qlinear_w4g32_rows_on_tiled is 0 (2..4 rows while the staged rows stay within 64 KB) are served from part 1
 * by the 4x4x4-MFMA kernel - `packed` may then be a part-1-only buffer (qlinear_w4g32_repack_gemv of the permuted weights).
 * The same on part 2 alone (qlinear_w4g32_tile of the gate-interleaved part 1): */
int qlinear_w4g32_fwd_tiled_gated(const void* A, const void* tiled, const void* bias, void* C, int64_t M, int64_t N, int64_t K,
                                  int64_t lda, int64_t ldc, int dtype, void* stream);
/* Prefill row counts with the residual add of the block in the GEMM's epilogue (round 3): C = round(round(A . dequant(W) (+ bias)) +
 * residual) - `hidden = hidden + sublayer(...)`, chatglm_q/model.py:243,245, with the sublayer output rounded first as the reference
 * materialises it; bit-equal to qlinear_w4g32_fwd_tiled + an elementwise add.  residual (M, N) with row stride ldr; must not overlap C.
 * QL_ERR_UNSUPPORTED unless the 256 x 256-tile kernel serves the row count (callers then add the residual themselves). */
int qlinear_w4g32_fwd_tiled_residual(const void* A, const void* tiled, const void* bias, const void* residual, void* C, int64_t M,
                                     int64_t N, int64_t K, int64_t lda, int64_t ldc, int64_t ldr, int dtype, void* stream);

/* The same prologue (QL_PRO_ADDNORM, optionally | QL_EPI_SILU_GATE) for 2..4 contiguous rows (batched decode), on the 4x4x4-MFMA
 * kernel: A, delta (nullable), hout (nullable; written when delta is given) are (M, K), C is (M, N) or (M, N / 2) with the gate
 * epilogue; bit-equal to qlinear_add_rmsnorm (qlinear_rmsnorm without delta) followed by the projection (and qlinear_silu_mul).
 * QL_ERR_UNSUPPORTED outside the row counts / shapes for which qlinear_w4g32_rows_on_tiled is 0, or K > 8192. */
int qlinear_w4g32_fwd_rows_fused(int prologue, const void* A, const void* packed, const void* bias, void* C, int64_t M, int64_t N,
                                 int64_t K, const void* delta, const void* ln_weight, void* hout, float eps, int dtype, void* stream);

/* One-row forward on the derived layout whose output is added to the residual stream in the EPILOGUE:
 * C[n] = round(y[n] + residual[n]), y = round(sum) (+ bias, rounded) - chatglm_q/model.py:243,245
 * (hidden = hidden + attention(...), hidden = hidden + ffn(...)).  The next projection's QL_PRO_ADDNORM prologue then
 * runs without delta / hout (one operand less to stage in every workgroup).  C may alias residual.  fp16 / bf16.
 * flags: 0 or QL_FLAG_STRICT_ROUNDING. */
int qlinear_w4g32_fwd_packed_residual(const void* A, const void* packed, const void* bias, const void* residual, void* C,
                                      int64_t N, int64_t K, int dtype, int flags, void* stream);

/* The int8 twin (fp16 activations, K-contiguous weight rows of stride ldw, per-channel scales S). */
int qlinear_w8_fwd_residual(const void* A, const int8_t* W, const void* S, const void* bias, const void* residual, void* C,
                            int64_t N, int64_t K, int64_t ldw, int dtype, void* stream);

/* One-row (decode) int8 forward with the add + RMSNorm PROLOGUE (QL_PRO_ADDNORM) and optionally the SiLU * gate
 * EPILOGUE (| QL_EPI_SILU_GATE: the N rows of W - and S, bias - come in (h_2t, h_2t+1, gate_2t, gate_2t+1) quads,
 * C receives N / 2 values): the int8 twin of qlinear_w4g32_fwd_packed_fused, same rounding sequence.
 * W (N, K) int8 row-major with row stride ldw_n (the module's buffer), fp16, K % 16 == 0, K <= 16384. */
int qlinear_w8_fwd_fused(int prologue, const void* A, const int8_t* W, const void* S, const void* bias, void* C, int64_t N,
                         int64_t K, int64_t ldw_n, const void* delta, const void* ln_weight, void* hout, float eps, int dtype,
                         void* stream);

/* Backward of the int8 product w.r.t. the activations:
 *   dA (M, K) = Gout (M, N) . (Wkn * S[None, :])^T     Wkn = the logical (K, N) matrix, CONTIGUOUS (row stride N),
 *                                                      i.e. module.weight.t().contiguous(); S (N); fp16 / bf16
 * every weight rounded to the activation dtype, fp32 accumulation, one output rounding - the arithmetic of
 * dynamic_quant_matmul_transposed (chatglm_q/int8/triton_ops.py:130-245) behind DynamicQuantizeMatMul.backward
 * (chatglm_q/int8/qlinear.py:41-52). */
int qlinear_w8_bwd_input(const void* Gout, const int8_t* Wkn, const void* S, void* dA, int64_t M, int64_t N, int64_t K,
                         int64_t ldg, int64_t ldda, int dtype, void* stream);

/* ---- int8 activations x int8 weights (true i8 x i8 -> i32 MFMA contraction) ---------------
 * Row-wise symmetric activation quantisation in fp32 arithmetic:
 *   a_scale[m] = max(max_k |A[m,k]| / 127, 1e-10);  Aq = clamp(rint(A / a_scale), -127, 127)
 * (quantize_int8, chatglm_q/int8/quantizer.py:11-19).  Aq is (M, K) contiguous. */
int qlinear_act_quant_i8_rowwise(const void* A, int8_t* Aq, float* a_scale, int64_t M, int64_t K,
                                 int64_t lda, int dtype, void* stream);
/* The same with `flags`: 0 = row-wise (identical to qlinear_act_quant_i8_rowwise), QL_FLAG_ACT_PER_TENSOR = one scale
 * for the whole tensor, a_scale[m] = max(max_{m,k} |A[m,k]| / 127, 1e-10) for every m (the clamp keeps the 0 / 0 of an
 * all-zero tensor out - the NaN the reference's comment at qlinear.py:65 mentions); rounding = round half to even,
 * saturated to [-127, 127] (ONNX QuantizeLinear; |x / scale| <= 127 by construction, so -128 never occurs). */
int qlinear_act_quant_i8(const void* A, int8_t* Aq, float* a_scale, int64_t M, int64_t K, int64_t lda, int dtype,
                         int flags, void* stream);
/* C[m,n] = round(acc_i32[m,n] * (a_scale[m] * w_scale[n])) (+ bias); W is (N, K) row-major. */
int qlinear_w8a8_fwd(const int8_t* Aq, const float* a_scale, const int8_t* W, const void* S, const void* bias,
                     void* C, int64_t M, int64_t N, int64_t K, int64_t ldc, int dtype, void* workspace,
                     size_t workspace_bytes, void* stream);

/* The same contraction with the weights in the tile-major derived copy of qlinear_w8_tile (a lane's 16 bytes are its
 * MFMA operand: W bypasses LDS; two K-parity wave groups per block).  K % 16 == 0.  No workspace. */
int qlinear_w8a8_fwd_tiled(const int8_t* Aq, const float* a_scale, const void* tiled, const void* S, const void* bias,
                           void* C, int64_t M, int64_t N, int64_t K, int64_t ldc, int dtype, void* stream);
/* The many-row kernel of qlinear_w8a8_fwd_tiled alone (round 3, w8a8_gemm256.hip: 256 x 256 output tiles, both operands global ->
 * LDS by LDS-DMA - the tile-major weights land as the MFMA fragments they are -, v_mfma_i32_32x32x32_i8; integer stage exact, same
 * epilogue).  qlinear_w8a8_fwd_tiled picks it by itself at prefill row counts; this entry runs it for any M.  QL_ERR_UNSUPPORTED
 * unless fp16 / bf16, K % 128 == 0, K >= 256 and M * K < 2^31. */
int qlinear_w8a8_fwd_tiled256(const int8_t* Aq, const float* a_scale, const void* tiled, const void* S, const void* bias, void* C,
                              int64_t M, int64_t N, int64_t K, int64_t ldc, int dtype, void* stream);
/* int8 ACTIVATIONS x the gate-interleaved tile-major copy of a first MLP projection (round 4): the many-row ring kernel with SiLU * gate
 * (chatglm_q/model.py:200-201) in its epilogue, C (M, N / 2) with 8-byte aligned rows; bit-equal to qlinear_w8a8_fwd_tiled followed by
 * qlinear_silu_mul.  QL_ERR_UNSUPPORTED when the 256 x 256-tile kernel does not serve the row count (qlinear_gated_serves(.., 88)). */
int qlinear_w8a8_fwd_tiled_gated(const int8_t* Aq, const float* a_scale, const void* tiled, const void* S, const void* bias, void* C,
                                 int64_t M, int64_t N, int64_t K, int64_t ldc, int dtype, void* stream);
/* Both steps of the int8-activation linear in ONE call (two launches): quantise A (M, K) row-wise (or per tensor:
 * flags & QL_FLAG_ACT_PER_TENSOR) into the workspace, then the tile-major GEMM.  workspace: qlinear_workspace_bytes(
 * QL_OP_W8A8_LINEAR_TILED, M, N, K, 0) bytes, 16-byte aligned; it holds Aq (M * K bytes) followed by a_scale (M floats)
 * and may be inspected afterwards. */
int qlinear_w8a8_linear_tiled(const void* A, const void* tiled, const void* S, const void* bias, void* C, int64_t M,
                              int64_t N, int64_t K, int64_t lda, int64_t ldc, int dtype, int flags, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- quantised embedding gathers ("next" row N3) -------------------------------------------
 * ids: (count) int64 token ids.  int4: Wq (V/2, D) packs along the vocabulary axis, S (V/group, D).
 * int8: W (V, D), S (D).  out: (count, D) activation dtype. */
int qlinear_qembedding_w4(const int64_t* ids, const uint8_t* Wq, const void* S, void* out,
                          int64_t count, int64_t V, int64_t D, int64_t group, int dtype, void* stream);
int qlinear_qembedding_w8(const int64_t* ids, const int8_t* W, const void* S, void* out,
                          int64_t count, int64_t V, int64_t D, int dtype, void* stream);

/* ---- fused neighbours of the QLinear calls in one decode step ("next" row N1) ----------------------
 * Same rounding sequence as the model graph (chatglm_q/model.py): every intermediate the reference
 * materialises in the activation dtype is rounded to it.
 * rmsnorm:           out[r,:] = round(round(x[r,:] * rsqrt(mean(x^2) + eps)) * w)            model.py:62-73
 * add_rmsnorm:       h = round(x + delta) written to Hout (the block's residual add, model.py:243,245), then
 *                    out = rmsnorm(h): one launch for both
 * rope_kv_write:     qkv (B*S, (H+2G)*D) -> q (B*S, H*D) rotated; k (rotated), v written to the caches
 *                    (B, capacity, G, D) at row widx[s]; table (max_pos, D/2, 2) = (cos, sin); pos (B*S)
 *                                                                                              model.py:139-155
 * decode_attention:  one query position: q (B, H*D), mask (B, capacity) additive fp32 -> out (B, H*D)
 *                                                                                              model.py:157-175
 * decode_attention_rope: rope_kv_write (S = 1) and decode_attention in ONE launch: qkv (B, (H+2G)*D) in, the
 *                    cache row widx[0] written by one block per (b, group), out (B, H*D).  The reference appends the
 *                    step's key / value at the END of its cache (model.py:148-151); here the cache is preallocated, so
 *                    rows behind widx[0] hold nothing of the sequence: the caller masks them (as it must for the
 *                    per-head kernels too) and the 16-heads-per-group kernel does not compute on them whatever the
 *                    mask says; with widx[0] outside [0, capacity) nothing is written and the mask alone decides
 * silu_mul:          in (rows, 2*hidden) -> out[r,i] = round(round(silu(in[r,i])) * in[r,hidden+i])   model.py:200-201
 * Bounds of the rotary entry points (no table length crosses the ABI): `table` must hold capacity + 1 positions; pos
 * values are clamped to [0, capacity] - positions are 1-based counts (model.py:307-308), a valid one is at most its
 * cache row + 1 - and a widx outside [0, capacity) writes no cache row. */
int qlinear_rmsnorm(const void* X, const void* W, void* Out, int64_t rows, int64_t dim, int64_t ldx, int64_t ldo,
                    float eps, int dtype, void* stream);
int qlinear_add_rmsnorm(const void* X, const void* Delta, const void* W, void* Hout, void* Out, int64_t rows,
                        int64_t dim, int64_t ld, float eps, int dtype, void* stream);
int qlinear_rope_kv_write(const void* QKV, const void* table, const int64_t* pos, const int64_t* widx, void* Qout,
                          void* Kcache, void* Vcache, int64_t B, int64_t S, int64_t H, int64_t G, int64_t D,
                          int64_t capacity, int64_t ldqkv, int dtype, void* stream);
int qlinear_decode_attention(const void* Q, const void* Kcache, const void* Vcache, const float* mask, void* Out,
                             int64_t B, int64_t H, int64_t G, int64_t D, int64_t capacity, int dtype, void* stream);
/* split_workspace (nullable, qlinear_decode_attention_split_bytes): long contexts - 256-position windows over
 * blockIdx.y leave (max, exp-sum, unnormalised output) there and a second launch combines them; the probabilities are
 * then not rounded to the activation dtype before P.V (same function within fp tolerance).  Without it one block per
 * (sequence, head) walks the whole cache with the reference's rounding points (capacity <= ~15 k).
 * H == 16 G, D == 128, fp16 / bf16, ldqkv % 8 == 0: one block per (sequence, group, window) on the matrix cores
 * (a single launch up to capacity 256, split_workspace needed above; QLINEAR_DISPATCH=nogroupattn turns it off). */
size_t qlinear_decode_attention_split_bytes(int64_t B, int64_t H, int64_t D, int64_t capacity);
int qlinear_decode_attention_rope(const void* QKV, const void* table, const int64_t* pos, const int64_t* widx, void* Kcache,
                                  void* Vcache, const float* mask, void* Out, int64_t B, int64_t H, int64_t G, int64_t D,
                                  int64_t capacity, int64_t ldqkv, int dtype, void* split_workspace,
                                  size_t split_workspace_bytes, void* stream);
/* The same launch, carrying extra workgroups that read the weights of the NEXT one-row linear on the stream (the
 * attention output projection) into L2 / the memory-side cache while the attention itself - a chain of round trips on
 * B * G workgroups - leaves the chip and HBM idle.  next_weights: QL_NEXT_W4G32_PACKED = buffer of
 * qlinear_w4g32_repack, QL_NEXT_W8_ROWS = contiguous (N, K) int8 rows; NULL: no prefetch.  Only the group kernel
 * (H == 16 G, D == 128, fp16 / bf16) prefetches; results never depend on it. */
#define QL_NEXT_W4G32_PACKED 1
#define QL_NEXT_W8_ROWS 2
int qlinear_decode_attention_rope_prefetch(const void* QKV, const void* table, const int64_t* pos, const int64_t* widx,
                                           void* Kcache, void* Vcache, const float* mask, void* Out, int64_t B, int64_t H,
                                           int64_t G, int64_t D, int64_t capacity, int64_t ldqkv, int dtype,
                                           void* split_workspace, size_t split_workspace_bytes, const void* next_weights,
                                           int next_kind, int64_t next_N, int64_t next_K, void* stream);
/* masked_softmax: P[r, :] = round(softmax_fp32(scores[r, :] + mask[r % mask_rows, :])) - the add / fp32 softmax / cast
 * between the two GEMMs of the many-position attention (chatglm_q/model.py:166-170) in one pass; mask nullable. */
int qlinear_masked_softmax(const void* scores, const float* mask, void* P, int64_t rows, int64_t T, int64_t mask_rows,
                           int64_t lds, int64_t ldm, int64_t ldp, int dtype, void* stream);
/* prefill_attention (round 3): the many-position attention between qkv_proj and o_proj of a prefill chunk in ONE launch
 * (chatglm_q/model.py:157-175: q / sqrt(d), q k^T, + mask, fp32 softmax, cast, p v) instead of two batched GEMMs around
 * qlinear_masked_softmax - the (heads x S x T) score matrix is never written.  Q (B, S, H, D) rotated queries (qlinear_rope_kv_write),
 * Kcache / Vcache (B, capacity, G, D) of which rows [0, T) are attended, mask (B, S, T) additive fp32 with row stride ldm
 * (nullable = no mask), Out (B, S, H * D).  Applied exactly as the reference applies it: round(score) + mask in fp32, so a row
 * whose keys are all blocked comes out as the uniform average.  tile_flags (nullable; uint8 (B, ceil(S / q_block), ceil(T / k_tile)),
 * block sizes from qlinear_prefill_attention_tiles) lets the kernel skip key tiles and mask loads:
 *   0 = every mask entry of the tile <= -1e9 AND every query row of the block has an entry >= -1e6 somewhere (the tile's
 *       probabilities are exactly 0 in fp32 for any fp16-range score): skipped;  2 = every entry == 0: no mask loads;  1 = otherwise.
 * The caller derives them from the SAME mask (fused_ops.attention_tile_flags); wrong flags give wrong results, not faults.
 * QL_ERR_UNSUPPORTED unless D == 128, H == 16 G and fp16 / bf16 (ChatGLM2's geometry): callers keep the GEMM route then. */
int qlinear_prefill_attention_tiles(int64_t* q_block, int64_t* k_tile);
int qlinear_prefill_attention(const void* Q, const void* Kcache, const void* Vcache, const float* mask, const uint8_t* tile_flags,
                              void* Out, int64_t B, int64_t S, int64_t T, int64_t H, int64_t G, int64_t D, int64_t capacity,
                              int64_t ldm, int dtype, void* stream);
int qlinear_silu_mul(const void* In, void* Out, int64_t rows, int64_t hidden, int64_t ldin, int64_t ldo, int dtype,
                     void* stream);
/* Quantising producers (round 3): the row a norm / activation kernel holds in registers is ALSO emitted as int8 + one fp32 scale
 * per row - bit for bit what qlinear_act_quant_i8 (row-wise: quantize_int8, chatglm_q/int8/quantizer.py:11-19) makes of the
 * rounded 16-bit output row - so that the int8-activation GEMM behind it (qlinear_w8a8_fwd_tiled / qlinear_w8a8_fwd) needs no
 * quantiser launch ("pre-quantized activations", north_star).  Aq is (rows, dim) contiguous, a_scale (rows).  Out is nullable
 * (nobody else reads the 16-bit row); Delta / Hout as in qlinear_add_rmsnorm (both null: plain qlinear_rmsnorm).  fp16 / bf16.
 * Callers: chatglm_q/model.py:213,244 (RMSNorm in front of qkv_proj / w_in), :200-201 (SiLU * gate in front of w_out). */
int qlinear_rmsnorm_quant_i8(const void* X, const void* Delta, const void* W, void* Hout, void* Out, int8_t* Aq, float* a_scale,
                             int64_t rows, int64_t dim, int64_t ld, float eps, int dtype, void* stream);
int qlinear_silu_mul_quant_i8(const void* In, void* Out, int8_t* Aq, float* a_scale, int64_t rows, int64_t hidden, int64_t ldin,
                              int64_t ldo, int dtype, void* stream);
/* greedy decode bookkeeping in one launch (chatglm_q/decoder.py:85,97 with temperature -> 0): tok[b] = argmax of logits
 * row b (lowest index on ties), pos[b] += 1, write_index[0] += 1, mask[b][new write_index] = 0 for every row. */
int qlinear_greedy_advance(const void* logits, int64_t B, int64_t N, int64_t ldl, int64_t* tok, int64_t* write_index,
                           int64_t* pos, float* mask, int64_t capacity, int dtype, void* stream);
/* The reference's decoding mode in one launch behind lm_head (chatglm_q/decoder.py:12-27 `top_p_sampling`, called per token at :85):
 *   probs = softmax(float(logits) / temperature); sort descending, keep top_k (ties: lowest index first); zero every entry whose
 *   PRECEDING cumulative mass exceeds top_p; renormalise; one multinomial draw; tok[b] = its token index.
 * logits (B, N) with row stride ldl, one workgroup per row, any N, top_k <= 1024 (QL_ERR_UNSUPPORTED above, unless N <= 1024).
 * dev_params (nullable, device float[3] = top_k, top_p, temperature) overrides the three scalars at run time, so that ONE captured
 * graph serves every sampler setting.  rng_state (device uint64[1 + B], nullable = seed 0 / counter 0): [0] the seed, [1 + b] row
 * b's draw counter, advanced by one per launch - the draw is u = (Philox4x32-10(counter = (ctr, b, 0), key = seed).x >> 8) / 2^24
 * and the token is the first sorted entry whose inclusive cumulative kept mass exceeds u * (kept mass): replays of a graph draw
 * fresh numbers, equal (seed, counter) reproduce the token.  top_k = 1 is qlinear_greedy_advance's argmax bit for bit.
 * write_index / pos / mask (all nullable together): the decode step's bookkeeping exactly as qlinear_greedy_advance does it.
 * probs_out (B, out_ld) / index_out (B, out_ld) (nullable together): the filtered, renormalised distribution in sorted order and its
 * token indices (the first min(top_k, N) entries of a row are written) - what the parity tests compare with the reference;
 * u_out (B, nullable): the uniform number each row drew. */
int qlinear_top_p_sample(const void* logits, int64_t B, int64_t N, int64_t ldl, int64_t top_k, float top_p, float temperature,
                         const float* dev_params, uint64_t* rng_state, int64_t* tok, int64_t* write_index, int64_t* pos, float* mask,
                         int64_t capacity, float* probs_out, int64_t* index_out, float* u_out, int64_t out_ld, int dtype, void* stream);
/* The tail of the reference's loss (chatglm_q/model.py:384-390: logits.float(), then F.cross_entropy) and of its perplexity run
 * (examples/evaluations/ppl.py) per token, in ONE pass over a block of logits rows - no fp32 copy of the logits, no second walk:
 *   lse[r] = log(sum_j exp(float(x[r][j])))   (fp32, relative to the row maximum)
 *   logprob_out[r] = float(x[r][targets[r]]) - lse[r];  0 when targets[r] == ignore_index;  NaN when targets[r] is any other value
 *   outside [0, N) (nothing is read out of bounds);  argmax_out[r] = lowest index of the row maximum.
 * logits (R, N) in the activation dtype with row stride ldl >= N and unit column stride, aligned to its element size only (rows
 * need no 16-byte alignment: the unaligned head and the ragged tail of a row are read element by element); any N >= 1; R == 0 is
 * QL_OK without a launch.  targets (R) int64 device memory.  lse_out / argmax_out are nullable.  One workgroup per row.  -inf entries
 * count as probability 0; a row of nothing but -inf yields lse = -inf and a NaN log-prob (as log_softmax does); a NaN logit makes
 * that row's lse and log-prob NaN and is skipped by the maximum search. */
int qlinear_token_logprob(const void* logits, int64_t R, int64_t N, int64_t ldl, const int64_t* targets, int64_t ignore_index,
                          float* logprob_out, float* lse_out, int64_t* argmax_out, int dtype, void* stream);
/* Batched generation step in one launch behind lm_head, one workgroup per row: per-row sampler settings, per-row generators, per-row
 * stop and the tokens recorded on the device, so that a captured graph runs many steps with no host read between them.
 *   row_params (B, 3) float: top_k, top_p, temperature of row b.  top_k is clamped to [1, min(1024, N)] (NaN: 1).
 *   row_rng (B, 2) uint64: row b's seed, row b's draw counter.  row_state (B, 2) int32: tokens generated so far (n_b); flags
 *   (bit 0 finished, bit 1 invalid logits).  budget (B) int32: tokens row b may generate.  out_tokens (B, out_ld) int64: row b's
 *   tokens in order.  live (1) int32: rows not finished.
 * A finished row draws nothing, keeps its counter, its tokens and its state; tok[b] = stop_id, or (stop_id < 0) its last token
 * (0 when it has none).  A live row selects t exactly as qlinear_top_p_sample does for one row with the same logits, parameters and
 * generator state, except that the Philox counter is (ctr_b, 0, 0) with key seed_b (the row index is not part of it: a row draws
 * the same whichever batch position it holds); top_k == 1 is qlinear_greedy_advance's argmax (lowest index on ties) in one walk.
 * Then out_tokens[b][n_b] = t, n_b += 1, ctr_b += 1, tok[b] = t; the row finishes when t == stop_id (stop_id >= 0), n_b == budget[b]
 * or n_b == out_ld, and then decrements live once (a live row armed with n_b >= budget[b] finishes without a draw).  A row without
 * finite positive mass (NaN or +inf logits, all -inf, temperature <= 0 or NaN - never divided by) takes the lowest index of its
 * largest non-NaN logit (0 if none), finishes and is flagged invalid: the token written is always in [0, N).
 * write_index / pos / mask (nullable together): advanced for every row as qlinear_greedy_advance does; null: nothing advanced (the
 * first token after a prefill).  probs_out / index_out (B, dist_ld) (nullable together, dist_ld >= min(1024, N)) and u_out (B):
 * as in qlinear_top_p_sample, for live rows.
 * QL_ERR_BAD_DTYPE; QL_ERR_BAD_SHAPE for ldl < N, out_ld < 1, N < 1 or stop_id >= N; QL_ERR_NULL_POINTER for a missing required
 * buffer; B == 0 is QL_OK without a launch. */
int qlinear_batch_sample_advance(const void* logits, int64_t B, int64_t N, int64_t ldl, const float* row_params, uint64_t* row_rng,
                                 int32_t* row_state, const int32_t* budget, int64_t* out_tokens, int64_t out_ld, int32_t* live,
                                 int64_t stop_id, int64_t* tok, int64_t* write_index, int64_t* pos, float* mask, int64_t capacity,
                                 float* probs_out, int64_t* index_out, float* u_out, int64_t dist_ld, int dtype, void* stream);
/* Sampling controls in one launch between lm_head and the selection entry points above: a repetition penalty, OpenAI-style presence
 * and frequency penalties and a sparse logit bias, applied IN PLACE to logits (B, N) (row stride ldl, unit column stride), with the
 * token history they need kept in device memory - the launch can sit inside a captured decode step.
 *   state (B, lds) int32, lds >= N: word [b][v] = bit 31: v is one of row b's prompt ids (P); bits 0..30: how often row b has generated
 *     v (G).  The caller zeroes it and sets the prompt bits when a generation starts; this entry point advances the counts.
 *   settings (B, 3) float: r (repetition penalty, > 0; 1 = off), p (presence penalty; 0 = off), f (frequency penalty; 0 = off).
 *   bias_ids / bias_vals (B, bias_cap) int32 / float, bias_len (B) int32: row b's bias list is its first bias_len[b] pairs (clamped to
 *     [0, bias_cap]); ids distinct and in [0, N) (others are ignored), values finite or -inf.  bias_cap <= QL_LOGIT_BIAS_MAX;
 *     bias_cap == 0: no lists, the three pointers may be null.  All of these are read from device memory at run time, so ONE
 *     captured graph serves every setting.
 *   tok (B) int64, nullable: the id fed into this step.  First, state[b][tok[b]] += 1 (an id outside [0, N) counts nothing; null - the
 *     first token after a prefill - counts nothing), so G always covers exactly the tokens generated so far.
 *   row_state (B, 2) int32, nullable: qlinear_batch_sample_advance's; a row whose finished bit (bit 0 of [b][1]) is set is left
 *     entirely untouched - no count, no write.
 * Then for every entry, x = float(logits[b][v]), each line ONE fp32 operation rounded to nearest (no fused multiply-add):
 *     P || G > 0 :  x = x > 0 ? x / r : x * r        (the Hugging Face rule; a NaN takes the multiply and stays NaN)
 *     G > 0      :  m = f * float(G);  x = x - m;  x = x - p
 *     biased     :  x = x + bias
 * and the result is rounded once to the logits dtype (nearest even) and stored.  An entry no rule touches keeps its bits.  -inf,
 * +inf and NaN logits pass through as IEEE arithmetic dictates.
 * Every entry is owned by exactly one thread (no atomics; plain vector loads and stores).  Any N >= 1; logits aligned to its element size
 * only: rows (of logits and of state) that are 16-byte aligned go through 16-byte accesses, the ragged end of a row and rows that
 * are not aligned go entry by entry.  Nothing outside [row, row + N) is touched.  One pass over B x N x (element + 4) bytes.
 * QL_ERR_BAD_DTYPE; QL_ERR_BAD_SHAPE for N < 1, ldl < N, lds < N, B > 65535 or bias_cap outside [0, QL_LOGIT_BIAS_MAX];
 * QL_ERR_NULL_POINTER for a missing logits / settings / state (or a missing bias array with bias_cap > 0); B == 0 is QL_OK without a
 * launch. */
#define QL_LOGIT_BIAS_MAX 64
int qlinear_logit_penalties(void* logits, int64_t B, int64_t N, int64_t ldl, const float* settings, const int32_t* bias_ids,
                            const float* bias_vals, const int32_t* bias_len, int64_t bias_cap, int32_t* state, int64_t lds,
                            const int64_t* tok, const int32_t* row_state, int dtype, void* stream);

/* Per-token log-probabilities DURING generation: one launch behind a step's selection entry point (qlinear_greedy_advance,
 * qlinear_top_p_sample or qlinear_batch_sample_advance - tok[b] already holds the id just chosen) that reads the logits row the
 * selection read (after qlinear_logit_penalties, before temperature / top-k / top-p) and appends, per row, the log-probability of
 * the chosen id and the n_top most likely ids with theirs to a record in device memory - the host reads it once at the end.
 *   tok (B) int64: the id chosen this step.  row_state (B, 2) int32, nullable: qlinear_batch_sample_advance's.
 *   count (B) int32: entries recorded so far per row.  chosen (B, cap) float.  top_ids / top_lp (B, cap, n_top) int32 / float
 *   (nullable when n_top == 0).  0 <= n_top <= QL_TOP_LOGPROBS_MAX, cap >= 1.
 * For row b, c = count[b]:
 *   skip:  row_state given and row_state[b][0] <= c - the row recorded no token in this step (it is finished, or its budget ran
 *          out): nothing is written.  (While a row is live its count trails its token count by exactly one at this point.)
 *   full:  c >= cap: nothing is written, count stays.
 *   otherwise, x = float(logits[b][:]), m = the row maximum, s = sum exp(x - m), computed exactly as qlinear_token_logprob's
 *   1024-thread kernel computes them (same chunk ownership, same arithmetic, same merge):
 *     chosen[b][c] = (x[tok[b]] - m) - log(s)            NaN when tok[b] is outside [0, N)
 *     top_ids[b][c][j], top_lp[b][c][j], j < min(n_top, N): the j-th entry of the row under the strict total order (value descending,
 *       index ascending - qlinear_top_p_sample's order; a NaN logit ranks as -inf) and its (x_j - m) - log(s);  j >= N: -1, -inf
 *     count[b] = c + 1
 *   so for B < 1024 every value written is BIT-EQUAL to what qlinear_token_logprob returns for the same row with that id as target.
 * The selection is exact for every row; rows whose candidate list would overflow (a sorted row, a row of mostly -inf, a tie group
 * of more than 1024 at the cut) take a slow path of n_top workgroup arg-max rounds.  One workgroup of 1024 threads per row; any
 * N >= 1; logits aligned to its element size only; nothing outside [row, row + N) is read; every output element has one owner,
 * plain vector loads and stores.
 * QL_ERR_BAD_DTYPE; QL_ERR_BAD_SHAPE for N < 1, ldl < N, B > 65535, cap < 1 or n_top outside [0, QL_TOP_LOGPROBS_MAX];
 * QL_ERR_NULL_POINTER for a missing logits / tok / count / chosen (or a missing top array with n_top > 0); QL_ERR_MISALIGNED for
 * logits not aligned to the element size; B == 0 is QL_OK without a launch. */
#define QL_TOP_LOGPROBS_MAX 20
int qlinear_step_logprobs(const void* logits, int64_t B, int64_t N, int64_t ldl, const int64_t* tok, const int32_t* row_state,
                          int32_t* count, float* chosen, int32_t* top_ids, float* top_lp, int64_t cap, int64_t n_top, int dtype,
                          void* stream);

/* The controls that depend on the ORDER of a row's tokens, in one launch between lm_head (behind qlinear_logit_penalties when that is
 * armed) and the selection entry points: no-repeat n-grams, banned multi-token sequences, stop sequences and a minimum length.  Edits
 * logits (B, N) IN PLACE (row stride ldl, unit column stride); the row's token history is kept in device memory and advanced by this
 * launch, and every control is read from device memory, so ONE captured graph serves every setting.
 *   hist (B, hist_ld) int32: row b's real prompt ids (no pads), then its generated ids.  hist_len (B) int32: L, how many of them are
 *     valid (clamped to [0, hist_ld]).  prompt_len (B) int32: P (clamped to [0, L]); g = L - P tokens have been generated.
 *   cfg (B, 2) int32: n, the no-repeat n-gram size (0 = off; clamped to [0, QL_CONSTRAINT_SEQ_LEN_MAX]), and min_new.
 *   seq_tok (B, QL_CONSTRAINT_SEQS_MAX, QL_CONSTRAINT_SEQ_LEN_MAX) int32, seq_len / seq_kind (B, QL_CONSTRAINT_SEQS_MAX) int32,
 *     seq_count (B) int32: row b's sequence table is its first seq_count[b] entries (clamped to [0, QL_CONSTRAINT_SEQS_MAX]); entry s
 *     has seq_len ids (clamped to [0, QL_CONSTRAINT_SEQ_LEN_MAX]; 0: the entry is ignored) and a kind, QL_CONSTRAINT_BAN / _STOP / _MIN
 *     (another value: ignored).  A MIN entry is one id.
 *   tok (B) int64, nullable: the id fed into this step, as in qlinear_logit_penalties.
 *   row_state (B, 2) int32 and live (1) int32: qlinear_batch_sample_advance's; nullable TOGETHER.
 * For row b, in this order:
 *   0. row_state given and the row's finished bit (bit 0 of [b][1]) set: the row is left entirely untouched - no append, no write.
 *   1. append: tok given and L < hist_ld: hist[b][L] = tok[b], L += 1 (hist_len is updated).  tok null (the first token after a
 *      prefill) or L == hist_ld: nothing is appended and the launch goes on with the history as it is.  An id outside [0, N) is stored
 *      as it is (one that no int32 holds: as -1); it never indexes the logits.
 *   2. stop (only when row_state is given): a STOP entry of length m <= g with hist[L-m : L] == its ids - the whole match in generated
 *      tokens - sets the finished bit and takes one off live[0] (one vector atomic, one thread per row); the row's logits stay as they
 *      are and the row is done.  The match is seen one step after the step that selected the sequence's last id: that step's selection
 *      for the row is qlinear_batch_sample_advance's fill id, and the row's recorded tokens end with the sequence.
 *   3. bans: logits[b][id] = -inf (in the logits dtype) for every id in [0, N) that one of these names:
 *        n >= 1: hist[i+n-1] for every i in [0, L-n] with hist[i : i+n-1] == hist[L-n+1 : L]   (the Hugging Face no-repeat rule; n = 1:
 *                every id of the history; L < n: none)
 *        a BAN entry of length m: its last id, when L >= m-1 and hist[L-m+1 : L] == its first m-1 ids   (m = 1: always; the prompt counts)
 *        a MIN entry: its id, while g < min_new
 *      An entry no rule names keeps its bits.  Nothing outside [row, row + N) is touched.
 * One workgroup per row; every thread reads the length and tok[b] itself, and one thread stores the appended id and the new length
 * behind a workgroup barrier that all threads cross after their own read; several lanes may store the same -inf to one address, no
 * logit is read.  Every logits index is range-checked in
 * the thread that stores, every history index is below the clamped L, every table index below the clamped counts.  A row with n = 0 and
 * no entries appends and returns.  Bound: one launch; 4 x L bytes of history read per row.
 * QL_ERR_BAD_DTYPE; QL_ERR_BAD_SHAPE for N < 1, ldl < N, hist_ld < 1 or B > 65535; QL_ERR_NULL_POINTER for a missing required buffer, or
 * for live without row_state or the reverse; QL_ERR_MISALIGNED for logits not aligned to the element size; B == 0 is QL_OK without a
 * launch. */
#define QL_CONSTRAINT_SEQS_MAX 32
#define QL_CONSTRAINT_SEQ_LEN_MAX 16
#define QL_CONSTRAINT_BAN 0
#define QL_CONSTRAINT_STOP 1
#define QL_CONSTRAINT_MIN 2
int qlinear_history_constraints(void* logits, int64_t B, int64_t N, int64_t ldl, int32_t* hist, int64_t hist_ld, int32_t* hist_len,
                                const int32_t* prompt_len, const int32_t* cfg, const int32_t* seq_tok, const int32_t* seq_len,
                                const int32_t* seq_kind, const int32_t* seq_count, const int64_t* tok, int32_t* row_state, int32_t* live,
                                int dtype, void* stream);

/* Regex-constrained generation: the mask of a byte-level DFA over the vocabulary, one launch between qlinear_history_constraints (or
 * qlinear_logit_penalties, or lm_head) and the selection entry points - the order is penalties, history, grammar, selection, log-prob
 * record.  Edits logits (B, N) IN PLACE (row stride ldl, unit column stride).  Everything a row's pattern decides is read from device
 * memory and the row's automaton state is kept there and advanced by this launch, so ONE captured graph serves every pattern.
 *   tok_off (n_tok + 1) int32, tok_bytes (n_bytes) uint8: the vocabulary's byte table, shared by all rows - token id's byte string is
 *     tok_bytes[tok_off[id] : tok_off[id + 1]]; an id >= n_tok has the empty string.  An EMPTY token is never allowed by a grammar.
 *   class_of (B, 256) uint8: row b's byte classes; n_classes = 1 + the largest entry.
 *   table (B, QL_GRAMMAR_TABLE_MAX) uint16: row b's transitions, table[s * n_classes + class] = the next state; an entry outside
 *     [0, n_states) - 0xFFFF by convention - is DEAD.  The start state is 0.
 *   accept (B, QL_GRAMMAR_STATES_MAX + 1) uint8: nonzero = accepting.
 *   cfg (B, 2) int32: n_states (<= 0: the row has no grammar; clamped to QL_GRAMMAR_STATES_MAX and to QL_GRAMMAR_TABLE_MAX / n_classes)
 *     and eos_id (outside [0, N), -1 by convention: none).
 *   state (B) int32: the row's current state s, a value outside [0, n_states) - -1 by convention - is dead.  ticket (B) int32: 0 between
 *     launches.
 *   tok (B) int64, nullable: the id fed into this step, as in qlinear_logit_penalties.  row_state (B, 2) int32, nullable:
 *     qlinear_batch_sample_advance's.
 * walk(s, bytes): from a live s follow table[s * n_classes + class_of[byte]] byte by byte; dead at the first DEAD entry; a dead s stays
 * dead; no bytes: s.  For row b, in this order:
 *   0. row_state given and the row's finished bit (bit 0 of [b][1]) set, or n_states <= 0: the row is left entirely untouched - nothing
 *      is read past that, nothing is written.
 *   1. advance: tok given: s' = walk(s, bytes(tok[b])).  An id outside [0, N) or [0, n_tok), or one with an empty byte string - the
 *      end token the greedy loop's speculated step is fed - leaves s' = s.  tok null (the first token after a prefill): s' = s.
 *   2. mask: for every id in [0, N) other than eos_id: logits[b][id] = -inf (in the logits dtype) when bytes(id) is empty or
 *      walk(s', bytes(id)) is dead.  For eos_id: logits[b][eos_id] = -inf unless s' is live and accepting; a dead s' leaves eos_id
 *      alone, so such a row ends.  No logit is read; an allowed entry keeps its bits; nothing outside [row, row + N) is touched.
 *   3. state[b] = s', stored exactly once per launch.
 * Grid ceil(N / QL_GRAMMAR_CHUNK) x B workgroups; each copies the row's class map and the live part of its table (n_states *
 * n_classes entries) into LDS, computes s' itself and walks its own QL_GRAMMAR_CHUNK tokens.  No workgroup reads in this launch
 * anything another workgroup of this launch wrote: every one reads the OLD state[b]; behind its last logit store and an agent-scope
 * release it draws a ticket (one agent-scope atomic add on ticket[b]); the one that draws the last ticket stores s' and puts the ticket
 * back to 0.  Nothing spins or waits on another workgroup.  ticket[b] must be 0 when a launch starts.
 * Every index is clamped: a corrupt table masks too much and never reads out of range - offsets must satisfy 0 <= tok_off[id] <=
 * tok_off[id + 1] <= n_bytes or the id is masked (the fed id: the state dies).  Bound: one launch; per row 4 (N + 1) bytes of offsets
 * plus the token bytes, and the DFA copy once per workgroup.
 * QL_ERR_BAD_DTYPE; QL_ERR_BAD_SHAPE for N < 1, ldl < N, n_tok < 1, n_bytes < 0, one of them >= 2^31 or B > 65535; QL_ERR_NULL_POINTER for
 * a missing required buffer (tok_bytes may be null when n_bytes == 0); QL_ERR_MISALIGNED for logits not aligned to the element size, a
 * table not aligned to 16 bytes or an int32 buffer not aligned to 4; B == 0 is QL_OK without a launch. */
#define QL_GRAMMAR_TABLE_MAX 16384
#define QL_GRAMMAR_STATES_MAX 4095
#define QL_GRAMMAR_CHUNK 256
int qlinear_grammar_mask(void* logits, int64_t B, int64_t N, int64_t ldl, const int32_t* tok_off, const uint8_t* tok_bytes, int64_t n_tok,
                         int64_t n_bytes, const uint8_t* class_of, const uint16_t* table, const uint8_t* accept, const int32_t* cfg,
                         int32_t* state, int32_t* ticket, const int64_t* tok, const int32_t* row_state, int dtype, void* stream);

/* JSON-constrained generation: the mask of a byte-level PUSHDOWN automaton over the vocabulary - deterministic, real-time (one move per
 * byte, no empty moves), one bounded stack - in the place of qlinear_grammar_mask: one launch between qlinear_history_constraints (or
 * qlinear_logit_penalties, or lm_head) and the selection entry points; a step takes this launch or qlinear_grammar_mask, never both.
 * Edits logits (B, N) IN PLACE (row stride ldl, unit column stride).  Everything a row's grammar decides is read from device memory and
 * the row's configuration - state and stack - is kept there and advanced by this launch, so ONE captured graph serves every grammar.
 *   tok_off, tok_bytes, n_tok, n_bytes, class_of (B, 256), accept (B, QL_GRAMMAR_STATES_MAX + 1), tok, row_state: qlinear_grammar_mask's.
 *   table (B, QL_GRAMMAR_TABLE_MAX) uint16: row b's moves, table[(s * (n_syms + 1) + top) * n_classes + class], top = 0 for an empty
 *     stack and otherwise the symbol on top, in 1..n_syms.  An entry: bits 0 - 11 the next state (>= n_states - 0xFFF by convention -
 *     is DEAD), bits 12 - 13 the op (0 none, 1 pop, 2 push, 3 DEAD), bits 14 - 15 the pushed symbol; 0xFFFF by convention = no move.
 *     The start configuration is state 0 with an empty stack.
 *   cfg (B, 4) int32: n_states (<= 0: the row has no grammar), eos_id (outside [0, N), -1 by convention: none), n_syms, max_depth.
 *   state (B) int32: the row's state s, -1 = dead.  depth (B) int32: the symbols on the row's stack.  stack (B, QL_PDA_DEPTH_MAX)
 *     uint8: the symbols, bottom first; entries at and past depth mean nothing.  ticket (B) int32: 0 between launches.
 * For row b, in this order:
 *   0. row_state given and the row's finished bit (bit 0 of [b][1]) set, or n_states <= 0: the row is left entirely untouched - nothing
 *      is read past that, nothing is written.
 *   6. (first, because everything below uses the clamped values) clamps: n_states to QL_GRAMMAR_STATES_MAX; n_syms to [0,
 *      QL_PDA_SYMS_MAX]; max_depth to [0, QL_PDA_DEPTH_MAX]; n_classes = 1 + the largest entry of class_of[b]; then n_states to
 *      QL_GRAMMAR_TABLE_MAX / ((n_syms + 1) * n_classes) (integer division).  A state outside [0, n_states), a depth outside [0,
 *      max_depth], or - at a depth > 0 - a top symbol stack[b][depth - 1] outside 1..n_syms makes the row DEAD.  Offsets must satisfy
 *      0 <= tok_off[id] <= tok_off[id + 1] <= n_bytes or the id is masked (the fed id: the row dies).  A corrupt row masks too much; it
 *      never indexes out of range.
 *   1. advance: tok given: (s', stack') = the walk of bytes(tok[b]) from (s, stack).  An id outside [0, N) or [0, n_tok), or one with an
 *      empty byte string, moves nothing; tok null: nothing moves.  A dead row stays dead.
 *   2. one move on byte x from a live (s, stack): e = table[(s * (n_syms + 1) + top) * n_classes + class_of[x]].  Dead when the next state
 *      is >= n_states or the op is 3; op 1 pops - dead at depth 0; op 2 pushes its symbol - dead when the symbol is 0 or > n_syms or when
 *      depth == max_depth.  Whenever a pop uncovers a symbol of the row's stack outside 1..n_syms, the walk is dead (clamp 6).
 *   3. the window rule: ONE token's walk may never hold more than QL_PDA_LOCAL_MAX symbols above the lowest depth it has reached during
 *      that walk - a push that would is dead.  (A thread keeps its own pushes in one 64-bit register, 2 bits per symbol, and reads the
 *      row's stack only for what it pops below them.  For JSON the rule excludes a token with 33 or more net-unclosed openers.)
 *      The fed id's walk in rule 1 obeys it as well.
 *   4. mask: for every id in [0, N) other than eos_id: logits[b][id] = -inf (in the logits dtype) when bytes(id) is empty or its walk
 *      from (s', stack') is dead.  For eos_id: logits[b][eos_id] = -inf unless s' is live and accepting and depth' == 0; a dead s'
 *      leaves eos_id alone, so such a row ends.  No logit is read; an allowed entry keeps its bits; nothing outside [row, row + N) is
 *      touched.
 *   5. store, exactly once per launch: state[b] = s' (-1 when dead); when s' is live also depth[b] = depth' and the symbols the advance
 *      pushed, stack[b][low .. depth') with low = the lowest depth the advance reached (entries below low keep their bytes, entries at
 *      and past depth' are not written); a dead row keeps its depth and stack bytes.
 * Grid ceil(N / QL_GRAMMAR_CHUNK) x B workgroups of 256 threads; each copies the row's class map, its stack and the live part of its
 * table (n_states * (n_syms + 1) * n_classes entries) into LDS, computes (s', stack') itself and walks its own QL_GRAMMAR_CHUNK tokens.
 * No workgroup reads in this launch anything another workgroup of this launch wrote: every one reads the OLD state, depth and stack;
 * behind its last logit store and an agent-scope release it draws a ticket (one agent-scope atomic add on ticket[b]); the one that
 * draws the last ticket makes the stores of rule 5 - ordinary vector stores - and puts the ticket back to 0.  Nothing spins or waits
 * on another workgroup.  ticket[b] must be 0 when a launch starts.
 * Errors as qlinear_grammar_mask's (depth and stack are required buffers, depth aligned to 4); B == 0 is QL_OK without a launch. */
#define QL_PDA_DEPTH_MAX 64
#define QL_PDA_LOCAL_MAX 32
#define QL_PDA_SYMS_MAX 3
int qlinear_pda_mask(void* logits, int64_t B, int64_t N, int64_t ldl, const int32_t* tok_off, const uint8_t* tok_bytes, int64_t n_tok,
                     int64_t n_bytes, const uint8_t* class_of, const uint16_t* table, const uint8_t* accept, const int32_t* cfg,
                     int32_t* state, int32_t* depth, uint8_t* stack, int32_t* ticket, const int64_t* tok, const int32_t* row_state,
                     int dtype, void* stream);

/* Beam search inside the decode step.  P prompts x B beams (1 <= B <= QL_BEAMS_MAX) are R = P * B batch rows; rows g*B .. g*B+B-1 are
 * group g, every row of a group holds the same prompt.  A beam step is the model step's launches plus three: qlinear_step_logprobs on a
 * one-slot record per row (cap = 1, n_top = 2B: the row's 2B best ids and their log-probs lp, 2B <= QL_TOP_LOGPROBS_MAX), then
 * qlinear_beam_advance, then qlinear_beam_gather.  All state is device memory, so one captured graph serves every search of the same B.
 *
 * qlinear_beam_advance - one workgroup per group:
 *   cand_ids / cand_lp (R, 2B) int32 / float32: the record step_logprobs wrote; cand_count (R) int32: its counts, reset to 0 here.
 *   beam_score (R) float32: the running beams' summed log-probs (armed 0 for a group's first row, -inf for the others: the first step
 *     expands beam 0 only).  tok (R) int64, parent (R) int32 (absolute row): written.  trellis (cap, R, 2) int32: (token, parent row) per
 *     row and step.  steps (P) int32: steps taken.  fin_score / fin_sum (P, B) float32, fin_len / fin_row (P, B) int32, fin_count (P) int32:
 *     the heap of finished hypotheses (normalised score, raw score, length, parent row).  done (P) int32; live (1) int32: groups not done.
 *     norm (cap + 1) float32: norm[len] = len ** length_penalty, built on the host.  cfg (2) int32: the end id (< 0: none), early_stopping.
 *   A group with done != 0 or steps >= cap rides along: tok = the end id (0 without one), parent = the row itself, nothing else changes.
 *   Otherwise, every operation one correctly rounded fp32 operation, t = steps + 1:
 *     merge: score = beam_score[row] + lp; the group's B * 2B candidates ordered by score descending (a NaN ranks as -inf), then row
 *            ascending, then in-row rank ascending; the first 2B are walked in order, until B running beams are filled:
 *     walk:  the end id at merged rank < B: a finished hypothesis (score / norm[t], score, t, row); at rank >= B: skipped; any other id: the
 *            next running beam (tok, parent = the candidate's row, beam_score = score).
 *     heap:  appended while fin_count < B; otherwise it replaces the worst entry (lowest score, on ties the highest slot) when its score
 *            is strictly greater.
 *     done:  early_stopping: fin_count == B; otherwise fin_count == B and the worst entry's score >= best new beam_score / norm[t].  A
 *            group that becomes done takes one off live[0] (one vector atomic); this step's beams are still written.
 *     trellis[steps][row] = (tok, parent) for the group's rows; steps = t.
 *   write_index (1) int64, pos (R) int64, mask (R, capacity) float32, nullable TOGETHER: the decode step's bookkeeping exactly as
 *   qlinear_greedy_advance does it (pos += 1, write_index += 1, the new position unmasked in every row), for done groups as well.
 *   Every index is bounded by the arguments: trellis slot < cap, norm index <= cap, heap slot < B.
 *   QL_ERR_BAD_SHAPE for B outside [1, QL_BEAMS_MAX], P > 65535, cap < 1; QL_ERR_NULL_POINTER for a missing buffer or an incomplete
 *   bookkeeping triple; P == 0 is QL_OK without a launch.
 *
 * qlinear_beam_gather - the reorder of the key/value cache by parent beam, IN PLACE (a captured graph and pre-bound launches hold the
 * buffers' addresses): for every buffer of table (n_buf device int64 base addresses; layout (R, capacity, pos_bytes)), every position p in
 * [max(first[0], 0), min(end[0], capacity)) and every row r: buf[r][p] = buf[parent[r]][p].  first (1) int32 and end (1) int64 are device
 * memory (end: the step's write index, already advanced).  parent values are clamped to the row's own group, so no table content can
 * address outside the buffers.  A thread owns one chunk (16 bytes; 4 or 2 when pos_bytes is no multiple of 16 / 4) of one position across
 * the B rows of a group, loads all B, then stores the rows that change: cycles and duplicates in parent are safe.  A group whose parents
 * are the identity reads parent and exits.  The grid is fixed by capacity; workgroups past the range exit.  Every base address must be
 * aligned to the chunk size.
 *   QL_ERR_BAD_SHAPE for B outside [1, QL_BEAMS_MAX], P or n_buf > 65535, capacity < 1, pos_bytes < 2 or odd; QL_ERR_NULL_POINTER; n_buf == 0
 *   or P == 0 is QL_OK without a launch. */
#define QL_BEAMS_MAX 10
int qlinear_beam_advance(int64_t P, int64_t B, const int32_t* cand_ids, const float* cand_lp, int32_t* cand_count, float* beam_score,
                         int64_t* tok, int32_t* parent, int32_t* trellis, int64_t cap, int32_t* steps, float* fin_score, float* fin_sum,
                         int32_t* fin_len, int32_t* fin_row, int32_t* fin_count, int32_t* done, int32_t* live, const float* norm,
                         const int32_t* cfg, int64_t* write_index, int64_t* pos, float* mask, int64_t capacity, void* stream);
int qlinear_beam_gather(const int64_t* table, int64_t n_buf, int64_t P, int64_t B, int64_t capacity, int64_t pos_bytes, const int32_t* parent,
                        const int32_t* first, const int64_t* end, void* stream);

/* GPTQ (chatglm_q/int4/quantizer.py:151-167, chatglm_q/int8/quantizer.py:126-137): the column walk of ONE block of bc <= 128 input
 * columns over all weight rows in one launch.  All arrays fp32 device memory (dtype must be QL_DTYPE_F32).
 *   W (n_rows, row stride ldw): the working weights, nn.Linear layout; columns [c0, c0 + bc) are read, nothing is written back.
 *   hinv_block: address of Hinv[c0][c0] of the upper Cholesky factor of the inverse Hessian, row stride ldh; rows / columns
 *     [0, bc) of the block are read (the upper triangle and the diagonal).
 *   bits 4: group must be 32 (QL_ERR_UNSUPPORTED otherwise), bc and c0 multiples of it; scale is the (n_columns / group, lds)
 *     array, lds >= n_rows: rows c0 / group .. (c0 + bc) / group - 1, entries [0, n_rows), are WRITTEN.
 *   bits 8: any 1 <= bc <= 128; scale (n_rows) is READ; group and lds are ignored.
 *   Q, Err, Loss (n_rows, bc) contiguous: written.
 * Per row r, for j = 0 .. bc-1, every line ONE fp32 operation rounded to nearest (no fused multiply-add), w[] the row's current
 * block values, d = hinv_block[j][j], qmax = 7 / 127:
 *     bits 4, j % group == 0:  m = max_{t<group} |w[j+t]|;  s = max(m / 7.0f, 1e-10f);  scale[(c0+j)/group][r] = s
 *     bits 8:                  s = scale[r]
 *     x = w[j] / s;  c = min(max(rintf(x), -qmax), qmax);  q = s * c                    Q[r][j] = q
 *     e = w[j] - q;  Loss[r][j] = ((e * e) / (d * d)) * 0.5f;  err = e / d              Err[r][j] = err
 *     for t in j+1 .. bc-1:  p = err * hinv_block[j][t];  w[t] = w[t] - p
 * Rows are independent: one lane per row, every output element has one owner, plain vector loads and stores, no atomics.  Nothing
 * outside the stated ranges is touched.  The caller applies Err to the columns right of the block (W[:, c0+bc:] -= Err . Hinv[c0:c0+bc,
 * c0+bc:]) before the next block.
 * QL_ERR_BAD_DTYPE; QL_ERR_UNSUPPORTED for bits other than 4 / 8 or an int4 group other than 32; QL_ERR_BAD_SHAPE for bc outside
 * [1, 128], ldw < c0 + bc, ldh < bc, (int4) bc or c0 no multiple of the group or lds < n_rows; QL_ERR_NULL_POINTER; n_rows == 0 is QL_OK
 * without a launch. */
int qlinear_gptq_block(const float* W, int64_t n_rows, int64_t ldw, int64_t c0, int64_t bc, const float* hinv_block, int64_t ldh, int bits,
                       int64_t group, float* Q, float* Err, float* Loss, float* scale, int64_t lds, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QLINEAR_HIP_H */
