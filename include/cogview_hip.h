/*
 * cogview_hip.h -- C ABI of libcogview_hip.so, the MI355X (gfx950) implementation of the CogView
 * training/inference hot path.
 *
 * The reference (THUDM/CogView) has no FFI of its own: its hot path reaches native code through
 * torch/apex/cuBLAS Python calls.  Each entry point below replaces one such call site; the citation
 * (file:line under the reference tree) names the Python interface whose arithmetic it implements.  The
 * Python package `cogview_amd` binds these symbols with ctypes and re-exposes the reference's own module
 * surface (mpu.*, model.GPT2Model, fp16.*, vqvae.*) on top of them; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name says "host"; nothing is allocated inside;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and is stream-ordered;
 *   - dtype codes: COGV_F16=0 (IEEE half), COGV_BF16=1, COGV_F32=2; "T" below is the 16-bit storage type;
 *   - return value: 0 = ok, 1 = bad argument (shape / alignment / dtype), 2 = launch failure,
 *     3 = unsupported combination.  No exceptions, no errno, no global state.
 *   - row-major everywhere; leading dimensions are in ELEMENTS.
 *   - dropout masks are a pure function of (seed, stream_id, element index): a counter-based generator
 *     (PCG hash of the 8-element group counter, xorshift-expanded), 16 random bits per element, keep iff
 *     bits >= round(p*65536), kept values scaled by 65536/(65536-round(p*65536)).  The backward kernels
 *     regenerate masks from the same triple, so nothing is stored (and activation-checkpoint recompute
 *     replays identical masks: reference mpu/random.py:308-310,353-355 does this by saving RNG states).
 */
#ifndef COGVIEW_HIP_H
#define COGVIEW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COGV_F16 0
#define COGV_BF16 1
#define COGV_F32 2

/* ------------------------------------------------------------------ library */
int cogv_version(void);                 /* ABI version, currently 1 */
const char* cogv_arch(void);            /* "gfx950" */

/* ------------------------------------------------------------------ GEMM (MFMA)
 * C[M,N] = epilogue(A_op[M,K] . B_op[N,K]^T), fp32 accumulation.
 *   trans_a = 0: A stored [M][K] (lda >= K);  trans_a = 1: A stored [K][M] (lda >= M)
 *   trans_b = 0: B stored [N][K] (ldb >= K);  trans_b = 1: B stored [K][N] (ldb >= N)
 * replaces F.linear at mpu/layers.py:243 (ColumnParallelLinear.forward), mpu/layers.py:319
 * (RowParallelLinear.forward), model/gpt2_modeling.py:117 (tied logits) and their autograd
 * (dgrad: trans_b=1; wgrad: trans_a=trans_b=1).
 * epilogue order: +bias -> [store pre-activation or gelu' to aux] -> GeLU | x gelu'(aux) | x aux -> dropout -> +C -> round
 * -> abs-max.   GeLU is the tanh form of mpu/sparse_transformer.py:172-176.
 */
#define COGV_EPI_BIAS 1     /* + bias[n]                                                             */
#define COGV_EPI_GELU 2     /* out = gelu(x); if aux != NULL the rounded pre-activation is stored     */
#define COGV_EPI_DGELU 4    /* out = x * gelu'(aux[m][n])                                             */
#define COGV_EPI_DROPOUT 8  /* out = dropout(out), element index m*N+n; a dropped element is written as -0.0, and in   *
                             * a 16-bit output no kept element is (see cogv_sandwich_ln_bwd_marked; an fp32 output  *
                             * keeps the zero sign its kept fp32 value has; COGV_EPI_ACCUM adds C after the marks)  */
#define COGV_EPI_ABSMAX 16  /* atomicMax(*absmax, max|out|) -- feeds the Sandwich-LN scale            */
#define COGV_EPI_ACCUM 32   /* out += C (gradient accumulation / tied embedding)                      */
#define COGV_EPI_COLSUM 64  /* column sums of the (rounded) output per 128-row slab -> colsum_partial:      *
                             * the bias gradient of the layer that produced the GEMM's A operand, without  *
                             * re-reading the output (generation-3 kernel only: M, N >= 256, K % 64 == 0)  */

#define COGV_EPI_GELU_DAUX 128 /* with COGV_EPI_GELU: aux receives gelu'(pre-activation) instead of the pre-activation --  *
                                * same bytes; the backward GEMM then uses COGV_EPI_MULAUX (one multiply per element)  *
                                * where COGV_EPI_DGELU re-evaluates the sigmoid (exp2 + rcp per element)              */
#define COGV_EPI_MULAUX 256    /* out = x * aux[m][n] (autograd of gelu, mpu/sparse_transformer.py:172-179, through   *
                                * the stored derivative); exclusive with COGV_EPI_DGELU                               */

typedef struct cogv_gemm_desc {
  int dtype;            /* COGV_F16 | COGV_BF16 : type of A, B, bias, aux and (unless out_f32) C */
  int trans_a, trans_b;
  int M, N, K;
  const void* A; int lda;
  const void* B; int ldb;
  void* C; int ldc;
  int out_f32;          /* 1: C is float */
  int flags;            /* COGV_EPI_* */
  const void* bias;     /* [N] */
  void* aux; int ldaux; /* [M][ldaux] */
  float* absmax;        /* device scalar, caller zeroes it */
  float dropout_p; uint64_t seed; uint64_t stream_id;
  int splitk;           /* >1: contraction split over this many workgroups + reduce pass */
  int kernel_variant;   /* 0 = auto; 1 = generation 1 (register-staged 128x128x64); 3 = generation 2 (256x128x32 LDS-DMA ring); 9 = generation 3 (256x256x64, 8 waves ping-pong, persistent); 10 = generation 4 (256x256x64, 4 waves of 128x128, persistent: what auto picks for M, N >= 256) */
  void* workspace; size_t workspace_bytes;   /* >= cogv_gemm_workspace_bytes() when splitk > 1 */
  float* colsum_partial;                     /* COGV_EPI_COLSUM: [cogv_gemm_colsum_rows(M)][N] fp32, fully written */
  /* COGV_EPI_DROPOUT: this call computes rows [dropout_row0, dropout_row0 + M) of a larger [rows][N] tensor and draws the mask
   * of element (m, n) at linear index (dropout_row0 + m) * N + n -- a row-parallel Linear (mpu/layers.py:312-326) computed in
   * row chunks, each chunk's all-reduce running under the next chunk's GEMM, drops exactly what the whole-tensor call drops. */
  long long dropout_row0;
} cogv_gemm_desc;

int cogv_gemm(const cogv_gemm_desc* d, void* stream);
size_t cogv_gemm_workspace_bytes(const cogv_gemm_desc* d);
int cogv_gemm_pick_splitk(int M, int N, int K);
int cogv_gemm_colsum_rows(int M);            /* slabs of COGV_EPI_COLSUM partial sums: 2 * ceil(M / 256) */
/* out[n] (+)= sum over `rows` partial rows; the second half of cogv_colsum, also used after COGV_EPI_COLSUM */
int cogv_colsum_finalize(int dtype, const float* partial, int rows, int N, void* out, int accumulate, void* stream);
/* Up to 16 GEMMs of one dtype and layout (same trans_a / trans_b) in ONE persistent launch: the weight gradients
 * dW = dY^T X of the four linears of a layer -- or of several layers -- (autograd of mpu/layers.py:243,319) fill the
 * 256 CUs together where each alone would leave a partial last round.  COGV_ERR_UNSUPPORTED when a problem does not fit the 256x256x64
 * kernel (M, N >= 256, K % 64 == 0, A and B each span < 4 GiB): issue them one by one then.  Split-K as in cogv_gemm, per problem. */
int cogv_gemm_grouped(const cogv_gemm_desc* descs, int count, void* stream);
/* Note: the persistent GEMM kernel distributes tiles through per-XCD atomic work queues; the library keeps their
 * counters in 4 KiB of device memory per GPU that it allocates itself on the first GEMM call (its only allocation). */
int cogv_gemm_pick_splitk_tiles(int tiles_256x256, int K);
/* Model parallelism: the persistent GEMM kernels (one workgroup per CU, each owning its CU's register file) leave `n` CUs
 * free from now on (n = 0: none, the default; n < 0: query only) -- room for the channel workgroups of an all-reduce that
 * runs concurrently with the launch: the row-parallel Linear of mpu/layers.py:312-326 computed in row chunks, chunk i's
 * reduce (mpu/mappings.py:22-31) under chunk i + 1's GEMM.  Process-wide, not thread safe; returns the previous value. */
int cogv_gemm_reserve_cus(int n);
/* Host-only query (no device is touched, no pointer of a descriptor is dereferenced): what cogv_gemm (count = 0: descs[0] -- F.linear
 * at mpu/layers.py:243,319, model/gpt2_modeling.py:117 and their autograd) or cogv_gemm_grouped (count >= 1) would launch on a
 * device of num_cus CUs (0: this device's, 256 without one) under the current cogv_gemm_reserve_cus -- from the function those
 * launches use (csrc/gemm_plan.h) -- and exactly the error they would return before launching (out is left untouched then).
 * out: COGV_GEMM_PLAN_INTS ints per problem = { family (0: a tile kernel; 1: cogv_gemm's skinny-M case, the rest 0: see
 * cogv_gemv_plan), generation (1 .. 4 = kernel_variant 1, 3, 9, 10), tile M, tile N, tiles M, tiles N, effective splitk, k-tiles (of
 * 64) per split, first item of the problem in the launch's work list, items of the launch, grid x, grid y, threads, dynamic LDS
 * bytes, blocks of the split-K reduce (0: none), exact prefetch across items (generation 4), layout index (0 NT, 1 NN: trans_b,
 * 2 TN: both, 3: trans_a only) }. */
#define COGV_GEMM_PLAN_INTS 17
int cogv_gemm_plan(const cogv_gemm_desc* descs, int count, int num_cus, int* out);

/* Decode-step matrix-vector product with the layer's LayerNorms as prologue (M <= 8 rows, K = hidden size <= 4096,
 * K % 512 == 0; trans_a = trans_b = 0; epilogue flags BIAS | GELU | ABSMAX only; d->A is ignored):
 *     t    = gamma_post ? residual + LN_{eps (|z|max/8)^2}(z) * gamma_post + beta_post : z        (t_out, if given, receives t)
 *     x_in = LN_{eps (|t|max/8)^2}(t) * gamma + beta ;   C = epilogue(x_in . B^T)
 * i.e. mpu/sparse_transformer.py:326-341 -- `x + LN3(attn)` feeding `LN2`, or `y + LN4(mlp)` feeding the next layer's
 * `LN1` / the final LayerNorm -- fused into the GEMV that consumes it (every workgroup recomputes the few-KB vectors;
 * four Sandwich-LN launches per layer disappear from a decode step).  |t|max is taken over all M rows.  z_absmax: device
 * scalar with max|z| as z's producer published it (COGV_EPI_ABSMAX), or NULL: the kernel then takes max|z| itself (post-LN
 * form; same value, no atomics in the producer's tail) / max|t| (plain input). */
typedef struct cogv_ln_prologue {
  const void* z; const float* z_absmax;
  const void* gamma_post; const void* beta_post; const void* residual; void* t_out;
  const void* gamma; const void* beta;
  float eps;
  int stream_f32;      /* 1: residual, t_out and (without a post-LN) z are fp32 rows -- the fp32 residual stream (see
                          cogv_sandwich_ln_fwd); t is then formed and normalised without intermediate roundings */
} cogv_ln_prologue;
int cogv_gemv_ln(const cogv_gemm_desc* d, const cogv_ln_prologue* ln, void* stream);
/* Decode step, attention-output projection (mpu/sparse_transformer.py:163-166 after the attention of :652-673): the M <= 8
 * row matrix-vector product C = epilogue(att . B^T) whose input att [M][heads * 64] is COMBINED inside the kernel from the
 * split partials cogv_attention_decode left in its workspace (skip_combine = 1; `capacity` as in that call) -- one launch
 * per layer less than combine + GEMV.  d->A is ignored; K = heads * 64, K % 512 == 0; flags BIAS | ABSMAX only. */
int cogv_gemv_attn(const cogv_gemm_desc* d, const void* partials, int heads, int capacity, void* stream);

/* ------------------------------------------------------------------ 8-bit weights for the decode step (OCP E4M3, one scale per row)
 * A decode step (generation/sampling.py:139-148: one model call per generated token) reads every Linear weight once per
 * token: it is a weight stream, and its cost is the weights' bytes.  cogv_quantize_rows_e4m3 stores a weight matrix
 * W[N][K] (F16 | BF16, rows ldw elements apart) as q[N][K] uint8 in OCP E4M3 ("e4m3fn": no infinities, largest value 448;
 * rows ldq bytes apart) with one fp32 scale per row:
 *     scale[n] = max_k |W[n][k]| / 448 in fp32 (1.0 for an all-zero row);  q[n][k] = rne_e4m3(float(W[n][k]) / scale[n])
 * -- a true fp32 division, so torch's float8_e4m3fn conversion of w.float() / scale reproduces the bytes.  Deterministic, no
 * atomics.  K % 8 == 0, ldw % 8 == 0, ldq % 8 == 0 (the products below want ldq % 16 == 0 and q, scale 16-byte aligned).
 * Replaces nothing in the reference (it keeps fp16 weights: mpu/layers.py:243,319); it prepares the operand of the three
 * products below. */
int cogv_quantize_rows_e4m3(int dtype, const void* w, int ldw, int N, int K, void* q, int ldq, float* scale, void* stream);
/* The 8-bit weight operand: it takes the place of d->B / d->ldb (ignored) in the three calls below.  C[m][n] =
 * epilogue(scale[n] * sum_k X[m][k] * e4m3(q[n][k])): the bytes are converted exactly, the sum is the fp32 sum of the 16-bit
 * kernels, the scale multiplies it once, then the same fused epilogue (bias, GeLU, rounding to T, abs-max). */
typedef struct cogv_w8_weight {
  const void* q; int ldq;      /* [N][ldq] uint8 E4M3 */
  const float* scale;          /* [N] fp32 */
} cogv_w8_weight;
/* cogv_gemm's skinny case (M <= 8: F.linear at mpu/layers.py:243,319 and the tied logits model/gpt2_modeling.py:117 inside a
 * decode step) on an 8-bit weight; trans_a = trans_b = 0, flags BIAS | GELU | ABSMAX.  3 (unsupported) outside the kernels'
 * classes -- there is no other kernel to fall back to: M > 8, N % 8, K % 512, K > 10240, K not in {4096, 10240} above 5120
 * with M >= 2, more than 4 rows in a guarded class above K = 3072. */
int cogv_gemm_w8(const cogv_gemm_desc* d, const cogv_w8_weight* w, void* stream);
/* cogv_gemv_ln (mpu/sparse_transformer.py:326-341 fused into the consuming product) on an 8-bit weight; same arguments and
 * limits (K <= 4096; more than 4 rows: K <= 3072). */
int cogv_gemv_ln_w8(const cogv_gemm_desc* d, const cogv_ln_prologue* ln, const cogv_w8_weight* w, void* stream);
/* cogv_gemv_attn (the attention-output projection mpu/sparse_transformer.py:163-166 with the split combine as prologue) on
 * an 8-bit weight; bit-identical to the combine launch followed by cogv_gemm_w8. */
int cogv_gemv_attn_w8(const cogv_gemm_desc* d, const cogv_w8_weight* w, const void* partials, int heads, int capacity, void* stream);
/* Host-only query (no device is touched, no pointer of d or w is dereferenced): what the skinny-M product of `kind` would launch
 * for this descriptor -- cogv_gemm's M <= 8 case, cogv_gemv_attn, cogv_gemv_ln, or with w != NULL cogv_gemm_w8, cogv_gemv_attn_w8,
 * cogv_gemv_ln_w8 -- from the function those launches use, and their errors for the descriptor (1 bad argument, 3 not taken; out
 * is left untouched then).  nsplit: the key splits the attention kind combines ((capacity + 127) / 128; ignored otherwise).
 * out = { generation (2: a kernel of the class list in csrc/gemv_plan.h; 1: the first-generation kernel behind the 16-bit
 * products, also under COGV_GEMV2=0 -- the fields up to `two halves` are 0 then, rows excepted), form (0 V: one row, 1 M: 2 .. 8
 * rows on the matrix core), columns per wave J (V) | waves per 16-column tile NWK (M), 512-chunks of K KCMAX (V) | loads per lane
 * LMAX (M), guarded (1: a class for every K up to its maximum), rows MT (M rounded up to 1, 2, 4, 8), 16-column tiles per workgroup,
 * two halves (1: the x rows are staged in two halves of K), threads per workgroup, workgroups, dynamic LDS bytes }. */
#define COGV_GEMV_PLAIN 0
#define COGV_GEMV_ATTN 1
#define COGV_GEMV_LN 2
#define COGV_GEMV_PLAN_INTS 11
int cogv_gemv_plan(int kind, const cogv_gemm_desc* d, const cogv_w8_weight* w, int nsplit, int out[COGV_GEMV_PLAN_INTS]);

/* ------------------------------------------------------------------ 4-bit weights for the decode step (OCP MXFP4: E2M1 codes, one E8M0 scale per 32)
 * The second format of the decode step's weight stream (generation/sampling.py:139-148: one model call per generated token):
 * 0.53 bytes per weight.  cogv_quantize_rows_mxfp4 stores a weight matrix W[N][K] (F16 | BF16, rows ldw elements apart) as
 * q[N][K / 2] uint8 (rows ldq bytes apart; element 2i of a row is the low nibble of byte i, element 2i + 1 the high one; a nibble is
 * the sign in bit 3 and a 3-bit E2M1 code of the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6) and scale[N][K / 32] uint8 (rows lds
 * bytes apart; an E8M0 exponent per block of 32 consecutive elements of a row, value 2^(scale - 127)).  Per block, amax = max |x|:
 *     e = clamp(floor(log2(amax)) - 2, -126, 127), scale = e + 127 (127 for an all-zero block; never 0, never 255);
 *     code = the E2M1 value nearest to float(x) / 2^e, ties to the even code, magnitudes above 6 saturate to 6
 * -- integer arithmetic on the bit patterns, which a CPU reproduces exactly (ops.dequantize_rows_mxfp4 reads the result back).  A
 * code of magnitude zero may carry either sign bit; NaN and infinity are outside the contract.  Deterministic, no atomics.
 * K % 32 == 0, ldw % 8 == 0, ldq % 4 == 0, ldq >= K / 2, lds >= K / 32, w 16-byte and q 4-byte aligned, else 1; fp16 / bf16, else 3
 * (the products below want ldq % 16 == 0 and q 16-byte aligned).  Replaces nothing in the reference (it keeps fp16 weights:
 * mpu/layers.py:243,319); it prepares the operand of the three products below. */
int cogv_quantize_rows_mxfp4(int dtype, const void* w, int ldw, int N, int K, void* q, int ldq, void* scale, int lds, void* stream);
/* The 4-bit weight operand: it takes the place of d->B / d->ldb (ignored) in the three calls below.  C[m][n] =
 * epilogue(sum_k X[m][k] * code(q[n][k]) * 2^(scale[n][k / 32] - 127)): the codes are converted with their block scale folded in
 * (exact in fp32 and bf16; in fp16 wherever the value is a multiple of 2^-24 below 65520), the sum is the fp32 sum of the 16-bit
 * kernels, then the same fused epilogue (bias, GeLU, rounding to T, abs-max). */
typedef struct cogv_w4_weight {
  const void* q; int ldq;      /* [N][ldq] uint8: two E2M1 codes per byte */
  const void* scale; int lds;  /* [N][lds] uint8: E8M0 block scales */
} cogv_w4_weight;
/* cogv_gemm's skinny case (M <= 8: F.linear at mpu/layers.py:243,319 and the tied logits model/gpt2_modeling.py:117 inside a
 * decode step) on a 4-bit weight; trans_a = trans_b = 0, flags BIAS | GELU | ABSMAX.  1 for a NULL or misaligned operand or lds <
 * K / 32; 3 (unsupported) outside the kernels' classes -- there is no other kernel to fall back to: M > 8, N % 8, K % 512,
 * K > 10240, K not in {4096, 10240} above 5120 with M >= 2, more than 4 rows in a guarded class above K = 3072. */
int cogv_gemm_w4(const cogv_gemm_desc* d, const cogv_w4_weight* w, void* stream);
/* cogv_gemv_ln (mpu/sparse_transformer.py:326-341 fused into the consuming product) on a 4-bit weight; same arguments, errors
 * and limits (K <= 4096; more than 4 rows: K <= 3072). */
int cogv_gemv_ln_w4(const cogv_gemm_desc* d, const cogv_ln_prologue* ln, const cogv_w4_weight* w, void* stream);
/* cogv_gemv_attn (the attention-output projection mpu/sparse_transformer.py:163-166 with the split combine as prologue) on a
 * 4-bit weight; bit-identical to the combine launch followed by cogv_gemm_w4. */
int cogv_gemv_attn_w4(const cogv_gemm_desc* d, const cogv_w4_weight* w, const void* partials, int heads, int capacity, void* stream);
/* cogv_gemv_plan for the three calls above (w != NULL, else 1): host only, the same 11 integers, the same errors as the launches.
 * The J of a one-row class counts columns per wave as ever; a wave's slot covers 2048 contraction elements of a column here. */
int cogv_gemv_w4_plan(int kind, const cogv_gemm_desc* d, const cogv_w4_weight* w, int nsplit, int out[COGV_GEMV_PLAN_INTS]);

/* Wide decode step: F.linear at mpu/layers.py:243,319 and the tied logits model/gpt2_modeling.py:117 inside a decode step of up
 * to 64 rows (9 and more: the reference's --max-inference-batch-size defaults to 12), as a weight stream like cogv_gemm's skinny
 * case: every byte of B is requested once, by one workgroup.  C[M][N] = epilogue(A[M][K] . B[N][K]^T) on 16-bit weights with
 * 1 <= M <= 64, N >= 8, N % 8 == 0, 512 <= K <= 10240, K % 512 == 0, trans_a = trans_b = 0, flags BIAS | GELU | ABSMAX (the skinny
 * case's epilogue, rounding point for rounding point), no aux, 16-bit C.  1 (bad argument) as cogv_gemm reports it, and for a
 * leading dimension shorter than its row; 3 (unsupported) for every other descriptor: this entry point has no other kernel.
 * Deterministic; a row's bits do not depend on the other rows of the call; no floating-point atomics. */
int cogv_gemm_rows(const cogv_gemm_desc* d, void* stream);
/* Host-only query (no device is touched, no pointer of d is dereferenced): what cogv_gemm_rows would launch for this descriptor,
 * from the function the launch uses (csrc/gemv_wide_plan.h), and exactly the error it would return (out is left untouched then).
 * out = { row groups RG = ceil(M / 16) (accumulator tiles per column tile), waves per 16-column tile NWK (they split the
 * contraction), column tiles per workgroup (1 | 2), weight loads of 16 bytes per lane, guarded (1: a class for every K up to its
 * maximum), contraction elements of x staged in LDS per phase (0: x is read from L2 as MFMA fragments, never staged), threads per
 * workgroup, workgroups, dynamic LDS bytes (the partial tiles of the tail), load pairs a wave keeps in flight (= weight loads / (2 *
 * tiles): every load is requested at the top) }. */
#define COGV_GEMM_ROWS_PLAN_INTS 10
int cogv_gemm_rows_plan(const cogv_gemm_desc* d, int out[COGV_GEMM_ROWS_PLAN_INTS]);
/* cogv_gemm_rows (F.linear at mpu/layers.py:243,319 and the tied logits model/gpt2_modeling.py:117 inside a decode step of 9 to 64
 * rows) on an 8-bit weight: the operand of cogv_gemm_w8 in d->B / d->ldb's place (ignored), C[m][n] = epilogue(scale[n] * sum_k
 * A[m][k] * e4m3(q[n][k])) with the bytes converted exactly and the scale multiplied into the finished fp32 sum once.  The
 * arguments, limits, errors and guarantees of cogv_gemm_rows (1 <= M <= 64, 512 <= K <= 10240, K % 512 == 0, flags BIAS | GELU |
 * ABSMAX; deterministic, a row's bits do not depend on the other rows, no floating-point atomics), and 1 for a NULL operand, q or
 * scale not 16-byte aligned, ldq % 16 or ldq < K.  cogv_gemm_w8 keeps refusing M > 8: above 8 rows this is the entry point. */
int cogv_gemm_rows_w8(const cogv_gemm_desc* d, const cogv_w8_weight* w, void* stream);
/* cogv_gemm_rows (mpu/layers.py:243,319, model/gpt2_modeling.py:117 inside a decode step of 9 to 64 rows) on a 4-bit weight: the
 * operand of cogv_gemm_w4, C[m][n] = epilogue(sum_k A[m][k] * code(q[n][k]) * 2^(scale[n][k / 32] - 127)), the block scale folded
 * into the conversion as there.  As cogv_gemm_rows_w8; 1 for a NULL operand, q not 16-byte aligned, ldq % 16, ldq < K / 2 or
 * lds < K / 32. */
int cogv_gemm_rows_w4(const cogv_gemm_desc* d, const cogv_w4_weight* w, void* stream);
/* cogv_gemm_rows_plan for the two calls above (the products of mpu/layers.py:243,319 and model/gpt2_modeling.py:117 on a quantized
 * weight): host only, no device is touched and no pointer of d or w is dereferenced; the same 10 integers from the function the
 * launches use (csrc/gemv_wide_plan.h, GWQ_CLASSES), exactly the error the launch would return.  A wave's unit of the contraction
 * is 128 elements here (two 16-byte loads of E4M3 bytes, one of MXFP4 codes): out[3] counts 16-byte weight loads per lane as
 * ever, out[9] the units a wave keeps in flight. */
int cogv_gemm_rows_w8_plan(const cogv_gemm_desc* d, const cogv_w8_weight* w, int out[COGV_GEMM_ROWS_PLAN_INTS]);
int cogv_gemm_rows_w4_plan(const cogv_gemm_desc* d, const cogv_w4_weight* w, int out[COGV_GEMM_ROWS_PLAN_INTS]);

/* ------------------------------------------------------------------ Sandwich-LN
 * y = [residual +] LayerNorm_{eps*(amax/8)^2}(x) * gamma + beta ; amax = *absmax_in (NULL: plain LN).
 * replaces mpu/sparse_transformer.py:40-44 (LayerNorm = FusedLayerNorm(x / (x.abs().max()/8))) and the
 * residual adds at :329 and :340.  mean/rstd ([rows] fp32, may be NULL) are saved for backward.
 * absmax_out (may be NULL): atomicMax of |y| -- the next LayerNorm's scale.
 * stream_mode -- which tensors are the fp32 RESIDUAL STREAM of the transformer (the hidden state that runs through the
 * layer loop mpu/sparse_transformer.py:571-613 and its gradient; kept in fp32 so that depth does not cost precision):
 *   COGV_LN_ALL_T       every tensor in the storage type T (stand-alone LayerNorm; with a residual the LN output is
 *                       rounded to T before the add, the reference's rounding point at :326-329)
 *   COGV_LN_STREAM_IN   x (backward: x, add_in, dx) fp32, y (backward: dy) T -- LN1, LN2, final LN; no residual
 *   COGV_LN_STREAM_OUT  x (backward: x, dx) T, residual and y (backward: dy) fp32 -- LN3, LN4; residual required,
 *                       y = residual + LN(x) evaluated in fp32 without an intermediate rounding
 */
#define COGV_LN_ALL_T 0
#define COGV_LN_STREAM_IN 1
#define COGV_LN_STREAM_OUT 2
int cogv_sandwich_ln_fwd(int dtype, const void* x, const void* gamma, const void* beta, const void* residual,
                         void* y, float* mean, float* rstd, const float* absmax_in, float* absmax_out,
                         int rows, int h, float eps, int stream_mode, void* stream);
/* dx = [add_in +] dropout_mask( LN'(dy) ) ; dgamma/dbeta/colsum (T, [h], any may be NULL) get the column
 * reductions (colsum = column sums of the written dx: the bias gradient of the Linear that produced x). */
int cogv_sandwich_ln_bwd(int dtype, const void* dy, const void* x, const void* gamma, const float* mean,
                         const float* rstd, const void* add_in, void* dx, void* dgamma, void* dbeta, void* colsum,
                         int accumulate_param_grads, int rows, int h, float dropout_p, uint64_t seed,
                         uint64_t stream_id, void* workspace, size_t workspace_bytes, int stream_mode, void* stream);
/* The same with the dropout mask READ FROM x (round 6; COGV_LN_ALL_T / COGV_LN_STREAM_OUT: x is 16-bit): cogv_gemm's dropout
 * epilogue (COGV_EPI_DROPOUT) writes every dropped element as -0.0 and never writes a kept element as -0.0 ("marked zeros";
 * numerically the reference's dropout(x), mpu/sparse_transformer.py:163-168,231-233), so "16-bit pattern 0x8000" IS the forward
 * mask and the backward of the Sandwich-LN that follows that GEMM (mpu/sparse_transformer.py:326-329,337-340) needs neither
 * the generator nor stored bits.  dropout_p only supplies the scale 1 / (1 - p) (same 16-bit threshold arithmetic as the
 * replaying form; 0 = no dropout).  Bit-identical to cogv_sandwich_ln_bwd with the producing GEMM's (p, seed, stream). */
int cogv_sandwich_ln_bwd_marked(int dtype, const void* dy, const void* x, const void* gamma, const float* mean,
                                const float* rstd, const void* add_in, void* dx, void* dgamma, void* dbeta, void* colsum,
                                int accumulate_param_grads, int rows, int h, float dropout_p, void* workspace,
                                size_t workspace_bytes, int stream_mode, void* stream);
/* LN2' and LN3' of a transformer layer in ONE pass over their rows (round 6).  In backward the two Sandwich-LNs are neighbours
 * with no GEMM between them (mpu/sparse_transformer.py:326-341 read backwards: y = x + LN3(ao) feeds LN2 and the second
 * residual add):
 *     dy   = dout + LN2'(dc ; y)        dc [rows][h] T, y / dout / dy fp32 (the residual stream and its gradient)
 *     d_ao = mask( LN3'(dy ; ao) )      ao / d_ao T; dropout_p > 0: ao carries cogv_gemm's marked zeros (see above), 0: no mask
 * dy still goes to memory (LN1' adds it later) but is not read back: 18 instead of 22 bytes per element for the pair.  dy and
 * d_ao are bit-identical to cogv_sandwich_ln_bwd(STREAM_IN, add_in = dout) followed by cogv_sandwich_ln_bwd_marked(STREAM_OUT);
 * the five column reductions (dgamma2, dbeta2, dgamma3, dbeta3, colsum of d_ao; T, [h], any may be NULL) equal theirs up to the
 * fp32 summation order.  1536 < h <= 4096, h % 8 == 0: at least four waves per row (narrower rows: COGV_ERR_UNSUPPORTED, issue
 * the two launches). */
int cogv_sandwich_ln_bwd_pair(int dtype, const void* dc, const void* y, const void* gamma2, const float* mean2,
                              const float* rstd2, const void* dout, void* dy, void* dgamma2, void* dbeta2,
                              const void* ao, const void* gamma3, const float* mean3, const float* rstd3, void* d_ao,
                              void* dgamma3, void* dbeta3, void* colsum, int accumulate_param_grads, int rows, int h,
                              float dropout_p, void* workspace, size_t workspace_bytes, void* stream);
size_t cogv_ln_bwd_pair_workspace_bytes(int rows, int h);
size_t cogv_ln_bwd_workspace_bytes(int rows, int h);
int cogv_ln_bwd_num_blocks(int rows);   /* upper bound of the backward kernel's workgroup count (workspace sizing) */
/* Host-only queries (no device is touched): what cogv_sandwich_ln_bwd[_marked] (marked = 1: the _marked entry point) and
 * cogv_sandwich_ln_bwd_pair would launch for these arguments, from the function the launch itself uses.  out = { rows in flight,
 * lean form, mask from marked zeros, workgroups, threads per workgroup }; the argument errors of the launching entry points. */
int cogv_ln_bwd_plan(int stream_mode, int rows, int h, float dropout_p, int marked, int has_add_in, int out[5]);
int cogv_ln_bwd_pair_plan(int rows, int h, float dropout_p, int out[5]);

/* ------------------------------------------------------------------ attention (head dim 64)
 * replaces standard_attention, mpu/sparse_transformer.py:652-673, plus the head permutes at :112-120,:159.
 * Tensor element (b, row, head, d) lives at base + b*bs + row*rs + head*64 + d.
 * Mask: key j visible to query i iff j <= i + (s_k - s_q) or j < sep + (s_k - s_q) (sep = 0: causal);
 * masked scores are exactly -10000 as in the reference.  lse: [B][H][s_q] fp32; dvec: backward workspace
 * [2][B][H][s_q] 4-byte words (softmax-backward row term D, then the per-row dropout keys), written by the dQ kernel.
 */
typedef struct cogv_attn_desc {
  int dtype; int B, H, s_q, s_k, head_dim; int sep;
  float scale;                       /* 1/sqrt(head_dim), applied to QK^T */
  float dropout_p; uint64_t seed; uint64_t stream_id;
  const void* q; const void* k; const void* v; void* o;
  const void* dout; void* dq; void* dk; void* dv;
  float* lse; float* dvec;
  long long q_bs, k_bs, v_bs, o_bs, do_bs, dq_bs, dk_bs, dv_bs;
  int q_rs, k_rs, v_rs, o_rs, do_rs, dq_rs, dk_rs, dv_rs;
  /* backward only, optional: per-workgroup column sums of the stored dq | dk | dv (the bias gradient of the fused
   * QKV projection, mpu/sparse_transformer.py:101-110) -> colsum_partial[B * ceil(s/128)][3 * H * 64] fp32, columns
   * ordered [q heads | k heads | v heads]; requires s_q == s_k; finish with cogv_colsum_finalize. */
  float* colsum_partial;
  /* optional (forward only unless sparse_window > 0): gathered keys (sparse_attention_inference, mpu/sparse_transformer.py:727-750): key slot j of
   * batch b is row kv_index[b * kv_index_bs + j] of k and v; s_k is the number of slots (<= 4096).  The left-to-right
   * rule applies to SLOTS: the last s_q slots are the queries' own positions.  Bit 31 of an entry marks a masked slot
   * (score -10000): a decode step over a fixed-capacity key/value cache flags the slots it has not written yet, so the
   * launch parameters stay constant from step to step (HIP-graph replay, cogview_amd/generation/decoder.py). */
  const int* kv_index; long long kv_index_bs;
  /* sparse TRAINING form (sparse_attention, mpu/sparse_transformer.py:675-725) in "slot space": sparse_window > 0 (the
   * reference's query_window, a multiple of 128 dividing s_q).  Each block of sparse_window queries has its own index
   * row (kv_index_gs entries apart) of s_k slots: first sparse_pivots pivot slots, then the key_window_times *
   * sparse_window window slots ending with the block's own positions.  Bit 31 of an entry marks a masked slot (an
   * invisible pivot, front padding): score -10000.  Pivot slots add sparse_pivot_bias = log(s // n_pivots) to the
   * scaled score; the left-to-right rule applies to the last sparse_window slots. */
  long long kv_index_gs; int sparse_window, sparse_pivots; float sparse_pivot_bias;
  /* optional (dense form, dropout_p > 0): cogv_attention_keep_bits_bytes(B, H, s_q, s_k) bytes, 4-byte aligned.  The forward
   * call WRITES the keep decisions of its attention dropout there (1 bit per score the kernel evaluated: the reference's
   * dropout mask at mpu/sparse_transformer.py:667-669, which autograd keeps for the backward pass); the backward call given
   * the same buffer READS them instead of regenerating the draws.  Results are bit-identical with and without it.  NULL:
   * backward regenerates (also for the gathered / sparse forms, which ignore the field). */
  void* keep_bits;
  /* optional (dense form only; excludes kv_index and keep_bits): an ARBITRARY mask tensor M in the storage type, [B][s_q][s_k]
   * (mask_bs = s_q * s_k) or [s_q][s_k] shared by the batch (mask_bs = 0), applied exactly as the reference does for any
   * real M -- scaled score * M - 10000 * (1 - M), mpu/sparse_transformer.py:661-663 -- in forward and backward; `sep` is ignored
   * (no left-to-right rule: the tensor decides).  The left-to-right masks the reference's callers build go through `sep`
   * instead (causal block skipping); this is the general path of the module surface, not a hot path. */
  const void* mask; long long mask_bs;
} cogv_attn_desc;
int cogv_attention_fwd(const cogv_attn_desc* d, void* stream);
int cogv_attention_bwd(const cogv_attn_desc* d, void* stream);
/* Host-only query (no device is touched, none of the descriptor's pointers is dereferenced): what cogv_attention_fwd (backward = 0)
 * or cogv_attention_bwd (backward = 1) would launch for this descriptor, from the function the launch itself uses, and the argument
 * errors of those entry points (out is left untouched then).  out = { form (0 dense without dropout, 1 dense regenerating the
 * dropout draws, 2 dense with stored keep bits, 3 flexible: gathered / sparse keys, mask tensor), threads per workgroup,
 * workgroups and dynamic LDS bytes of the forward or dQ launch, workgroups and dynamic LDS bytes of the dK.dV launch (0 forward),
 * planes of the dK.dV grid (B; sparse training form backward: B * s_q / sparse_window), sep_k: keys [0, sep_k) are visible to
 * every query (a mask tensor: s_k) }. */
int cogv_attention_plan(const cogv_attn_desc* d, int backward, int out[8]);
size_t cogv_attention_keep_bits_bytes(int B, int H, int s_q, int s_k);
/* Decode step (generation/sampling.py:139-148: one model call per generated token; mems mpu/sparse_transformer.py:526-546):
 * ONE query token per batch row against a fixed-capacity key/value cache.  qkv: the QKV projection of the new token,
 * [B][3 * H * 64] = q | k | v (qkv_bs elements between batch rows); cache: [B][capacity][2 * H * 64] keys | values
 * (cache_bs / cache_rs: batch / slot strides in elements).  *pos (device int64) = slot of the new token = number of
 * slots already valid: the kernel attends slots [0, *pos] -- the new token's key / value are taken from qkv and WRITTEN
 * into slot *pos -- so no launch parameter depends on the length (HIP-graph replay).  out: [B][H * 64] (out_bs elements
 * between rows).  Keys are split over workgroups (capacity / 128 per head); a second launch combines the partial softmax
 * results in split order.  workspace: cogv_attention_decode_workspace_bytes() bytes (partials; no initialisation needed).
 * first (optional; NULL: the launch described above, the same kernel and the same bits): device int32 [B], 4-byte aligned
 * (else 1, bad argument).  Row b attends slots [first[b], *pos]: the rows of one launch hold right-aligned contexts of
 * different lengths (generate_samples.py:202-221 walks a file of prompts; here several of them share one decode step), slots
 * below first[b] are padding and have no influence whatever they hold, NaN included.  first[b] < 0 counts as 0; first[b] >
 * *pos attends the new token's own slot only.  A key split that lies wholly in the padding leaves the partial (-inf, 0,
 * 0...) that a split past *pos leaves.  Only slot *pos is written, as without it. */
typedef struct cogv_attn_decode_desc {
  int dtype; int B, H, capacity, head_dim;
  float scale;                       /* 1/sqrt(head_dim) */
  const void* qkv; long long qkv_bs;
  void* cache; long long cache_bs; int cache_rs;
  void* out; long long out_bs;
  const long long* pos;
  void* workspace; size_t workspace_bytes;
  int skip_combine;                  /* 1: leave the split partials in `workspace` (66 floats per (row, head, split): max,
                                        sum, 64 outputs) for cogv_gemv_attn to combine; `out` is not written and may be NULL */
  const int* first;                  /* NULL, or int32 [B]: row b attends slots [first[b], *pos] */
} cogv_attn_decode_desc;
size_t cogv_attention_decode_workspace_bytes(int B, int H, int capacity);
int cogv_attention_decode(const cogv_attn_decode_desc* d, void* stream);
/* Decode step of m tokens per cache row (generation/sampling.py:139-148 makes one model call per token, also for a token that
 * is already known; a run of m known tokens is one call here).  Rows r = b * m + j, j = 0 ... m - 1, as the QKV projection of
 * [B * m] hidden rows leaves them: qkv [B * m][3 * H * 64] (qkv_rs elements between consecutive rows), out [B * m][H * 64]
 * (out_rs).  Row (b, j) is the token in slot *pos + j of cache row b and attends slots [first[b], *pos + j]; the keys / values
 * of slots [*pos, *pos + j] are the chunk's own rows, taken from qkv, and all m of them are WRITTEN into slots [*pos, *pos + m).
 * A slot at or past `capacity` is neither written nor attended, whatever *pos holds.  first: as in cogv_attn_decode_desc, per
 * row (b, j) against its own slot (NULL: 0; negative: 0; beyond *pos + j: that slot only).  *pos stays device data and the
 * cache loads are issued before it is read.  Grid, the 128 keys per split and the 66-float partials are those of
 * cogv_attention_decode with B * m rows -- workspace: cogv_attention_decode_workspace_bytes(B * m, H, capacity); skip_combine,
 * cogv_gemv_attn and cogv_gemv_attn_w8 (M = B * m) as there -- but a workgroup loads its 128 keys and values ONCE for the m
 * queries.  Output, partials and cache are bit-identical to m successive cogv_attention_decode calls at *pos, *pos + 1, ...;
 * m = 1 is that call.  The 8-bit cache's form is cogv_attention_decode_chunk_kv8.
 * 1 (bad argument): m outside [1, 8], misaligned qkv / cache (16 B) / first (4 B), strides % 8, short workspace; 3
 * (unsupported): other dtypes, head_dim != 64. */
typedef struct cogv_attn_decode_chunk_desc {
  int dtype; int B, H, capacity, head_dim;
  int m;                             /* tokens per cache row, 1 ... 8 */
  float scale;                       /* 1/sqrt(head_dim) */
  const void* qkv; long long qkv_rs;
  void* cache; long long cache_bs; int cache_rs;
  void* out; long long out_rs;
  const long long* pos;
  void* workspace; size_t workspace_bytes;
  int skip_combine;
  const int* first;                  /* NULL, or int32 [B] */
} cogv_attn_decode_chunk_desc;
int cogv_attention_decode_chunk(const cogv_attn_decode_chunk_desc* d, void* stream);
/* ------------------------------------------------------------------ 8-bit key/value cache for the decode step (OCP E4M3, one scale per head)
 * The decode attention requests every slot of the fixed-capacity cache on every step (generation/sampling.py:139-148: one
 * model call per generated token), so a step streams the whole cache.  Here the cache holds E4M3 bytes with one fp32 scale per
 * (slot, head, K | V), head-major:
 *     q     uint8 [B][2][H][capacity][64]   plane 0: keys, plane 1: values   (q_bs: BYTES between batch rows)
 *     scale fp32  [B][2][H][capacity]                                        (scale_bs: floats between batch rows)
 * by the rule of cogv_quantize_rows_e4m3 on the 64 elements of one head of one slot: scale = max|x| / 448 (1.0 when all are
 * zero), q = rne_e4m3(float(x) / scale) with a true fp32 division.  136 bytes per (slot, head) for its key and value instead of 256.
 * cogv_kv_quantize_e4m3 (the memories of a prefill, mpu/sparse_transformer.py:526-546): kv = the 16-bit K | V rows
 * [B][n][2 * H * 64] (kv_bs / kv_rs: batch / row strides in elements) -> slots [slot0, slot0 + n) of q / scale; bit-identical to
 * cogv_quantize_rows_e4m3 on the [rows, 64] view.  q 16-byte aligned, scale 4-byte; fp16 / bf16, else 3 (unsupported). */
int cogv_kv_quantize_e4m3(int dtype, const void* kv, long long kv_bs, long long kv_rs, int B, int n, int H, void* q, long long q_bs,
                          float* scale, long long scale_bs, int capacity, int slot0, void* stream);
/* cogv_attention_decode on that cache (generation/sampling.py:139-148): same contract -- one query row per batch row, slots
 * [0, *pos] attended, *pos device data, every load issued before it is read, slots past *pos or the capacity without influence
 * whatever bytes they hold -- except that the new token's key / value are QUANTIZED FIRST, stored into slot *pos as bytes +
 * scale, and attended in their dequantized form (a token's key has one value in every step that reads it).  128 keys per split
 * and the 66-float partials of cogv_attention_decode: workspace, skip_combine, cogv_gemv_attn and cogv_gemv_attn_w8 as there.
 * first: as in cogv_attn_decode_desc (NULL: slots [0, *pos], the same kernel and bits as without the field); a padding slot's
 * bytes AND scales are without influence.
 * 1 (bad argument): misaligned kv_q (16 B) / kv_scale (4 B) / first (4 B), head_dim != 64, short workspace; 3 (unsupported):
 * other dtypes. */
typedef struct cogv_attn_decode_kv8_desc {
  int dtype; int B, H, capacity, head_dim;
  float scale;                       /* 1/sqrt(head_dim) */
  const void* qkv; long long qkv_bs;
  void* kv_q; long long kv_q_bs;
  float* kv_scale; long long kv_scale_bs;
  void* out; long long out_bs;
  const long long* pos;
  void* workspace; size_t workspace_bytes;
  int skip_combine;
  const int* first;
} cogv_attn_decode_kv8_desc;
/* one decode step's attention per layer on the 8-bit cache (the model call of generation/sampling.py:139-148) */
int cogv_attention_decode_kv8(const cogv_attn_decode_kv8_desc* d, void* stream);
/* cogv_attention_decode_chunk on that cache (generation/sampling.py:139-148 makes one model call per token, also for a token that
 * is already known; a run of m known tokens is one call here, on the 8-bit cache as on the 16-bit one).  Rows r = b * m + j: qkv
 * [B * m][3 * H * 64] (qkv_rs), out [B * m][H * 64] (out_rs), as in cogv_attn_decode_chunk_desc; kv_q / kv_scale as in
 * cogv_attn_decode_kv8_desc.  The chunk's m keys and m values are QUANTIZED FIRST (the rule of cogv_kv_quantize_e4m3), WRITTEN into
 * slots [*pos, *pos + m) below the capacity as bytes + scales, and attended in their dequantized form; row (b, j) attends slots
 * [first[b], *pos + j].  A slot that a row does not attend -- past its own, below first[b], at or past the capacity -- is without
 * influence whatever bytes AND scales it holds (NaN included); a row whose slot lies at or past the capacity writes nothing and
 * attends [first[b], capacity).  *pos stays device data and the cache loads are issued before it is read.  Grid, the 128 keys per
 * split and the 66-float partials are cogv_attention_decode's with B * m rows: workspace
 * cogv_attention_decode_workspace_bytes(B * m, H, capacity); skip_combine, cogv_gemv_attn and cogv_gemv_attn_w8 (M = B * m) as
 * there.  Output, partials and the cache's bytes and scales are bit-identical to m successive cogv_attention_decode_kv8 calls at
 * *pos, *pos + 1, ...; m = 1 is that call.
 * 1 (bad argument): m outside [1, 8], B * m > 2^20, misaligned qkv / kv_q (16 B) / kv_scale / first (4 B), qkv_rs % 8, kv_q_bs % 16,
 * short kv_q_bs / kv_scale_bs / workspace; 3 (unsupported): a NULL descriptor, other dtypes, head_dim != 64. */
typedef struct cogv_attn_decode_chunk_kv8_desc {
  int dtype; int B, H, capacity, head_dim;
  int m;                             /* tokens per cache row, 1 ... 8 */
  float scale;                       /* 1/sqrt(head_dim) */
  const void* qkv; long long qkv_rs;
  void* kv_q; long long kv_q_bs;
  float* kv_scale; long long kv_scale_bs;
  void* out; long long out_rs;
  const long long* pos;
  void* workspace; size_t workspace_bytes;
  int skip_combine;
  const int* first;                  /* NULL, or int32 [B] */
} cogv_attn_decode_chunk_kv8_desc;
int cogv_attention_decode_chunk_kv8(const cogv_attn_decode_chunk_kv8_desc* d, void* stream);
/* Sparse training form, backward: cogv_attention_bwd with sparse_window > 0 writes dq as usual, but dk / dv are
 * SLOT-SPACE buffers [B * s_q / sparse_window][s_k slots][H][64] (dk_bs / dv_bs = the stride of one (batch, query block)
 * plane) -- the gradient of each gathered copy of a key, the same quantity the reference's autograd holds for pivot_k
 * / window_k before torch.gather / the padded-window view scatter it back (mpu/sparse_transformer.py:689-705).
 * cogv_sparse_slot_reduce folds them onto the keys: dk[b][r] = sum over the window slots of r (blocks r/w ... r/w +
 * times - 1) + the pivot slot pivot_inv[b][r] (-1: r is no pivot; pivots are distinct per sample, as the reference's
 * random.sample draws them) of the blocks that see it.  fp32 sums in a fixed order (deterministic).
 * dk_slots / dv_slots: contiguous [B][s / window][n_pivots + times * window][H * 64]. */
int cogv_sparse_slot_reduce(int dtype, const void* dk_slots, const void* dv_slots, const int* pivot_inv, void* dk, void* dv,
                            long long dk_bs, int dk_rs, long long dv_bs, int dv_rs, int B, int s, int H, int window,
                            int times, int n_pivots, void* stream);

/* ------------------------------------------------------------------ embedding
 * out = dropout( table[ids - vocab_start] (0 outside the shard) [+ pos_table[pos_ids]] ), abs-max of out.
 * replaces VocabParallelEmbedding.forward mpu/layers.py:117-133 and the position add + dropout at
 * mpu/sparse_transformer.py:522-524.  ids == NULL: the word part is read from x_in (model-parallel path,
 * after the all-reduce).  Backward: dtable[id] += the fp32 sum, in ascending token order, of the (dropout-masked)
 * gradient rows of the tokens carrying id, rounded once (torch's embedding_dense_backward under
 * mpu/layers.py:117-133 accumulates in fp32 too); dpos likewise per position id.  Deterministic: no floating-point
 * atomics.  workspace: cogv_embedding_bwd_workspace_bytes(vocab_end - vocab_start (0 without dtable), n_pos (0 without
 * dpos)) bytes of scratch, 16-byte aligned (cleared by the call itself).
 */
int cogv_embedding_fwd(int dtype, const int64_t* ids, const void* table, int64_t vocab_start, int64_t vocab_end,
                       const void* x_in, const int64_t* pos_ids, const void* pos_table, int64_t n_pos, void* out,
                       float* absmax_out, int64_t n_tok, int h, float dropout_p, uint64_t seed, uint64_t stream_id,
                       int out_f32, void* stream);
int cogv_embedding_bwd(int dtype, const void* dout, const int64_t* ids, void* dtable, int64_t vocab_start,
                       int64_t vocab_end, const int64_t* pos_ids, void* dpos, int64_t n_pos, void* dx,
                       int64_t n_tok, int h, float dropout_p, uint64_t seed, uint64_t stream_id, void* workspace,
                       size_t workspace_bytes, int dout_f32, void* stream);
size_t cogv_embedding_bwd_workspace_bytes(int64_t table_rows, int64_t n_pos);

/* ------------------------------------------------------------------ element-wise (n % 8 == 0)
 * gelu: mpu/sparse_transformer.py:172-179; dropout: torch.nn.Dropout call sites :167,:233,:524 */
int cogv_gelu_fwd(int dtype, const void* x, void* y, size_t n, void* stream);
int cogv_gelu_bwd(int dtype, const void* dy, const void* x, void* dx, size_t n, void* stream);
int cogv_dropout(int dtype, const void* x, void* y, size_t n, float p, uint64_t seed, uint64_t stream_id,
                 float* absmax_out, void* stream);
int cogv_add(int dtype, const void* a, const void* b, void* out, size_t n, float* absmax_out, void* stream);
int cogv_scale(int dtype, const void* x, void* y, size_t n, float scale, void* stream);
int cogv_absmax(int dtype, const void* x, size_t n, float* out, void* stream);      /* atomicMax into *out; dtype may be COGV_F32 (n % 4 == 0) */
/* out(fp32) = a(fp32) + b(T): a branch output joins the fp32 residual stream (the residual adds of
 * mpu/sparse_transformer.py:329,:340 when the layer is composed op by op); abs-max of out like cogv_add */
int cogv_add_stream(int dtype, const float* a, const void* b, float* out, size_t n, float* absmax_out, void* stream);
/* out[n] (+)= sum_m dy[m][n]  -- bias gradients of the Linear layers */
int cogv_colsum(int dtype, const void* dy, int M, int N, int ld, void* out, int accumulate, void* workspace,
                size_t workspace_bytes, void* stream);
size_t cogv_colsum_workspace_bytes(int M, int N);

/* ------------------------------------------------------------------ vocab-parallel cross entropy
 * replaces _VocabParallelCrossEntropy, mpu/cross_entropy.py:25-104.  logits [rows][V_local] in
 * logits_dtype (F16/BF16/F32), target int64 global ids, shard = [vocab_start, vocab_start+V_local).
 * fwd writes per-row shard statistics: rowmax, sumexp (relative to rowmax), predicted logit (0 when the
 * target is outside the shard) and, for a single shard, loss = log(sumexp) + rowmax - predicted.
 * bwd writes dlogits = (exp(logit - gmax)/gsum - onehot) * grad[row] in logits_dtype (may alias logits).
 */
int cogv_ce_fwd(int logits_dtype, const void* logits, const int64_t* target, int64_t vocab_start, int rows,
                int v_local, float* rowmax, float* sumexp, float* predicted, float* loss, void* stream);
int cogv_ce_bwd(int logits_dtype, const void* logits, const int64_t* target, int64_t vocab_start, int rows,
                int v_local, const float* gmax, const float* gsum, const float* grad, void* dlogits, void* stream);

/* ------------------------------------------------------------------ optimizer (flat buffers, chunk table)
 * One launch over the whole flat parameter space replaces FP16_Optimizer's per-tensor passes
 * (fp16/fp16.py:399-453,556-567), the per-tensor overflow check (fp16/loss_scaler.py:107-145), the
 * per-tensor norm of mpu/grads.py:59-73 and apex FusedAdam (call site pretrain_gpt2.py:139-140).
 * Chunk c covers flat elements [chunk_start[c], chunk_start[c]+chunk_len[c]), belongs to hyper-parameter
 * group chunk_group[c] (< 8) and counts toward the norm iff chunk_norm[c] != 0 (model-parallel dedup of
 * mpu/grads.py:61).  chunk_start % 8 == 0.
 */
/* stats[0] += sum of squares of grads in counted chunks (double; per-workgroup partials summed in a fixed order: the same
 * bits run after run), stats[1] = 1.0 if any grad is inf/nan.  workspace: cogv_grad_stats_workspace_bytes() bytes of scratch
 * owned by the caller (8-byte aligned, no initialisation; one per stream that may run the pass concurrently).  dtype may be
 * COGV_F32: the fp32 master gradients of FP16_Optimizer's generic path / of an fp32 model (mpu/grads.py:62-84). */
int cogv_grad_stats(int dtype, const void* grads, const int64_t* chunk_start, const int32_t* chunk_len,
                    const uint8_t* chunk_norm, int nchunks, double* stats, void* workspace, size_t workspace_bytes,
                    void* stream);
size_t cogv_grad_stats_workspace_bytes(void);
typedef struct cogv_adam_desc {
  int dtype;                       /* dtype of model params / grads (F16|BF16) */
  void* params; const void* grads; /* flat model params (written) and their (scaled) grads */
  float* master; float* exp_avg; float* exp_avg_sq;   /* flat fp32 */
  const int64_t* chunk_start; const int32_t* chunk_len; const uint8_t* chunk_group; int nchunks;
  float lr[8]; float weight_decay[8];
  float beta1, beta2, eps; int step; int bias_correction; int adam_w_mode;
  double beta1_d, beta2_d;         /* the same betas in double (1-beta and beta^step are formed in double) */
  float inv_loss_scale;            /* grads are multiplied by this */
  float max_grad_norm;             /* > 0: clip by global norm computed from stats */
  const double* stats;             /* from cogv_grad_stats (device); stats[1] != 0 => whole step skipped */
  const double* norm_sumsq_override; /* optional device scalar with the MP-reduced sum of squares */
} cogv_adam_desc;
int cogv_adamw_step(const cogv_adam_desc* d, void* stream);
/* master[i] = (float)params[i]  /  params[i] = (T)master[i]  over the chunk table */
int cogv_cast_flat(int dtype, const void* src_half, float* dst_f32, size_t n, void* stream);
int cogv_cast_flat_back(int dtype, const float* src_f32, void* dst_half, size_t n, void* stream);

/* ------------------------------------------------------------------ token sampling
 * replaces the host sampling of generation/sampling.py:24-50 (top_k_logits) and :168-186 (temperature, invalid slices,
 * softmax, multinomial, gather + log into the beam score).  One draw per row of logits[rows][vocab] (row_stride elements
 * apart; 0 = every row reads the same logits, e.g. nb draws from one prefill row):
 *   x = float(logit) / temperature (a division); ids outside [allow_lo, allow_hi) -> -inf;
 *   top_k > 0: keep x >= the k-th largest value (ties at the threshold are all kept; 1 <= top_k <= allow_hi - allow_lo);
 *   top_p > 0 (after top-k): keep the smallest descending prefix whose softmax mass exceeds top_p (first id always kept);
 *   softmax over the kept ids; u from the counter-based generator keyed (seed, *offset), counter = row; the first kept id
 *   (index order) whose inclusive prefix mass exceeds u * Z is drawn.  Fixed summation order: same (seed, *offset), same ids.
 * Every output pointer may be NULL: ids int64 [rows]; logp fp32 [rows] = log p(id); scores fp32 [rows] += logp;
 * probs fp32 [rows][vocab] = the filtered distribution.  vocab <= 65536.
 * Decode-graph bookkeeping (generation/decoder.py SamplingDecoder; active when pos_index != NULL), with p = *pos_index:
 *   tok[row] = id; pos[row] += 1; table[row][p + 1] = p + 1 (if < capacity); out_tokens[row][p + 1 - out_base] = id (if in
 *   [0, out_len)); then the last workgroup to finish sets *pos_index = p + 1 and *offset += 1 and re-zeroes *counter, a
 *   zero-initialised device word owned by this call site.  With these a replayed decode graph generates one token per replay.
 * Given ids (decode mode only; NULL: none): given int64 [capacity], indexed by sequence position, shared by all rows
 *   (given_stride = 0), or one table per row, given int64 [rows][given_stride] with given_stride >= capacity (several images
 *   on one decode graph, generation/sampling.py DeviceBatchFiller: every row carries its own given ids, indexed by slot).
 *   With g = given[row * given_stride + p + 1]: where g >= 0 that id is fed to this row instead of drawn (a position
 *   filling_sequence copies from its input): the logits are not read, ids[row] = tok[row] = out_tokens[row][p + 1 - out_base]
 *   = g, logp[row] = 0, scores and probs are left as they are; pos / table / *pos_index / *offset advance exactly as for a
 *   draw.  Every row decides for itself: in one launch some rows may be fed while the others draw. */
typedef struct cogv_sample_desc {
  int dtype; int rows; int vocab; int64_t row_stride;
  const void* logits;
  float temperature; int top_k; float top_p; int allow_lo; int allow_hi;
  uint64_t seed; int64_t* offset;        /* offset: device int64 (NULL: 0); advanced only when counter != NULL */
  int64_t* ids; float* logp; float* scores; float* probs;
  int64_t* tok; int64_t* pos; int64_t* pos_index; int32_t* table; int capacity;
  int64_t* out_tokens; int64_t out_len; int64_t out_base;
  uint32_t* counter;
  int64_t given_stride;                  /* elements between the rows' given tables; 0: one table shared by all rows */
  const int64_t* given;
} cogv_sample_desc;
int cogv_sample_logits(const cogv_sample_desc* d, void* stream);

/* ------------------------------------------------------------------ candidate scoring
 * replaces the host tail of the post-selection score, generation/sampling.py:214-230 (logits.float(), -inf over the image
 * codes, log_softmax, gather of the next token, sum over the text positions).  Per row of logits[rows][vocab]:
 *   x_i = float(logit_i) for i in [allow_lo, allow_hi) (raw logits: no temperature); ids outside the range are excluded;
 *   logp[row] = x_target - max - log(sum exp(x_i - max)) in fp32; a target outside the range gives -inf.
 * scores[g] = logp[g * group] + ... + logp[g * group + group - 1], added in that order by one thread (a second launch on the
 * same stream); it is formed from the stored per-row values, so scores != NULL needs logp != NULL.  The row is streamed, never
 * held in registers: any vocab >= 1.  16-byte loads when `logits` and row_stride * sizeof(element) are multiples of 16, scalar
 * loads otherwise.  Every sum has a fixed order and there are no floating-point atomics: same input, same bits.
 * 1: null logits / target, rows <= 0, group <= 0, rows % group != 0, an empty or out-of-vocabulary allow range,
 * row_stride < vocab;  3: rows > 65535. */
typedef struct cogv_score_desc {
  int dtype; int rows; int vocab; int64_t row_stride;   /* logits[rows][vocab], F16 | BF16 | F32, rows row_stride elements apart */
  const void* logits; const int64_t* target;            /* target[rows]: the id whose log-probability is wanted */
  int allow_lo; int allow_hi;                           /* ids outside [allow_lo, allow_hi) are excluded from the softmax (-inf) */
  int group;                                            /* rows per scored sequence; rows % group == 0 */
  float* logp;                                          /* [rows] (may be NULL when scores is NULL too) */
  float* scores;                                        /* [rows / group] (may be NULL): sum of the group's logp */
} cogv_score_desc;
int cogv_score_targets(const cogv_score_desc* d, void* stream);

/* ------------------------------------------------------------------ VQ-VAE tokenizer (fp32, exact-fp32 MFMA)
 * replaces the conv stacks of vqvae/vqvae_zc.py:121-129,159-164 (Encoder) and :172-192 (Decoder), the
 * nearest-code search :41-54 and embed_code :95-96 for the production config of vqvae/api.py:12-20.
 * Activations NHWC fp32; weights repacked by the caller to [parity][Cout][tap][Cin]:
 *   COGV_CONV_4X4_S2  (Conv2d k4 s2 p1)        taps = ky*4+kx, 1 parity,  W_packed[co][ky*4+kx][ci] = W[co][ci][ky][kx]
 *   COGV_CONV_1X1                              1 tap
 *   COGV_CONV_3X3_S1  (Conv2d k3 s1 p1)        taps = ky*3+kx, 1 parity,  W_packed[co][ky*3+kx][ci] = W[co][ci][ky][kx]
 *                                              (the non-production encoders :147, :154 and ResBlock :105)
 *   COGV_CONVT_4X4_S2 (ConvTranspose2d k4 s2 p1) 4 parities z = py*2+px (output pixel (2y+py, 2x+px)), 4 taps
 *        W_packed[z][co][ty*2+tx][ci] = W[ci][co][ky][kx],  ky = (py ? 2*ty : 1+2*ty),  kx = (px ? 2*tx : 1+2*tx)
 * Opt-in: cogv_conv_desc.precision = COGV_CONV_BF16X3 runs a layer on bf16 MFMA at fp32 accuracy (three bf16 limbs per operand).
 */
#define COGV_CONV_4X4_S2 0
#define COGV_CONV_1X1 1
#define COGV_CONVT_4X4_S2 2
#define COGV_CONV_3X3_S1 3
typedef struct cogv_conv_desc {
  int kind; int B, IH, IW, Cin, Cout; int relu;     /* relu: applied to the output */
  const void* in; const void* w; const void* bias; void* out;
  /* optional: the decoder's final 1x1 convolution to RGB (vqvae/vqvae_zc.py:190) fused into this layer's epilogue.
   * rgb_w = its weights [3][Cout] (fp32); rgb_partial receives [Cout / 128][B * OH * OW][4] fp32 partial sums INSTEAD
   * of the output tensor (out may be NULL; relu must be set; Cout % 128 == 0); finish with cogv_rgb_finalize_f32. */
  const void* rgb_w; void* rgb_partial;
  /* ResBlock support (vqvae/vqvae_zc.py:99-114: ReLU, conv3x3, ReLU, conv1x1, `out += input`): relu_in applies ReLU to the INPUT
   * activations inside the kernel (the block's leading ReLU; also the ReLU that follows the last block, :159); residual
   * (same NHWC shape as out, 16-byte aligned, may be NULL) is added after bias / ReLU, through max(., 0) when relu_residual is
   * set -- the reference's leading nn.ReLU(inplace=True) overwrites the block's input, so what it adds back is relu(input). */
  int relu_in; const void* residual; int relu_residual;
  /* precision: COGV_CONV_FP32 (0: a zeroed field is the exact-fp32 path, v_mfma_f32_32x32x2_f32) or COGV_CONV_BF16X3 (the
   * same layer, same epilogues, on v_mfma_f32_32x32x16_bf16: every fp32 operand is the exact sum of three bf16 limbs and the
   * six limb products with i + j <= 2 are accumulated in fp32, smallest first, in a fixed order (the five small ones apart from
   * x0*y0, joined at the end) -- fp32-class accuracy, NOT the bits of the exact path).  BF16X3 reads the weights from w_limbs (cogv_conv_split_weights of the same packed tensor `w`,
   * 16-byte aligned); `w` must still be valid.  Any other precision, or BF16X3 with w_limbs NULL or misaligned: COGV_ERR_ARG
   * before any launch. */
  int precision; const void* w_limbs;
} cogv_conv_desc;
#define COGV_CONV_FP32 0
#define COGV_CONV_BF16X3 1
/* COGV_ERR_ARG before any launch also for: odd IH / IW with COGV_CONV_4X4_S2, Cin % 4, Cout % 8, and more pixels than the
 * kernels index in int (B * GH * GW > 2^31 - 1 - 128, GH x GW the iteration grid: the input's for 1x1 / 3x3 / transposed, half
 * of it for 4x4 stride 2); COGV_ERR_UNSUPPORTED for an unknown kind.  The geometry is the weight gradient's (below). */
int cogv_conv2d_nhwc_f32(const cogv_conv_desc* d, void* stream);
/* The three bf16 limb planes of a packed fp32 weight tensor of n elements (any of the layouts above; n % 4 == 0), for
 * COGV_CONV_BF16X3 -- the fast mode of the F.conv2d / F.conv_transpose2d calls cogv_conv2d_nhwc_f32 replaces
 * (vqvae/vqvae_zc.py:121-129, :159-164, :172-192, ResBlock :105-108).  limbs = 3 * n uint16 (6 n bytes, 16-byte aligned):
 * plane p (0 = most significant) occupies elements [p * n, (p + 1) * n) in the element order of w, and holds the top 16
 * bits of r_p, with r_0 = w, r_{p+1} = r_p - bf16bits(r_p) (truncation: every subtraction is exact, the limbs sum back to w
 * exactly for |w| above about 2^-110, where the third limb is still inside bf16's exponent range -- and nothing can overflow). */
int cogv_conv_split_weights(const float* w, void* limbs, size_t n, void* stream);
/* out NCHW [B,3,H,W] = (sum over the ntiles partial planes + bias[c]) * scale[c] + shift[c] (scale/shift: 3 HOST floats or NULL) */
int cogv_rgb_finalize_f32(const float* partial, int ntiles, const float* bias, float* out, int B, int H, int W,
                          const float* scale3_host, const float* shift3_host, void* stream);
/* ids[m] = argmin_j (|x_m|^2 - 2 x_m.E_j) + |E_j|^2, first minimum on ties; embed_t = E^T [n_embed][D], embed_sq = |E_j|^2 */
int cogv_vq_argmin_f32(const float* x, const float* embed_t, const float* embed_sq, int64_t* ids, int M, int D,
                       int n_embed, void* stream);
int cogv_nchw3_to_nhwc4_f32(const float* in, float* out, int B, int H, int W, void* stream);
int cogv_embed_code_f32(const int64_t* ids, const float* embed_t, float* out, int64_t npix, int D, int n_embed,
                        void* stream);
/* NHWC [B,H,W,Cin] -> NCHW [B,3,H,W]: (w[3][Cin] . x + bias) * scale + shift (scale/shift: 3 HOST floats or NULL) */
int cogv_conv1x1_to_rgb_f32(const float* in, const float* w, const float* bias, float* out, int B, int H, int W,
                            int Cin, const float* scale3_host, const float* shift3_host, void* stream);

/* ------------------------------------------------------------------ VQ-VAE tokenizer training (fp32, exact-fp32 MFMA)
 * replaces the autograd of the conv stacks of vqvae/vqvae_zc.py:116-214 (F.conv2d / F.conv_transpose2d backward for the weights,
 * the ReLU and bias backward) and the training branch of Quantize.forward_ :67-86 (EMA codebook, straight-through estimator).
 * The DATA gradient of a layer is cogv_conv2d_nhwc_f32 with repacked weights (k4 s2 conv <-> k4 s2 transposed conv, 1x1 with
 * W^T).  No floating-point atomics: every result is bitwise reproducible.
 *
 * Weight gradient of the layer a cogv_conv_desc with the same kind / B / IH / IW / Cin / Cout describes (F.conv2d's
 * grad_weight at :121-129, F.conv_transpose2d's at :172-192):
 *   dw[z][co][t][ci] = sum over the pixels m of the forward iteration grid of dy[out(m, z)][co] * x[in(m, t, z)][ci],
 * taps outside the image contributing zero -- in the PACKED layout [parity][Cout][tap][Cin] the forward kernel reads.
 *   x  [B][IH][IW][Cin] the layer's input, dy [B][OH][OW][Cout] the gradient of its pre-activation output, both NHWC fp32.
 *   splits: the pixel range is cut into that many pieces, each summed into a slab of its own in `workspace`, and a second
 *   launch adds the slabs in order; 0 = the plan's choice (enough to fill the chip).
 *   relu_x (0 / 1): 1 contracts against max(x, 0) instead of x -- the weight gradient of a layer whose forward ran with
 *   relu_in (a ResBlock's 3x3, the convolution behind the ReLU that closes a ResBlock chain); x is the saved PRE-ReLU input,
 *   -0.0, +0.0 and negatives contribute nothing.  Valid for every kind.
 *   topologies (0 / 1): 0 = the kinds and tiles of the n_res_block=0 stride-6 tokenizer: COGV_CONV_3X3_S1 is refused and a
 *   tile is 128 output channels wide.  1 (opt-in; a later change makes it the default) also takes COGV_CONV_3X3_S1
 *   (K = 9 * Cin: ResBlocks, the stride-4 / stride-2 encoders) and, where Cout <= 32, runs tiles 32 output channels wide
 *   (a ResBlock's 3x3 has Cout = n_res_channel), the plan's Cout tiles counted in that width.  The order of the pixel sum
 *   of an element is the same in both widths.  A zero-initialised descriptor behaves as before these fields existed.
 * COGV_ERR_ARG: null or misaligned (16 B) pointers, Cin % 4, Cout % 8, odd IH / IW for the k4 s2 convolution, a workspace
 * smaller than cogv_conv_wgrad_workspace_bytes, relu_x or topologies other than 0 / 1; COGV_ERR_UNSUPPORTED:
 * COGV_CONV_3X3_S1 with topologies == 0. */
typedef struct cogv_conv_wgrad_desc {
  int kind; int B, IH, IW, Cin, Cout;
  int splits;
  const void* x; const void* dy; void* dw;
  void* workspace; size_t workspace_bytes;
  int relu_x;
  int topologies;
} cogv_conv_wgrad_desc;
/* HOST ONLY (pointers are not looked at): plan = {splits, pixels per split, workgroups, Cout tiles, tap*Cin tiles, parities} */
#define COGV_CONV_WGRAD_PLAN_INTS 6
int cogv_conv_wgrad_plan(const cogv_conv_wgrad_desc* d, int* plan);
/* HOST ONLY: bytes of slabs the plan needs (0 for one split or a refused descriptor) */
size_t cogv_conv_wgrad_workspace_bytes(const cogv_conv_wgrad_desc* d);
int cogv_conv_wgrad_nhwc_f32(const cogv_conv_wgrad_desc* d, void* stream);
/* ReLU backward fused with the bias gradient (nn.ReLU / the bias of F.conv2d at :121-129, :172-192), rows of C floats:
 *   dx[m][c] = act[m][c] > 0 ? dy[m][c] : 0   (act: the saved POST-ReLU activation; NULL: no mask; dx may be dy, or NULL)
 *   db[c]    = sum_m of that -- the gradient of the layer's pre-activation output summed per channel (act == NULL: of dy).
 * Per-workgroup partial sums in `workspace`, added in workgroup order by a second launch.  C % 4 == 0. */
size_t cogv_relu_bias_bwd_workspace_bytes(int64_t M, int C);
int cogv_relu_bias_bwd_f32(const float* dy, const float* act, float* dx, float* db, float* workspace, size_t workspace_bytes,
                           int64_t M, int C, void* stream);
/* Codebook statistics (:68-69 embed_onehot.sum(0), flatten.transpose(0, 1) @ embed_onehot) through an inverted index
 * instead of the one-hot product: count[j] = #{m : ids[m] == j} (int32 [n_embed]), sum[j][:] = sum of x[m][:] over those m
 * in ascending m ([n_embed][D], zeros for a code without pixels).  x [M][D]; D % 4 == 0, D <= 1024, n_embed <= 32768
 * (COGV_ERR_UNSUPPORTED beyond); ids outside [0, n_embed) are ignored. */
size_t cogv_vq_code_stats_workspace_bytes(int M, int D, int n_embed);
int cogv_vq_code_stats_f32(const int64_t* ids, const float* x, int* count, float* sum, void* workspace, size_t workspace_bytes,
                           int M, int D, int n_embed, void* stream);
/* The EMA update :74-83 in place: cluster_size [n_embed], embed_avg and embed [D][n_embed] (the reference's layout);
 *   cluster_size = cluster_size * decay + (1 - decay) * count;  embed_avg = embed_avg * decay + (1 - decay) * sum^T;
 *   n = sum(cluster_size) -> n_out[0];  embed = embed_avg / ((cluster_size + eps) / (n + n_embed * eps) * n). */
int cogv_vq_ema_update_f32(const int* count, const float* sum, float* cluster_size, float* embed_avg, float* embed, float* n_out,
                           double decay, double eps, int D, int n_embed, void* stream);
/* Backward of :85-86 (diff = (quantize.detach() - input).pow(2).mean(); quantize = input + (quantize - input).detach()):
 *   g_x = g_q + g_diff[0] * 2 (x - q) / n;  g_q (may be NULL) arrives at the quantised map, g_diff (device scalar, may be
 *   NULL) at diff; n = number of elements, n % 4 == 0. */
int cogv_vq_ste_bwd_f32(const float* g_q, const float* g_diff, const float* x, const float* q, float* g_x, int64_t n,
                        void* stream);

/* ------------------------------------------------------------------ tokenizer ingest: raw uint8 images -> encoder input
 * replaces transforms.Resize(S) / CenterCrop(S) / ToTensor() / Normalize(mean, std) on PIL images at
 * data_utils/vqvae_tokenizer.py:72-82 (read_img) and preprocess_entry.py:87-106, and the layout launch
 * cogv_nchw3_to_nhwc4_f32 behind them.  The uint8 stage is Pillow's Image.resize(BILINEAR) followed by the crop, bit for
 * bit: per axis in -> out, scale = in / out, support = max(scale, 1); output xx reads the source pixels
 * [xmin, xmin + count) = [max(int(c - support + .5), 0), min(int(c + support + .5), in)) around c = (xx + .5) * scale with the
 * triangle weights, normalised by their left-to-right sum, as integers k = (int)(w * 2^22 + .5); a pixel is
 * clip8((2^21 + sum p * k) >> 22); the horizontal pass is rounded to uint8 before the vertical pass; an axis that keeps its
 * size is copied.  Resized size: short side S, long side int(S * long / short); crop offsets round((n - S) / 2), half to even.
 *
 * cogv_resample_coeffs: HOST ONLY (all pointers are host memory, no device is touched): the tables of one axis,
 *   xmin[out], count[out], k[out][max_taps] (zero beyond count).  3 when some output needs more than max_taps pixels. */
int cogv_resample_coeffs(int in, int out, int* xmin, int* count, int* k, int max_taps);
/* HOST ONLY: what cogv_image_prep_u8 does with one H x W image at size S, and whether it takes it:
 *   plan = {resized H, resized W, crop top, crop left, taps horizontal, taps vertical (largest count of the axis),
 *           output rows per workgroup, output columns per workgroup, LDS rows of the horizontal pass, LDS bytes}.
 *   1: S <= 0, S % 8 != 0 or an empty image; 3: an axis needs more than 65 taps (count <= 2 * scale + 1, so no scale up to 32
 *   does) or a side beyond 2^24. */
#define COGV_IMAGE_PREP_PLAN_INTS 10
int cogv_image_prep_plan(int H, int W, int S, int* plan);
/* out [B][S][S][4] fp32 (channel 3 zero) = lut[c][resize + crop of image b][c].  One launch for images of different sizes:
 *   pack        the images' bytes, each HWC, 3 channels, contiguous, at any byte offset; 16-byte aligned, pack_bytes % 4 == 0
 *   table       [B][8] int32: {offset low, offset high, H, W, htab, vtab, taps horizontal, taps vertical}; table_host is the
 *               same table in HOST memory (the arguments are checked on it before anything is launched)
 *   coeffs      int32 tables; htab / vtab index the image's column / row table: xmin[S], count[S], k[taps][S] of the S outputs
 *               inside the crop (rows of cogv_resample_coeffs from the crop offset on, k transposed)
 *   lut         [3][256] fp32: ((u / 255) - mean[c]) / std[c], computed by the caller in fp32 (ToTensor, Normalize)
 * B <= 65535.  Returns as cogv_image_prep_plan for the first image it refuses, 1 for a table entry outside pack / coeffs. */
int cogv_image_prep_u8(const uint8_t* pack, size_t pack_bytes, const int* table, const int* table_host, const int* coeffs,
                       size_t coeffs_ints, int B, int S, const float* lut, float* out, void* stream);
/* the device half of make_super_resolution_batch (preprocess/pretokenized_data.py:100-124) on x [b][S][S][4], S % 16 == 0:
 *   patches [b * k][S/2][S/2][4], image-major: patch i * k + j = image i at rows ph[p] .. + S/2, columns pw[p] .. + S/2,
 *           p = positions[j] in 0..8 (device int32 [k]), pw = {0, S/4, S/2} x 3, ph = {0,0,0, S/4,S/4,S/4, S/2,S/2,S/2};
 *   overview [b][S/2][S/2][4] = F.interpolate(x, size=(S/2, S/2), mode='bilinear'): every weight is 0.5 at this factor,
 *           computed as 0.5 * (0.5 a + 0.5 b) + 0.5 * (0.5 c + 0.5 d), horizontal pairs first. */
int cogv_sr_patches_nhwc4_f32(const float* x, const int* positions, float* patches, float* overview, int b, int S, int k,
                              void* stream);

/* ------------------------------------------------------------------ image egress: decoded fp32 images -> uint8 image grid
 * replaces F.interpolate + torchvision.utils.save_image(..., normalize=True) at generate_samples.py:175-199
 * (generate_images_once) and :236-244 (super_resolution), and save_image(..., normalize=False, nrow=len(imgs)) at
 * preprocess/utils.py:25-31: make_grid, then save_image's mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8),
 * byte for byte as torch computes them on CPU tensors.
 *   images   B images of 3 x H x W in K source batches: contiguous fp32 NCHW [n][3][h][w] with an integer factor f in
 *            {1, 2, 4, 8}, h * f == H, w * f == W; image pixel (i, j) reads source pixel (i / f, j / f) -- F.interpolate's
 *            default nearest mode at these factors.
 *   table    [K][8] int32: {pointer low, pointer high, n, h, w, f, first image (the n of the batches in front), 0}, sum n == B,
 *            every pointer 16-byte aligned; table_host is the same table in HOST memory (the arguments are checked on it
 *            before anything is launched).
 *   grid     B == 1: the image itself, [H][W][3].  Otherwise xmaps = min(nrow, B), ymaps = ceil(B / xmaps), the grid is
 *            [(H + padding) * ymaps + padding][(W + padding) * xmaps + padding][3], image k has its top-left at row
 *            (k / xmaps) * (H + padding) + padding, column (k % xmaps) * (W + padding) + padding; everything else is padding.
 *   bytes    t = y * 255 (rounded), t + 0.5 (rounded; never one fused multiply-add), clamped to [0, 255], truncated; the
 *            padding byte is the same of pad_value.  y = x, or with a normalisation
 *            y = (min(max(x, low), high) - low) / d, d = (float)max((double)high - (double)low, 1e-5), a true fp32 division.
 * Returns 1: B == 0 or B > 65535, nrow <= 0, padding < 0, a null or misaligned pointer, a table whose n do not add up to B,
 *   high < low, an out or range smaller than the plan's; 3: another factor, h * f != H, w * f != W, H, W or padding beyond
 *   32768, a grid side beyond 2^28.
 *
 * cogv_image_grid_plan: HOST ONLY.  plan = {xmaps, ymaps, grid H, grid W, out bytes, range workspace bytes}; table_host may be
 *   NULL (geometry only), otherwise the sources are checked as the launches check them. */
#define COGV_IMAGE_GRID_PLAN_INTS 6
int cogv_image_grid_plan(const int* table_host, int K, int B, int H, int W, int nrow, int padding, int scale_each, int64_t* plan);
/* range (device, the plan's range workspace bytes, 4-byte aligned): one slot for all images, or one per image with
 * scale_each; a slot is two uint32 {~key(minimum), key(maximum)}, key(v) = bits(v) ^ (v < 0 ? 0xffffffff : 0x80000000), which
 * orders as the floats do, so that integer atomics give the exact extremes in any order.  Zeroes the slots (a memset node
 * under capture), then one launch; nothing is read back. */
int cogv_image_range_f32(const int* table, const int* table_host, int K, int B, int H, int W, int scale_each, void* range,
                         size_t range_bytes, void* stream);
/* out (device, 16-byte aligned, at least the plan's out bytes): every byte of the grid written exactly once by one launch.
 * norm: NONE; FIXED: low, high as given (value_range; d from the doubles, the clamp and the subtraction on their fp32
 * roundings, as torch reads Python scalars); RANGE / RANGE_EACH: slot 0 / slot k of cogv_image_range_f32's range. */
#define COGV_GRID_NORM_NONE 0
#define COGV_GRID_NORM_FIXED 1
#define COGV_GRID_NORM_RANGE 2
#define COGV_GRID_NORM_RANGE_EACH 3
int cogv_image_grid_u8(const int* table, const int* table_host, int K, int B, int H, int W, int nrow, int padding,
                       double pad_value, int norm, const void* range, double low, double high, uint8_t* out, size_t out_bytes,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COGVIEW_HIP_H */
