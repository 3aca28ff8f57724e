// Skinny-M (M <= 8) matrix-vector kernels of the decode step, second generation (round 4).
//
//   C[M,N] = epilogue( X[M,K] * B[N,K]^T ),   X = A | LayerNorm prologue of a stream row | combine of the decode attention
//
// A decode step of the 4B model reads its 7.9 GB of weights once per generated token: every launch is a pure HBM stream of
// B, 13-52 MB long, i.e. 2-7 us at the memory's speed -- the same order as a launch's fixed costs.  The first generation
// (gemm.hip: gemv_kernel, gemv_ln_kernel, gemv_attn_kernel) gave a workgroup 8 columns and dealt the 512-element chunks of K
// to its four waves round robin: at K = 2560 wave 0 fetched two chunks ONE AFTER THE OTHER (two exposed HBM latencies), at
// K = 10240 every wave five; a wave never had more than 8 KB in flight, and the LayerNorm prologue's own small loads queued
// BEHIND the first weight chunk (the vector-memory counter retires in order).  Measured in the captured 4B step: 2.6 TB/s
// inside the kernels (profiles/r02_decode_kernel_stats_head.csv).
//
// Here a WAVE owns J whole columns (all of K), J * K / 512 <= 20 (40 at K = 10240) independent 16-byte loads per lane,
// all requested at the top of the kernel -- 20 KB in flight per wave, every byte of B requested once, immediately:
//     [the prologue's own inputs]  [ALL weight loads]  [prologue -> x in LDS]  barrier  [dot products as the chunks land]
// The small loads go first so that the prologue starts as soon as THEY arrive and runs while the weights stream in.
// The per-lane accumulation runs over the chunks in ascending order (fp32 fmaf chain), then one DPP wave sum per
// (row, column): no cross-wave reduction.  Lane 0 of the first NW * J / 8 waves runs the shared fused epilogue on 8 columns.
// That is the form for ONE row (FormV: fp32 fmaf chains on the vector ALU).  With 2 .. 8 rows its accumulators, unpacked x rows
// and weight slots no longer fit next to each other: the kernels fell to one or two waves per SIMD, a second round of
// workgroups, and in places spilled INSIDE the request phase (profiles/r04_decode_batch_*: 2.77 ms per token at one row, 3.48 /
// 4.88 / 9.29 at 2 / 4 / 8).  Rows 2 .. 8 therefore take FormM: the same weight stream, but the products go to the matrix
// core -- v_mfma_f32_16x16x32 with the WEIGHTS as the A operand (a lane's 16-byte load IS its fragment: column n0 + lane % 16,
// contraction slots 8 (lane / 16) ..), the x rows as B (from LDS, rows past M are don't-care columns of the result) and a
// 16 x 16 accumulator of 4 registers per lane whatever the row count.  A workgroup owns 16 columns; its waves split the 32-deep
// contraction steps (in pairs: one 128-byte line of a weight row) round robin and their partial tiles meet in LDS in wave order.
// The three kernels use the same association for the same K, so the combine-prologue form and the two-launch form of the
// attention-output projection still agree bit for bit (tests/test_kernels_gpu.py).
//
// THE WEIGHT OPERAND.  FormV and FormM are written once and take what B holds as a type parameter: W16 (the dtype's 16 bits) or W8
// (OCP E4M3 bytes with one fp32 scale per row, cogv_quantize_rows_e4m3; the format: e4m3_stream.cuh).  The decode step is a
// weight stream, so half the bytes is the lever that is left: the same three kernels on the same two forms -- the prologues do
// not know what a weight is.  The bytes are converted in registers (v_cvt_pk_f32_fp8, exact), the arithmetic and every rounding
// point stay those of the 16-bit operand, and the fp32 sum of column n is multiplied by scale[n] once, in front of the shared
// epilogue.  A slot of the same shape holds half the bytes, so the class table changes to keep 16-20 KB in flight per wave: FormV
// on W8 gives a wave twice the columns (8-byte slots: a lane keeps its 8 contraction elements), FormM on W8 gives a 16-column
// tile half the waves (a 16-byte load is two MFMA fragments).  The classes of both formats: gemv_plan.h.
//
// A third operand, W4 (OCP MXFP4 blocks, cogv_quantize_rows_mxfp4; the format: mxfp4_stream.cuh), halves the bytes again: see
// the struct for its slot and fragment mapping.  The three operands live in gemv_operand.cuh, which gemv_wide.hip shares.
//
// Compiled as two translation units (-DCOGV_GEMV_TU=0: bf16, 1: fp16; build.py) for the 16-bit operand, two more with
// -DCOGV_GEMV_W8 for the 8-bit operand and two with -DCOGV_GEMV_W4 for the 4-bit one; without the macro this file is empty.  The
// merge of the forms left the device code of the first four units what it was (tools/device_code_diff.py,
// profiles/r16_gemv_forms_parent_vs_head.log), and so did the 4-bit operand (profiles/r21_gemv_w4_parent_vs_head.log).
#include "gemv_operand.cuh"
#include "gemv_plan.h"

#include <cstdlib>
#include <type_traits>

#ifdef COGV_GEMV_TU

namespace {

// bias of the 8 columns n .. n + 7 a finishing lane will need, requested ahead of its use.  Unconditional: without a bias (or
// in a lane that finishes nothing) a valid stand-in address is read and the value ignored.
// Through the VECTOR memory path (an offset the compiler cannot see through): as a wave-uniform address this would become a
// scalar load, and the scalar counter has to reach zero -- for the kernel arguments -- before the first weight load can be
// issued: the weight stream would start one memory latency late.
template <typename T>
__device__ __forceinline__ u32x4 gv2_bias(const GemmArgs& p, int n) {
  const T* src = (p.flags & COGV_EPI_BIAS) ? reinterpret_cast<const T*>(p.bias) : reinterpret_cast<const T*>(p.B);
  return gload16(src + (n < p.N ? n : p.N - 8) + gv2_vzero());
}

// =====================================================================================================================
// FormV: one row (MT = 1; the row-count template parameter is kept general).  A wave owns J whole columns.
template <typename W, int J, int KCMAX, bool GUARD_, int MT, int NW_>
struct FormV {
  typedef typename W::T T;
  // CH contraction elements per slot of a wave, SC such slots per column (W16, W8: the 512-chunks themselves)
  static constexpr int CH = 64 * W::EPL, SC = (KCMAX * 512 + CH - 1) / CH;
  static constexpr int NW = NW_, COLS = NW_ * J, XPAD = 0, NS = SC * J, XCHUNKS = KCMAX;
  // NG groups of 8 columns, finished by lanes 0 .. GPW - 1 of every wave (J <= 8: GPW = 1, lane 0 of the first NG waves)
  static constexpr int NG = (NW_ * J) / 8, GPW = (NG + NW_ - 1) / NW_;
  static constexpr bool GUARD = GUARD_;
  struct Regs { typename W::Slot w[NS]; };
  struct Shared { float outp[MT][NW_ * J]; };
  // slot s of a wave = (chunk c = s / J, column j = s % J): chunk-major, the order the dot products consume them.  Columns
  // past N (a wave at the ragged end of the matrix) re-read the last row; their results are never stored.
  template <int S0, int S1>
  static __device__ __forceinline__ void issue(Regs& r, const GemmArgs& p, int n0, int K, int wave, int lane) {
    if constexpr (W::EPL == 8) {
    const typename W::Elem* B = reinterpret_cast<const typename W::Elem*>(p.B);
    const int nw = n0 + wave * J, kc = K >> 9;
#pragma unroll
    for (int s = S0; s < S1; ++s) {
      const int c = s / J, j = s % J;
      const int n = nw + j < p.N ? nw + j : p.N - 1;
      if (!GUARD || c < kc) r.w[s] = W::load(B + (size_t)n * p.ldb + c * 512 + lane * 8);
    }
    } else {
      // W4: the lane's block of slot-chunk c, or the row's last block where the column ends inside the chunk
      const int nw = n0 + wave * J;
#pragma unroll
      for (int s = S0; s < S1; ++s) {
        const int c = s / J, j = s % J;
        const int n = nw + j < p.N ? nw + j : p.N - 1;
        const int k = c * CH + lane * W::EPL;
        if (!GUARD || c * CH < K) r.w[s] = W::load(p, n, (k < K ? k : K - W::EPL) >> 5);
      }
    }
  }
  // the group of 8 columns this lane finishes (lanes < GPW)
  static __device__ __forceinline__ int group(int wave, int lane) { return wave * GPW + (lane < GPW ? lane : 0); }
  static __device__ __forceinline__ u32x4 bias(const GemmArgs& p, int n0, int wave, int lane) { return gv2_bias<T>(p, n0 + group(wave, lane) * 8); }
  // W4: the per-lane sums over the slot-chunks (a lane's 32 elements of each, ascending); lanes past the column's end add zeros
  static __device__ __forceinline__ void sums4(const Regs& r, const T* xs, int XS, int K, int lane, float (&acc)[MT][J]) {
#pragma unroll
    for (int c = 0; c < SC; ++c) {
      if (!GUARD || c * CH < K) {
        const int k0 = c * CH + lane * W::EPL;
        const bool ok = k0 < K;
        const int k = ok ? k0 : K - W::EPL;
        // (8 elements of x at a time against all J columns: 8 registers of x instead of 32; a column's chain stays ascending)
#pragma unroll
        for (int u = 0; u < W::EPL / 8; ++u) {
          float x[MT][8];
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            unpack8<T>(*reinterpret_cast<const u32x4*>(xs + (size_t)m * XS + k + u * 8), x[m]);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[m][e] = ok ? x[m][e] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < J; ++j) {
            float wf[8];
            W::unpack(r.w[c * J + j], u, wf);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
              float t = acc[m][j];
#pragma unroll
              for (int e = 0; e < 8; ++e) t = fmaf(x[m][e], wf[e], t);
              acc[m][j] = t;
            }
          }
        }
      }
    }
  }
  // acc[m][j] += sum over this lane's 8 elements of every chunk (ascending): x rows from LDS, 16 bytes per lane and row; then
  // one DPP wave sum per (row, column), LDS, and the finishing lane of group g runs the fused epilogue on columns n0 + 8g .. + 7.
  // The tail of these launches is a chain of dependent latencies on one lane, so the bias it needs is requested ahead.  A
  // requested abs-max (COGV_EPI_ABSMAX) still costs the tail a memory-side read + atomic per finishing lane; the decode chain
  // does not ask for it any more (cogv_ln_prologue.z_absmax = NULL).  Measured with one returning-nothing atomic per lane
  // instead of atomic_max_nonneg's "read first": the 320 workgroups of the 4h -> h launch finish together and their
  // same-address atomics serialise, 14.6 -> 16.2 us (profiles/r04_decode_gemv2_kernel_stats*.csv).
  static __device__ __forceinline__ void product(const Regs& r, const GemmArgs& p, const T* xs, int XS, int K, Shared& sh, int n0, int wave,
                                                 int lane, const u32x4& bias_pre) {
    const int kc = K >> 9;
    const int g = group(wave, lane);
    const typename W::Scale sc = W::scale(p, n0, g);
    float acc[MT][J];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < J; ++j) acc[m][j] = 0.f;
    if constexpr (W::EPL != 8) sums4(r, xs, XS, K, lane, acc);
    else
#pragma unroll
    for (int c = 0; c < KCMAX; ++c) {
      if (!GUARD || c < kc) {
        float x[MT][8];
#pragma unroll
        for (int m = 0; m < MT; ++m) unpack8<T>(*reinterpret_cast<const u32x4*>(xs + (size_t)m * XS + c * 512 + lane * 8), x[m]);
#pragma unroll
        for (int j = 0; j < J; ++j) {
          float wf[8];
          W::unpack(r.w[c * J + j], wf);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            float t = acc[m][j];
#pragma unroll
            for (int e = 0; e < 8; ++e) t = fmaf(x[m][e], wf[e], t);
            acc[m][j] = t;
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const float t = wave_sum_uniform(acc[m][j]);
        if (lane == 0) sh.outp[m][wave * J + j] = t;
      }
    __syncthreads();
    // (unsigned compare: at GPW = 1 it folds to lane == 0 before the form is inlined into its kernel -- the compare the 16-bit
    // kernels were written with; a signed "lane < 1" reaches the same code by another road and moves their compares and branches)
    if ((unsigned)lane < (unsigned)GPW && g < NG) {
      const int n = n0 + g * 8;
      if (n < p.N) {
        const typename W::Factors s8 = W::factors(sc);
        uint32_t am = 0u;
        for (int m = 0; m < p.M && m < MT; ++m) {
          float v[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] = W::mul(sh.outp[m][g * 8 + i], s8, i);
          am = absmax_pk(am, epilogue8<T>(p, m, n, v, &bias_pre));
        }
        if (p.flags & COGV_EPI_ABSMAX) {
          const uint32_t wv = max(am & 0xffffu, am >> 16);
          atomic_max_nonneg(p.absmax, bits_to_f<T>((uint16_t)wv));
        }
      }
    }
  }
};

// =====================================================================================================================
// FormM: 2 .. 8 rows on the matrix core.  A workgroup owns TW tiles of 16 columns, NWK waves per tile: wave kw of a tile takes the
// load PAIRS q = kw, kw + NWK, .. (loads 2q and 2q + 1 of KL contraction elements each: one 128-byte line of each of the 16
// weight rows), L = K / KL / NWK loads of 16 bytes per lane, all requested at the top like FormV's slots.  Per fragment of a load:
//   A operand = weights: lane l supplies row (l & 15) -> column n0 + (l & 15), 8 contraction slots of the lane's 16 bytes
//   B operand = x:       lane l supplies column (l & 15) -> row m = l & 15 (lanes past the row count re-read the last row: those
//                        result columns are never looked at), the same contraction slots, from LDS (rows padded by 16 bytes
//                        so that the rows of one step fall into different banks)
//   D: lane l holds C[m = l & 15][n0 + 4 (l >> 4) + i], i = 0 .. 3.
// The waves' partial tiles are summed in wave order (deterministic), regrouped through LDS into 8 consecutive columns per
// (row, half) and finished by lanes 0 .. 2M - 1 of the tile's first wave in parallel.
// TW = 2 (eight waves, 32 columns) serves the LayerNorm-prologue kernel at 4 and 8 rows: one 8-element vector per thread and row
// in the prologue instead of two, and half as many workgroups recomputing it.
template <typename W, int NWK, int TW, int LMAX, bool GUARD_, int MT>
struct FormM {
  typedef typename W::T T;
  typedef typename W::Scale Scale;
  static constexpr int KL = W::KL, FR = W::FR;
  static constexpr int NW = NWK * TW, COLS = 16 * TW, XPAD = 8, NS = LMAX, XCHUNKS = (LMAX * NWK * KL + 511) / 512;
  static constexpr bool GUARD = GUARD_;
  typedef typename W::template MRegs<LMAX> Regs;
  struct Shared { f32x4 red[NW][64]; float outp[TW][16][16]; };
  static __device__ __forceinline__ int kstep(int kw, int i) { return 2 * (kw + NWK * (i >> 1)) + (i & 1); }
  template <int S0, int S1>
  static __device__ __forceinline__ void issue(Regs& r, const GemmArgs& p, int n0, int K, int wave, int lane) {
    const int L = K / (KL * NWK), kw = wave % NWK, nt = n0 + (wave / NWK) * 16 + (lane & 15);
    const int n = nt < p.N ? nt : p.N - 1;
    const typename W::Elem* row = reinterpret_cast<const typename W::Elem*>(p.B) + (size_t)n * p.ldb + (lane >> 4) * (KL / 4 / W::PK);
#pragma unroll
    for (int i = S0; i < S1; ++i)
      if (!GUARD || i < L) {
        r.w[i] = gload16(row + (KL / W::PK) * kstep(kw, i));     // (default policy: the non-temporal form measured 12-14 % SLOWER here, profiles/r05_decode_nt_ab.log)
        if constexpr (W::PK == 2) r.s[i] = W::block_scale(p, n, (lane >> 4) + 4 * kstep(kw, i));      // W4: the load IS block 4 step + lane / 16 of its row
      }
  }
  // lanes 0 .. 15 of a tile's first wave finish: lane t -> row t >> 1, columns (tile) + 8 (t & 1) ..
  static __device__ __forceinline__ int col(int n0, int wave, int lane) { return n0 + (wave / NWK) * 16 + (lane & 1) * 8; }
  static __device__ __forceinline__ u32x4 bias(const GemmArgs& p, int n0, int wave, int lane) { return gv2_bias<T>(p, col(n0, wave, lane)); }
  // loads I0 .. I1 - 1 of this wave; xs holds the x rows from contraction index kofs on
  template <int I0, int I1>
  static __device__ __forceinline__ void accumulate(const Regs& r, const T* xs, int XS, int K, int kofs, int wave, int lane, f32x4& acc) {
    typedef typename HT<T>::v8 v8;
    const int L = K / (KL * NWK), kw = wave % NWK;
    const int mrow = (lane & 15) < MT ? (lane & 15) : MT - 1;
    const T* xrow = xs + (size_t)mrow * XS + (lane >> 4) * (KL / 4) - kofs;
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      if (!GUARD || i < L) {
        v8 b[FR];
#pragma unroll
        for (int f = 0; f < FR; ++f) b[f] = *reinterpret_cast<const v8*>(xrow + KL * kstep(kw, i) + 8 * f);
#pragma unroll
        for (int f = 0; f < FR; ++f) {
          if constexpr (W::PK == 2) acc = HT<T>::mfma16(W::frag(r.w[i], r.s[i], f), b[f], acc);
          else acc = HT<T>::mfma16(W::frag(r.w[i], f), b[f], acc);
        }
      }
    }
  }
  // (the two-halves kernel calls this form: its scales are requested here, in the tail)
  static __device__ __forceinline__ void finish(f32x4 acc, const GemmArgs& p, Shared& sh, int n0, int wave, int lane, const u32x4& bias_pre) {
    finish(acc, p, sh, n0, wave, lane, bias_pre, W::scale(p, n0 + (wave / NWK) * 16, lane & 1));
  }
  static __device__ __forceinline__ void finish(f32x4 acc, const GemmArgs& p, Shared& sh, int n0, int wave, int lane, const u32x4& bias_pre,
                                                const Scale& sc) {
    const int tile = wave / NWK, kw = wave % NWK;
    sh.red[wave][lane] = acc;
    __syncthreads();
    if (kw == 0) {
      f32x4 s = sh.red[tile * NWK][lane];
#pragma unroll
      for (int w = 1; w < NWK; ++w) s += sh.red[tile * NWK + w][lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) sh.outp[tile][lane & 15][(lane >> 4) * 4 + i] = s[i];
    }
    __syncthreads();
    if (kw == 0) {
      const int m = lane >> 1, n = col(n0, wave, lane);
      uint32_t am = 0u;
      if (m < p.M && m < MT && n < p.N) {
        const typename W::Factors s8 = W::factors(sc);
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = W::mul(sh.outp[tile][m][(lane & 1) * 8 + i], s8, i);
        am = epilogue8<T>(p, m, n, v, &bias_pre);
      }
      if (p.flags & COGV_EPI_ABSMAX) {
        uint32_t wv = max(am & 0xffffu, am >> 16);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wv = max(wv, (uint32_t)__shfl_xor((int)wv, o, 64));
        if (lane == 0) atomic_max_nonneg(p.absmax, bits_to_f<T>((uint16_t)wv));
      }
    }
  }
  static __device__ __forceinline__ void product(const Regs& r, const GemmArgs& p, const T* xs, int XS, int K, Shared& sh, int n0, int wave,
                                                 int lane, const u32x4& bias_pre) {
    const Scale sc = W::scale(p, n0 + (wave / NWK) * 16, lane & 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    accumulate<0, LMAX>(r, xs, XS, K, 0, wave, lane, acc);
    finish(acc, p, sh, n0, wave, lane, bias_pre, sc);
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// plain form: X = A (rows of the storage type, a few KB, L2-resident)
template <typename T, typename F, int MT>
__global__ __launch_bounds__(F::NW * 64) void gemv2_kernel(const GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char gv2_smem[];      // x [MT][K + pad] as T
  __shared__ typename F::Shared sh;
  T* xs = reinterpret_cast<T*>(gv2_smem);
  constexpr int NT = F::NW * 64;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = F::GUARD ? p.K : F::XCHUNKS * 512, nvec = K >> 3, XS = K + F::XPAD;
  const int n0 = blockIdx.x * F::COLS;
  // x rows first: the copy to LDS below waits for these loads only
  constexpr int XV = (F::XCHUNKS * 64 + NT - 1) / NT;
  u32x4 xr[MT][XV];
  const T* A = reinterpret_cast<const T*>(p.A);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int row = m < p.M ? m : p.M - 1;
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = threadIdx.x + NT * u;
      if (v < nvec) xr[m][u] = gload16(A + (size_t)row * p.lda + v * 8);
    }
  }
  const u32x4 bias_pre = F::bias(p, n0, wave, lane);
  typename F::Regs w;
  F::template issue<0, F::NS>(w, p, n0, K, wave, lane);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int u = 0; u < XV; ++u) {
      const int v = threadIdx.x + NT * u;
      if (v < nvec) *reinterpret_cast<u32x4*>(xs + (size_t)m * XS + v * 8) = xr[m][u];
    }
  __syncthreads();
  F::product(w, p, xs, XS, K, sh, n0, wave, lane, bias_pre);
}

// plain form in TWO contraction halves (FormM, exact-K classes): x rows of K = 10240 with 4 / 8 rows are 80 / 160 KB -- more LDS
// than a workgroup can have next to anything else.  A wave's loads 0 .. L/2 - 1 lie in the first half of K and the others in
// the second (its step pairs ascend with the load index), so the rows are staged half by half: all weights are requested at
// the top as ever; the second half of x follows them in the memory queue, i.e. arrives right behind the last weight.
template <typename T, typename F, int MT>
__global__ __launch_bounds__(F::NW * 64) void gemv2_k2_kernel(const GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char gv2_smem[];      // x [MT][K / 2 + pad] as T
  __shared__ typename F::Shared sh;
  T* xs = reinterpret_cast<T*>(gv2_smem);
  constexpr int NT = F::NW * 64, K = F::XCHUNKS * 512, KH = K / 2, XS = KH + F::XPAD, NVEC = KH >> 3, XV = (NVEC + NT - 1) / NT;
  static_assert(!F::GUARD && F::NS % 4 == 0, "exact classes with an even number of step pairs per wave");
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = blockIdx.x * F::COLS;
  const T* A = reinterpret_cast<const T*>(p.A);
  u32x4 xr[MT][XV];
  auto fetch = [&](int kofs) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int row = m < p.M ? m : p.M - 1;
#pragma unroll
      for (int u = 0; u < XV; ++u) {
        const int v = threadIdx.x + NT * u;
        if (v < NVEC) xr[m][u] = gload16(A + (size_t)row * p.lda + kofs + v * 8);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int u = 0; u < XV; ++u) {
        const int v = threadIdx.x + NT * u;
        if (v < NVEC) *reinterpret_cast<u32x4*>(xs + (size_t)m * XS + v * 8) = xr[m][u];
      }
  };
  fetch(0);
  const u32x4 bias_pre = F::bias(p, n0, wave, lane);
  typename F::Regs w;
  F::template issue<0, F::NS>(w, p, n0, K, wave, lane);
  stage();
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  F::template accumulate<0, F::NS / 2>(w, xs, XS, K, 0, wave, lane, acc);
  fetch(KH);
  __syncthreads();                       // every wave is done with the first half of x
  stage();
  __syncthreads();
  F::template accumulate<F::NS / 2, F::NS>(w, xs, XS, K, KH, wave, lane, acc);
  F::finish(acc, p, sh, n0, wave, lane, bias_pre);
}

// ---------------------------------------------------------------------------------------------------------------------
// attention-output projection with the COMBINE of the decode attention's key splits as prologue (see gemv_attn_kernel in
// gemm.hip for the partials' layout and the arithmetic: same association, att rounded to the storage type).  The waves
// share the combine (chunk c belongs to wave c % NW) and hand the combined vector over in LDS.  Only the first weight slots
// are requested in front of the combine: its reads of the partials would queue behind every load issued before them.
template <typename T, typename F, int MT>
__global__ __launch_bounds__(F::NW * 64) void gemv2_attn_kernel(const GemmArgs p, const float* __restrict__ part_ws, int H, int nsplit) {
  extern __shared__ __attribute__((aligned(16))) char gv2_smem[];
  __shared__ typename F::Shared sh;
  T* xs = reinterpret_cast<T*>(gv2_smem);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = F::GUARD ? p.K : F::XCHUNKS * 512, kc = K >> 9, XS = K + F::XPAD;
  const int n0 = blockIdx.x * F::COLS;
  constexpr int PRE = F::NS < 8 ? F::NS : 8;
  typename F::Regs w;
  F::template issue<0, PRE>(w, p, n0, K, wave, lane);
  for (int c = wave; c < kc; c += F::NW) {
    const int k = (c << 9) + lane * 8;
    const int head = k >> 6, dd = k & 63;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int row = m < p.M ? m : p.M - 1;
      const float* base = part_ws + ((size_t)row * H + head) * nsplit * 66;
      float mx = -INFINITY;
      for (int sp = 0; sp < nsplit; ++sp) mx = fmaxf(mx, base[sp * 66]);
      float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      float tl[32];                                         // l_s 2^(m_s - M) per split (nsplit <= 32), zero beyond
#pragma unroll
      for (int i = 0; i < 32; ++i) tl[i] = 0.f;
#pragma unroll
      for (int sp = 0; sp < 32; ++sp) {
        if (sp < nsplit) {
          const float mi = base[sp * 66];
          const float wgt = (mi == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mi - mx);
          tl[sp] = base[sp * 66 + 1] * wgt;
          const float* po = base + sp * 66 + 2 + dd;        // 8-byte aligned (66 floats per partial)
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = fmaf(po[e], wgt, o[e]);
        }
      }
      // the sum in the association of attn_decode_combine_kernel's xor-butterfly (lanes >= nsplit hold zeros there too)
#pragma unroll
      for (int w2 = 16; w2 > 0; w2 >>= 1)
#pragma unroll
        for (int i = 0; i < w2; ++i) tl[i] += tl[i + w2];
      const float L = tl[0];
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = o[e] / L;
      *reinterpret_cast<u32x4*>(xs + (size_t)m * XS + k) = pack8<T>(x);     // the attention output in its storage type
    }
  }
  F::template issue<PRE, F::NS>(w, p, n0, K, wave, lane);
  const u32x4 bias_pre = F::bias(p, n0, wave, lane);
  __syncthreads();
  F::product(w, p, xs, XS, K, sh, n0, wave, lane, bias_pre);
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm-prologue form (see GemvLnArgs in gemm_shared.cuh and gemv_ln_kernel in gemm.hip: the chain
//     z --[post-LN, Sandwich scale |z|max]--> + residual --> t --[pre-LN, Sandwich scale |t|max]--> x_in ;  y = epilogue(x_in W^T + b)
// of mpu/sparse_transformer.py:314-342 inside every workgroup; same arithmetic and rounding points).  K <= 4096: a thread owns
// NV = 512 / threads 8-element vectors (two with 4 waves, one with 8).  With up to two rows the whole weight stream of the wave
// is requested in front of the prologue; with more rows the prologue's registers leave room for the first 8 slots only.
// (one row: three waves per SIMD -- 168 registers -- so that the 640 workgroups of the h -> 4h launch are resident at once)
template <typename T, typename F, int MT, bool SF>
__global__ __launch_bounds__(F::NW * 64) __attribute__((amdgpu_waves_per_eu(MT == 1 ? 3 : 1)))
void gemv2_ln_kernel(const GemvLnArgs q) {
  typedef Row8<T, SF> SR;                // a stream row slice
  constexpr int NW = F::NW;
  extern __shared__ __attribute__((aligned(16))) char gv2_smem[];           // x_in [MT][K + pad] as T
  __shared__ float part[NW][MT][2];
  __shared__ float pstat[MT][2];            // post-LayerNorm: mean, rstd per row
  __shared__ typename F::Shared sh;
  __shared__ uint32_t redm[16];
  __shared__ float s_amax;
  constexpr int NT = NW * 64, NV = 512 / NT;
  static_assert(NW == 4 || NW == 8, "the prologue's block sums pair 4 or 8 wave partials");
  const GemmArgs& p = q.g;
  T* xs = reinterpret_cast<T*>(gv2_smem);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int K = F::GUARD ? p.K : F::XCHUNKS * 512, nvec = K >> 3, XS = K + F::XPAD;
  const float inv_k = 1.0f / (float)K;
  const bool has_post = q.gamma_p != nullptr;
  int vv[NV]; bool okv[NV];
#pragma unroll
  for (int u = 0; u < NV; ++u) { vv[u] = threadIdx.x + NT * u; okv[u] = vv[u] < nvec; }
  // ---- the prologue's own inputs FIRST (a few KB, L2-resident), then the weight stream.  The small loads are UNCONDITIONAL
  //      (clamped vector / row indices, a stand-in pointer where an operand is absent; the unwanted values are replaced by
  //      zeros below): a conditional load ends in a control-flow join at which the compiler drains the memory counter, and
  //      the weight loads behind it would start one memory latency late.
  const T* Z = reinterpret_cast<const T*>(q.z);
  const T* gpp = reinterpret_cast<const T*>(has_post ? q.gamma_p : q.gamma);
  const T* bpp = reinterpret_cast<const T*>(has_post ? q.beta_p : q.beta);
  const void* rsrc = has_post ? q.res : q.z;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  u32x4 zr[MT][NV], gpr[NV], bpr[NV], gnr[NV], bnr[NV];
  typename SR::raw rr[MT][NV];           // the stream rows: the residual (post-LN form) or z itself (plain-input form)
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const int v = okv[u] ? vv[u] : 0;
    gnr[u] = gload16(reinterpret_cast<const T*>(q.gamma) + v * 8);
    bnr[u] = gload16(reinterpret_cast<const T*>(q.beta) + v * 8);
    gpr[u] = gload16(gpp + v * 8);
    bpr[u] = gload16(bpp + v * 8);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int row = m < p.M ? m : p.M - 1;
      zr[m][u] = gload16(Z + (size_t)row * K + v * 8);        // (fp32 plain input: in bounds of the wider rows, discarded)
      rr[m][u] = SR::ld(rsrc, (size_t)row * K + v * 8);
    }
  }
  // (the published abs-max of z: a vector load as well, for gv2_bias's reason)
  const float zamax_raw = *((const COGV_GLOBAL float*)(q.z_absmax ? q.z_absmax : reinterpret_cast<const float*>(q.gamma)) + gv2_vzero());
  const int n0 = blockIdx.x * F::COLS;
  constexpr int PRE = MT <= 2 ? F::NS : (F::NS < 8 ? F::NS : 8);
  typename F::Regs w;
  F::template issue<0, PRE>(w, p, n0, K, wave, lane);
  float zamax = q.z_absmax ? zamax_raw : 0.f;
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    const bool ok = okv[u];
    gnr[u] = ok ? gnr[u] : zero4;
    bnr[u] = ok ? bnr[u] : zero4;
    gpr[u] = (ok && has_post) ? gpr[u] : zero4;
    bpr[u] = (ok && has_post) ? bpr[u] : zero4;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      zr[m][u] = (ok && m < p.M && (has_post || !SF)) ? zr[m][u] : zero4;
      rr[m][u] = (ok && m < p.M && (has_post || SF)) ? rr[m][u] : SR::zero();
    }
  }
  // sums over the workgroup of MT values at once (one LDS round for all rows); pairwise over the waves
  auto block_sums = [&](float (&a)[MT]) {
#pragma unroll
    for (int m = 0; m < MT; ++m) a[m] = wave_sum_uniform(a[m]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int m = 0; m < MT; ++m) part[wave][m][0] = a[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float s = (part[0][m][0] + part[1][m][0]) + (part[2][m][0] + part[3][m][0]);
      if (NW == 8) s += (part[4 % NW][m][0] + part[5 % NW][m][0]) + (part[6 % NW][m][0] + part[7 % NW][m][0]);
      a[m] = s;
    }
  };
  float tv[MT][NV][8];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      if (SF && !has_post) SR::to_f(rr[m][u], tv[m][u]);         // the plain input IS the fp32 stream
      else unpack8<T>(zr[m][u], tv[m][u]);
    }
  if (has_post) {                 // t = residual + LN_post(z), rounded where ln_fwd_kernel rounds
    if (!q.z_absmax) {
      // max |z| over all rows taken HERE instead of published by z's producer: the vectors are in registers anyway, and the
      // producer (a skinny-M launch whose workgroups all finish together) is spared a burst of same-address atomics in its tail
      uint32_t zpk = 0u;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int u = 0; u < NV; ++u) zpk = absmax_pk8(zpk, zr[m][u]);       // rows >= M and vectors past K are zero
      zamax = absmax_pk_block<T>(zpk, redm);
    }
    const float c = zamax * 0.125f;
    const float eps_p = q.eps * c * c;
    // mean and rstd per row as ln_fwd_kernel takes them (one wave per row, common.cuh: ln_row_stats_wave) from the z rows in
    // LDS -- x_in's place, which is written much later: t is the Sandwich-LN kernel's to the bit whatever the form's wave count
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int u = 0; u < NV; ++u)
        if (okv[u]) *reinterpret_cast<u32x4*>(xs + (size_t)m * XS + vv[u] * 8) = zr[m][u];
    __syncthreads();
    for (int m = wave; m < MT; m += NW) {
      float mean = 0.f, rstd = 0.f;                                  // rows >= M: zeros nobody reads
      if (m < p.M) ln_row_stats_wave<T>(xs + (size_t)m * XS, K, inv_k, eps_p, lane, mean, rstd);
      if (lane == 0) { pstat[m][0] = mean; pstat[m][1] = rstd; }
    }
    __syncthreads();
    float gp[NV][8], bp[NV][8];
#pragma unroll
    for (int u = 0; u < NV; ++u) { unpack8<T>(gpr[u], gp[u]); unpack8<T>(bpr[u], bp[u]); }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float mean = pstat[m][0], rstd = pstat[m][1];
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        float r[8], o[8];
        SR::to_f(rr[m][u], r);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = fmaf((tv[m][u][i] - mean) * rstd, gp[u][i], bp[u][i]);   // ln_fwd_kernel's: one fused multiply-add
        if (!SF) { u32x4 lo = pack8<T>(o); unpack8<T>(lo, o); }   // all-T form: LayerNorm output rounded before the residual add
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] += r[i];
        if (!SF) { const u32x4 ov = pack8<T>(o); unpack8<T>(ov, o); }   // t rounded to its storage type
#pragma unroll
        for (int i = 0; i < 8; ++i) tv[m][u][i] = o[i];
        if (!okv[u]) {
#pragma unroll
          for (int i = 0; i < 8; ++i) tv[m][u][i] = 0.f;
        } else if (blockIdx.x == 0 && q.t_out && m < p.M)
          (void)SR::st(q.t_out, (size_t)m * K + vv[u] * 8, o, 0u);
      }
    }
  }
  // pre-LN: Sandwich scale = max |t| over all rows (x.abs().max(), mpu/sparse_transformer.py:40-44) -- the published
  // abs-max when t is the plain input, else taken here -- then mean / variance per row
  float amax;
  if (!has_post && q.z_absmax) {
    amax = zamax;
  } else {
    uint32_t amax_pk = 0u;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int u = 0; u < NV; ++u) {                                // rows >= M and vectors past K are zero
        if (SF) {
#pragma unroll
          for (int i = 0; i < 8; ++i) amax_pk = max(amax_pk, __float_as_uint(tv[m][u][i]) & 0x7fffffffu);
        } else amax_pk = absmax_pk8(amax_pk, pack8<T>(tv[m][u]));
      }
    __syncthreads();
    const float a = SF ? absmax_f32_block(amax_pk, redm) : absmax_pk_block<T>(amax_pk, redm);
    if (threadIdx.x == 0) s_amax = a;
    __syncthreads();
    amax = s_amax;
  }
  {
    const float c = amax * 0.125f;
    const float eps_n = q.eps * c * c;
    float s[MT], qq[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      s[m] = 0.f;
#pragma unroll
      for (int u = 0; u < NV; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) s[m] += tv[m][u][i];
    }
    block_sums(s);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float mean = s[m] * inv_k;
      qq[m] = 0.f;
#pragma unroll
      for (int u = 0; u < NV; ++u)
        if (okv[u])
#pragma unroll
          for (int i = 0; i < 8; ++i) { const float d = tv[m][u][i] - mean; qq[m] += d * d; }
    }
    block_sums(qq);
    float gn[NV][8], bn[NV][8];
#pragma unroll
    for (int u = 0; u < NV; ++u) { unpack8<T>(gnr[u], gn[u]); unpack8<T>(bnr[u], bn[u]); }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float mean = s[m] * inv_k, rstd = 1.0f / sqrtf(qq[m] * inv_k + eps_n);
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        if (okv[u]) {
          float o[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] = (tv[m][u][i] - mean) * rstd * gn[u][i] + bn[u][i];
          *reinterpret_cast<u32x4*>(xs + (size_t)m * XS + vv[u] * 8) = pack8<T>(o);
        }
      }
    }
  }
  F::template issue<PRE, F::NS>(w, p, n0, K, wave, lane);
  // the epilogue's bias: requested here, behind the weights (it is needed after the last of them; the prologue's registers are
  // free again), still far ahead of its use
  const u32x4 bias_pre = F::bias(p, n0, wave, lane);
  __syncthreads();
  // ---- the matrix-vector product proper
  F::product(w, p, xs, XS, K, sh, n0, wave, lane, bias_pre);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: from a launch plan (gemv_plan.h: the class list, and gv_plan(), which gemm.hip asked) to the instantiation.  This
// unit expands its format's rows of that list once, in gv2_run; nothing here decides anything.
using TT = std::conditional<COGV_GEMV_TU != 0, f16_t, bf16_t>::type;

#define GV2_CAT2(a, b) a##b
#define GV2_CAT(a, b) GV2_CAT2(a, b)
#if defined(COGV_GEMV_W4)   // (units gemv_w4_<dtype>.o: the same kernels on the 4-bit operand)
using WT = W4<TT>;
#define GV2_CLASSES GV_CLASSES_4
#define GV2_RUN GV2_CAT(cogv_gemv2_w4_run_, COGV_GEMV_TU)
#elif !defined(COGV_GEMV_W8)
using WT = W16<TT>;
#define GV2_CLASSES GV_CLASSES_16
#define GV2_RUN GV2_CAT(cogv_gemv2_run_, COGV_GEMV_TU)
#else   // (units gemv_w8_<dtype>.o: the same kernels on the 8-bit operand; nothing of the 16-bit operand is instantiated here)
using WT = W8<TT>;
#define GV2_CLASSES GV_CLASSES_8
#define GV2_RUN GV2_CAT(cogv_gemv2_w8_run_, COGV_GEMV_TU)
#endif
template <int J, int KCMAX, bool G> using GvV = FormV<WT, J, KCMAX, G, 1, 4>;
template <int NWK, int LMAX, bool G, int MT, int TW> using GvM = FormM<WT, NWK, TW, LMAX, G, MT>;

// One class at one MT: F its form with one tile per workgroup (plain and attention kind), FL the LayerNorm kind's.  Only the
// kinds in KINDS are instantiated, the plain one as the two-halves kernel where K2 says so.
template <typename F, typename FL, int FORM, int P0, int TWL, int MT, int KINDS, bool K2>
int gv2_launch(int kind, const GvPlan& pl, const GvCall& c) {
  static_assert(F::NW * 64 == gv_threads(FORM, P0, 1) && F::COLS == gv_cols(FORM, P0, 1) && F::XPAD == gv_xpad(FORM), "gemv_plan.h");
  static_assert(FL::NW * 64 == gv_threads(FORM, P0, TWL) && FL::COLS == gv_cols(FORM, P0, TWL) && FL::XPAD == gv_xpad(FORM), "gemv_plan.h");
  const dim3 grid(pl.grid), block(pl.threads);
  const size_t lds = (size_t)pl.lds;
  hipStream_t st = reinterpret_cast<hipStream_t>(c.stream);
  if constexpr ((KINDS & GV_LN) != 0) {
    if (kind == GV_LN) {
      const GemvLnArgs& a = *reinterpret_cast<const GemvLnArgs*>(c.args);
      if (c.stream_f32) hipLaunchKernelGGL((gemv2_ln_kernel<TT, FL, MT, true>), grid, block, lds, st, a);
      else hipLaunchKernelGGL((gemv2_ln_kernel<TT, FL, MT, false>), grid, block, lds, st, a);
      return COGV_OK;
    }
  }
  const GemmArgs& a = *reinterpret_cast<const GemmArgs*>(c.args);
  if constexpr ((KINDS & GV_ATTN) != 0) {
    if (kind == GV_ATTN) {
      hipLaunchKernelGGL((gemv2_attn_kernel<TT, F, MT>), grid, block, lds, st, a, c.partials, c.heads, c.nsplit);
      return COGV_OK;
    }
  }
  if constexpr ((KINDS & GV_PLAIN) != 0) {
    if (kind == GV_PLAIN) {
      if constexpr (K2) {
        // the two-halves kernel: LDS for half the row length; above 64 KB in all by attribute
        static bool attr = false;
        if (!attr) {
          if (lds > (size_t)GV_MAX_SHMEM &&
              hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv2_k2_kernel<TT, F, MT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return COGV_ERR_UNSUPPORTED;
          attr = true;
        }
        hipLaunchKernelGGL((gemv2_k2_kernel<TT, F, MT>), grid, block, lds, st, a);
      } else {
        hipLaunchKernelGGL((gemv2_kernel<TT, F, MT>), grid, block, lds, st, a);
      }
      return COGV_OK;
    }
  }
  return COGV_ERR_UNSUPPORTED;
}

#define GV2_RUN_V(P0, P1, G, KINDS, K2MTS, TW2, TW48) gv2_launch<GvV<P0, P1, G>, GvV<P0, P1, G>, GV_FORM_V, P0, 1, 1, KINDS, false>(kind, pl, c)
#define GV2_RUN_MT(P0, P1, G, KINDS, K2MTS, TWL, MT) \
  gv2_launch<GvM<P0, P1, G, MT, 1>, GvM<P0, P1, G, MT, TWL>, GV_FORM_M, P0, TWL, MT, KINDS, ((K2MTS) & MT) != 0>(kind, pl, c)
#define GV2_RUN_M(P0, P1, G, KINDS, K2MTS, TW2, TW48)                                  \
  (pl.mt == 2 ? GV2_RUN_MT(P0, P1, G, KINDS, K2MTS, TW2, 2)                            \
              : pl.mt == 4 ? GV2_RUN_MT(P0, P1, G, KINDS, K2MTS, TW48, 4) : GV2_RUN_MT(P0, P1, G, KINDS, K2MTS, TW48, 8))
#define GV2_RUN_ROW(NAME, FORM, KF, KT, P0, P1, G, KINDS, STOP, K2MTS, TW2, TW48) \
  case GVC_##NAME: return GV2_RUN_##FORM(P0, P1, G, KINDS, K2MTS, TW2, TW48);

}  // namespace


// the unit's one entry point: the kernel of plan `pl` (generation 2, of this unit's format) for a product of `kind`
extern "C" __attribute__((visibility("hidden"))) int GV2_RUN(int kind, const GvPlan* plan, const GvCall* call) {
  const GvPlan& pl = *plan;
  const GvCall& c = *call;
  switch (pl.cls) {
    GV2_CLASSES(GV2_RUN_ROW)
    default: return COGV_ERR_UNSUPPORTED;
  }
}

#endif  // COGV_GEMV_TU
