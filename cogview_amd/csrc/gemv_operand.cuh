// The weight operand of the decode step's weight-streaming kernels: what B's rows hold (16-bit elements, E4M3 bytes with a row
// scale, MXFP4 blocks) and how a load of them becomes arithmetic.  Shared by gemv.hip (FormV / FormM, 1 .. 8 rows) and
// gemv_wide.hip (1 .. 64 rows); device code only, and nothing here is instantiated until a kernel names it.
#pragma once
#include "gemm_shared.cuh"
#include "mxfp4_stream.cuh"

namespace {

// a zero the compiler cannot see through, in a vector register: added to a wave-uniform address it keeps the load on the
// vector memory path (see gv2_bias)
__device__ __forceinline__ int gv2_vzero() {
  int zero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
  return zero;
}

// =====================================================================================================================
// The weight operand of a form: what B's rows hold and how a load of them becomes arithmetic.  Nothing else of a form depends
// on the format.
//   T, Elem, Slot       the dtype of x and C; a row element of B; what one lane loads per FormV slot (its 8 contraction elements)
//   load, unpack        a FormV slot from memory (streamed: e4m3_stream.cuh), and as 8 floats
//   KL, FR, frag        FormM: contraction elements of the 16 rows x 16 bytes one load covers, the MFMA fragments that is, and
//                       fragment f of a load as the A operand
//   Scale, scale        what a finishing lane requests for its 8 columns n + 8g .. + 7, behind the weights and far ahead of the tail.
//                       (n and g apart: W16 asks for nothing, and a column computed at the call only to be dropped moved the
//                       compares and branches of every 16-bit FormV kernel)
//   Factors, factors, mul   the same as the 8 factors of the column sums, built once in front of the row loop, and the multiply
template <typename T_>
struct W16 {
  typedef T_ T;
  typedef T_ Elem;
  typedef u32x4 Slot;
  static constexpr int KL = 32, FR = 1, EPL = 8, PK = 1;
  template <int L> struct MRegs { u32x4 w[L]; };
  struct Scale {};
  static __device__ __forceinline__ Slot load(const Elem* q) { return ld_stream<u32x4>(q); }
  static __device__ __forceinline__ void unpack(const Slot& w, float* f) { unpack8<T>(w, f); }
  static __device__ __forceinline__ typename HT<T>::v8 frag(const u32x4& w, int) { return __builtin_bit_cast(typename HT<T>::v8, w); }
  typedef Scale Factors;
  static __device__ __forceinline__ Scale scale(const GemmArgs&, int, int) { return Scale{}; }
  static __device__ __forceinline__ Factors factors(const Scale&) { return Factors{}; }
  static __device__ __forceinline__ float mul(float x, const Factors&, int) { return x; }
};

// 8-bit weights (see the file header): B is uint8 OCP E4M3 [N][ldb], p.wscale [N] fp32.
// the row scales of the 8 columns n .. n + 7 a finishing lane multiplies its sums by: requested BEHIND the weights (the memory
// counter retires in order: they arrive right after the last weight, long before the sums are complete).  Unconditional, with a
// clamped column, for gv2_bias's reason.
struct Scale8 { f32x4 a, b; };
__device__ __forceinline__ Scale8 gv2_scale(const GemmArgs& p, int n) {
  const float* s = p.wscale + (n < p.N ? n : p.N - 8) + gv2_vzero();
  return Scale8{*(const COGV_GLOBAL f32x4*)s, *(const COGV_GLOBAL f32x4*)(s + 4)};
}
// A FormV slot is 8 BYTES = the same 8 contraction elements of a column as a 16-bit slot, so the x side, the fmaf chain and its
// order do not change; a slot is half as many bytes, so a wave owns twice as many columns (J).  A FormM load holds 16
// contraction elements of its row: TWO fragments -- lane l supplies row (l & 15), elements 16 (l >> 4) .. + 15 of the load's
// 64-element block, the first 8 to one v_mfma_f32_16x16x32 and the last 8 to the next, and the x operand of each takes the same 8
// elements of its row from LDS (a contraction is a sum over all slots: any slot-to-lane mapping serves as long as both operands
// use it).  E4M3 -> T is exact (fp16 and bf16 hold every E4M3 value), through fp32 in registers.
template <typename T_>
struct W8 {
  typedef T_ T;
  typedef uint8_t Elem;
  typedef u32x2 Slot;
  static constexpr int KL = 64, FR = 2, EPL = 8, PK = 1;
  template <int L> struct MRegs { u32x4 w[L]; };
  typedef Scale8 Scale;
  static __device__ __forceinline__ Slot load(const Elem* q) { return ld_stream<u32x2>(q); }
  static __device__ __forceinline__ void unpack(const Slot& w, float* f) { unpack8_e4m3(w[0], w[1], f); }
  static __device__ __forceinline__ typename HT<T>::v8 frag(const u32x4& w, int f) {
    float x[8];
    unpack8_e4m3(w[2 * f], w[2 * f + 1], x);
    return __builtin_bit_cast(typename HT<T>::v8, pack8<T>(x));
  }
  static __device__ __forceinline__ Scale scale(const GemmArgs& p, int n, int g) { return gv2_scale(p, n + g * 8); }
  struct Factors { float s[8]; };
  static __device__ __forceinline__ Factors factors(const Scale& sc) { return Factors{{sc.a[0], sc.a[1], sc.a[2], sc.a[3], sc.b[0], sc.b[1], sc.b[2], sc.b[3]}}; }
  static __device__ __forceinline__ float mul(float x, const Factors& f, int i) { return x * f.s[i]; }      // the row scale, once, in front of the shared epilogue
};

// 4-bit weights (OCP MXFP4: mxfp4_stream.cuh): B is uint8 [N][ldb], two E2M1 codes per byte, p.bscale [N][ldbs] one E8M0 byte per
// block of 32 contraction elements.  ONE 16-BYTE LOAD OF A LANE IS ONE BLOCK: 32 consecutive contraction elements of one weight row
// and one scale byte, which is requested right behind it on the vector memory path (a per-lane address) and folded into the
// conversion (v_cvt_scalef32_pk_*_fp4: two elements per instruction, what W8 pays) -- there is no per-column factor.
//   FormV: a slot is the lane's block, EPL = 32 elements: a wave's load covers 2048 contraction elements of a column, and the x side
//          reads the same 32 elements from LDS.  A column whose K is no multiple of 2048 ends inside a slot: the lanes past K
//          re-read the row's last block (the same request as the lane that owns it: no byte of HBM more) against zeros for x.
//   FormM: a load is FOUR fragments (KL = 128): lane l supplies row (l & 15), elements 32 (l >> 4) .. + 31 of the load's 128-element
//          step, 8 to each v_mfma_f32_16x16x32, converted to T with the scale folded in (exact in bf16; in fp16 wherever code * 2^e
//          is a multiple of 2^-24 below 65520); the x operand of each takes the same 8 elements of its row from LDS.
// The alternative -- a 4-byte slot that keeps W8's 8-element mapping, a scale byte per slot -- asks FormV for four times the loads
// and two registers per 8 elements where this one takes 5 per 32.
template <typename T_>
struct W4 {
  typedef T_ T;
  typedef uint8_t Elem;
  struct Slot { u32x4 q; uint32_t s; };
  static constexpr int KL = 128, FR = 4, EPL = 32, PK = 2;       // PK: contraction elements per Elem
  template <int L> struct MRegs { u32x4 w[L]; uint32_t s[L]; };
  struct Scale {};
  // block kb (32 elements) of row n
  static __device__ __forceinline__ uint32_t block_scale(const GemmArgs& p, int n, int kb) {
    return *(const COGV_GLOBAL uint8_t*)(p.bscale + (size_t)n * p.ldbs + kb);
  }
  static __device__ __forceinline__ Slot load(const GemmArgs& p, int n, int kb) {
    Slot w;
    w.q = ld_stream<u32x4>(reinterpret_cast<const Elem*>(p.B) + (size_t)n * p.ldb + kb * 16);
    w.s = block_scale(p, n, kb);
    return w;
  }
  // elements 8 sub .. + 7 of a slot as floats
  static __device__ __forceinline__ void unpack(const Slot& w, int sub, float* f) { unpack8_mxfp4(w.q[sub], mxfp4_scale_f32(w.s), f); }
  static __device__ __forceinline__ typename HT<T>::v8 frag(const u32x4& w, uint32_t s, int f) {
    return __builtin_bit_cast(typename HT<T>::v8, unpack8_mxfp4_to<T>(w[f], mxfp4_scale_f32(s)));
  }
  typedef Scale Factors;
  static __device__ __forceinline__ Scale scale(const GemmArgs&, int, int) { return Scale{}; }
  static __device__ __forceinline__ Factors factors(const Scale&) { return Factors{}; }
  static __device__ __forceinline__ float mul(float x, const Factors&, int) { return x; }
};

}  // namespace
