// GDN forward for n <= 127 sensors with the neighbour aggregation on the bf16/f16 matrix cores.
//
// The gather-aggregate of models/graph_layer.py:110-117,  z_i = sum_j alpha_ij * xlin_j  over the ~k
// neighbours of every target, is a [n x n] x [n x d] product whose left factor has k+1 non-zeros per
// row.  For n <= 127 the DENSE product on v_mfma_f32_32x32x16 costs 3 x 512 matrix-pipe cycles per
// window and CU, against ~10 k VALU cycles for the sparse row-gather of gdn_forward.hip (which is
// VALU-issue bound: profiles/r02_sq_counters*.json).  fp32 inputs are kept at fp32 accuracy by
// splitting BOTH factors into two f16 terms (x = hi + lo, each rounded to nearest: |x - hi - lo| <=
// 2^-24 |x|) and issuing hi*hi + lo*hi + hi*lo: three products, fp32 accumulate.  With bf16 STORAGE
// (BASELINE configs[2]/[4]: x and the projected tile xlin are bf16) the tile is one exact bf16 term
// and only alpha is split (two bf16 terms): two products.
//
// One workgroup = NT waves = one window at a time (persistent loop over windows); wave wv owns
// sensors 32wv .. 32wv+31 both as SOURCES (projection rows) and as TARGETS (softmax rows, outputs).
//
//   P  projection on the matrix cores: xlin'[32 rows, d] = x_tile . lin'^T (+ C-in), lin' and C-in
//      carry the eval BatchNorm of models/GDN.py:77 folded in (softmax weights sum to 1, so an affine
//      map per column commutes with the aggregation); a third 32-column tile whose columns 0 / 1 are
//      a_i / a_j yields the attention scalars s_i, s_j of every sensor (graph_layer.py:94-104).
//      The accumulators (column on the lane, source rows in the registers) ARE the A operand of the
//      aggregation product Z^T = X^T . A^T (k order permuted, see pos()): they are split and
//      broadcast to the other waves through LDS — 32 KB per window, no transposition anywhere.
//   S  softmax of one target per lane pair (16 list slots each, logits in registers, one DPP
//      exchange), weights split into two 16-bit terms and SCATTERED into the wave's private dense
//      [32 targets x K] LDS image (zeroed once: the sensor graph is the same for every window, so
//      every window rewrites exactly the same positions).
//   M  8 k-steps x d/32 column blocks x 3 products of v_mfma_f32_32x32x16; operands by ds_read_b128.
//   E  epilogue on the Z^T accumulators (target on the lane, columns in the registers): ReLU, x
//      embedding, BatchNorm, ReLU, Linear(d->1) — the final sum over columns is lane-local.
//
// Two barriers per window; the next window's x values are loaded into registers before P and stored
// to LDS after E.
//
// The FUSED kernel with fp32 storage runs P and M in the other order (DCfg::XAGG).  GraphLayer's lin has no
// bias, so  z_i = sum_j alpha_ij (lin' x_j) + C = lin' (sum_j alpha_ij x_j) + C:  it aggregates the raw window
// (16 WK columns: ONE 32-column block instead of d/32) and projects the 32 aggregated rows of each wave afterwards.
//   X  the staging thread of (k-step s, lane half h, column w) holds the 8 sources of that operand slot, splits
//      them once and writes them as a ready X^T fragment (besides the row-major tile the scalar tile reads);
//   P0 only the scalar tile (s_i, s_j) is left of P;
//   M  Zx^T[w, target] += X^T . A^T, one column block; the accumulator (target on the lane, w in the registers)
//      IS the B operand of the projection in k order "element j of half h = w 16wk + 8(j>>2) + 4h + (j&3)";
//      w <= 16 (DCfg::XHALF): 2 passes (ahi, alo) x 8 k-steps = 16 products instead of 24, 4 ds_read_b128 less per
//      pass pair and k-step: product rows 16 .. 31, which no window column fills, carry the lo term of X^T and are
//      added to rows 0 .. 15 (accumulator registers 8 + j to j) in front of P1; the two passes multiply the SAME
//      X^T fragment, which DCfg::XKEEP k-steps keep in registers from the first to the second;
//   P1 out^T[c, target] = lin' . Zx + C (C-in from the table block), the layout E consumes.
// With bf16 storage the projected tile must be rounded to bf16 as the staged path stores it: that order stays.
#include "gdn_common.hpp"

#include <stdlib.h>

int gdn_dense_fused_op_d128(int op, const void* args, int bf16, unsigned* plan_out, long long* bytes,
                            hipStream_t st);   // gdn_forward_dense_d128.hip

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef __bf16 b2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// [r18] the three parts of the window loop's VALU trim, each switchable for same-box A/B builds
// (tools/_diag/build_variant.sh ... -DGDN_TRIM_PACK=0): all on in the product
#ifndef GDN_TRIM_SPLIT
#define GDN_TRIM_SPLIT 1    // Fmt<FMT_F16>::split2: three instructions per pair of values
#endif
#ifndef GDN_TRIM_RELU
#define GDN_TRIM_RELU 1     // relu_acc: one instruction on an MFMA result
#endif
#ifndef GDN_TRIM_PACK
#define GDN_TRIM_PACK 1     // Pk2: v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 on register pairs
#endif

// Elementwise fp32 arithmetic on PAIRS of values: one v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 per pair (a
// broadcast operand costs nothing: op_sel_hi), written out as vector operations as in axpy_pack of gdn_forward.hip —
// the vectoriser does not pack these loops by itself.  Each half rounds exactly like the scalar instruction, and the
// window loop uses them only where no ORDER of additions changes (never for the softmax sum / max, the head's
// `part`, the butterfly).  PACK = false: the same operations one value at a time (DCfg::PACK).
template <bool PACK>
struct Pk2 {
  static __device__ __forceinline__ f32x2 mul(f32x2 a, f32x2 b) {
    if constexpr (PACK) return a * b;
    return f32x2{a[0] * b[0], a[1] * b[1]};
  }
  static __device__ __forceinline__ f32x2 mul(f32x2 a, float b) { return mul(a, f32x2{b, b}); }
  static __device__ __forceinline__ f32x2 add(f32x2 a, f32x2 b) {
    if constexpr (PACK) return a + b;
    return f32x2{a[0] + b[0], a[1] + b[1]};
  }
  static __device__ __forceinline__ f32x2 add(f32x2 a, float b) { return add(a, f32x2{b, b}); }
  static __device__ __forceinline__ f32x2 sub(f32x2 a, float b) {
    if constexpr (PACK) return a - f32x2{b, b};
    return f32x2{a[0] - b, a[1] - b};
  }
  static __device__ __forceinline__ f32x2 fma(f32x2 a, f32x2 b, f32x2 c) {
    if constexpr (PACK) return __builtin_elementwise_fma(a, b, c);
    return f32x2{__builtin_fmaf(a[0], b[0], c[0]), __builtin_fmaf(a[1], b[1], c[1])};
  }
};

// ReLU of a matrix-core accumulator register.  fmaxf(acc, 0) costs TWO instructions there: IEEE maxnum must quiet a
// signalling NaN, the compiler cannot prove that an MFMA result is none and puts a canonicalising v_max_f32 v, v, v in
// front.  IEEE maximum needs no such step: ONE v_maximum3_f32 v, v, 0, 0 on gfx950.  It differs from fmaxf for a NaN
// accumulator only, which it hands on as NaN where fmaxf returned 0 (and max(-0, +0) is +0 for certain): a window
// with a NaN input is flagged by the range guard of planned launches and recomputed by the row-gather kernel, and an
// unguarded launch on such a window now yields NaN outputs for the targets the NaN reaches instead of finite numbers
// that meant nothing.
__device__ __forceinline__ float relu_acc(float v) {
#if GDN_TRIM_RELU
  return __builtin_elementwise_maximum(v, 0.f);
#else
  return fmaxf(v, 0.f);
#endif
}

// [r27] DCfg::XKEEP / DCfg::BLDS: -1 = the table in DCfg, otherwise forced for every instantiation of the family
#ifndef GDN_XKEEP
#define GDN_XKEEP -1
#endif
#ifndef GDN_BL_LDS
#define GDN_BL_LDS -1
#endif

enum { FMT_F16 = 0, FMT_BF16 = 1 };
#define GDN_LOG2E 1.44269504088896340736f
// f16 terms: alpha is scaled by 2^12 and the projected tile by 2^3 before they are split, so that the
// lo terms of small weights / small features stay above the f16 subnormal floor (6e-8); the product is
// unscaled by 2^-15 inside the epilogue constants.  |xlin'| must stay below 65504 / 8.
#define GDN_F16_ALPHA_SCALE 4096.0f
#define GDN_F16_X_SCALE 8.0f
// The fused fp32-storage kernel aggregates the RAW window and projects afterwards (see its head): the x operand
// of the aggregation carries 2^3, the aggregated row is brought from 2^15 back to 2^3 (x 2^-12, exact) before
// it is split for the projection, whose lin' operand carries GDN_F16_X_SCALE: the result is unscaled by 2^-6.
#define GDN_F16_XT_SCALE 8.0f
#define GDN_F16_Z_SCALE 8.0f

// ---- 16-bit term splitting ------------------------------------------------------------------------
template <int FMT>
struct Fmt;

template <>
struct Fmt<FMT_F16> {
  // round to nearest even (v_cvt_pk_f16_f32 or two v_cvt_f16_f32).  NOT inline asm: the result is an MFMA
  // operand, and hipcc inserts the VALU-write -> MFMA-read wait states only for instructions it can see (an
  // asm conversion directly in front of the product fed it stale registers: wrong first column block)
  // The two EMPTY asm statements (nothing executes in them) pin a and b as MATERIALISED fp32 values.  Without them
  // a product feeding the conversion — pk(x * s, ...) after inlining — is contracted into one v_fma_mixlo_f16,
  // which rounds the EXACT product to f16, while res0 / res1 subtract from the fp32-ROUNDED product: where the
  // two roundings disagree (a double-rounding case, one value in ~2^13) the compiler had materialised two
  // different "hi" values, hi + lo missed the value by a whole f16 ulp (2^-11 relative) and the forward was off by
  // 1.2e-6 instead of 3e-8 (4 of the 8192 lin' operand halves of a plan; found in round 3 by comparing plans
  // built by two compilations of the same source, tools/_diag/plan_words_probe.py).
  // What pk pins is its own by-value COPY of each argument: a caller that goes on using the value (res0 / res1 do)
  // pays a v_mov per value for it, and a residual routed through pk again is rounded twice (v_fma_mix_f32, then
  // v_cvt_f16_f32).  Fine for a lone conversion (a store of two values) and for code outside the window loop; a
  // SPLIT inside it goes through split2 below, which pins in place and leaves the residual un-pinned.
  static __device__ __forceinline__ unsigned pk(float a, float b) {
    asm("" : "+v"(a));
    asm("" : "+v"(b));
    const h2 p = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(unsigned, p);
  }
  // x - float(half of p): exact in fp32 (p is x rounded to 11 bits).  Plain C (v_cvt_f32_f16 + v_sub, or a
  // v_fma_mix the compiler picks itself): hipcc pads hazards only around instructions it can see
  // x - float(half) as fma(float(half), -1, x) with the -1 hidden from the optimiser in a scalar register
  // (an EMPTY asm: nothing executes in it), so that instruction selection sees fma(fpext(f16), s, f32) and
  // emits ONE v_fma_mix_f32 instead of v_cvt_f32_f16 + v_sub_f32 (the split is ~25 % of the kernel's VALU work)
  static __device__ __forceinline__ float neg_one() {
    float v = -1.0f;
    asm("" : "+s"(v));
    return v;
  }
  static __device__ __forceinline__ float res0(unsigned p, float x) {
    return __builtin_fmaf((float)__builtin_bit_cast(h2, p)[0], neg_one(), x);
  }
  static __device__ __forceinline__ float res1(unsigned p, float x) {
    return __builtin_fmaf((float)__builtin_bit_cast(h2, p)[1], neg_one(), x);
  }
  // Both terms of a pair of values in THREE instructions (v_cvt_pk_f16_f32, v_fma_mixlo_f16, v_fma_mixhi_f16), where
  // pk(a, b) + pk(res0, res1) above compile to ten for a pair whose values the caller computed itself ([r18]: a v_mov
  // per value because pk pins a by-value COPY while the residual still needs the value, and the residual rounded
  // twice, v_fma_mix_f32 + v_cvt_f16_f32).  Same bits.  Four EMPTY asm statements, nothing executes in any of them:
  //   a, b  pinned IN PLACE, in the caller's variables: the conversion and the residual both read the one materialised
  //         fp32 value (a product in front of it cannot be contracted into either: the round-3 bug at pk), no copy;
  //   p     the converted pair as ONE packed register: without the pin the residual re-converts each value on its own
  //         (two v_cvt_f16_f32 besides the v_cvt_pk_f16_f32) instead of reading the halves of p through op_sel;
  //   l0    the first lo half: without it the vectoriser pairs the two residuals into v_cvt_f32_f16 x 2 +
  //         v_pk_fma_f32 + v_cvt_pk_f16_f32.
  // The RESIDUAL fma(float(hi), -1, a) itself is not pinned and needs none: it is exact in fp32 (hi is a rounded to 11
  // bits), so converting the exact value once (v_fma_mixlo/hi_f16) or the fp32-rounded value (v_fma_mix_f32, then
  // v_cvt_f16_f32) is one and the same rounding — there is no second "hi" to disagree with.
  static __device__ __forceinline__ void split2(float& a, float& b, unsigned& hi, unsigned& lo) {
#if !GDN_TRIM_SPLIT
    hi = pk(a, b);
    lo = pk(res0(hi, a), res1(hi, b));
    return;
#endif
    asm("" : "+v"(a));
    asm("" : "+v"(b));
    h2 p = {(_Float16)a, (_Float16)b};
    asm("" : "+v"(p));
    const float m1 = neg_one();
    _Float16 l0 = (_Float16)__builtin_fmaf((float)p[0], m1, a);
    const _Float16 l1 = (_Float16)__builtin_fmaf((float)p[1], m1, b);
    asm("" : "+v"(l0));
    const h2 l = {l0, l1};
    hi = __builtin_bit_cast(unsigned, p);
    lo = __builtin_bit_cast(unsigned, l);
  }
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
  }
};

template <>
struct Fmt<FMT_BF16> {
  static __device__ __forceinline__ unsigned pk(float a, float b) {
    asm("" : "+v"(a));                         // (materialised fp32 inputs: see Fmt<FMT_F16>::pk)
    asm("" : "+v"(b));
    const b2 p = {(__bf16)a, (__bf16)b};       // v_cvt_pk_bf16_f32, round to nearest even (not asm: see above)
    return __builtin_bit_cast(unsigned, p);
  }
  static __device__ __forceinline__ float res0(unsigned p, float x) { return x - __uint_as_float(p << 16); }
  static __device__ __forceinline__ float res1(unsigned p, float x) { return x - __uint_as_float(p & 0xffff0000u); }
  // (the same arithmetic as before [r18]; the pins stay on by-value copies: see DESIGN 3.1 [r18])
  static __device__ __forceinline__ void split2(float& a, float& b, unsigned& hi, unsigned& lo) {
    hi = pk(a, b);
    lo = pk(res0(hi, a), res1(hi, b));
  }
  static __device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
  }
};

// 8 fp32 values -> NTERM operand fragments (element j of the fragment = v[j]); term t+1 holds the
// rounding residual of terms 0..t
// (TRIM = false: term by term through pk / res0 / res1 as before [r18]; gdn_dense_project_kernel keeps that form:
// split2 costs it 2 .. 5 registers, which takes a wave per SIMD from its w <= 16 instantiations)
template <int FMT, int NTERM, bool TRIM = true>
__device__ __forceinline__ void split8(const float (&v)[8], u32x4 (&out)[NTERM]) {
  float r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = v[j];
  if constexpr (NTERM == 2 && TRIM) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned hi, lo;
      Fmt<FMT>::split2(r[2 * j], r[2 * j + 1], hi, lo);
      out[0][j] = hi;
      out[NTERM - 1][j] = lo;
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < NTERM; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned p = Fmt<FMT>::pk(r[2 * j], r[2 * j + 1]);
      out[t][j] = p;
      if (t + 1 < NTERM) {
        r[2 * j] = Fmt<FMT>::res0(p, r[2 * j]);
        r[2 * j + 1] = Fmt<FMT>::res1(p, r[2 * j + 1]);
      }
    }
}

// Position of source sensor `src` inside a row of the dense attention image.  The projection
// accumulator hands k-step s of a wave's 32 sources to the aggregation product in the order
// "element j of lane half h = source 16s + 8(j>>2) + 4h + (j&3)" (accumulator row map of
// v_mfma_f32_32x32x*); the alpha operand must present the same source in the same k slot 8h + j, so a
// row stores source `src` at src with bits 2 and 3 exchanged and a lane reads 16 contiguous bytes.
__host__ __device__ __forceinline__ int pos_of_source(int src) {
  return (src & ~12) | ((src & 4) << 1) | ((src & 8) >> 1);
}

// ---- compile-time geometry ---------------------------------------------------------------------
enum { DMODE_FUSED = 0 };

template <int NT, int DC, int WK, int SL, int FMT>
struct DCfg {
  static constexpr int KS = 2 * NT;                    // k-steps of 16 sources: 32 NT >= n + 1
  static constexpr int ROWS = 32 * NT;
  static constexpr int THREADS = 64 * NT;
  static constexpr int AROW = KS * 32 + 16;            // bytes per target row of one plane (+16: rows
                                                       // land on distinct 16-B slots, ds_read_b128 conflict-free)
  static constexpr int AWAVE = 32 * AROW;              // ONE 16-bit plane of a wave's 32 targets: the hi and the
                                                       // lo term of alpha take turns in it (scatter hi, its
                                                       // products, scatter lo over the same positions, its
                                                       // product), which halves the image: 2 workgroups per CU
  static constexpr bool XAGG = FMT == FMT_F16;         // aggregate the raw window, project afterwards (file head)
  static constexpr int MCB = XAGG ? 1 : DC;            // 32-column blocks of the aggregation product
  static constexpr int NPX = FMT == FMT_F16 ? 2 : 1;   // terms of the aggregated tile (XAGG: of x^T)
  static constexpr int NTL = FMT == FMT_F16 ? 2 : 3;   // terms of lin.weight / a_i / a_j
  static constexpr int NTXIN = FMT == FMT_F16 ? 2 : 1; // terms of the x values (bf16 storage: exact)
  static constexpr int XP = 16 * WK + 4;               // x tile pitch in floats (odd number of 16-B slots)
  static constexpr int XU = 8 * WK;                    // x values per thread per window
  // XAGG, WK = 1: rows 16 .. 31 of X^T do not exist, so a fragment holds the 16 lanes of each lane half that carry
  // window columns, and the lanes l32 >= 16 read the LO term of their neighbour's slot where the lanes l32 < 16 read
  // the hi term: rows 16 .. 31 of the product Zx^T are the lo-term contribution to rows 0 .. 15 (accumulator
  // registers 8 + j and j of one lane), which P1 adds before it splits the aggregated row (see M in the kernel)
  static constexpr bool XHALF = XAGG && WK == 1;
  static constexpr int XFL = XHALF ? 16 : 32;          // stored lanes per lane half of an X^T fragment
  static constexpr int XFRAG = 2 * XFL * 16;           // bytes per (k-step, block, term)
  static constexpr int OFF_A = 0;
  static constexpr int OFF_XF = NT * AWAVE;            // [KS][MCB][NPX][2 XFL lanes] x 16 B
  static constexpr int OFF_XS = OFF_XF + KS * MCB * NPX * XFRAG;
  static constexpr int OFF_SI = OFF_XS + (XAGG ? 0 : ROWS * XP * 4);   // (XAGG: no row-major x tile)
  static constexpr int OFF_SJ = OFF_SI + ROWS * 4;
  static constexpr int OFF_EC = OFF_SJ + ROWS * 4;     // epilogue column constants: 4 tables of 32 DC floats
  static constexpr int OFF_CS = OFF_EC + 4 * 32 * DC * 4;   // C-in of the scalar tile: [c_i | c_j | zeros][ROWS]
  static constexpr int CS_WORDS = XAGG ? 0 : 3 * ROWS;      // (XAGG: no scalar tile, c_i / c_j are LaneConsts::sadd)
  // [r27] M of the w <= 16 kernel (XHALF) reads the SAME X^T fragment in its ahi and in its alo pass.  XKEEP k-steps
  // keep theirs in registers from the first pass to the second: 4 registers and one ds_read_b128 less per wave and
  // window each.  BLDS pays for them where they do not fit: lin', the A operand of P1 (LaneConsts::bl, 4 DC NTL
  // registers, the same for every wave and every window), waits in LDS behind the table block and is read in front
  // of P1 (DC NTL reads), when the kept fragments are dead.  Only the family built for three workgroups per CU and
  // its NT = 1, 2 siblings (DC = 2, SL <= 16), chosen by compiling (profiles/r27_xkeep_kernel_resources.txt: the
  // fewest reads with no scratch and three waves per SIMD): short lists keep every fragment; SL = 16 keeps all 8 at
  // NT = 4 with lin' in LDS (-8 + 4 reads) and 2 below (lin' in LDS would return what 4 or 6 kept fragments save).
  // GDN_XKEEP / GDN_BL_LDS override both for A/B builds (tools/_diag/build_variant.sh).  DESIGN 3.1 [r27]
  static constexpr bool XKFAM = XHALF && DC == 2 && SL <= 16;
  static constexpr int XKEEP_TABLE = SL <= 8 || NT == 4 ? KS : 2;
  static constexpr int XKEEP = !XKFAM ? 0 : GDN_XKEEP < 0 ? XKEEP_TABLE : GDN_XKEEP < KS ? GDN_XKEEP : KS;
  static constexpr bool BLDS = XKFAM && (GDN_BL_LDS < 0 ? SL > 8 && NT == 4 : GDN_BL_LDS != 0);
  static constexpr int OFF_BL = OFF_CS + CS_WORDS * 4;  // BLDS: [DC][WK][NTL] fragments of 64 lanes x 16 B
  static constexpr int LDS = OFF_BL + (BLDS ? DC * WK * NTL * 1024 : 0);
  // x staging (see the kernel): a thread owns column tid % CW of XU rows.  XAGG: its values 8q .. 8q+7 are one
  // operand slot of X^T, slot tid / CW + q RS = 2 (k-step) + (lane half), in the k order of pos_of_source
  static constexpr int CW = 16 * WK, RS = THREADS / CW;
  static __host__ __device__ constexpr int xrow0(int xsl) { return XAGG ? 16 * (xsl >> 1) + 4 * (xsl & 1) : xsl; }
  static __host__ __device__ constexpr int xro(int u) {
    return XAGG ? 16 * NT * (u >> 3) + 8 * ((u & 7) >> 2) + (u & 3) : u * RS;
  }
  // Workgroups per CU the kernel is compiled for (__launch_bounds__: the register budget follows from it) and is
  // launched at (fused_op refuses a launch whose occupancy query reports fewer).  Three with fp32 storage where a
  // third of the CU's 160 KB of LDS, allocated in units of 1280 bytes, holds the workgroup (3 x NT waves on 4 SIMDs:
  // <= 168 registers at NT = 4; the kernel takes 167 and no scratch); two (<= 256 registers) for bf16 storage, whose
  // row-major tile and 175+ registers do not fit three; the long-list / long-window variants take the whole
  // register file (accumulator registers as spill space) at one.
  static constexpr int LDS_UNIT = 1280;
  static constexpr int LDS_ALLOC = (LDS + LDS_UNIT - 1) / LDS_UNIT * LDS_UNIT;
  // packed fp32 arithmetic in the window loop (Pk2): a v_pk_* operand is an ALIGNED register pair, which costs an
  // instantiation at its register budget a few registers.  Off for the long-list variants (SL > 16), which take the
  // whole register file and spill into accumulator registers as it is: with packing they spilled 2 .. 5 more
  // (DESIGN 3.1 [r18]; no instantiation has scratch either way).  Off for bf16 storage: its kernel sits at its
  // budget too, gained nothing measurable from packing, and keeps the bits of its softmax split (softmax_split)
  static constexpr bool PACK = GDN_TRIM_PACK != 0 && SL <= 16 && FMT == FMT_F16;
  static constexpr int WGS = !(DC == 2 && NT >= 3 && SL <= 16 && WK == 1) ? 1
                             : XAGG && 3 * LDS_ALLOC <= 160 * 1024 ? 3 : 2;
};

struct DArgs {
  const void* x;            // [B, n, w] fp32 (FMT_F16) / bf16 (FMT_BF16), or the raw series [n, series_len]
  int series_len;           // > 0: window b = series[:, series_first + b : series_first + b + w]
  int series_first;
  int batch, n, w, pitch, d;
  const float* lin_w;       // [d, w]
  const float* node_terms;  // [a_i(64) | a_j(64) | c_i(n) | c_j(n)]
  const uint16_t* nbr;      // [n, pitch]
  const float* gnn_bias;    // [d]
  const float* emb;         // [n, d]
  const float* bn1;         // [scale(d) | shift(d)]
  const float* bn2;
  const float* out_w;       // [d]
  const float* out_b;       // [1]
  float* out;               // [B, n]
  const unsigned* plan;     // gdn_fused_plan_build output, or null
  // optional scoring hand-off: keys[sensor * key_pitch + b] = |out - key_gt| in float64 (the radix keys of
  // gdn_score_select, evaluate.py:48-50), written by the epilogue instead of a separate transposing kernel
  const float* key_gt;      // [B, n] ground truth
  double* keys;             // [n, key_pitch]
  int key_pitch;
  // optional range guard (fp32 storage only): set to 1 when an input value lies outside the range the 16-bit
  // operand terms represent (|x| >= the plan's x limit, or NaN) — the launch's results are then not to be used
  // and the caller's gated row-gather launch (gdn_forward_fused_gated) recomputes them in fp32
  int* range_flag;
};

__device__ __forceinline__ float lds_f32(const char* smem, int byte_off) {
  return *reinterpret_cast<const float*>(smem + byte_off);
}
__device__ __forceinline__ u32x4 lds_frag(const char* smem, int byte_off) {
  return *reinterpret_cast<const u32x4*>(smem + byte_off);
}

// Softmax of one target over the 2 x SL list slots of a lane pair (graph_layer.py:106-110 + PyG softmax),
// in the log2 domain (s_i, s_j carry a factor log2 e; LeakyReLU commutes with a positive scale).  Returns
// the weights split into two 16-bit terms, packed in slot pairs (and, WANT_ALPHA, the fp32 weights).
// The elementwise steps (s_i + s_j, 0.2 v, e - m, e inv) run on slot pairs (Pk2); max, exp2 and the ORDER of the max
// and sum reductions are what they were.
template <int SL, int FMT, bool WANT_ALPHA, bool PACK = GDN_TRIM_PACK != 0>
__device__ __forceinline__ void softmax_split(const char* smem, int si_off, const int (&sjoff)[SL],
                                              unsigned (&ph)[SL / 2], unsigned (&pl)[SL / 2], float (&alpha)[SL]) {
  using F = Fmt<FMT>;
  using P = Pk2<PACK>;
  const float sti = lds_f32(smem, si_off);
  float e[SL];
#pragma unroll
  for (int q = 0; q < SL; ++q) e[q] = lds_f32(smem, sjoff[q]);    // all gathers in flight together
  __builtin_amdgcn_sched_barrier(0);
  float m = -3.0e38f;   // keeps pad targets (all slots = sentinel) finite
#pragma unroll
  for (int q = 0; q < SL; q += 2) {
    const f32x2 v = P::add(f32x2{e[q], e[q + 1]}, sti);
    const f32x2 vs = P::mul(v, GDN_NEG_SLOPE);                    // leaky(v) = max(v, 0.2 v)
    e[q] = fmaxf(v[0], vs[0]);
    e[q + 1] = fmaxf(v[1], vs[1]);
    m = fmaxf(m, e[q]);
    m = fmaxf(m, e[q + 1]);
  }
  m = fmaxf(m, dpp_f<GDN_DPP_XOR1>(m));
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < SL; q += 2) {
    const f32x2 v = P::sub(f32x2{e[q], e[q + 1]}, m);
    e[q] = __builtin_amdgcn_exp2f(v[0]);
    e[q + 1] = __builtin_amdgcn_exp2f(v[1]);
    sum += e[q];
    sum += e[q + 1];
  }
  sum += dpp_f<GDN_DPP_XOR1>(sum);
  constexpr float ASC = FMT == FMT_F16 ? GDN_F16_ALPHA_SCALE : 1.f;   // inv = ASC / (sum + eps)
  const float inv = __builtin_amdgcn_rcpf(fmaf(sum, 1.f / ASC, GDN_SOFTMAX_EPS / ASC));
#pragma unroll
  for (int q = 0; q < SL; q += 2) {
    float a0, a1;
    if constexpr (PACK) {
      const f32x2 a = P::mul(f32x2{e[q], e[q + 1]}, inv);
      a0 = a[0];
      a1 = a[1];
      F::split2(a0, a1, ph[q / 2], pl[q / 2]);   // (pins a0, a1 where they stand: the products, materialised)
    } else {
      // long lists and bf16 storage: this step WORD FOR WORD as before [r18] (DCfg::PACK).  With bf16 terms the
      // residual a - float(hi) of the un-pinned scalar product is contracted into fma(e, inv, -hi), the residual of
      // the EXACT product; any other spelling (a product materialised first, a packed product) changes the last
      // bit of some lo terms and with it the bits of the bf16-storage forward
      a0 = e[q] * inv;
      a1 = e[q + 1] * inv;
      ph[q / 2] = F::pk(a0, a1);
      pl[q / 2] = F::pk(F::res0(ph[q / 2], a0), F::res1(ph[q / 2], a1));
    }
    if constexpr (WANT_ALPHA) {
      alpha[q] = a0 * (1.f / ASC);
      alpha[q + 1] = a1 * (1.f / ASC);
    }
  }
}

template <int SL>
__device__ __forceinline__ void scatter_terms(char* smem, const int (&scoff)[SL], const unsigned (&p)[SL / 2]) {
#pragma unroll
  for (int q = 0; q < SL; q += 2) {
    *reinterpret_cast<uint16_t*>(smem + scoff[q]) = (uint16_t)p[q / 2];
    *reinterpret_cast<uint16_t*>(smem + scoff[q + 1]) = (uint16_t)(p[q / 2] >> 16);
  }
}

// One step of the halving butterfly of the attention scalars (fused kernel, X): a lane carries 2M partial sums, keeps
// M of them (the upper half where `upper`), hands the other M to its partner (DPP pattern CTRL, whose `upper` is the
// opposite) and adds what the partner hands over: M sums over twice as many lanes.
template <int M, int CTRL, int N>
__device__ __forceinline__ void halve_sources(float (&r)[N], bool upper) {
  static_assert(2 * M <= N, "");
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const float keep = upper ? r[i + M] : r[i], give = upper ? r[i] : r[i + M];
    r[i] = keep + dpp_f<CTRL>(give);
  }
}

#ifdef GDN_STAMPS   // diagnostic build only: shader-clock stamps of workgroup 0 / wave 0 (tools/probe_stamps.py)
__device__ unsigned long long g_dense_stamps[64];
#define GDN_STAMP(i)                                                                      \
  if (blockIdx.x == 0 && threadIdx.x == 0) {                                              \
    unsigned long long t_;                                                                \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");       \
    g_dense_stamps[i] = t_;                                                               \
  }
#else
#define GDN_STAMP(i)
#endif

// clamped unconditional global load + select: the prologue's loads all issue back to back
__device__ __forceinline__ float ld_or(const float* p, int idx, bool ok, float other = 0.f) {
  const float v = p[ok ? idx : 0];
  return ok ? v : other;
}

// ---- per-launch constants of the fused kernel -----------------------------------------------------
// Everything a lane keeps in registers for the whole launch (list offsets, weight operand fragments,
// epilogue factors) and the two small LDS tables depend only on the parameters and on the sensor graph,
// not on the windows.  They are computed ONCE per parameter update by gdn_fused_plan_build into a
// "plan" in device memory (lane-major words, so a workgroup's prologue is ~90 coalesced dword loads per
// lane instead of ~1000 VALU instructions and a chain of dependent gathers); gdn_forward_fused without a
// plan computes them in the prologue of every workgroup (same code, DArgs::plan == null).
template <int NT, int DC, int WK, int SL, int FMT>
struct LaneConsts {
  using C = DCfg<NT, DC, WK, SL, FMT>;
  int sjoff[SL], scoff[SL];
  u32x4 bl[DC][WK][C::NTL], bs[WK][C::NTL];            // bs: the scalar tile's B operand (not XAGG)
  // XAGG: the attention scalars are fp32 dot products reduced over the CW lanes that hold a source's columns (see
  // the kernel).  A lane ends with ONE scalar: kind (s_i / s_j) = bit CW/2 of its column, source = row
  // xrow0 + xro(column % (CW/2)).  sk = folded a_kind'[own column], sp = a_kind'[column of the first exchange's
  // partner], sadd = c_kind of that source (-inf at the list sentinel, 0 on pad rows): the values of compute_tables
  float sk, sp, sadd;
  float e2[DC][16];
  float out_b;
  static constexpr int WORDS = 2 * SL + 4 * DC * WK * C::NTL + (C::XAGG ? 3 : 4 * WK * C::NTL) + 16 * DC + 1;
  static constexpr int TABLE_WORDS = 4 * 32 * DC + C::CS_WORDS;     // [ec | cs] as they sit in LDS
  static constexpr size_t LIMIT_WORD = (size_t)TABLE_WORDS + (size_t)WORDS * C::THREADS;   // the x limit (float)
  static constexpr size_t PLAN_BYTES = (LIMIT_WORD + 1) * 4;

  // visits every 32-bit word in a fixed order: f(word index, reference to the word as unsigned)
  template <class Fn>
  __device__ __forceinline__ void each_word(Fn&& f) {
    int i = 0;
#pragma unroll
    for (int q = 0; q < SL; ++q) f(i++, reinterpret_cast<unsigned&>(sjoff[q]));
#pragma unroll
    for (int q = 0; q < SL; ++q) f(i++, reinterpret_cast<unsigned&>(scoff[q]));
#pragma unroll
    for (int cb = 0; cb < DC; ++cb)
#pragma unroll
      for (int wk = 0; wk < WK; ++wk)
#pragma unroll
        for (int t = 0; t < C::NTL; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            unsigned tmp = bl[cb][wk][t][e];
            f(i++, tmp);
            bl[cb][wk][t][e] = tmp;
          }
    if constexpr (C::XAGG) {
      f(i++, reinterpret_cast<unsigned&>(sk));
      f(i++, reinterpret_cast<unsigned&>(sp));
      f(i++, reinterpret_cast<unsigned&>(sadd));
    } else {
#pragma unroll
      for (int wk = 0; wk < WK; ++wk)
#pragma unroll
        for (int t = 0; t < C::NTL; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            unsigned tmp = bs[wk][t][e];
            f(i++, tmp);
            bs[wk][t][e] = tmp;
          }
    }
#pragma unroll
    for (int cb = 0; cb < DC; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) f(i++, reinterpret_cast<unsigned&>(e2[cb][r]));
    f(i++, reinterpret_cast<unsigned&>(out_b));
  }
};

template <int NT, int DC, int WK, int SL, int FMT>
__device__ __forceinline__ void compute_lane_consts(const DArgs& a, LaneConsts<NT, DC, WK, SL, FMT>& k) {
  using C = DCfg<NT, DC, WK, SL, FMT>;
  constexpr bool FOLD = FMT == FMT_F16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int n = a.n, w = a.w, d = 32 * DC;
  // S: this lane's half of one target's neighbour list
  const int ti = 32 * wv + (lane >> 1);
  const int half = lane & 1;
  {
    const uint16_t* row = a.nbr + (size_t)min(ti, n - 1) * a.pitch + half * SL;
#pragma unroll
    for (int q = 0; q < SL; ++q) {
      const int jj = (int)row[q];
      const int j = ti < n ? jj : n;
      k.sjoff[q] = C::OFF_SJ + j * 4;
      k.scoff[q] = C::OFF_A + wv * C::AWAVE + (lane >> 1) * C::AROW + pos_of_source(j) * 2;
    }
  }
  // P: B operand = lin'^T (k on the registers, output column on the lane), split once.  XAGG: the same registers
  // are the A operand of P1, whose k order is the row map of the aggregation accumulator (slot 8h + j = window
  // column 16wk + 8(j>>2) + 4h + (j&3)); C-in is the sh1' row of the table block
#pragma unroll
  for (int cb = 0; cb < DC; ++cb) {
    const int c = cb * 32 + l32;
    const float sc = FOLD ? a.bn1[c] * GDN_F16_X_SCALE : 1.f;
#pragma unroll
    for (int wk = 0; wk < WK; ++wk) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kk = wk * 16 + (C::XAGG ? 8 * (j >> 2) + 4 * h + (j & 3) : 8 * h + j);
        v[j] = ld_or(a.lin_w, c * w + kk, kk < w) * sc;
      }
      split8<FMT, C::NTL>(v, k.bl[cb][wk]);
    }
  }
  if constexpr (C::XAGG) {
    // a_i / a_j are stored zero padded to 64; the first exchange of the reduction pairs column c with c ^ (CW - 1)
    // (WK = 1: row mirror) or c ^ 16 (WK = 2: the other DPP row)
    const int xcol = tid & (C::CW - 1), kind = xcol / (C::CW / 2);
    const int pcol = WK == 1 ? xcol ^ 15 : xcol ^ 16;
    const int row = C::xrow0(tid / C::CW) + C::xro(xcol & (C::CW / 2 - 1));
    k.sk = ld_or(a.node_terms, kind * GDN_A_PITCH + xcol, xcol < w) * GDN_LOG2E;
    k.sp = ld_or(a.node_terms, kind * GDN_A_PITCH + pcol, pcol < w) * GDN_LOG2E;
    k.sadd = ld_or(a.node_terms, 2 * GDN_A_PITCH + kind * n + row, row < n) * GDN_LOG2E;
    if (kind == 1 && row == n) k.sadd = -INFINITY;
  } else {
#pragma unroll
    for (int wk = 0; wk < WK; ++wk) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int kk = wk * 16 + 8 * h + j;   // a_i / a_j are stored zero padded to 64
        v[j] = ld_or(a.node_terms, l32 * GDN_A_PITCH + kk, l32 < 2) * GDN_LOG2E;
      }
      split8<FMT, C::NTL>(v, k.bs[wk]);
    }
  }
  // E: embedding x BatchNorm scale of this lane's target, per (column block, register)
  const int tgt = 32 * wv + l32;
#pragma unroll
  for (int cb = 0; cb < DC; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      k.e2[cb][r] = ld_or(a.emb, tgt * d + c, tgt < n) * a.bn2[c] *
                    (FMT == FMT_F16 ? 1.f / (GDN_F16_Z_SCALE * GDN_F16_X_SCALE) : 1.f);
    }
  k.out_b = a.out_b[0];
}

// the two LDS tables, written to `dst` (LDS or the plan): epilogue column constants
// [sh2 | out_w | sc1 | sh1'] (sc1 is used without the BatchNorm fold; sh1' = bias * sc1 + sh1 is the epilogue's
// shift there, and with the fold (fp32 storage) the C-in of P1, in the scale of its accumulator), then the C-in of the
// scalar tile [c_i | c_j | zeros][ROWS] in the log2 domain (row n, the list sentinel, gets s_j = -inf;
// the lanes of the 30 unused columns read the zero row)
template <int NT, int DC, int FMT>
__device__ __forceinline__ void compute_tables(const DArgs& a, float* dst) {
  constexpr int ROWS = 32 * NT, THREADS = 64 * NT, d = 32 * DC;
  const int tid = threadIdx.x, n = a.n;
  for (int c = tid; c < d; c += THREADS) {
    dst[c] = a.bn2[d + c];
    dst[d + c] = a.out_w[c];
    dst[2 * d + c] = a.bn1[c];
    dst[3 * d + c] = fmaf(a.gnn_bias[c], a.bn1[c], a.bn1[d + c]) *
                     (FMT == FMT_F16 ? GDN_F16_Z_SCALE * GDN_F16_X_SCALE : 1.f);
  }
  if constexpr (FMT == FMT_F16) return;     // (DCfg::XAGG: no scalar tile)
  float* ct = dst + 4 * d;
  for (int t = tid; t < 3 * ROWS; t += THREADS) {
    const int which = t / ROWS, row = t - which * ROWS;
    float v = ld_or(a.node_terms, 2 * GDN_A_PITCH + which * n + row, which < 2 && row < n) * GDN_LOG2E;
    if (which == 1 && row == n) v = -INFINITY;
    ct[t] = v;
  }
}

// Largest |x| the fp32-storage kernel represents (the "x limit" of a plan).  With the aggregation in front of the
// projection (DCfg::XAGG) the 16-bit operand chain of a window is
//   x             two f16 terms, unscaled (scalar tile) and times 2^3 (X^T fragments):   8 |x| < 65504
//   alpha * 2^12  two f16 terms, <= 4096 (1 + 2^-11)                                     whatever x
//   Zx * 2^3      the aggregated row sum_j alpha_ij x_j, two f16 terms: a convex combination of the window's
//                 values up to the rounding of alpha (sum_j alpha_hi <= 1 + 2^-11):      8 |Zx| <= 8 max|x| (1 + 2^-10)
//   lin' * 2^3    two f16 terms, parameters only:                                        8 max|lin'[c, w]| < 65504
// and everything behind them (products, C-in, the projected row) is fp32.  So limit = 60000 / 2^3 = 7500 (60000:
// 9 % of head room for the roundings above), or 0 when a lin' entry (or C-in) is out of range or not finite: every
// launch is then flagged.  The projected tile itself no longer exists in 16 bits, so neither its L1 bound
// max|x| sum_w |lin'[c, w]| nor C-in enter.  bf16 storage: x is one exact bf16 term with fp32's exponent range,
// the tile is rounded to bf16: no limit (+inf).
template <int NT, int DC, int FMT>
__device__ __forceinline__ float compute_xlimit(const DArgs& a) {
  if constexpr (FMT != FMT_F16) return INFINITY;
  __shared__ unsigned m_lin, m_c;
  const int tid = threadIdx.x, d = 32 * DC;
  if (tid == 0) { m_lin = 0u; m_c = 0u; }
  __syncthreads();
  for (int c = tid; c < d; c += 64 * NT) {
    const float sc = a.bn1[c] * GDN_F16_X_SCALE;
    float lmax = 0.f;
    for (int q = 0; q < a.w; ++q) {
      const float v = fabsf(a.lin_w[c * a.w + q] * sc);
      lmax = v > lmax || v != v ? v : lmax;
    }
    const float cin = fabsf(fmaf(a.gnn_bias[c], a.bn1[c], a.bn1[d + c]));
    // non-negative floats order like their bits; NaN / inf parameters compare as huge: limit 0
    atomicMax(&m_lin, __float_as_uint(lmax));
    atomicMax(&m_c, __float_as_uint(cin));
  }
  __syncthreads();
  const float lmax = __uint_as_float(m_lin), cmax = __uint_as_float(m_c);
  if (!(lmax < 60000.f) || !(cmax < 3.0e38f)) return 0.f;
  return 60000.f / GDN_F16_XT_SCALE;
}

// The plan also ORDERS each lane's list slots.  A lane may visit its SL slots in any order (softmax and the
// scatter do not care), and the order decides which LDS banks the 32 lanes of a half-wave hit together in
// step q: the s_j gather (ds_read_b32) and, twice per window, the scatter into the dense alpha image
// (ds_write_b16) — with the lists in rank order those were 30 % of the kernel's LDS cycles
// (SQ_LDS_BANK_CONFLICT, profiles/r02_sq_counters_*).  Greedy, once per plan: step by step, lane by lane,
// take the unused slot whose banks are least loaded so far in this step.
template <int NT, int DC, int WK, int SL, int FMT>
__global__ __launch_bounds__(64 * NT) void gdn_dense_plan_kernel(const DArgs a, unsigned* plan) {
  using K = LaneConsts<NT, DC, WK, SL, FMT>;
  constexpr int T = 64 * NT;
  __shared__ int s_sj[T][SL], s_sc[T][SL];
  __shared__ unsigned char s_perm[T][SL];
  K k;
  compute_lane_consts(a, k);
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < SL; ++q) {
    s_sj[tid][q] = k.sjoff[q];
    s_sc[tid][q] = k.scoff[q];
  }
  __syncthreads();
  if ((tid & 31) == 0) {
    unsigned used[32];
    for (int l = 0; l < 32; ++l) used[l] = 0;
    for (int step = 0; step < SL; ++step) {
      unsigned char cw[32], cr[32];
      for (int i = 0; i < 32; ++i) cw[i] = cr[i] = 0;
      for (int l = 0; l < 32; ++l) {
        int best = -1, best_cost = 1 << 30;
        for (int q = 0; q < SL; ++q) {
          if (used[l] >> q & 1u) continue;
          const int bw = (s_sc[tid + l][q] >> 2) & 31, br = (s_sj[tid + l][q] >> 2) & 31;
          // a second writer on a bank is free (2-way ds_write), a third costs; the scatter runs twice per window
          const int cost = 2 * (cw[bw] >= 1 ? 1 + 4 * (cw[bw] - 1) : 0) + (cr[br] >= 1 ? 1 + 4 * (cr[br] - 1) : 0);
          if (cost < best_cost) { best_cost = cost; best = q; }
        }
        used[l] |= 1u << best;
        s_perm[tid + l][step] = (unsigned char)best;
        ++cw[(s_sc[tid + l][best] >> 2) & 31];
        ++cr[(s_sj[tid + l][best] >> 2) & 31];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < SL; ++q) {
    k.sjoff[q] = s_sj[tid][s_perm[tid][q]];
    k.scoff[q] = s_sc[tid][s_perm[tid][q]];
  }
  compute_tables<NT, DC, FMT>(a, reinterpret_cast<float*>(plan));
  unsigned* lanes = plan + K::TABLE_WORDS;
  k.each_word([&](int i, unsigned& wd) { lanes[i * T + threadIdx.x] = wd; });
  const float xlim = compute_xlimit<NT, DC, FMT>(a);
  if (threadIdx.x == 0) plan[K::LIMIT_WORD] = __float_as_uint(xlim);
}

#ifndef GDN_DENSE_EXTRA_DC
// The same greedy as gdn_dense_plan_kernel, but producing a reordered COPY OF THE LISTS: row i of `out` holds the
// entries of row i of `nbr`, permuted inside each half (slots [0, SL) and [SL, 2 SL): the two lanes that share a
// target) so that step q of the 32 lanes of a half-wave spreads over the LDS banks in the s_j gather and in the
// two scatters.  The staged kernels (gdn_dense_attn_kernel, gdn_dense_project has no lists) read their lists from
// whatever table they are given, and softmax / aggregation do not depend on the order of a target's slots, so a
// caller that does not need alpha in rank order hands them this table (the fused kernel gets the same order from
// its plan).  The bank of a slot depends on NT only: OFF_SJ is a multiple of 128 bytes in both kernels' LDS plans,
// an image row starts (lane >> 1) * (16 NT + 4) dwords into a wave's block and a wave's block is a multiple of
// 128 bytes.  One workgroup of 64 NT threads.
template <int NT, int SL>
__global__ __launch_bounds__(64 * NT) void gdn_bank_order_kernel(const uint16_t* __restrict__ nbr, int n, int pitch,
                                                                 uint16_t* __restrict__ out) {
  constexpr int T = 64 * NT;
  __shared__ unsigned short s_j[T][SL];
  __shared__ unsigned char s_perm[T][SL];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ti = 32 * wv + (lane >> 1), half = lane & 1;
  const uint16_t* row = nbr + (size_t)min(ti, n - 1) * pitch + half * SL;
#pragma unroll
  for (int q = 0; q < SL; ++q) s_j[tid][q] = ti < n ? row[q] : (unsigned short)n;
  __syncthreads();
  if ((tid & 31) == 0) {
    unsigned used[32];
    for (int l = 0; l < 32; ++l) used[l] = 0;
    for (int step = 0; step < SL; ++step) {
      unsigned char cw[32], cr[32];
      for (int i = 0; i < 32; ++i) cw[i] = cr[i] = 0;
      for (int l = 0; l < 32; ++l) {
        const int rowdw = (((tid + l) & 63) >> 1) * (16 * NT + 4);
        int best = -1, best_cost = 1 << 30;
        for (int q = 0; q < SL; ++q) {
          if (used[l] >> q & 1u) continue;
          const int j = s_j[tid + l][q];
          const int bw = (rowdw + (pos_of_source(j) >> 1)) & 31, br = j & 31;
          const int cost = 2 * (cw[bw] >= 1 ? 1 + 4 * (cw[bw] - 1) : 0) + (cr[br] >= 1 ? 1 + 4 * (cr[br] - 1) : 0);
          if (cost < best_cost) { best_cost = cost; best = q; }
        }
        used[l] |= 1u << best;
        s_perm[tid + l][step] = (unsigned char)best;
        const int jb = s_j[tid + l][best];
        ++cw[(rowdw + (pos_of_source(jb) >> 1)) & 31];
        ++cr[jb & 31];
      }
    }
  }
  __syncthreads();
  if (ti < n) {
    uint16_t* dst = out + (size_t)ti * pitch + half * SL;
#pragma unroll
    for (int q = 0; q < SL; ++q) dst[q] = s_j[tid][s_perm[tid][q]];
  }
}
#endif

#ifdef GDN_DENSE_EXTRA_DC   // d = 128: one workgroup per CU and the whole 512-register file per wave (the default
#define GDN_FUSED_ATTR __attribute__((amdgpu_waves_per_eu(1, 1)))   // heuristic keeps 2 waves/SIMD where LDS allows, and spills)
#else
#define GDN_FUSED_ATTR
#endif
// Wave priorities per phase (s_setprio): the two workgroups of a CU share every SIMD, and with equal priorities a
// wave in its matrix-core phases (P: projection, M: aggregation product) waits for issue slots behind the other
// workgroup's VALU-heavy phases (S: softmax, E: head).  Same-box A/B over 13 settings (tools/_diag/build_variant.sh,
// tools/probe_fused_time.py), us per 32768 windows fp32 / bf16 storage: none 289.3 / 233.8; P3 S0 M3 E0 279.0 /
// 216.9; every setting with M highest, P and E in between and S lowest 269-272 / 214-217 (P2 S0 M3 E1 kept):
// -6.6 % / -8 %.  Same arithmetic, same bits.
#ifndef GDN_K8_PRIO_T       // the staged gather-aggregate: tile staging, softmax, product, z stores
#define GDN_K8_PRIO_T 2
#define GDN_K8_PRIO_S 0
#define GDN_K8_PRIO_M 3
#define GDN_K8_PRIO_Z 1
#endif
#ifndef GDN_PRIO_P
#define GDN_PRIO_P 2
#define GDN_PRIO_S 0
#define GDN_PRIO_M 3
#define GDN_PRIO_E 1
#endif
#ifndef GDN_PRIO_P1         // the projection behind the aggregation (fp32 storage): matrix-core work, like M
#define GDN_PRIO_P1 3
#endif
template <int NT, int DC, int WK, int SL, int FMT>
// DCfg::WGS workgroups per CU
__global__ __launch_bounds__(64 * NT, (DCfg<NT, DC, WK, SL, FMT>::WGS)) GDN_FUSED_ATTR void gdn_dense_fused_kernel(const DArgs a) {
  using C = DCfg<NT, DC, WK, SL, FMT>;
  using F = Fmt<FMT>;
  using P = Pk2<C::PACK>;
  extern __shared__ uint4 smem_u4[];
  char* smem = reinterpret_cast<char*>(smem_u4);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int n = a.n, w = a.w, d = 32 * DC;
  constexpr bool FOLD = FMT == FMT_F16;   // bf16 storage rounds xlin itself, so BatchNorm stays in the epilogue
  GDN_STAMP(0)

  // ---------------------------------------------------------------- once per workgroup
  for (int t = lane; t < C::AWAVE / 16; t += 64)
    reinterpret_cast<uint4*>(smem + C::OFF_A + wv * C::AWAVE)[t] = make_uint4(0, 0, 0, 0);
  {   // pad columns CW .. XP-1 of the x tile are never read; columns w .. CW-1 and rows >= n are stored as 0
  }
  // (XAGG: every window rewrites the whole X^T fragment area, pad rows and columns as 0)
  // per-launch constants: from the plan, or computed here (gdn_forward_fused without a plan)
  LaneConsts<NT, DC, WK, SL, FMT> k;
  float xlim = INFINITY;                       // range guard (fp32 storage): see compute_xlimit
  if (a.plan) {
    const unsigned* lanes = a.plan + LaneConsts<NT, DC, WK, SL, FMT>::TABLE_WORDS;
    k.each_word([&](int i, unsigned& wd) { wd = lanes[i * C::THREADS + tid]; });
    unsigned* tab = reinterpret_cast<unsigned*>(smem + C::OFF_EC);
    for (int t = tid; t < LaneConsts<NT, DC, WK, SL, FMT>::TABLE_WORDS; t += C::THREADS) tab[t] = a.plan[t];
    if constexpr (FMT == FMT_F16)
      if (a.range_flag) xlim = __uint_as_float(a.plan[LaneConsts<NT, DC, WK, SL, FMT>::LIMIT_WORD]);
  } else {
    compute_lane_consts(a, k);     // (no plan, no x limit: the range guard is a feature of planned launches)
    compute_tables<NT, DC, FMT>(a, reinterpret_cast<float*>(smem + C::OFF_EC));
  }
  if constexpr (C::BLDS) {   // lin' to LDS (wave 0: the operand does not depend on the wave); visible after the barrier below
    if (wv == 0) {
#pragma unroll
      for (int cb = 0; cb < DC; ++cb)
#pragma unroll
        for (int wk = 0; wk < WK; ++wk)
#pragma unroll
          for (int t = 0; t < C::NTL; ++t)
            *reinterpret_cast<u32x4*>(smem + C::OFF_BL + (((cb * WK + wk) * C::NTL + t) << 10) + lane * 16) = k.bl[cb][wk][t];
    }
  }
  // out-of-range lanes, as a wave-uniform mask in scalar registers (the bf16-storage and long-window variants sit
  // AT their 256-VGPR budget: a per-lane flag cost 20 more spilled registers and 9 % of the launch)
  unsigned long long out_of_range = 0ull;
  const int si_off = C::OFF_SI + (32 * wv + (lane >> 1)) * 4;
  const int cs_off = C::OFF_CS + (min(l32, 2) * C::ROWS + 32 * wv + 4 * h) * 4;   // + 32 (r >> 2): 4 rows (not XAGG)
  const int tgt = 32 * wv + l32;

  // x staging: a thread owns column (tid % CW) of rows row0 + xro(0), row0 + xro(1), ...; global offsets are one
  // VGPR plus a scalar step per row (buffer loads: reads past the end of the input return 0), LDS
  // offsets one VGPR plus an immediate.  Pad rows / columns are stored as 0 every window.
  //   row0 = tid / CW, xro(u) = u RS: the rows of a thread are RS apart; or,
  //   XAGG: the thread's values 8q .. 8q+7 are one operand slot of X^T (k-step s, lane half hh) in the k order of
  //   pos_of_source: slot 2s + hh = tid / CW + q RS, row0 = 16 s + 4 hh, xro(8q + j) = 16 NT q + 8 (j >> 2) + (j & 3).
  constexpr int CW = C::CW, RS = C::RS;
  static_assert(C::XU * RS == C::ROWS, "x staging covers the tile");
  static_assert(!C::XAGG || RS * WK == 2 * C::KS, "one operand slot per thread and pass");
  constexpr int ESZ = FMT == FMT_F16 ? 4 : 2;
  const int xcol = tid & (CW - 1), xsl = tid / CW;
  const int xrow0 = C::xrow0(xsl);
  auto xro = [](int u) constexpr { return C::xro(u); };
  const int rstride = a.series_len > 0 ? a.series_len : w;
  const int xvoff = (min(xrow0, n - 1) * rstride + min(xcol, w - 1)) * ESZ;
  const int xstep = rstride * ESZ;
  const int xst_off = C::OFF_XS + (xrow0 * C::XP + xcol) * 4;                      // x tile (not XAGG)
  const int xf_st = C::OFF_XF + (xsl >> 1) * C::NPX * C::XFRAG + ((xsl & 1) * C::XFL + xcol) * 16;   // XAGG: + (q NT NPX + t) XFRAG
  // XAGG: where this lane's attention scalar goes (LaneConsts::sk): s_i / s_j of one source
  const int xs_dst = (xcol / (CW / 2) ? C::OFF_SJ : C::OFF_SI) + (xrow0 + C::xro(xcol & (CW / 2 - 1))) * 4;
  bool xok[C::XU];
#pragma unroll
  for (int u = 0; u < C::XU; ++u) xok[u] = xcol < w && xrow0 + xro(u) < n;
  const size_t win_stride = a.series_len > 0 ? 1 : (size_t)n * w;
  const size_t x0 = a.series_len > 0 ? (size_t)a.series_first : 0;
  const size_t x_total = (a.series_len > 0 ? (size_t)n * a.series_len : (size_t)a.batch * n * w) * ESZ;
  float xr[C::XU];
  auto load_window = [&](int bb) {
    const size_t first = (x0 + (size_t)bb * win_stride) * ESZ;          // wave uniform
    const size_t rem = x_total - first;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(a.x)) + first, 0,
        (int)(rem > 0xffffffffull ? 0xffffffffu : (unsigned)rem), 0x00020000);
#pragma unroll
    for (int u = 0; u < C::XU; ++u) {
      if constexpr (FMT == FMT_F16) {
        xr[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, xvoff, xro(u) * xstep, 0));
      } else {
        xr[u] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsrc, xvoff, xro(u) * xstep, 0) << 16);
      }
    }
  };
  GDN_STAMP(1)
  load_window(blockIdx.x);
  __syncthreads();   // zero fills done
  GDN_STAMP(2)

  const int arow_off = C::OFF_A + wv * C::AWAVE + l32 * C::AROW + h * 16;   // alpha operand of this lane
  const int xrow_off = C::OFF_XS + ((32 * wv + l32) * C::XP + 8 * h) * 4;  // x operand of this lane (not XAGG)
  const int ec_off = C::OFF_EC + 16 * h;                                   // + 32 (r >> 2) + 128 cb: 4 columns
  // XHALF: the X^T operand of this lane in M, + k-step: product rows l32 < 16 take the hi term of window column l32,
  // rows l32 >= 16 (which no window column has) the lo term of column l32 - 16, one term (XFRAG bytes) further on
  const int xf_half = C::OFF_XF + (h * 16 + (l32 & 15)) * 16 + (l32 >> 4) * C::XFRAG;

  for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
    if constexpr (C::XAGG) {
      // ---------------------------------------------------------- X  (fp32 storage: no x tile, no P0)
      __builtin_amdgcn_s_setprio(GDN_PRIO_P);
      if (b == (int)blockIdx.x) { GDN_STAMP(3) }
      __syncthreads();     // B1: every wave is past S and M of window b - 1, the last readers of s_i / s_j and of
                           // the fragment area (the alpha image is wave private)
      float xv[C::XU];
#pragma unroll
      for (int u = 0; u < C::XU; ++u) {
        xv[u] = xok[u] ? xr[u] : 0.f;
#ifndef GDN_NO_GUARD
        out_of_range |= __builtin_amdgcn_ballot_w64(!(fabsf(xv[u]) < xlim));   // (NaN too)
#endif
      }
      // X^T operand fragments of window b
#pragma unroll
      for (int q = 0; q < WK; ++q) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          const f32x2 t = P::mul(f32x2{xv[8 * q + j], xv[8 * q + j + 1]}, GDN_F16_XT_SCALE);
          v[j] = t[0];
          v[j + 1] = t[1];
        }
        u32x4 xf[C::NPX];
        split8<FMT, C::NPX>(v, xf);
#pragma unroll
        for (int t = 0; t < C::NPX; ++t)
          *reinterpret_cast<u32x4*>(smem + xf_st + (q * NT * C::NPX + t) * C::XFRAG) = xf[t];
      }
      // Attention scalars s_i / s_j of every source (graph_layer.py:94-104), log2 domain: fp32 dot products of
      // length w over the CW lanes that hold a source's columns, all 2 XU of a thread reduced together by a halving
      // butterfly: the first exchange decides the kind (lanes with bit CW/2 of the column clear keep s_i, the others
      // s_j, so the coefficient of either side is a per-lane constant: no select), every later one halves the
      // sources a lane carries (keep one half, hand the other to the partner), until lane c holds the whole sum of
      // one (kind, source): 2 XU - 1 exchanges instead of 2 XU x log2(CW).
      float sr[C::XU];
#pragma unroll
      for (int u = 0; u < C::XU; u += 2) {
        const f32x2 other = {WK == 1 ? dpp_f<GDN_DPP_MIRROR>(xv[u]) : __shfl_xor(xv[u], 16),
                             WK == 1 ? dpp_f<GDN_DPP_MIRROR>(xv[u + 1]) : __shfl_xor(xv[u + 1], 16)};
        const f32x2 s = P::fma(other, f32x2{k.sp, k.sp}, P::mul(f32x2{xv[u], xv[u + 1]}, k.sk));
        sr[u] = s[0];
        sr[u + 1] = s[1];
      }
      if constexpr (WK == 2) halve_sources<8, GDN_DPP_MIRROR>(sr, (xcol & 8) != 0);
      halve_sources<4, GDN_DPP_HALF_MIRROR>(sr, (xcol & 4) != 0);
      halve_sources<2, GDN_DPP_XOR3>(sr, (xcol & 2) != 0);
      halve_sources<1, GDN_DPP_XOR1>(sr, (xcol & 1) != 0);
      *reinterpret_cast<float*>(smem + xs_dst) = sr[0] + k.sadd;
      load_window(min(b + (int)gridDim.x, a.batch - 1));         // lands under the math (last round: re-read)
      if (b == (int)blockIdx.x) { GDN_STAMP(4) }
    } else {
      // ---------------------------------------------------------- bf16 storage: x tile, then P
#pragma unroll
      for (int u = 0; u < C::XU; ++u) {
        const float xv = xok[u] ? xr[u] : 0.f;
        *reinterpret_cast<float*>(smem + xst_off + xro(u) * (C::XP * 4)) = xv;
      }
      if (b == (int)blockIdx.x) { GDN_STAMP(3) }
      __syncthreads();                                           // B1: x tile of window b visible
      load_window(min(b + (int)gridDim.x, a.batch - 1));         // lands under the math (last round: re-read)
      if (b == (int)blockIdx.x) { GDN_STAMP(4) }

      // ------------------------------------------------------------ P
      {
        __builtin_amdgcn_s_setprio(GDN_PRIO_P);
        f32x16 acc1[DC], accs;
#pragma unroll
        for (int cb = 0; cb < DC; ++cb)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc1[cb][r] = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 t = *reinterpret_cast<const float4*>(smem + cs_off + 32 * g);
          accs[4 * g] = t.x; accs[4 * g + 1] = t.y; accs[4 * g + 2] = t.z; accs[4 * g + 3] = t.w;
        }
#pragma unroll
        for (int wk = 0; wk < WK; ++wk) {
          float v[8];
          const float4 v0 = *reinterpret_cast<const float4*>(smem + xrow_off + wk * 64);
          const float4 v1 = *reinterpret_cast<const float4*>(smem + xrow_off + wk * 64 + 16);
          v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w;
          v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
          u32x4 ax[C::NTXIN];
          split8<FMT, C::NTXIN>(v, ax);
#pragma unroll
          for (int tx = 0; tx < C::NTXIN; ++tx)
#pragma unroll
            for (int tl = 0; tl < C::NTL; ++tl)
              if (tx + tl < (C::NTXIN > C::NTL ? C::NTXIN : C::NTL)) {
#pragma unroll
                for (int cb = 0; cb < DC; ++cb) acc1[cb] = F::mfma(ax[tx], k.bl[cb][wk][tl], acc1[cb]);
                accs = F::mfma(ax[tx], k.bs[wk][tl], accs);
              }
        }
        // attention scalars: columns 0 / 1 of the scalar tile
        if (l32 < 2) {
          float* sdst = reinterpret_cast<float*>(smem + (l32 == 0 ? C::OFF_SI : C::OFF_SJ)) + 32 * wv + 4 * h;
#pragma unroll
          for (int r = 0; r < 16; ++r) sdst[(r & 3) + 8 * (r >> 2)] = accs[r];
        }
        // the projected tile as operand fragments of the aggregation product: k-steps 2wv, 2wv+1
#pragma unroll
        for (int cb = 0; cb < DC; ++cb)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = acc1[cb][8 * s + j];
            u32x4 xf[C::NPX];
            split8<FMT, C::NPX>(v, xf);
#pragma unroll
            for (int t = 0; t < C::NPX; ++t)
              *reinterpret_cast<u32x4*>(smem + C::OFF_XF + ((((2 * wv + s) * DC + cb) * C::NPX + t) << 10) + lane * 16) = xf[t];
          }
      }
    }   // bf16 storage (not XAGG)
    __builtin_amdgcn_s_setprio(GDN_PRIO_S);
    if (b == (int)blockIdx.x) { GDN_STAMP(5) }
    __syncthreads();                                           // B2: operand fragments + scalars visible
    if (b == (int)blockIdx.x) { GDN_STAMP(6) }

    // ------------------------------------------------------------ S
    // log2 domain: a_i, a_j, c_i, c_j carry a factor log2(e) (LeakyReLU commutes with a positive
    // scale), so the weights are exp2(e - m) and v_exp_f32 needs no multiply in front of it
    unsigned ph[SL / 2], pl[SL / 2];
    {
      float unused[SL];
      softmax_split<SL, FMT, false, C::PACK>(smem, si_off, k.sjoff, ph, pl, unused);
    }
    // ------------------------------------------------------------ M
    // The image is wave private and LDS executes one wave's accesses in order: scatter the hi term,
    // read it as operands, scatter the lo term over the same positions, read again — no barrier.
    // Operand reads run one k-step ahead of the products (two named fragment sets).
    float ygt = 0.f;                                  // issued here, consumed after the products
    // [r27] XKEEP: the three per-lane global addresses of a target (ground truth, out, keys) are rebuilt per window
    // from its index, which an EMPTY asm hides from the loop-invariant hoisting, instead of living in three register
    // pairs across the whole loop, and ygt waits as the float it was loaded as (its float64 form was computed ahead
    // of M): five registers for the kept fragments.  Same values, same stores.
    unsigned tg = (unsigned)tgt;
    if constexpr (C::XKEEP > 0) {
      asm("" : "+v"(tg));
      if (a.keys && h == 0 && tgt < n) ygt = (a.key_gt + (size_t)b * n)[tg];
    } else {
      if (a.keys && h == 0 && tgt < n) ygt = a.key_gt[(size_t)b * n + tgt];
    }
    constexpr int MCB = C::MCB;                         // XAGG: one block, Zx^T[w, target]
    f32x16 acc2[MCB];
#pragma unroll
    for (int cb = 0; cb < MCB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[cb][r] = 0.f;
    constexpr int XF_KS = MCB * C::NPX * C::XFRAG;      // bytes of fragments per k-step
    if (b == (int)blockIdx.x) { GDN_STAMP(7) }
    __builtin_amdgcn_s_setprio(GDN_PRIO_M);      // see the note at the kernel's head
    if constexpr (C::XHALF) {
      // ONE X fragment per lane and k-step for both passes (xf_half): rows 0 .. 15 of the product multiply the hi
      // term of X^T, rows 16 .. 31 its lo term.  Summation order per (w, target), fp32:
      //   registers 0 .. 7   (rows r):       sum_ks Xhi.ahi, then + sum_ks Xhi.alo   (16 products, one chain)
      //   registers 8 .. 15  (rows 16 + r):  sum_ks Xlo.ahi, then + sum_ks Xlo.alo   (16 products, one chain)
      // and P1 adds register 8 + j to register j once.  The lo pass keeps the SAME addressing rather than the
      // neighbour's hi fragment (which would put a second Xhi.alo into the rows that are folded) or a fold between
      // the passes (VALU work inside the accumulator chain): no register, no instruction, and Xlo.alo is the fourth
      // term of (Xhi + Xlo)(ahi + alo), 2^-22 of the product, which the three-product form left out.
      // [r27] the fragment of k-step ks < XKEEP is read in the first pass only and stays in fk[ks] for the second
      // (the scatter between the passes writes the alpha image, never the fragment area)
      u32x4 fa[2], fx[2], fk[C::XKEEP > 0 ? C::XKEEP : 1];
      auto fetch = [&](int ks, int buf, int pass) {
        fa[buf] = lds_frag(smem, arow_off + ks * 32);
        if (ks >= C::XKEEP) fx[buf] = lds_frag(smem, xf_half + ks * XF_KS);
        else if (pass == 0) fk[ks] = lds_frag(smem, xf_half + ks * XF_KS);
      };
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        scatter_terms<SL>(smem, k.scoff, pass == 0 ? ph : pl);
        __builtin_amdgcn_sched_barrier(0);
        fetch(0, 0, pass);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < C::KS; ++ks) {
          if (ks + 1 < C::KS) fetch(ks + 1, (ks + 1) & 1, pass);
          __builtin_amdgcn_sched_barrier(0);
          acc2[0] = F::mfma(ks < C::XKEEP ? fk[ks < C::XKEEP ? ks : 0] : fx[ks & 1], fa[ks & 1], acc2[0]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    } else {
    const int xf_lane = C::OFF_XF + lane * 16;
    u32x4 fa[2], fx[2][MCB][C::NPX];
    auto fetch_hi = [&](int ks, int buf) {
      fa[buf] = lds_frag(smem, arow_off + ks * 32);
#pragma unroll
      for (int cb = 0; cb < MCB; ++cb)
#pragma unroll
        for (int t = 0; t < C::NPX; ++t) fx[buf][cb][t] = lds_frag(smem, xf_lane + ks * XF_KS + (cb * C::NPX + t) * C::XFRAG);
    };
    auto fetch_lo = [&](int ks, int buf) {
      fa[buf] = lds_frag(smem, arow_off + ks * 32);
#pragma unroll
      for (int cb = 0; cb < MCB; ++cb) fx[buf][cb][0] = lds_frag(smem, xf_lane + ks * XF_KS + cb * C::NPX * C::XFRAG);
    };
    scatter_terms<SL>(smem, k.scoff, ph);
    __builtin_amdgcn_sched_barrier(0);
    fetch_hi(0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      if (ks + 1 < C::KS) fetch_hi(ks + 1, (ks + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < MCB; ++cb)
#pragma unroll
        for (int t = 0; t < C::NPX; ++t) acc2[cb] = F::mfma(fx[ks & 1][cb][t], fa[ks & 1], acc2[cb]);
      __builtin_amdgcn_sched_barrier(0);
    }
    scatter_terms<SL>(smem, k.scoff, pl);
    __builtin_amdgcn_sched_barrier(0);
    fetch_lo(0, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      if (ks + 1 < C::KS) fetch_lo(ks + 1, (ks + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < MCB; ++cb) acc2[cb] = F::mfma(fx[ks & 1][cb][0], fa[ks & 1], acc2[cb]);
      __builtin_amdgcn_sched_barrier(0);
    }
    }   // not XHALF
    if (b == (int)blockIdx.x) { GDN_STAMP(8) }
    // ------------------------------------------------------------ P1 (XAGG)
    // out^T[c, target] = lin' . Zx + C.  Registers 8wk .. 8wk+7 of the aggregation accumulator (target on the lane)
    // are k slots 8h .. 8h+7 of the B operand as they stand (window column 16wk + 8(j>>2) + 4h + (j&3): the order
    // k.bl was built in); they carry 2^12 (alpha) x 2^3 (x) and go back to 2^3, an exact power of two, before the
    // split.  C-in is the accumulator's initial value: the sh1' row of the table block, column on the registers.
    f32x16 acc3[DC];
    if constexpr (C::XAGG) {
      __builtin_amdgcn_s_setprio(GDN_PRIO_P1);
      // BLDS: lin' from LDS (contiguous ds_read_b128, conflict free), under the tail of M's accumulator chain
      u32x4 blr[C::BLDS ? DC : 1][WK][C::NTL];
      if constexpr (C::BLDS) {
#pragma unroll
        for (int cb = 0; cb < DC; ++cb)
#pragma unroll
          for (int wk = 0; wk < WK; ++wk)
#pragma unroll
            for (int t = 0; t < C::NTL; ++t)
              blr[cb][wk][t] = lds_frag(smem, C::OFF_BL + (((cb * WK + wk) * C::NTL + t) << 10) + lane * 16);
      }
      auto lin = [&](int cb, int wk, int t) -> const u32x4& {
        if constexpr (C::BLDS) return blr[cb][wk][t];
        else return k.bl[cb][wk][t];
      };
#pragma unroll
      for (int cb = 0; cb < DC; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 t = *reinterpret_cast<const float4*>(smem + ec_off + 12 * d + 128 * cb + 32 * g);
          acc3[cb][4 * g] = t.x; acc3[cb][4 * g + 1] = t.y; acc3[cb][4 * g + 2] = t.z; acc3[cb][4 * g + 3] = t.w;
        }
#pragma unroll
      for (int wk = 0; wk < WK; ++wk) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          // XHALF: row 16 + r of the accumulator is register 8 + j of the same lane: the lo term of X^T (see M)
          f32x2 z = {acc2[0][8 * wk + j], acc2[0][8 * wk + j + 1]};
          if constexpr (C::XHALF) z = P::add(f32x2{acc2[0][j], acc2[0][j + 1]}, f32x2{acc2[0][8 + j], acc2[0][9 + j]});
          z = P::mul(z, GDN_F16_Z_SCALE / (GDN_F16_ALPHA_SCALE * GDN_F16_XT_SCALE));
          v[j] = z[0];
          v[j + 1] = z[1];
        }
        u32x4 zf[2];
        split8<FMT, 2>(v, zf);
#pragma unroll
        for (int tz = 0; tz < 2; ++tz)
#pragma unroll
          for (int tl = 0; tl < C::NTL; ++tl)
            if (tz + tl < 2) {
#pragma unroll
              for (int cb = 0; cb < DC; ++cb) acc3[cb] = F::mfma(lin(cb, wk, tl), zf[tz], acc3[cb]);
            }
      }
    } else {
#pragma unroll
      for (int cb = 0; cb < DC; ++cb) acc3[cb] = acc2[cb < MCB ? cb : 0];
    }

    __builtin_amdgcn_s_setprio(GDN_PRIO_E);
    if (b == (int)blockIdx.x) { GDN_STAMP(9) }
    // ------------------------------------------------------------ E  (models/GDN.py:77-79,175-184)
    float part = 0.f;
#pragma unroll
    for (int cb = 0; cb < DC; ++cb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 sh2 = *reinterpret_cast<const float4*>(smem + ec_off + 128 * cb + 32 * g);
        const float4 wo = *reinterpret_cast<const float4*>(smem + ec_off + 4 * d + 128 * cb + 32 * g);
        const float sh2a[4] = {sh2.x, sh2.y, sh2.z, sh2.w}, woa[4] = {wo.x, wo.y, wo.z, wo.w};
        float sc1a[4] = {1.f, 1.f, 1.f, 1.f}, sh1a[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (!FOLD) {
          const float4 t0 = *reinterpret_cast<const float4*>(smem + ec_off + 8 * d + 128 * cb + 32 * g);
          const float4 t1 = *reinterpret_cast<const float4*>(smem + ec_off + 12 * d + 128 * cb + 32 * g);
          sc1a[0] = t0.x; sc1a[1] = t0.y; sc1a[2] = t0.z; sc1a[3] = t0.w;
          sh1a[0] = t1.x; sh1a[1] = t1.y; sh1a[2] = t1.z; sh1a[3] = t1.w;
        }
#pragma unroll
        for (int i = 0; i < 4; i += 2) {
          const int r = 4 * g + i;
          f32x2 v = {acc3[cb][r], acc3[cb][r + 1]};
          // first ReLU.  FOLD: straight on the P1 accumulator, one instruction (relu_acc: a NaN stays NaN); bf16
          // storage has no range guard and its ReLU follows an fma (one v_max_f32 already): fmaxf as before
          if constexpr (FOLD) {
            v = f32x2{relu_acc(v[0]), relu_acc(v[1])};
          } else {
            v = P::fma(v, f32x2{sc1a[i], sc1a[i + 1]}, f32x2{sh1a[i], sh1a[i + 1]});
            v = f32x2{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f)};
          }
          v = P::fma(v, f32x2{k.e2[cb][r], k.e2[cb][r + 1]}, f32x2{sh2a[i], sh2a[i + 1]});
          part = fmaf(fmaxf(v[0], 0.f), woa[i], part);            // (`part`: one chain, in column order)
          part = fmaf(fmaxf(v[1], 0.f), woa[i + 1], part);
        }
      }
    part += __shfl_xor(part, 32);
    if (h == 0 && tgt < n) {
      const float o = part + k.out_b;
      if constexpr (C::XKEEP > 0) {
        asm("" : "+v"(ygt));
        (a.out + (size_t)b * n)[tg] = o;
        if (a.keys) (a.keys + b)[(size_t)tg * (unsigned)a.key_pitch] = fabs((double)o - (double)ygt);
      } else {
        a.out[(size_t)b * n + tgt] = o;
        if (a.keys) a.keys[(size_t)tgt * a.key_pitch + b] = fabs((double)o - (double)ygt);
      }
    }
    if (b == (int)blockIdx.x) { GDN_STAMP(10) }
  }
  if constexpr (FMT == FMT_F16)
    if (a.range_flag && out_of_range != 0ull && lane == 0) a.range_flag[0] = 1;     // (same value from every writer)
  GDN_STAMP(11)
}

#ifndef GDN_DENSE_EXTRA_DC   // the d = 128 translation unit instantiates the fused family only
// ------------------------------------------------------------------ staged gather-aggregate (K8)
// z[b] = alpha[b] . xlin[b] + bias for windows whose projected tile xlin[n, 64] and attention scalars
// come from HBM (gdn_project_fwd): models/graph_layer.py:65-74,82-117.  Same softmax / scatter /
// matrix-core product as the fused kernel; the tile is staged ROW-major in 16-bit terms (fp32 storage:
// two f16 terms per value; bf16 storage: the stored value itself) and read back TRANSPOSED by
// ds_read_b64_tr_b16 as the B operand (k = source sensor on the registers, column on the lane), so
// Z = A . X comes out with the target in the registers and the column on the lane: every accumulator
// register is one 128-byte row segment of z.
//
// Tile image: [ROWS][64] 16-bit, 128-byte rows, the two 64-byte halves of a row exchanged on rows with
// bit 1 set: the four rows of one transposed read then cover all 64 banks (conflict-free).
typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int NT, int SL, int FMT>
struct KCfg {
  static constexpr int KS = 2 * NT;
  static constexpr int ROWS = 32 * NT;
  static constexpr int THREADS = 64 * NT;
  static constexpr int AROW = KS * 32 + 16;
  static constexpr int AWAVE = 32 * AROW;
  static constexpr int NPX = FMT == FMT_F16 ? 2 : 1;
  static constexpr int TPLANE = ROWS * 128;
  static constexpr int OFF_A = 0;
  static constexpr int OFF_T = NT * AWAVE;
  static constexpr int OFF_SI = OFF_T + NPX * TPLANE;
  static constexpr int OFF_SJ = OFF_SI + ROWS * 4;
  static constexpr int LDS = OFF_SJ + ROWS * 4;
  // tile staging: 16-byte pieces per row (fp32: 4 columns, bf16: 8 columns) and per thread
  static constexpr int PPR = FMT == FMT_F16 ? 16 : 8;
  static constexpr int RSTEP = THREADS / PPR;           // rows between a thread's pieces (multiple of 4)
  static constexpr int TU = ROWS / RSTEP;               // pieces per thread: 8 (fp32) / 4 (bf16)
};

struct KArgs {
  const void* xlin;        // [BN, 64] fp32 / bf16
  const float* si;         // [BN]
  const float* sj;
  const uint16_t* nbr;     // [n, pitch]
  const float* bias;       // [64]
  int batch, n, pitch;
  void* z;                 // [BN, 64] fp32 / bf16
  float* alpha;            // [BN, pitch] or null
};

// (Measured, round 3: the bf16-storage variant compiles to 175 VGPRs — two waves per SIMD although its 51 KB of LDS
// would allow three workgroups per CU.  Forcing three with the launch bound (168 VGPRs, 7 spilled) was SLOWER:
// 281 vs 250 us per 32768 windows.  The kernel is bound by the LDS pipe, not by latency.)
template <int NT, int SL, int FMT, bool WANT_ALPHA>
__global__ __launch_bounds__(64 * NT, SL <= 16 ? 2 : 1) void gdn_dense_attn_kernel(const KArgs a) {
  using C = KCfg<NT, SL, FMT>;
  using F = Fmt<FMT>;
  constexpr int DC = 2;
  extern __shared__ uint4 smem_u4[];
  char* smem = reinterpret_cast<char*>(smem_u4);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int n = a.n;
  constexpr int ESZ = FMT == FMT_F16 ? 4 : 2;

  // ---------------------------------------------------------------- once per workgroup
  for (int t = lane; t < C::AWAVE / 16; t += 64)
    reinterpret_cast<uint4*>(smem + C::OFF_A + wv * C::AWAVE)[t] = make_uint4(0, 0, 0, 0);
  const int ti = 32 * wv + (lane >> 1);
  const int half = lane & 1;
  int sjoff[SL], scoff[SL];
  {
    const uint16_t* row = a.nbr + (size_t)min(ti, n - 1) * a.pitch + half * SL;
#pragma unroll
    for (int q = 0; q < SL; ++q) {
      const int jj = (int)row[q];
      const int j = ti < n ? jj : n;
      sjoff[q] = C::OFF_SJ + j * 4;
      scoff[q] = C::OFF_A + wv * C::AWAVE + (lane >> 1) * C::AROW + pos_of_source(j) * 2;
    }
  }
  const int si_off = C::OFF_SI + ti * 4;
  float bias[DC];
#pragma unroll
  for (int cb = 0; cb < DC; ++cb)
    bias[cb] = a.bias[cb * 32 + l32] * (FMT == FMT_F16 ? GDN_F16_ALPHA_SCALE : 1.f);

  // tile staging: piece u of this thread = row prow0 + u RSTEP, 16-byte piece ppc of the row
  const int ppc = tid % C::PPR, prow0 = tid / C::PPR;
  const int t_st = C::OFF_T + prow0 * 128 +
                   (FMT == FMT_F16 ? (((ppc >> 3) ^ ((prow0 >> 1) & 1)) * 64 + (ppc & 7) * 8)
                                   : (((ppc >> 2) ^ ((prow0 >> 1) & 1)) * 64 + (ppc & 3) * 16));
  const int t_voff = (prow0 * 64 + ppc * (16 / ESZ)) * ESZ;       // bytes from the window's first row
  bool tok[C::TU];
#pragma unroll
  for (int u = 0; u < C::TU; ++u) tok[u] = prow0 + u * C::RSTEP < n;
  const size_t t_total = (size_t)a.batch * n * 64 * ESZ;
  uint4 pre[C::TU];
  float psi, psj;
  const int sn = min(tid, n - 1);
  auto load_window = [&](int bb) {
    const size_t first = (size_t)bb * n * 64 * ESZ;
    const size_t rem = t_total - first;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(a.xlin)) + first, 0,
        (int)(rem > 0xffffffffull ? 0xffffffffu : (unsigned)rem), 0x00020000);
#pragma unroll
    for (int u = 0; u < C::TU; ++u) {
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, t_voff, u * (C::RSTEP * 64 * ESZ), 0);
      pre[u] = __builtin_bit_cast(uint4, v);
    }
    psi = a.si[(size_t)bb * n + sn];
    psj = a.sj[(size_t)bb * n + sn];
  };
  // rows >= n of the tile (the list sentinel n and the pad rows) stay zero: they are never stored again
  for (int t = tid; t < C::NPX * C::TPLANE / 16; t += C::THREADS)
    reinterpret_cast<uint4*>(smem + C::OFF_T)[t] = make_uint4(0, 0, 0, 0);
  if (tid == 0) *reinterpret_cast<float*>(smem + C::OFF_SJ + n * 4) = -INFINITY;
  load_window(blockIdx.x);
  __syncthreads();

  const int arow_off = C::OFF_A + wv * C::AWAVE + l32 * C::AROW + h * 16;   // alpha operand (A) of this lane
  // transposed reads: lane 4q+p of a 16-lane group addresses row q, columns 4p .. 4p+3 of its block
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  const int tsw = (tq >> 1) & 1;
  const int tr_base = C::OFF_T + (4 * h + tq) * 128 + 32 * (g & 1) + 8 * tp;   // + (cb ^ tsw) 64 + ks 2048 + rd 1024
  using lds_s16x4 = __attribute__((address_space(3))) s16x4;

  for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
    // ---- tile of window b -> LDS (16-bit terms), scalars -> LDS (log2 domain)
    __builtin_amdgcn_s_setprio(GDN_K8_PRIO_T);     // phase priorities: see gdn_dense_fused_kernel
#pragma unroll
    for (int u = 0; u < C::TU; ++u) {
      if (!tok[u]) continue;        // pad rows stay zero (the loads past row n read the next window)
      char* dst = smem + t_st + u * (C::RSTEP * 128);
      if constexpr (FMT == FMT_F16) {
        float v0 = __uint_as_float(pre[u].x), v1 = __uint_as_float(pre[u].y);
        float v2 = __uint_as_float(pre[u].z), v3 = __uint_as_float(pre[u].w);
        unsigned h0, h1, l0, l1;
        F::split2(v0, v1, h0, l0);
        F::split2(v2, v3, h1, l1);
        *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(dst + C::TPLANE) = make_uint2(l0, l1);
      } else {
        *reinterpret_cast<uint4*>(dst) = pre[u];
      }
    }
    if (tid < n) {
      *reinterpret_cast<float*>(smem + C::OFF_SI + tid * 4) = psi * GDN_LOG2E;
      *reinterpret_cast<float*>(smem + C::OFF_SJ + tid * 4) = psj * GDN_LOG2E;
    }
    __syncthreads();                                           // B1
    load_window(min(b + (int)gridDim.x, a.batch - 1));
    __builtin_amdgcn_s_setprio(GDN_K8_PRIO_S);

    // ---- S
    unsigned ph[SL / 2], pl[SL / 2];
    {
      float al[SL];
      softmax_split<SL, FMT, WANT_ALPHA, GDN_TRIM_PACK != 0 && SL <= 16 && FMT == FMT_F16>(smem, si_off, sjoff, ph, pl, al);
      if constexpr (WANT_ALPHA) {
        if (ti < n) {
          float4* dst = reinterpret_cast<float4*>(a.alpha + ((size_t)b * n + ti) * a.pitch + half * SL);
#pragma unroll
          for (int q = 0; q < SL; q += 4) dst[q / 4] = make_float4(al[q], al[q + 1], al[q + 2], al[q + 3]);
        }
      }
    }
    // ---- M: Z = A . X, target on the registers, column on the lane; C-in = bias
    f32x16 acc[DC];
#pragma unroll
    for (int cb = 0; cb < DC; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[cb][r] = bias[cb];   // (bias carries the alpha scale)
    u32x4 fa[2], fx[2][DC][C::NPX];
    auto fetch = [&](int ks, int buf, int nterms) {
      fa[buf] = lds_frag(smem, arow_off + ks * 32);
#pragma unroll
      for (int cb = 0; cb < DC; ++cb)
#pragma unroll
        for (int t = 0; t < C::NPX; ++t) {
          if (t >= nterms) continue;
          const char* p0 = smem + tr_base + t * C::TPLANE + ks * 2048;
          const int co = cb == 0 ? tsw * 64 : (tsw ^ 1) * 64;
          const s16x4 r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + co));
          const s16x4 r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + co + 1024));
          const uint2 u0 = __builtin_bit_cast(uint2, r0), u1 = __builtin_bit_cast(uint2, r1);
          fx[buf][cb][t] = u32x4{u0.x, u0.y, u1.x, u1.y};
        }
    };
    __builtin_amdgcn_s_setprio(GDN_K8_PRIO_M);
    scatter_terms<SL>(smem, scoff, ph);
    __builtin_amdgcn_sched_barrier(0);
    fetch(0, 0, C::NPX);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      if (ks + 1 < C::KS) fetch(ks + 1, (ks + 1) & 1, C::NPX);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < DC; ++cb)
#pragma unroll
        for (int t = 0; t < C::NPX; ++t) acc[cb] = F::mfma(fa[ks & 1], fx[ks & 1][cb][t], acc[cb]);
      __builtin_amdgcn_sched_barrier(0);
    }
    scatter_terms<SL>(smem, scoff, pl);
    __builtin_amdgcn_sched_barrier(0);
    fetch(0, 0, 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      if (ks + 1 < C::KS) fetch(ks + 1, (ks + 1) & 1, 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < DC; ++cb) acc[cb] = F::mfma(fa[ks & 1], fx[ks & 1][cb][0], acc[cb]);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- z rows: register r = target 32wv + (r&3) + 8(r>>2) + 4h, lane = column
    __builtin_amdgcn_s_setprio(GDN_K8_PRIO_Z);
    constexpr float UNSCALE = FMT == FMT_F16 ? 1.f / GDN_F16_ALPHA_SCALE : 1.f;
#pragma unroll
    for (int cb = 0; cb < DC; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * wv + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float v = acc[cb][r] * UNSCALE;
        if constexpr (FMT == FMT_F16) {
          if (row < n) reinterpret_cast<float*>(a.z)[((size_t)b * n + row) * 64 + cb * 32 + l32] = v;
        } else {
          const float nb = dpp_f<GDN_DPP_XOR1>(v);            // the odd neighbour's column
          if (row < n && (lane & 1) == 0)
            reinterpret_cast<unsigned*>(a.z)[(((size_t)b * n + row) * 64 + cb * 32 + l32) >> 1] = F::pk(v, nb);
        }
      }
    __syncthreads();                                           // B2: tile and scalars free
  }
}

// ------------------------------------------------------------------ backward of the gather-aggregate
// Autograd of models/graph_layer.py:106-117 (what gdn_attn_aggregate_bwd computes with row gathers) as two
// dense matrix-core products per window:
//   G  = dZ . X^T   [targets x sources, K = 64]   g_iq = G[i][nbr(i,q)] = d_z_i . xlin_j  (d alpha)
//   dX = A^T . dZ   [sources x 64, K = targets]   the reverse gather
// and between them, per (target, slot) lane as in the forward's softmax phase:
//   de = alpha (g - sum_q alpha g),  dl = de * LeakyReLU'(s_i + s_j),  d_s_i = sum_q dl,  d_s_j = column sums.
// d_z (gradients of a mean loss sit around 1e-6, below the f16 normal range) is scaled per window by a power
// of two chosen from max|d_z|, exactly, and every output is unscaled by the same power.  The d_z tile is staged
// as two f16 terms in K8's row-major swizzled layout (the dX product reads it transposed, ds_read_b64_tr_b16,
// against ONE transposed attention image shared by the workgroup: a wave's 32 output rows are sources, whose
// weights come from every target; the G product reads its rows as A fragments), the xlin tile directly in
// operand order (B fragments of G, conflict free).  G goes through LDS once (each wave its own 32 target
// rows, gathered by the same wave: no barrier); DL takes its place (the wave clears its rows and writes dl where
// an edge exists) and d_s_j = its column sums in a fixed order: deterministic, no atomics, no reverse lists.
// d_bias = column sums of d_z.  One workgroup per CU (134 KB of LDS at n = 127).
struct BwArgs {
  const float* d_z;        // [BN, 64]
  const float* xlin;       // [BN, 64]
  const float* alpha;      // [BN, pitch] (padding slots 0)
  const float* si;         // [BN]
  const float* sj;
  const uint16_t* nbr;     // [n, pitch]
  int batch, n, pitch;
  float* d_xlin;           // [BN, 64]
  float* d_si;             // [BN]
  float* d_sj;
  float* d_bias;           // [64], written (fixed-order sum of the workgroups' partial rows: gdn_colsum_ticket)
  float* bias_ws;          // ticket + [grid][64] partial rows
};

template <int NT, int SL>
struct BwCfg {
  static constexpr int KS = 2 * NT;
  static constexpr int ROWS = 32 * NT;
  static constexpr int THREADS = 64 * NT;
  static constexpr int AROW = KS * 32 + 16;
  static constexpr int AIMG = ROWS * AROW;
  static constexpr int TPLANE = ROWS * 128;
  static constexpr int GROW = ROWS * 4;                 // one row of G / DL^T: ROWS fp32
  static constexpr int GBYTES = ROWS * GROW;
  static constexpr int OFF_A = 0;
  static constexpr int OFF_DZ = AIMG;
  static constexpr int OFF_X = OFF_DZ + 2 * TPLANE;     // the xlin tile, later G, later DL^T
  static constexpr int OFF_G = OFF_X;
  static constexpr int GREG = GBYTES > 2 * TPLANE ? GBYTES : 2 * TPLANE;
  static constexpr int OFF_SI = OFF_G + GREG;
  static constexpr int OFF_SJ = OFF_SI + ROWS * 4;
  static constexpr int OFF_MAX = OFF_SJ + ROWS * 4;
  static constexpr int LDS = OFF_MAX + 16;
  static constexpr int RSTEP = THREADS / 16;
  static constexpr int TU = ROWS / RSTEP;               // 16-byte pieces per thread and tile: 8
};

template <int NT, int SL>
__global__ __launch_bounds__(64 * NT) __attribute__((amdgpu_waves_per_eu(1, 1)))
void gdn_dense_attn_bwd_kernel(const BwArgs a) {
  using C = BwCfg<NT, SL>;
  using F = Fmt<FMT_F16>;
  constexpr int DC = 2;
  extern __shared__ uint4 smem_u4[];
  char* smem = reinterpret_cast<char*>(smem_u4);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int n = a.n;
  unsigned* wmax = reinterpret_cast<unsigned*>(smem + C::OFF_MAX);     // [2]: max |d_z| of a window (bits), by parity

  // ---------------------------------------------------------------- once per workgroup
  for (int t = tid; t < C::AIMG / 16; t += C::THREADS) reinterpret_cast<uint4*>(smem + C::OFF_A)[t] = make_uint4(0, 0, 0, 0);
  for (int t = tid; t < (2 * C::TPLANE + C::GREG) / 16; t += C::THREADS)       // pad rows of both tiles stay zero
    reinterpret_cast<uint4*>(smem + C::OFF_DZ)[t] = make_uint4(0, 0, 0, 0);
  if (tid < 2) wmax[tid] = 0u;
  const int ti = 32 * wv + (lane >> 1);
  const int half = lane & 1;
  int scoff[SL], sjoff[SL], goff[SL];
  {
    const uint16_t* row = a.nbr + (size_t)min(ti, n - 1) * a.pitch + half * SL;
    const int col = pos_of_source(ti) * 2;
#pragma unroll
    for (int q = 0; q < SL; ++q) {
      const int jj = (int)row[q];
      const int j = ti < n ? jj : n;                    // row / column n = the sentinel: zeros only
      scoff[q] = C::OFF_A + j * C::AROW + col;
      sjoff[q] = C::OFF_SJ + j * 4;
      goff[q] = C::OFF_G + ti * C::GROW + j * 4;        // G / DL [target ti][source j] (this wave's own rows)
    }
  }
  const int si_off = C::OFF_SI + ti * 4;
  // tile staging (K8's layout): piece u of this thread = row prow0 + u RSTEP, 16-byte piece ppc of the row
  const int ppc = tid % 16, prow0 = tid / 16;
  const int t_st = prow0 * 128 + (((ppc >> 3) ^ ((prow0 >> 1) & 1)) * 64 + (ppc & 7) * 8);
  const int t_voff = (prow0 * 64 + ppc * 4) * 4;
  bool tok[C::TU];
#pragma unroll
  for (int u = 0; u < C::TU; ++u) tok[u] = prow0 + u * C::RSTEP < n;
  const size_t t_total = (size_t)a.batch * n * 64 * 4;
  uint4 pdz[C::TU], px[C::TU];
  float psi, psj;
  const int sn = min(tid, n - 1);
  auto load_window = [&](int bb) {
    const size_t first = (size_t)bb * n * 64 * 4;
    const size_t rem = t_total - first;
    const int lim = (int)(rem > 0xffffffffull ? 0xffffffffu : (unsigned)rem);
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(a.d_z)) + first, 0, lim, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(a.xlin)) + first, 0, lim, 0x00020000);
#pragma unroll
    for (int u = 0; u < C::TU; ++u) {
      pdz[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rz, t_voff, u * (C::RSTEP * 256), 0));
      px[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rx, t_voff, u * (C::RSTEP * 256), 0));
    }
    psi = a.si[(size_t)bb * n + sn];
    psj = a.sj[(size_t)bb * n + sn];
  };
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};               // d_bias: this thread's columns 4 ppc .. 4 ppc + 3
  load_window(blockIdx.x);
  __syncthreads();
  if (tid == 0) *reinterpret_cast<float*>(smem + C::OFF_SJ + n * 4) = 0.f;

  // operand addressing
  const int rsw = (l32 >> 1) & 1;
  auto piece = [&](int ks) { return (((ks >> 1) ^ rsw) * 64) + ((32 * ks + 16 * h) & 63); };   // bytes inside a row
  const int arow_off = C::OFF_A + wv * (32 * C::AROW) + l32 * C::AROW + h * 16;   // image rows 32wv + l32 (sources)
  const int g4 = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  const int tsw = (tq >> 1) & 1;
  const int tr_base = C::OFF_DZ + (4 * h + tq) * 128 + 32 * (g4 & 1) + 8 * tp;
  using lds_s16x4 = __attribute__((address_space(3))) s16x4;

  GDN_STAMP(20)
  int par = 0;
  for (int b = blockIdx.x; b < a.batch; b += gridDim.x, par ^= 1) {
    // ---- attention weights of this lane's slots (issued first: consumed several barriers later)
    float al[SL];
    {
      const float4* src = reinterpret_cast<const float4*>(a.alpha + ((size_t)b * n + min(ti, n - 1)) * a.pitch + half * SL);
#pragma unroll
      for (int q = 0; q < SL; q += 4) {
        const float4 v = src[q / 4];
        al[q] = v.x; al[q + 1] = v.y; al[q + 2] = v.z; al[q + 3] = v.w;
      }
      if (ti >= n) {
#pragma unroll
        for (int q = 0; q < SL; ++q) al[q] = 0.f;
      }
    }
if (b == (int)blockIdx.x) { GDN_STAMP(21) }
        // ---- scale of the window (2^kexp, max|d_z| 2^kexp in [2^12, 2^13)) and the d_bias partial sums
    float mx = 0.f;
#pragma unroll
    for (int u = 0; u < C::TU; ++u) {
      if (!tok[u]) continue;
      const float v0 = __uint_as_float(pdz[u].x), v1 = __uint_as_float(pdz[u].y);
      const float v2 = __uint_as_float(pdz[u].z), v3 = __uint_as_float(pdz[u].w);
      bsum[0] += v0; bsum[1] += v1; bsum[2] += v2; bsum[3] += v3;
      mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3))));
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) mx = fmaxf(mx, __shfl_xor(mx, dd));
    if (lane == 0) atomicMax(&wmax[par], __float_as_uint(mx));   // non-negative floats order like their bits
    __syncthreads();                                             // B0 (also: previous window fully retired)
if (b == (int)blockIdx.x) { GDN_STAMP(22) }
        const unsigned mbits = wmax[par];
    if (tid == 0) wmax[par ^ 1] = 0u;                            // the next window's slot
    int kexp = 12 - ((int)((mbits >> 23) & 255u) - 127);
    kexp = mbits == 0u ? 0 : max(-100, min(100, kexp));
    const float scale = __uint_as_float((unsigned)(kexp + 127) << 23);
    const float unscale = __uint_as_float((unsigned)(127 - kexp) << 23);
#pragma unroll
    for (int u = 0; u < C::TU; ++u) {
      if (!tok[u]) continue;
      {
        char* dst = smem + C::OFF_DZ + t_st + u * (C::RSTEP * 128);
        const float v0 = __uint_as_float(pdz[u].x) * scale, v1 = __uint_as_float(pdz[u].y) * scale;
        const float v2 = __uint_as_float(pdz[u].z) * scale, v3 = __uint_as_float(pdz[u].w) * scale;
        const unsigned h0 = F::pk(v0, v1), h1 = F::pk(v2, v3);
        const unsigned l0 = F::pk(F::res0(h0, v0), F::res1(h0, v1)), l1 = F::pk(F::res0(h1, v2), F::res1(h1, v3));
        *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
        *reinterpret_cast<uint2*>(dst + C::TPLANE) = make_uint2(l0, l1);
      }
    }
    // the xlin tile in OPERAND order — [k-step][source tile][term][lane] x 16 bytes, what the G product reads as
    // its B fragments with consecutive lanes on consecutive banks (read as rows of the swizzled row-major
    // layout the same fragments are 8-way bank conflicts); rows >= n are written as zeros every window (the
    // region held G / DL of the previous one)
#pragma unroll
    for (int u = 0; u < C::TU; ++u) {
      const int row = prow0 + u * C::RSTEP;
      char* dst = smem + C::OFF_X + ((((ppc >> 2) * NT + (row >> 5)) * 2) * 64 + (row & 31) + 32 * ((ppc & 3) >> 1)) * 16 +
                  8 * (ppc & 1);
      unsigned h0 = 0u, h1 = 0u, l0 = 0u, l1 = 0u;
      if (tok[u]) {
        const float v0 = __uint_as_float(px[u].x), v1 = __uint_as_float(px[u].y);
        const float v2 = __uint_as_float(px[u].z), v3 = __uint_as_float(px[u].w);
        h0 = F::pk(v0, v1); h1 = F::pk(v2, v3);
        l0 = F::pk(F::res0(h0, v0), F::res1(h0, v1)); l1 = F::pk(F::res0(h1, v2), F::res1(h1, v3));
      }
      *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(dst + 1024) = make_uint2(l0, l1);
    }
    if (tid < n) {
      *reinterpret_cast<float*>(smem + C::OFF_SI + tid * 4) = psi;
      *reinterpret_cast<float*>(smem + C::OFF_SJ + tid * 4) = psj;
    }
    if (tid == n) *reinterpret_cast<float*>(smem + C::OFF_SJ + n * 4) = 0.f;   // the sentinel (d_s_j partials reuse this array)
    __syncthreads();                                             // B1: tiles + scalars ready
if (b == (int)blockIdx.x) { GDN_STAMP(23) }
        load_window(min(b + (int)gridDim.x, a.batch - 1));

    // ---- G = dZ . X^T : A = d_z rows of this wave's targets, B = xlin rows (sources) of column tile tn
    f32x16 accg[NT];
#pragma unroll
    for (int tn = 0; tn < NT; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) accg[tn][r] = 0.f;
    {
      u32x4 fdz[2][2], fxx[2][NT][2];                 // [buffer][..][hi, lo]
      auto fetch_g = [&](int ks, int buf) {
        const int po = piece(ks);
        fdz[buf][0] = lds_frag(smem, C::OFF_DZ + (32 * wv + l32) * 128 + po);
        fdz[buf][1] = lds_frag(smem, C::OFF_DZ + C::TPLANE + (32 * wv + l32) * 128 + po);
#pragma unroll
        for (int tn = 0; tn < NT; ++tn) {
          fxx[buf][tn][0] = lds_frag(smem, C::OFF_X + (((ks * NT + tn) * 2) * 64 + lane) * 16);
          fxx[buf][tn][1] = lds_frag(smem, C::OFF_X + (((ks * NT + tn) * 2 + 1) * 64 + lane) * 16);
        }
      };
      fetch_g(0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks + 1 < 4) fetch_g(ks + 1, (ks + 1) & 1);   // lands under this k-step's products
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tn = 0; tn < NT; ++tn) {
          accg[tn] = F::mfma(fdz[ks & 1][0], fxx[ks & 1][tn][0], accg[tn]);
          accg[tn] = F::mfma(fdz[ks & 1][1], fxx[ks & 1][tn][0], accg[tn]);
          accg[tn] = F::mfma(fdz[ks & 1][0], fxx[ks & 1][tn][1], accg[tn]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
if (b == (int)blockIdx.x) { GDN_STAMP(24) }
        __syncthreads();                                             // B2: every wave is done with the xlin tile
    // G rows of this wave -> its own block of the G region (register r = target 32wv + (r&3) + 8(r>>2) + 4h)
#pragma unroll
    for (int tn = 0; tn < NT; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * wv + (r & 3) + 8 * (r >> 2) + 4 * h;
        *reinterpret_cast<float*>(smem + C::OFF_G + row * C::GROW + (32 * tn + l32) * 4) = accg[tn][r];
      }
if (b == (int)blockIdx.x) { GDN_STAMP(25) }
        // ---- softmax backward per (target, slot): in-order LDS within the wave, no barrier needed for its own rows
    float dl[SL];
    {
      const float sti = lds_f32(smem, si_off);
      float g[SL], sjv[SL];
#pragma unroll
      for (int q = 0; q < SL; ++q) {
        g[q] = lds_f32(smem, goff[q]);
        sjv[q] = lds_f32(smem, sjoff[q]);
      }
      float dot = 0.f;
#pragma unroll
      for (int q = 0; q < SL; ++q) dot = fmaf(al[q], g[q], dot);
      dot += dpp_f<GDN_DPP_XOR1>(dot);
      // d_s_i = sum_q slope_q de_q.  The de_q of a target sum to 0 (softmax), so sum_q slope_q de_q =
      // (0.2 - 1) * sum over the slots with a NEGATIVE logit: the slope-1 terms, whose sum is pure rounding noise
      // when they cancel, are never added.  A target whose logits are all positive gets its exact gradient, 0
      // (near-uniform attention at initialisation: most targets), instead of ~1e-7 of its largest term.
      float dsi = 0.f;
#pragma unroll
      for (int q = 0; q < SL; ++q) {
        const float de = al[q] * (g[q] - dot);
        const bool pos = (sti + sjv[q]) > 0.f;
        dl[q] = pos ? de : de * GDN_NEG_SLOPE;
        dsi += pos ? 0.f : de;
      }
      dsi += dpp_f<GDN_DPP_XOR1>(dsi);
      if (half == 0 && ti < n) a.d_si[(size_t)b * n + ti] = dsi * ((GDN_NEG_SLOPE - 1.f) * unscale);
    }
if (b == (int)blockIdx.x) { GDN_STAMP(26) }
    // DL[target][source] takes the place of G: the wave clears its own 32 rows (its gathers are done: LDS is
    // in order within a wave) and writes dl where an edge exists — no barrier, no workgroup-wide zero fill
    for (int t = lane; t < 32 * C::GROW / 16; t += 64)
      reinterpret_cast<uint4*>(smem + C::OFF_G + 32 * wv * C::GROW)[t] = make_uint4(0, 0, 0, 0);
if (b == (int)blockIdx.x) { GDN_STAMP(27) }
#pragma unroll
    for (int q = 0; q < SL; ++q) *reinterpret_cast<float*>(smem + goff[q]) = dl[q];    // (padding slots: column n, value 0)
    // the two 16-bit terms of the weights; hi terms into the shared transposed image
    unsigned ph[SL / 2], pl[SL / 2];
#pragma unroll
    for (int q = 0; q < SL; q += 2) {
      const float a0 = al[q] * GDN_F16_ALPHA_SCALE, a1 = al[q + 1] * GDN_F16_ALPHA_SCALE;
      ph[q / 2] = F::pk(a0, a1);
      pl[q / 2] = F::pk(F::res0(ph[q / 2], a0), F::res1(ph[q / 2], a1));
    }
    scatter_terms<SL>(smem, scoff, ph);
    __syncthreads();                                             // B5: DL^T and the hi image complete
if (b == (int)blockIdx.x) { GDN_STAMP(28) }
        // d_s_j = column sums of DL: lane = column (a wave's reads fall on consecutive banks), two threads per
    // source (even / odd targets), fixed order; the halves meet after the next barrier
    float* dsj_part = reinterpret_cast<float*>(smem + C::OFF_SI);       // [2][ROWS]: s_i / s_j are dead by now
    if (tid < 2 * C::ROWS || C::THREADS < 2 * C::ROWS) {
      for (int cc = tid; cc < 2 * C::ROWS; cc += C::THREADS) {
        const int j = cc % C::ROWS, hf = cc / C::ROWS;
        const char* colp = smem + C::OFF_G + hf * C::GROW + j * 4;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
        for (int t = 0; t < C::ROWS / 2; t += 4) {
          s0 += lds_f32(colp, (t + 0) * 2 * C::GROW);
          s1 += lds_f32(colp, (t + 1) * 2 * C::GROW);
          s2 += lds_f32(colp, (t + 2) * 2 * C::GROW);
          s3 += lds_f32(colp, (t + 3) * 2 * C::GROW);
        }
        dsj_part[cc] = (s0 + s1) + (s2 + s3);
      }
    }
if (b == (int)blockIdx.x) { GDN_STAMP(29) }
        // ---- dX = A^T . dZ
    f32x16 acc[DC];
#pragma unroll
    for (int cb = 0; cb < DC; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
    u32x4 fa[2], fx[2][DC][2];
    auto fetch = [&](int ks, int buf, int nterms) {
      fa[buf] = lds_frag(smem, arow_off + ks * 32);
#pragma unroll
      for (int cb = 0; cb < DC; ++cb)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          if (t >= nterms) continue;
          const char* p0 = smem + tr_base + t * C::TPLANE + ks * 2048;
          const int co = cb == 0 ? tsw * 64 : (tsw ^ 1) * 64;
          const s16x4 r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + co));
          const s16x4 r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + co + 1024));
          const uint2 u0 = __builtin_bit_cast(uint2, r0), u1 = __builtin_bit_cast(uint2, r1);
          fx[buf][cb][t] = u32x4{u0.x, u0.y, u1.x, u1.y};
        }
    };
    fetch(0, 0, 2);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      if (ks + 1 < C::KS) fetch(ks + 1, (ks + 1) & 1, 2);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < DC; ++cb)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[cb] = F::mfma(fa[ks & 1], fx[ks & 1][cb][t], acc[cb]);
      __builtin_amdgcn_sched_barrier(0);
    }
if (b == (int)blockIdx.x) { GDN_STAMP(30) }
        __syncthreads();                                             // B6: every wave is done with the hi image
    if (tid < n) a.d_sj[(size_t)b * n + tid] = (dsj_part[tid] + dsj_part[C::ROWS + tid]) * unscale;
    scatter_terms<SL>(smem, scoff, pl);
    __syncthreads();                                             // B7: lo image complete
    fetch(0, 0, 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) {
      if (ks + 1 < C::KS) fetch(ks + 1, (ks + 1) & 1, 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int cb = 0; cb < DC; ++cb) acc[cb] = F::mfma(fa[ks & 1], fx[ks & 1][cb][0], acc[cb]);
      __builtin_amdgcn_sched_barrier(0);
    }
if (b == (int)blockIdx.x) { GDN_STAMP(31) }
        // ---- d_xlin rows: register r = source 32wv + (r&3) + 8(r>>2) + 4h, lane = column
    const float un2 = unscale * (1.f / GDN_F16_ALPHA_SCALE);
#pragma unroll
    for (int cb = 0; cb < DC; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * wv + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < n) a.d_xlin[((size_t)b * n + row) * 64 + cb * 32 + l32] = acc[cb][r] * un2;
      }
    if (b == (int)blockIdx.x) { GDN_STAMP(32) }
    // (the next iteration's B0 orders these reads of the image / tiles before they are rewritten)
  }
  GDN_STAMP(33)
  // ---- d_bias: column sums over this workgroup's windows (16 row groups per column piece)
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem + C::OFF_G);
#pragma unroll
  for (int v = 0; v < 4; ++v) red[(tid / 16) * 64 + ppc * 4 + v] = bsum[v];
  __syncthreads();
  float* brow = reinterpret_cast<float*>(smem + C::OFF_DZ);
  if (tid < 64) {
    float t = 0.f;
    for (int r = 0; r < C::THREADS / 16; ++r) t += red[r * 64 + tid];
    brow[tid] = t;
  }
  __syncthreads();
  gdn_colsum_ticket(a.bias_ws, brow, 64, a.d_bias, reinterpret_cast<float*>(smem + C::OFF_A));
  GDN_STAMP(34)
}

// ------------------------------------------------------------------ staged projection
// xlin[b] = x[b] . lin^T (models/graph_layer.py:56) and the attention scalars s_i, s_j of every sensor
// (graph_layer.py:94-104 folded: s = x_row . a + c[sensor]) on the 16-bit matrix cores: the P phase of
// the fused kernel without the BatchNorm fold, results written to HBM.  fp32 storage: x and lin are
// split into two f16 terms (three products, fp32-grade); bf16 storage: x is exact, lin three bf16 terms,
// xlin rounded to bf16 once.
struct PArgs {
  const void* x;            // [B, n, w] fp32 / bf16
  const float* lin_w;       // [64, w]
  const float* node_terms;
  int batch, n, w;
  void* xlin;               // [BN, 64] fp32 / bf16
  float* si;
  float* sj;
};

template <int NT, int WK, int FMT>
__global__ __launch_bounds__(64 * NT) void gdn_dense_project_kernel(const PArgs a) {
  using F = Fmt<FMT>;
  constexpr int DC = 2, ROWS = 32 * NT, THREADS = 64 * NT, XP = 16 * WK + 4, XU = 8 * WK;
  constexpr int NTL = FMT == FMT_F16 ? 2 : 3, NTXIN = FMT == FMT_F16 ? 2 : 1;
  constexpr int OFF_XS = 0, OFF_CS = ROWS * XP * 4, LDS = OFF_CS + 3 * ROWS * 4;
  __shared__ uint4 smem_u4[LDS / 16 + 1];
  char* smem = reinterpret_cast<char*>(smem_u4);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l32 = lane & 31, h = lane >> 5;
  const int n = a.n, w = a.w;

  u32x4 bl[DC][WK][NTL], bs[WK][NTL];
#pragma unroll
  for (int wk = 0; wk < WK; ++wk) {
#pragma unroll
    for (int cb = 0; cb < DC; ++cb) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = wk * 16 + 8 * h + j;
        v[j] = ld_or(a.lin_w, (cb * 32 + l32) * w + k, k < w);
      }
      split8<FMT, NTL, false>(v, bl[cb][wk]);
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ld_or(a.node_terms, l32 * GDN_A_PITCH + wk * 16 + 8 * h + j, l32 < 2);
    split8<FMT, NTL, false>(v, bs[wk]);
  }
  {
    float* ct = reinterpret_cast<float*>(smem + OFF_CS);
    for (int t = tid; t < 3 * ROWS; t += THREADS) {
      const int which = t / ROWS, row = t - which * ROWS;
      ct[t] = ld_or(a.node_terms, 2 * GDN_A_PITCH + which * n + row, which < 2 && row < n);
    }
  }
  const int cs_off = OFF_CS + (min(l32, 2) * ROWS + 32 * wv + 4 * h) * 4;

  constexpr int CW = 16 * WK, RS = THREADS / CW;
  constexpr int ESZ = FMT == FMT_F16 ? 4 : 2;
  const int xcol = tid & (CW - 1), xrow0 = tid / CW;
  const int xvoff = (min(xrow0, n - 1) * w + min(xcol, w - 1)) * ESZ;
  const int xstep = RS * w * ESZ;
  const int xst_off = OFF_XS + (xrow0 * XP + xcol) * 4;
  bool xok[XU];
#pragma unroll
  for (int u = 0; u < XU; ++u) xok[u] = xcol < w && xrow0 + u * RS < n;
  const size_t x_total = (size_t)a.batch * n * w * ESZ;
  float xr[XU];
  auto load_window = [&](int bb) {
    const size_t first = (size_t)bb * n * w * ESZ;
    const size_t rem = x_total - first;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(a.x)) + first, 0,
        (int)(rem > 0xffffffffull ? 0xffffffffu : (unsigned)rem), 0x00020000);
#pragma unroll
    for (int u = 0; u < XU; ++u) {
      if constexpr (FMT == FMT_F16) {
        xr[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, xvoff, u * xstep, 0));
      } else {
        xr[u] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsrc, xvoff, u * xstep, 0) << 16);
      }
    }
  };
  load_window(blockIdx.x);
  __syncthreads();
  const int xrow_off = OFF_XS + ((32 * wv + l32) * XP + 8 * h) * 4;

  for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
#pragma unroll
    for (int u = 0; u < XU; ++u)
      *reinterpret_cast<float*>(smem + xst_off + u * (RS * XP * 4)) = xok[u] ? xr[u] : 0.f;
    __syncthreads();
    load_window(min(b + (int)gridDim.x, a.batch - 1));
    f32x16 acc1[DC], accs;
#pragma unroll
    for (int cb = 0; cb < DC; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[cb][r] = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 t = *reinterpret_cast<const float4*>(smem + cs_off + 32 * g);
      accs[4 * g] = t.x; accs[4 * g + 1] = t.y; accs[4 * g + 2] = t.z; accs[4 * g + 3] = t.w;
    }
#pragma unroll
    for (int wk = 0; wk < WK; ++wk) {
      float v[8];
      const float4 v0 = *reinterpret_cast<const float4*>(smem + xrow_off + wk * 64);
      const float4 v1 = *reinterpret_cast<const float4*>(smem + xrow_off + wk * 64 + 16);
      v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w;
      v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
      u32x4 ax[NTXIN];
      split8<FMT, NTXIN, false>(v, ax);
#pragma unroll
      for (int tx = 0; tx < NTXIN; ++tx)
#pragma unroll
        for (int tl = 0; tl < NTL; ++tl)
          if (tx + tl < (NTXIN > NTL ? NTXIN : NTL)) {
#pragma unroll
            for (int cb = 0; cb < DC; ++cb) acc1[cb] = F::mfma(ax[tx], bl[cb][wk][tl], acc1[cb]);
            accs = F::mfma(ax[tx], bs[wk][tl], accs);
          }
    }
    __syncthreads();   // x tile free for the next window
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * wv + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (row < n) {
        const size_t grow = (size_t)b * n + row;
        if (l32 == 0) a.si[grow] = accs[r];
        if (l32 == 1) a.sj[grow] = accs[r];
      }
#pragma unroll
      for (int cb = 0; cb < DC; ++cb) {
        const float v = acc1[cb][r];
        if constexpr (FMT == FMT_F16) {
          if (row < n) reinterpret_cast<float*>(a.xlin)[((size_t)b * n + row) * 64 + cb * 32 + l32] = v;
        } else {
          const float nb = dpp_f<GDN_DPP_XOR1>(v);
          if (row < n && (lane & 1) == 0)
            reinterpret_cast<unsigned*>(a.xlin)[(((size_t)b * n + row) * 64 + cb * 32 + l32) >> 1] = F::pk(v, nb);
        }
      }
    }
  }
}

#endif  // GDN_DENSE_EXTRA_DC

// ------------------------------------------------------------------ host side
// resident workgroups per CU / CU count: the thread-safe per-device caches of gdn_common.hpp
static inline int blocks_per_cu(const void* fn, int threads, int lds) { return gdn_blocks_per_cu(fn, threads, lds); }
static inline int cu_count() { return gdn_cu_count(); }

enum { DOP_LAUNCH = 0, DOP_PLAN_BUILD = 1, DOP_PLAN_BYTES = 2 };

template <int NT, int DC, int WK, int SL, int FMT>
int fused_op(int op, const DArgs& a, unsigned* plan_out, long long* bytes, hipStream_t stream) {
  using C = DCfg<NT, DC, WK, SL, FMT>;
  using K = LaneConsts<NT, DC, WK, SL, FMT>;
  static_assert(C::LDS <= 160 * 1024, "LDS plan exceeds one CU");
  static_assert(C::OFF_CS == C::OFF_EC + 4 * 32 * DC * 4, "the two LDS tables are one block of the plan");
  if (op == DOP_PLAN_BYTES) {
    *bytes = (long long)K::PLAN_BYTES;
    return GDN_OK;
  }
  if (op == DOP_PLAN_BUILD) {
    hipLaunchKernelGGL((gdn_dense_plan_kernel<NT, DC, WK, SL, FMT>), dim3(1), dim3(C::THREADS), 0, stream, a, plan_out);
    return gdn_launch_status();
  }
  auto kern = gdn_dense_fused_kernel<NT, DC, WK, SL, FMT>;
  const int occ = blocks_per_cu(reinterpret_cast<const void*>(kern), C::THREADS, C::LDS);
  // the kernel is compiled for C::WGS resident workgroups per CU (registers by its launch bound, LDS by DCfg): a
  // device that holds fewer is not the one this build is for, and running thinner in silence would hide it.
  // GDN_DENSE_MAX_OCC caps the grid at that many workgroups per CU instead (A/B runs; read once per process).
  if (occ < C::WGS) return GDN_ERR_LAUNCH;
  const int occ_cap = GDN_ENV_INT_ONCE("GDN_DENSE_MAX_OCC", 0);
  const int occ_used = occ_cap > 0 ? min(occ, occ_cap) : occ;
  // A launch that cannot fill the machine twice over (one minibatch of 512 windows on 256 CUs) gets TWO windows
  // per workgroup instead of one: every workgroup pays the prologue (~3 us: 84-101 plan words per lane, the zero
  // fill of the alpha image), and the CU slots the thinner grid leaves free are what a concurrent launch on another stream runs
  // in.  Measured at 512-window launches (bench.py --coalesce 1): one stream 46.6 -> 45.1 M windows/s, two
  // streams 60.0 -> 71.3 M.  GDN_DENSE_MIN_WPW overrides (A/B runs; read once per process).
  const int slots = cu_count() * occ_used;
  int wpw = GDN_ENV_INT_ONCE("GDN_DENSE_MIN_WPW", 0);
  if (wpw <= 0) wpw = (a.batch > cu_count() && a.batch <= slots) ? 2 : 1;
  const int grid = max(1, min((a.batch + wpw - 1) / wpw, slots));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(C::THREADS), C::LDS, stream, a);
  return gdn_launch_status();
}

template <int NT, int DC, int WK, int FMT>
int select_sl(int op, const DArgs& a, unsigned* plan_out, long long* bytes, hipStream_t st) {
  switch (a.pitch) {
    case 16: return fused_op<NT, DC, WK, 8, FMT>(op, a, plan_out, bytes, st);
    case 32: return fused_op<NT, DC, WK, 16, FMT>(op, a, plan_out, bytes, st);
    case 48: return fused_op<NT, DC, WK, 24, FMT>(op, a, plan_out, bytes, st);
    case 64: return fused_op<NT, DC, WK, 32, FMT>(op, a, plan_out, bytes, st);
  }
  return GDN_ERR_UNSUPPORTED;
}

template <int NT, int FMT, int DC>
int select_wk(int op, const DArgs& a, unsigned* plan_out, long long* bytes, hipStream_t st) {
  if (a.w <= 16) return select_sl<NT, DC, 1, FMT>(op, a, plan_out, bytes, st);
  return select_sl<NT, DC, 2, FMT>(op, a, plan_out, bytes, st);
}

template <int FMT, int DC>
int select_nt(int op, const DArgs& a, unsigned* plan_out, long long* bytes, hipStream_t st) {
  switch ((a.n + 1 + 31) / 32) {
    case 1: return select_wk<1, FMT, DC>(op, a, plan_out, bytes, st);
    case 2: return select_wk<2, FMT, DC>(op, a, plan_out, bytes, st);
    case 3: return select_wk<3, FMT, DC>(op, a, plan_out, bytes, st);
    case 4: return select_wk<4, FMT, DC>(op, a, plan_out, bytes, st);
  }
  return GDN_ERR_UNSUPPORTED;
}

#ifdef GDN_DENSE_EXTRA_DC
}  // namespace
// Entry of the extra translation unit (gdn_forward_dense_d128.hip): the fused family at d = 32 * GDN_DENSE_EXTRA_DC.
// `args` is the DArgs of the main unit (same definition, compiled from the same text).
int gdn_dense_fused_op_d128(int op, const void* args, int bf16, unsigned* plan_out, long long* bytes,
                            hipStream_t st) {
  const DArgs& a = *static_cast<const DArgs*>(args);
  return bf16 ? select_nt<FMT_BF16, GDN_DENSE_EXTRA_DC>(op, a, plan_out, bytes, st)
              : select_nt<FMT_F16, GDN_DENSE_EXTRA_DC>(op, a, plan_out, bytes, st);
}
#else

template <int NT, int SL, int FMT, bool WANT_ALPHA>
int launch_attn(const KArgs& a, hipStream_t stream) {
  using C = KCfg<NT, SL, FMT>;
  static_assert(C::LDS <= 160 * 1024, "LDS plan exceeds one CU");
  auto kern = gdn_dense_attn_kernel<NT, SL, FMT, WANT_ALPHA>;
  const int occ = blocks_per_cu(reinterpret_cast<const void*>(kern), C::THREADS, C::LDS);
  const int grid = max(1, min(a.batch, cu_count() * occ));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(C::THREADS), C::LDS, stream, a);
  return gdn_launch_status();
}

template <int NT, int FMT, bool WANT_ALPHA>
int attn_select_sl(const KArgs& a, hipStream_t st) {
  switch (a.pitch) {
    case 16: return launch_attn<NT, 8, FMT, WANT_ALPHA>(a, st);
    case 32: return launch_attn<NT, 16, FMT, WANT_ALPHA>(a, st);
    case 48: return launch_attn<NT, 24, FMT, WANT_ALPHA>(a, st);
    case 64: return launch_attn<NT, 32, FMT, WANT_ALPHA>(a, st);
  }
  return GDN_ERR_UNSUPPORTED;
}

template <int FMT, bool WANT_ALPHA>
int attn_select_nt(const KArgs& a, hipStream_t st) {
  switch ((a.n + 1 + 31) / 32) {
    case 1: return attn_select_sl<1, FMT, WANT_ALPHA>(a, st);
    case 2: return attn_select_sl<2, FMT, WANT_ALPHA>(a, st);
    case 3: return attn_select_sl<3, FMT, WANT_ALPHA>(a, st);
    case 4: return attn_select_sl<4, FMT, WANT_ALPHA>(a, st);
  }
  return GDN_ERR_UNSUPPORTED;
}

}  // namespace

template <int NT, int FMT>
int launch_project(const PArgs& a, hipStream_t stream) {
  const int grid = max(1, min(a.batch, cu_count() * 8));
  if (a.w <= 16) hipLaunchKernelGGL((gdn_dense_project_kernel<NT, 1, FMT>), dim3(grid), dim3(64 * NT), 0, stream, a);
  else hipLaunchKernelGGL((gdn_dense_project_kernel<NT, 2, FMT>), dim3(grid), dim3(64 * NT), 0, stream, a);
  return gdn_launch_status();
}

int gdn_dense_project(const void* x, int is_bf16, const float* lin_w, const float* node_terms, int batch, int n,
                      int w, int d, void* xlin, float* s_i, float* s_j, hipStream_t stream) {
  if (!gdn_dense_supported(n, w, d, 1)) return GDN_ERR_UNSUPPORTED;
  PArgs a = {x, lin_w, node_terms, batch, n, w, xlin, s_i, s_j};
  switch ((n + 1 + 31) / 32) {
    case 1: return is_bf16 ? launch_project<1, FMT_BF16>(a, stream) : launch_project<1, FMT_F16>(a, stream);
    case 2: return is_bf16 ? launch_project<2, FMT_BF16>(a, stream) : launch_project<2, FMT_F16>(a, stream);
    case 3: return is_bf16 ? launch_project<3, FMT_BF16>(a, stream) : launch_project<3, FMT_F16>(a, stream);
    case 4: return is_bf16 ? launch_project<4, FMT_BF16>(a, stream) : launch_project<4, FMT_F16>(a, stream);
  }
  return GDN_ERR_UNSUPPORTED;
}

template <int NT, int SL>
static int launch_attn_bwd(const BwArgs& a, hipStream_t stream) {
  using C = BwCfg<NT, SL>;
  static_assert(C::LDS <= 160 * 1024, "LDS plan exceeds one CU");
  auto kern = gdn_dense_attn_bwd_kernel<NT, SL>;
  const int occ = blocks_per_cu(reinterpret_cast<const void*>(kern), C::THREADS, C::LDS);
  const int grid = max(1, min(min(a.batch, cu_count() * occ), GDN_COLSUM_MAX_ROWS));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(C::THREADS), C::LDS, stream, a);
  return gdn_launch_status();
}

template <int NT>
static int attn_bwd_select_sl(const BwArgs& a, hipStream_t st) {
  switch (a.pitch) {
    case 16: return launch_attn_bwd<NT, 8>(a, st);
    case 32: return launch_attn_bwd<NT, 16>(a, st);
    case 48: return launch_attn_bwd<NT, 24>(a, st);
    case 64: return launch_attn_bwd<NT, 32>(a, st);
  }
  return GDN_ERR_UNSUPPORTED;
}

int gdn_dense_attn_bwd(const float* d_z, const float* xlin, const float* alpha, const float* s_i, const float* s_j,
                       const uint16_t* nbr, int batch, int n, int k, float* d_xlin, float* d_si, float* d_sj,
                       float* d_bias, float* bias_ws, hipStream_t stream) {
  if (!gdn_dense_supported(n, 1, 64, k)) return GDN_ERR_UNSUPPORTED;
  BwArgs a = {d_z, xlin, alpha, s_i, s_j, nbr, batch, n, gdn_nbr_pitch(k), d_xlin, d_si, d_sj, d_bias, bias_ws};
  switch ((n + 1 + 31) / 32) {
    case 1: return attn_bwd_select_sl<1>(a, stream);
    case 2: return attn_bwd_select_sl<2>(a, stream);
    case 3: return attn_bwd_select_sl<3>(a, stream);
    case 4: return attn_bwd_select_sl<4>(a, stream);
  }
  return GDN_ERR_UNSUPPORTED;
}

int gdn_dense_attn_aggregate(const void* xlin, int is_bf16, const float* s_i, const float* s_j, const uint16_t* nbr,
                             const float* bias, int batch, int n, int d, int k, void* z, float* alpha,
                             hipStream_t stream) {
  if (!gdn_dense_supported(n, 1, d, k)) return GDN_ERR_UNSUPPORTED;
  KArgs a = {};
  a.xlin = xlin; a.si = s_i; a.sj = s_j; a.nbr = nbr; a.bias = bias;
  a.batch = batch; a.n = n; a.pitch = gdn_nbr_pitch(k); a.z = z; a.alpha = alpha;
  if (is_bf16) return alpha ? attn_select_nt<FMT_BF16, true>(a, stream) : attn_select_nt<FMT_BF16, false>(a, stream);
  return alpha ? attn_select_nt<FMT_F16, true>(a, stream) : attn_select_nt<FMT_F16, false>(a, stream);
}

// Shapes the dense matrix-core path takes: n <= 127, w <= 32, list pitch <= 64 (k <= 63); d = 64 for the
// staged kernels, d = 64 or 128 for the fused one.
bool gdn_dense_supported(int n, int w, int d, int k) {
  return n >= 1 && n <= 127 && d == 64 && w >= 1 && w <= 32 && k >= 1 && k <= n && gdn_nbr_pitch(k) <= 64;
}
bool gdn_dense_fused_supported(int n, int w, int d, int k) {
  return gdn_dense_supported(n, w, 64, k) && (d == 64 || d == 128);
}

static int fused_dispatch(int op, const DArgs& a, int bf16, unsigned* plan_out, long long* bytes, hipStream_t st) {
  if (a.d == 128) return gdn_dense_fused_op_d128(op, &a, bf16, plan_out, bytes, st);
  return bf16 ? select_nt<FMT_BF16, 2>(op, a, plan_out, bytes, st) : select_nt<FMT_F16, 2>(op, a, plan_out, bytes, st);
}

int gdn_dense_forward_fused(const void* x, int x_is_bf16, int series_len, int series_first, const float* lin_w,
                            const float* node_terms, const uint16_t* nbr, const float* gnn_bias,
                            const float* emb, const float* bn1, const float* bn2, const float* out_w,
                            const float* out_b, int batch, int n, int w, int d, int k, float* out,
                            hipStream_t stream) {
  if (!gdn_dense_fused_supported(n, w, d, k)) return GDN_ERR_UNSUPPORTED;
  DArgs a = {};
  a.x = x; a.series_len = series_len; a.series_first = series_first;
  a.batch = batch; a.n = n; a.w = w; a.pitch = gdn_nbr_pitch(k); a.d = d;
  a.lin_w = lin_w; a.node_terms = node_terms; a.nbr = nbr; a.gnn_bias = gnn_bias; a.emb = emb;
  a.bn1 = bn1; a.bn2 = bn2; a.out_w = out_w; a.out_b = out_b; a.out = out;
  return fused_dispatch(DOP_LAUNCH, a, x_is_bf16, nullptr, nullptr, stream);
}

#ifdef GDN_STAMPS
extern "C" int gdn_debug_read_stamps(unsigned long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dense_stamps), sizeof(g_dense_stamps)) == hipSuccess ? 0 : -2;
}
#endif

// ---- bank-ordered neighbour lists (C ABI: include/gdn_hip.h) -------------------------------------------
template <int NT>
static int bank_order_select_sl(const uint16_t* nbr, int n, int pitch, uint16_t* out, hipStream_t st) {
  switch (pitch) {
    case 16: hipLaunchKernelGGL((gdn_bank_order_kernel<NT, 8>), dim3(1), dim3(64 * NT), 0, st, nbr, n, pitch, out); break;
    case 32: hipLaunchKernelGGL((gdn_bank_order_kernel<NT, 16>), dim3(1), dim3(64 * NT), 0, st, nbr, n, pitch, out); break;
    case 48: hipLaunchKernelGGL((gdn_bank_order_kernel<NT, 24>), dim3(1), dim3(64 * NT), 0, st, nbr, n, pitch, out); break;
    case 64: hipLaunchKernelGGL((gdn_bank_order_kernel<NT, 32>), dim3(1), dim3(64 * NT), 0, st, nbr, n, pitch, out); break;
    default: return GDN_ERR_UNSUPPORTED;
  }
  return gdn_launch_status();
}

extern "C" int gdn_graph_bank_order(const uint16_t* nbr, int n, int k, uint16_t* nbr_ordered, void* stream) {
  if (!nbr || !nbr_ordered || n <= 0 || k <= 0) return GDN_ERR_ARG;
  if (!gdn_dense_supported(n, 1, 64, k)) return GDN_ERR_UNSUPPORTED;
  const int pitch = gdn_nbr_pitch(k);
  hipStream_t st = (hipStream_t)stream;
  switch ((n + 1 + 31) / 32) {
    case 1: return bank_order_select_sl<1>(nbr, n, pitch, nbr_ordered, st);
    case 2: return bank_order_select_sl<2>(nbr, n, pitch, nbr_ordered, st);
    case 3: return bank_order_select_sl<3>(nbr, n, pitch, nbr_ordered, st);
    case 4: return bank_order_select_sl<4>(nbr, n, pitch, nbr_ordered, st);
  }
  return GDN_ERR_UNSUPPORTED;
}

// ---- plans (C ABI: include/gdn_hip.h) -----------------------------------------------------------------
extern "C" long long gdn_fused_plan_bytes(int n, int w, int d, int k, int bf16_storage) {
  if (!gdn_dense_fused_supported(n, w, d, k)) return 0;
  DArgs a = {};
  a.n = n; a.w = w; a.d = d; a.pitch = gdn_nbr_pitch(k);
  long long bytes = 0;
  const int rc = fused_dispatch(DOP_PLAN_BYTES, a, bf16_storage, nullptr, &bytes, nullptr);
  return rc == GDN_OK ? bytes : 0;
}

extern "C" int gdn_fused_plan_build(const float* lin_w, const float* node_terms, const uint16_t* nbr,
                                    const int32_t* deg, const float* gnn_bias, const float* emb,
                                    const float* bn1_affine, const float* bn2_affine, const float* out_w,
                                    const float* out_b, int n, int w, int d, int k, int bf16_storage,
                                    void* plan, void* stream) {
  if (!lin_w || !node_terms || !nbr || !deg || !gnn_bias || !emb || !bn1_affine || !bn2_affine || !out_w ||
      !out_b || !plan)
    return GDN_ERR_ARG;
  if (!gdn_dense_fused_supported(n, w, d, k)) return GDN_ERR_UNSUPPORTED;
  DArgs a = {};
  a.n = n; a.w = w; a.d = d; a.pitch = gdn_nbr_pitch(k);
  a.lin_w = lin_w; a.node_terms = node_terms; a.nbr = nbr; a.gnn_bias = gnn_bias; a.emb = emb;
  a.bn1 = bn1_affine; a.bn2 = bn2_affine; a.out_w = out_w; a.out_b = out_b;
  unsigned* p = reinterpret_cast<unsigned*>(plan);
  return fused_dispatch(DOP_PLAN_BUILD, a, bf16_storage, p, nullptr, (hipStream_t)stream);
}

static int fused_with_plan(const void* x, int series_len, int first, const void* plan, int batch, int n, int w,
                           int d, int k, int bf16_storage, float* out, void* stream, const float* key_gt = nullptr,
                           double* keys = nullptr, int key_pitch = 0, int* range_guard = nullptr) {
  if (!x || !plan || !out) return GDN_ERR_ARG;
  if (batch <= 0 || n <= 0) return GDN_ERR_ARG;
  if (keys && (!key_gt || key_pitch < batch)) return GDN_ERR_ARG;
  if (!gdn_dense_fused_supported(n, w, d, k)) return GDN_ERR_UNSUPPORTED;
  DArgs a = {};
  a.x = x; a.series_len = series_len; a.series_first = first;
  a.batch = batch; a.n = n; a.w = w; a.pitch = gdn_nbr_pitch(k); a.d = d;
  a.out = out; a.plan = reinterpret_cast<const unsigned*>(plan);
  a.key_gt = key_gt; a.keys = keys; a.key_pitch = key_pitch;
  a.range_flag = bf16_storage ? nullptr : range_guard;
  return fused_dispatch(DOP_LAUNCH, a, bf16_storage, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int gdn_forward_fused_plan(const void* x, const void* plan, int batch, int n, int w, int d, int k,
                                      int bf16_storage, float* out, int* range_guard, void* stream) {
  return fused_with_plan(x, 0, 0, plan, batch, n, w, d, k, bf16_storage, out, stream, nullptr, nullptr, 0, range_guard);
}

extern "C" int gdn_forward_fused_series_plan(const float* series, int series_len, int first, const void* plan,
                                             int batch, int n, int w, int d, int k, float* out, int* range_guard,
                                             void* stream) {
  if (series_len <= 0 || first < 0 || (long long)first + batch - 1 + w > series_len) return GDN_ERR_ARG;
  return fused_with_plan(series, series_len, first, plan, batch, n, w, d, k, 0, out, stream, nullptr, nullptr, 0,
                         range_guard);
}

// the x limit of a plan, as a byte offset into it (the host reads one float there, once)
extern "C" long long gdn_fused_plan_limit_offset(int n, int w, int d, int k, int bf16_storage) {
  const long long bytes = gdn_fused_plan_bytes(n, w, d, k, bf16_storage);
  return bytes > 0 ? bytes - 4 : -1;
}

// The same two launches, also leaving the scoring keys |out - gt| (float64, [n, key_pitch], key_pitch >= batch)
extern "C" int gdn_forward_fused_plan_keys(const void* x, const void* plan, const float* gt, double* keys,
                                           int key_pitch, int batch, int n, int w, int d, int k, int bf16_storage,
                                           float* out, void* stream) {
  if (!gt || !keys) return GDN_ERR_ARG;
  return fused_with_plan(x, 0, 0, plan, batch, n, w, d, k, bf16_storage, out, stream, gt, keys, key_pitch);
}

extern "C" int gdn_forward_fused_series_plan_keys(const float* series, int series_len, int first, const void* plan,
                                                  const float* gt, double* keys, int key_pitch, int batch, int n,
                                                  int w, int d, int k, float* out, void* stream) {
  if (!gt || !keys) return GDN_ERR_ARG;
  if (series_len <= 0 || first < 0 || (long long)first + batch - 1 + w > series_len) return GDN_ERR_ARG;
  return fused_with_plan(series, series_len, first, plan, batch, n, w, d, k, 0, out, stream, gt, keys, key_pitch);
}
#endif  // GDN_DENSE_EXTRA_DC
