// Modal-Adapter attention cores (heads x HD, HD in {16, 32, 64}, E = heads * HD; 12 x 16 = 192 in both shipped configurations):
//   inject  : every patch row attends over the T <= 128 modal tokens of its pass       (AM:225-229 in AM:359-369)
//   extract : the T modal tokens attend over the L patch rows of their pass (split-L)   (AM:225-229 in AM:321-335)
//   token   : T x T self-attention among the modal tokens                               (AM:87)
// These are tiny-FLOP, HBM/latency-bound ops; they run on the VALU in fp32 with the small operand (the token
// side) resident in LDS, one streaming pass over the patch-side operand.
#include <cstddef>
#include <type_traits>

#include "common.h"

namespace {

constexpr int TMAX = 128;

// The cores are templated on the head dim HD and on HC, the head count when it is known at compile time (12: the shipped
// configuration, whose <16, 12> instantiations are the code this file held before the template) or 0 (`heads` is a kernel argument).
// What follows from HD:
//   NC  16-wide chunks of the head dim: a score block S = Q . K^T is a chain of NC v_mfma_f32_32x32x16_f16 on ONE accumulator
//       (a single accumulation chain of this instruction needs no interleaving);
//   NA  32-row output tiles of a transposed product with HD rows (O^T = V^T . P^T, dQ^T, dK^T, dV^T, phase-2 columns): one
//       accumulator at 16 (half of it unused) and 32, two at 64;  NG of its four 4-row groups per lane hold real rows;
//   KP  halves per row of a row-read fp16 image ([token][HD], 16-byte reads): HD + 8, i.e. 12 / 20 / 36 dwords = 4 x odd, so the sixteen
//       rows of a ds_read_b128 lane group start on sixteen different 16-byte slots of the 64-bank row;
//   TPV halves per row of a transposed image [HD][tokens] (8-byte reads, banked per 32-lane half): 68 dwords at HD = 16 (sixteen distinct
//       rows, 4 banks apart), 66 dwords at HD >= 32 (thirty-two distinct rows, 2 banks apart: each 8-byte read on its own bank pair);
//   VP  halves per row of the extractor forward's wave-private V block [32 keys][HD] (ds_read_b64_tr_b16: a 32-lane half reads four key
//       rows x 16 dwords): 12 dwords at 16; 16 dwords at 32 and 48 at 64, so the four rows land on the four quarters of the bank row.
template <int HD>
struct AdDim {
  static_assert(HD == 16 || HD == 32 || HD == 64, "adapter head dim");
  static constexpr int NC = HD / 16, NA = (HD + 31) / 32, NG = HD == 16 ? 2 : 4;
  static constexpr int KP = HD + 8;
  static constexpr int TPV = HD == 16 ? TMAX + 8 : TMAX + 4;
  static constexpr int VP = HD == 16 ? 24 : HD == 32 ? 32 : 96;
  static constexpr float SCALE = HD == 16 ? 0.25f : HD == 32 ? 0.17677669529663687f : 0.125f;   // 1/sqrt(HD)
};
// q / sqrt(HD) as an fp16 MFMA operand (extractor forward, backward and maps, which must agree to the bit): the fp32 product, rounded
// to fp16.  1/sqrt(32) is no power of two, and under -ffp-contract the compiler folds product and conversion into one v_fma_mixlo_f16,
// which rounds the EXACT product once -- about one value in 2^13 comes out one fp16 ulp away from fp32-then-fp16, enough to move a
// map entry by 3e-4 against a recomputation from the operands.  The empty asm pins the fp32 product at HD = 32 (16 and 64 scale by a
// power of two: exact either way, code unchanged).
template <int HD>
MT_DEVINL h16 scaled_h16(float x) {
  float p = x * AdDim<HD>::SCALE;
  if constexpr (HD == 32) asm volatile("" : "+v"(p));
  return (h16)p;
}
#define AD_DIMS                                                                                                          \
  using Dm = AdDim<HD>;                                                                                                  \
  constexpr int AD = HD, NC = Dm::NC, NA = Dm::NA, NG = Dm::NG, KP = Dm::KP, TPV = Dm::TPV;                              \
  constexpr float ASCALE = Dm::SCALE;                                                                                    \
  (void)NC; (void)NA; (void)NG; (void)KP; (void)TPV; (void)ASCALE;                                                       \
  const int AH = HC ? HC : heads, AE = AH * AD

// ---------------------------------------------------------------- shared stages ------------------
// The MFMA kernels below (injector, extractor, maps) are sequences of these stages; each states its register layout here, once.
// Every function that reads LDS reads ONE banking class (common.h): 16-byte rows, or 8-byte halves of a transposed image.
//
// Lane coordinates of a 256-thread workgroup: four waves; hh = the lane's 32-lane half, l31 = its row (A operand) / column (B operand
// and accumulator) of a 32 x 32 tile; drow = the row of a [HD][.] image it reads as an A operand (at HD = 16 lanes 16..31 of a half
// re-read rows 0..15: they fill the unused rows 16..31 of the accumulator).
#define AD_LANE                                                                                                          \
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, l31 = lane & 31;                        \
  const int drow = HD == 16 ? (l31 & 15) : l31;                                                                          \
  (void)wave; (void)drow
// v_mfma_f32_32x32x16_f16: A and B operands hold k = 8 hh .. 8 hh + 7 of row / column l31; element i of the accumulator is
// row acc_row(i, hh) of column l31 -- four groups of four consecutive rows, 8 apart, the upper half of the wave 4 further.
MT_DEVINL int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }
MT_DEVINL void zero(f32x16& a) {
#pragma unroll
  for (int i = 0; i < 16; ++i) a[i] = 0.f;
}
template <int N>
MT_DEVINL void zero(f32x16 (&a)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) zero(a[j]);
}
template <int N, int M>
MT_DEVINL void zero(f32x16 (&a)[N][M]) {
#pragma unroll
  for (int j = 0; j < N; ++j) zero(a[j]);
}
MT_DEVINL h16x8 cat8h(h16x4 lo, h16x4 hi) { return (h16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}; }
// B operands of one fp16 global row: frag[c] = dims 16 c + 8 hh .. + 7 (p already points at dim 8 hh); zero for a row out of range
template <int NC>
MT_DEVINL void row_frags(const h16* p, bool valid, h16x8 (&frag)[NC]) {
  const h16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < NC; ++c) frag[c] = valid ? ldg8(p + 16 * c) : zero8;
}
// Score chain: acc += A . B over the head dim, A = row `row` (32 tb + l31) of an fp16 row image [.][KP] in LDS (one 16-byte read per
// 16-dim chunk), B = the register fragments of row_frags; NC MFMAs on the one accumulator.
template <int HD>
MT_DEVINL void score_chain(const h16* img, int row, int hh, const h16x8 (&frag)[AdDim<HD>::NC], f32x16& acc) {
#pragma unroll
  for (int c = 0; c < AdDim<HD>::NC; ++c) {
    const h16x8 af = *reinterpret_cast<const h16x8*>(&img[row * AdDim<HD>::KP + 16 * c + 8 * hh]);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, frag[c], acc, 0, 0, 0);
  }
}
// A operand from a transposed fp16 image [HD][TPV]: row 32 j + drow, k = tokens tok + {0..3} and tok + 8 + {0..3} with
// tok = 32 tb + 16 s2 + 4 hh -- the accumulator-order permutation of k, so that elements 8 s2 .. 8 s2 + 7 of a score accumulator are
// the matching B operand as they stand (two 8-byte reads).
template <int HD>
MT_DEVINL h16x8 tr_frag(const h16* img, int j, int drow, int tok) {
  const h16* p = &img[(32 * j + drow) * AdDim<HD>::TPV + tok];
  return cat8h(*reinterpret_cast<const h16x4*>(p), *reinterpret_cast<const h16x4*>(p + 8));
}
// Initial accumulator from a per-token fp32 vector in LDS (vec points at token 32 tb): element i = vec[acc_row(i, hh)], four 16-byte reads
MT_DEVINL f32x16 acc_from_rows(const float* vec, int hh) {
  f32x16 a;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(&vec[8 * g4 + 4 * hh]);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[4 * g4 + e] = x[e];
  }
  return a;
}
// Store of a [dim][row] accumulator tile (O^T, dQ^T, dK^T, dV^T) to the lane's fp16 row: rows d = 32 j + acc_row(i, hh) (i < 8 at
// HD = 16), so group g of accumulator j is the four consecutive dims 32 j + 8 g + 4 hh .. + 3: one 8-byte store.  scale: the injector
// forward's 1 / l, applied as an fp32 product before the rounding; the other callers leave it at 1 (exact, folded away).
template <int HD>
MT_DEVINL void store_dim_tile(h16* dst, const f32x16 (&acc)[AdDim<HD>::NA], int hh, float scale = 1.f) {
#pragma unroll
  for (int j = 0; j < AdDim<HD>::NA; ++j)
#pragma unroll
    for (int g = 0; g < AdDim<HD>::NG; ++g)
      *reinterpret_cast<h16x4*>(dst + 32 * j + 8 * g + 4 * hh) = (h16x4){(h16)(acc[j][4 * g] * scale), (h16)(acc[j][4 * g + 1] * scale),
                                                                        (h16)(acc[j][4 * g + 2] * scale), (h16)(acc[j][4 * g + 3] * scale)};
}
// Staging of the token-side operand: G heads of tokens 0 .. NT - 1 of an fp32 [T][AE] operand (src at the pass's token 0, first head
// of the group) go to LDS as fp16 -- to a row image row[G][NT][KP], to a transposed image tr[HD][TPV] (G = 1), or both; zero past T.
// An image that is not wanted is passed as the literal nullptr: its TYPE switches the store off at compile time.  One loop stages up to
// two operands (their loads overlap).  SCALED: operand a goes through scaled_h16 (the extractor's q).
template <class R, class C>
struct TokOp {
  const float* src; R row; C tr;
  static constexpr bool ROW = !std::is_same_v<R, std::nullptr_t>, TR = !std::is_same_v<C, std::nullptr_t>;
};
template <class R, class C>
MT_DEVINL TokOp<R, C> tok_op(const float* src, R row, C tr) { return {src, row, tr}; }
using NoTokOp = TokOp<std::nullptr_t, std::nullptr_t>;
template <int HD, bool SCALED = false, class A, class B = NoTokOp>
MT_DEVINL void stage_token_rows(int tid, int T, int NT, int AE, int G, A a, B b = {nullptr, nullptr, nullptr}) {
  const int GE = G * HD;
  for (int i = tid; i < NT * GE; i += 256) {
    const int t = i / GE, e = i % GE;
    const bool ok = t < T;
    const int ro = ((e / HD) * NT + t) * AdDim<HD>::KP + e % HD, to = (e % HD) * AdDim<HD>::TPV + t;
    const float xa = ok ? a.src[(long)t * AE + e] : 0.f;
    const h16 ha = SCALED ? scaled_h16<HD>(xa) : (h16)xa;
    if constexpr (A::ROW) a.row[ro] = ha;
    if constexpr (A::TR) a.tr[to] = ha;
    if constexpr (B::ROW || B::TR) {
      const h16 hb = (h16)(ok ? b.src[(long)t * AE + e] : 0.f);
      if constexpr (B::ROW) b.row[ro] = hb;
      if constexpr (B::TR) b.tr[to] = hb;
    }
  }
}

// ---------------------------------------------------------------- injector -----------------------
// forward on MFMA: grid (ceil(rows/128), heads, B passes); wave = 32 patch rows (row = lane & 31).  With d = 16 one
// v_mfma_f32_32x32x16_f16 is a whole 32-token x 32-row score block (a chain of 2 / 4 at d = 32 / 64): S^T = K . Q^T (K rows from an fp16 LDS image, Q^T
// straight from global memory), softmax lane-local (row = lane, tokens in registers + one cross-half shuffle),
// O^T += V^T . P^T with P^T taken from the score accumulators (V^T from a transposed fp16 LDS image).
template <int HD, int HC>
__global__ __launch_bounds__(256) void inject_attn_fwd_kernel(const h16* __restrict__ q, int rows_per_pass, const float* __restrict__ k,
                                                              const float* __restrict__ v, int T, int heads, h16* __restrict__ a,
                                                              float* __restrict__ lse) {
  AD_DIMS;
  AD_LANE;
  __shared__ __attribute__((aligned(16))) h16 ksh[TMAX * KP];     // K[t][d]
  __shared__ __attribute__((aligned(16))) h16 vT[AD * TPV];       // V^T[d][t]
  const int h = blockIdx.y, b = blockIdx.z;
  const long tok0 = (long)b * T * AE + h * AD;
  stage_token_rows<HD>(tid, T, TMAX, AE, 1, tok_op(k + tok0, ksh, nullptr), tok_op(v + tok0, nullptr, vT));
  __syncthreads();
  const int ntb = (T + 31) / 32;
  const int r = blockIdx.x * 128 + wave * 32 + l31;
  const bool valid = r < rows_per_pass;
  const long m = (long)b * rows_per_pass + (valid ? r : 0);
  h16x8 qf[NC];                                                               // B operands: Q^T[d = 16 c + 8 hh + j][row]
  row_frags(q + m * AE + h * AD + 8 * hh, valid, qf);
  f32x16 sc[TMAX / 32];
  float mx = -1.0e30f;
#pragma unroll
  for (int tb = 0; tb < TMAX / 32; ++tb) {
    if (tb < ntb) {
      zero(sc[tb]);
      score_chain<HD>(ksh, tb * 32 + l31, hh, qf, sc[tb]);
#pragma unroll
      for (int i = 0; i < 16; ++i) {      // accumulator rows are tokens
        if (tb * 32 + acc_row(i, hh) >= T) sc[tb][i] = -1.0e30f;
        mx = fmaxf(mx, sc[tb][i]);
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float c = ASCALE * 1.4426950408889634f;
  f32x16 acc[NA];
  zero(acc);
  float l = 0.f;
#pragma unroll
  for (int tb = 0; tb < TMAX / 32; ++tb) {
    if (tb < ntb) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        h16x8 pf;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float pv = __builtin_amdgcn_exp2f((sc[tb][8 * s2 + e] - mx) * c);
          l += pv;
          pf[e] = (h16)pv;
        }
#pragma unroll
        for (int j = 0; j < NA; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tr_frag<HD>(vT, j, drow, tb * 32 + 16 * s2 + 4 * hh), pf, acc[j], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 32, 64);
  if (valid) {
    store_dim_tile<HD>(a + m * AE + h * AD, acc, hh, 1.0f / l);      // O^T
    if (lse && hh == 0) lse[m * AH + h] = mx * ASCALE + __logf(l);
  }
}

// backward: workgroup = 4 waves = ITILES x 128 rows of one (pass, head); everything on MFMA.
// Phase 1 (wave = 32 rows, row = lane): S^T = K . Q^T and dP^T = V . dA^T (a chain of HD / 16 32x32x16 MFMAs per 32-token block
// each), p = exp(s/sqrt(HD) - lse) (lse saved by the forward, same fp16 K), delta = a . da (flash identity), ds = p (dp - delta) / sqrt(HD),
// dQ^T += K^T . dS^T with dS^T taken from the accumulators; p / ds / q / da go to LDS TRANSPOSED ([token][row], [dim][row]).
// Phase 2: dk[t,d] += sum_rows ds[row,t] q[row,d] and dv[t,d] += sum_rows p[row,t] da[row,d] are 32x32x16 products with
// the row index as the reduction dimension -- both operands are plain 16-byte row reads of the transposed images
// (wave w: product w & 1, token blocks w >> 1 and (w >> 1) + 2).  The accumulators live across the row tiles: one
// atomic per (token, dim) per workgroup at the very end.  At HD = 64 the two phase-2 accumulators per token block double (dims 0..31
// and 32..63).  LDS at T = 128: 93 / 113 / 155 KiB at HD = 16 / 32 / 64; at T = 65: 56 / 75 / 112 KiB (two workgroups per CU at 16 and
// 32, one at 64).
constexpr int IBR = 128, ITILES = 4, RSTR = IBR + 8;   // RSTR: halves per transposed row (272 B: conflict-free b128)
constexpr int LDS_MAX = 160 * 1024;
// The LDS layout of each dynamic-LDS kernel is ONE struct, built as Lds{run-time arguments} by the kernel (which takes its pointers
// from the offsets) and by the launcher (which allocates bytes()): the two cannot drift apart.  Each member is the offset of an image in
// elements of the image's own type from the start of the allocation, computed from the members before it.
constexpr int tok_blocks(int T) { return (T + 31) / 32 * 32; }      // TB: T up to whole 32-token blocks
template <int HD>
struct InjectBwdLds {      // halves
  int T, TB = tok_blocks(T);
  int ksh = 0;                                  // [TB][KP]   K rows
  int vsh = ksh + TB * AdDim<HD>::KP;           // [TB][KP]   V rows
  int kT = vsh + TB * AdDim<HD>::KP;            // [HD][TPV]  K^T
  int psT = kT + HD * AdDim<HD>::TPV;           // [T][RSTR]
  int dssT = psT + T * RSTR;                    // [T][RSTR]
  int qT = dssT + T * RSTR;                     // [HD][RSTR]
  int daT = qT + HD * RSTR;                     // [HD][RSTR]
  int end = daT + HD * RSTR;
  constexpr size_t bytes() const { return sizeof(h16) * (size_t)end; }
};
// Phase 2 of both backward kernels, one 128-row tile: acc[j] += A . B with the tile's row index as the reduction dimension, A = row
// trow of a transposed image [tokens][RSTR] (ds or p), B = rows 32 j + drow of a transposed image [HD][RSTR] (q, da or k); 16-byte
// reads of both.  Accumulator rows are tokens, columns dims.
template <int HD>
MT_DEVINL void rowtile_product(const h16* A, int trow, const h16* B, int drow, int hh, f32x16 (&acc)[AdDim<HD>::NA]) {
#pragma unroll
  for (int kk = 0; kk < IBR / 16; ++kk) {
    const h16x8 afr = *reinterpret_cast<const h16x8*>(&A[trow * RSTR + kk * 16 + hh * 8]);
#pragma unroll
    for (int j = 0; j < AdDim<HD>::NA; ++j) {
      const h16x8 bfr = *reinterpret_cast<const h16x8*>(&B[(32 * j + drow) * RSTR + kk * 16 + hh * 8]);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(afr, bfr, acc[j], 0, 0, 0);
    }
  }
}
// The close of both backward kernels: the phase-2 accumulators of token block tb (rows = tokens 32 tb + acc_row(i, hh), column = dim
// 32 j + l31, 16 valid at HD = 16) go to the head's columns of the pass's [T][AE] block of dst [B][T][AE] -- one atomic per (token, dim);
// DET: of the partial workspace [gridDim.x][B][T][AE], slot blockIdx.x, with plain stores.
template <bool DET>
MT_DEVINL long flush_pass(int b) { return DET ? (long)blockIdx.x * gridDim.z + b : b; }
template <int HD, bool DET>
MT_DEVINL void flush_token_dim(float* dst, const f32x16 (&acc)[AdDim<HD>::NA], int tb, int T, int AE, int hh, int l31) {
  if (HD == 16 && l31 >= HD) return;
#pragma unroll
  for (int j = 0; j < AdDim<HD>::NA; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = tb * 32 + acc_row(i, hh);
      float* p = &dst[(long)t * AE + 32 * j + l31];
      if constexpr (DET) {
        if (t < T) *p = acc[j][i];
      } else {
        if (t < T) atomicAdd(p, acc[j][i]);
      }
    }
}
// DET (deterministic mode, det_reduce.hip): dk / dv are partial workspaces [gridDim.x][B][T][E]; the workgroup stores its sums to slot
// blockIdx.x (its row block) with plain stores -- every (t < T, column) of a slot is owned by one lane of one (head, pass) workgroup.
template <int HD, int HC, bool DET = false>
__global__ __launch_bounds__(256) void inject_attn_bwd_kernel(const h16* __restrict__ q, const h16* __restrict__ a,
                                                              const float* __restrict__ lse, const h16* __restrict__ da,
                                                              int rows_per_pass, const float* __restrict__ k,
                                                              const float* __restrict__ v, int T, int heads, h16* __restrict__ dq,
                                                              float* __restrict__ dk, float* __restrict__ dv) {
  AD_DIMS;
  AD_LANE;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ntb = (T + 31) / 32, TB = ntb * 32;
  const InjectBwdLds<HD> lds{T};
  h16* sh = reinterpret_cast<h16*>(smem);
  h16 *ksh = sh + lds.ksh, *vsh = sh + lds.vsh, *kT = sh + lds.kT, *psT = sh + lds.psT, *dssT = sh + lds.dssT, *qT = sh + lds.qT,
      *daT = sh + lds.daT;
  const int h = blockIdx.y, b = blockIdx.z;
  const long tok0 = (long)b * T * AE + h * AD;
  stage_token_rows<HD>(tid, T, TB, AE, 1, tok_op(k + tok0, ksh, kT), tok_op(v + tok0, vsh, nullptr));
  f32x16 acc[TMAX / 64][NA];        // phase 2: token blocks (wave >> 1) and (wave >> 1) + 2 of product (wave & 1), dims 32 j2 + lane
  zero(acc);
  const float c = ASCALE * 1.4426950408889634f;
  __syncthreads();
  for (int tile = 0; tile < ITILES; ++tile) {
    const int r0 = (blockIdx.x * ITILES + tile) * IBR;
    if (r0 >= rows_per_pass) break;                   // uniform
    const int rl = wave * 32 + l31;                   // row inside the tile
    const int r = r0 + rl;
    const bool valid = r < rows_per_pass;
    const long m = (long)b * rows_per_pass + (valid ? r : 0);
    h16x8 qf[NC], daf[NC];
    row_frags(q + m * AE + h * AD + 8 * hh, valid, qf);
    row_frags(da + m * AE + h * AD + 8 * hh, valid, daf);
    const float nl2 = valid ? -lse[m * AH + h] * 1.4426950408889634f : -1.0e30f;
    float delta = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const h16x8 af = ldg8(a + m * AE + h * AD + 16 * c + 8 * hh);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        delta = fmaf((float)af[e], (float)daf[c][e], delta);
        qT[(16 * c + 8 * hh + e) * RSTR + rl] = qf[c][e];
        daT[(16 * c + 8 * hh + e) * RSTR + rl] = daf[c][e];
      }
    }
    delta += __shfl_xor(delta, 32, 64);
    f32x16 dqa[NA];
    zero(dqa);
#pragma unroll
    for (int tb = 0; tb < TMAX / 32; ++tb) {
      if (tb < ntb) {
        f32x16 sc, dpv;
        zero(sc);
        zero(dpv);
        score_chain<HD>(ksh, tb * 32 + l31, hh, qf, sc);
        score_chain<HD>(vsh, tb * 32 + l31, hh, daf, dpv);
        h16x8 dsf[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int t = tb * 32 + acc_row(i, hh);      // accumulator rows are tokens
          const float pv = t < T ? __builtin_amdgcn_exp2f(fmaf(sc[i], c, nl2)) : 0.f;
          const float ds = pv * (dpv[i] - delta) * ASCALE;
          dsf[i >> 3][i & 7] = (h16)ds;
          if (t < T) {
            psT[t * RSTR + rl] = (h16)pv;
            dssT[t * RSTR + rl] = (h16)ds;
          }
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
          for (int j = 0; j < NA; ++j)
            dqa[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tr_frag<HD>(kT, j, drow, tb * 32 + 16 * s2 + 4 * hh), dsf[s2], dqa[j], 0, 0, 0);
      }
    }
    if (valid) store_dim_tile<HD>(dq + m * AE + h * AD, dqa, hh);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TMAX / 64; ++j) {
      const int tb = (wave >> 1) + 2 * j;
      // rows >= T: valid memory, results never flushed
      if (tb < ntb) rowtile_product<HD>((wave & 1) ? psT : dssT, min(tb * 32 + l31, T - 1), (wave & 1) ? daT : qT, drow, hh, acc[j]);
    }
    __syncthreads();
  }
  float* dst = ((wave & 1) ? dv : dk) + flush_pass<DET>(b) * T * AE + h * AD;
#pragma unroll
  for (int j = 0; j < TMAX / 64; ++j) {
    const int tb = (wave >> 1) + 2 * j;
    if (tb < ntb) flush_token_dim<HD, DET>(dst, acc[j], tb, T, AE, hh, l31);
  }
}

// ---------------------------------------------------------------- extractor ----------------------
// forward on MFMA: grid (nsplit, heads, B); 4 waves, wave w sweeps the 32-key blocks w, w + 4, ... of the split.
// S^T[key, token] = K . Q^T: K rows straight from global memory (A operand, key = lane & 31), Q^T (pre-scaled, fp16) in
// registers, a chain of HD / 16 32x32x16 MFMAs per 32-token block; online softmax lane-local (token = lane, keys in registers + one
// cross-half shuffle); O^T[d, token] += V^T . P^T with P^T from the accumulators and V^T read transposed
// (ds_read_b64_tr_b16) from a wave-private LDS copy of the 32 x HD V block.  The four waves' partials are merged
// through LDS into one partial per (split, token) for the reduce kernel below.  The merge image [4][T][HD + 2] fp32 is static at
// HD = 16 (36 KiB) and dynamic, sized by T, beyond (T = 128: 68 KiB at 32, 132 KiB at 64 -- one workgroup per CU there; the grid is
// nsplit x heads x B workgroups, about one per CU, so LDS does not set the occupancy of this kernel).
constexpr int EKT = 32, EFT = 256;
MT_DEVINL h16x4 ad_tr4(const h16* p) {
  s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4*)(__attribute__((address_space(3))) void*)p);
  return __builtin_bit_cast(h16x4, r);
}
// MT = the tokens the merge image is sized for: TMAX in the static form (HD = 16), T in the dynamic one
template <int HD>
struct ExtractFwdLds {
  static constexpr int VSH = 4 * 32 * AdDim<HD>::VP;      // halves: the waves' V blocks [4][32][VP], at offset 0
  static constexpr int MS = HD + 2;                       // floats per (wave, token) of the merge image: HD sums, m, l
  int MT, MW = MT * MS;                                   // floats per wave of the merge image
  int mrg = VSH / 2;                                      // floats: the merge image [4][MT][MS]
  constexpr size_t bytes() const { return sizeof(float) * ((size_t)mrg + 4 * (size_t)MW); }
};
template <int HD, int HC>
__global__ __launch_bounds__(EFT) void extract_attn_fwd_kernel(const float* __restrict__ q, const h16* __restrict__ kv, int T, int L, int heads,
                                                               int keys_per_split, float* __restrict__ part_acc, float* __restrict__ part_ml) {
  AD_DIMS;
  AD_LANE;
  using Lds = ExtractFwdLds<HD>;
  constexpr int VP = Dm::VP, MS = Lds::MS, NV = 4 * NG;      // NV: valid accumulator rows
  const Lds lds{HD == 16 ? TMAX : T};
  h16* vsh;                         // [4][32 * VP]
  float* mrg;                       // [4][MT][MS]
  if constexpr (HD == 16) {
    __shared__ __attribute__((aligned(16))) h16 vsh_s[Lds::VSH];
    __shared__ float mrg_s[4 * Lds{TMAX}.MW];
    vsh = vsh_s; mrg = mrg_s;
  } else {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    vsh = reinterpret_cast<h16*>(smem);
    mrg = smem + lds.mrg;
  }
  const int MW = lds.MW;                                    // floats per wave of the merge image
  const int sp = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int nsplit = gridDim.x;
  const int li = lane & 15, tq = li >> 2, tp = li & 3;
  const int ntb = (T + 31) / 32;
  h16x8 qf[TMAX / 32][NC];          // B operands: Q^T[d = 16 c + 8 hh + j][token]
  f32x16 acc[TMAX / 32][NA];
  float mrun[TMAX / 32], lrun[TMAX / 32];
  zero(acc);
#pragma unroll
  for (int tb = 0; tb < TMAX / 32; ++tb) {
    const int t = tb * 32 + l31;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[tb][c][e] = scaled_h16<HD>(t < T ? q[((long)b * T + t) * AE + h * AD + 16 * c + 8 * hh + e] : 0.f);
    mrun[tb] = -1.0e30f; lrun[tb] = 0.f;
  }
  const h16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const int kbeg = sp * keys_per_split, kend = min(L, kbeg + keys_per_split);
  h16* vw = vsh + wave * 32 * VP;
  const int dcol = HD == 16 ? 0 : 16 * (l31 >> 4);          // lanes 16..31 of a half transpose the next sixteen dims
  for (int k0 = kbeg + wave * EKT; k0 < kend; k0 += 4 * EKT) {
    const int key = k0 + l31;
    const bool valid = key < kend;
    const h16* row = kv + ((long)b * L + (valid ? key : kbeg)) * (2 * AE) + h * AD + 8 * hh;
    h16x8 kf[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      kf[c] = valid ? ldg8(row + 16 * c) : zero8;
      const h16x8 vf = valid ? ldg8(row + AE + 16 * c) : zero8;
      *reinterpret_cast<h16x8*>(&vw[l31 * VP + 16 * c + 8 * hh]) = vf;      // wave-private: no workgroup barrier needed
    }
    // V^T fragments (A operand of O^T += V^T . P^T), shared by the token blocks; at HD = 16 lanes >= 16 of a half produce the
    // unused d rows 16..31 from the same columns
    h16x8 vt[NA][2];
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const h16* vr = &vw[(s2 * 16 + 4 * hh + tq) * VP + 32 * j + dcol + 4 * tp];
        vt[j][s2] = cat8h(ad_tr4(vr), ad_tr4(vr + 8 * VP));
      }
#pragma unroll
    for (int tb = 0; tb < TMAX / 32; ++tb) {
      if (tb < ntb) {
        f32x16 sc;
        zero(sc);
#pragma unroll
        for (int c = 0; c < NC; ++c) sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[c], qf[tb][c], sc, 0, 0, 0);
        float mx = -1.0e30f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {      // accumulator rows are keys
          if (k0 + acc_row(i, hh) >= kend) sc[i] = -1.0e30f;
          mx = fmaxf(mx, sc[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(mrun[tb], mx);
        const float al = __expf(mrun[tb] - mn);
        float ls = 0.f;
        h16x8 pf[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float pv = __expf(sc[i] - mn);
          ls += pv;
          pf[i >> 3][i & 7] = (h16)pv;
        }
        ls += __shfl_xor(ls, 32, 64);
        lrun[tb] = lrun[tb] * al + ls;
        mrun[tb] = mn;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
#pragma unroll
          for (int i = 0; i < NV; ++i) acc[tb][j][i] *= al;
          acc[tb][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vt[j][0], pf[0], acc[tb][j], 0, 0, 0);
          acc[tb][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vt[j][1], pf[1], acc[tb][j], 0, 0, 0);
        }
      }
    }
  }
  // per-wave partials -> LDS: O^T rows d = 32 j + acc_row(i, hh) (i < 8 at HD = 16), column = token
#pragma unroll
  for (int tb = 0; tb < TMAX / 32; ++tb) {
    const int t = tb * 32 + l31;
    if (tb < ntb && t < T) {
      float* mr = mrg + wave * MW + t * MS;
#pragma unroll
      for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int i = 0; i < NV; ++i) mr[32 * j + acc_row(i, hh)] = acc[tb][j][i];
      if (hh == 0) { mr[AD] = mrun[tb]; mr[AD + 1] = lrun[tb]; }
    }
  }
  __syncthreads();
  if (tid < T) {
    const float* mt = mrg + tid * MS;
    float m2 = -1.0e30f;
    for (int wv = 0; wv < 4; ++wv) m2 = fmaxf(m2, mt[wv * MW + AD]);
    float l2 = 0.f, a2[AD];
#pragma unroll
    for (int d = 0; d < AD; ++d) a2[d] = 0.f;
    for (int wv = 0; wv < 4; ++wv) {
      const float wgt = __expf(mt[wv * MW + AD] - m2);
      l2 = fmaf(wgt, mt[wv * MW + AD + 1], l2);
#pragma unroll
      for (int d = 0; d < AD; ++d) a2[d] = fmaf(wgt, mt[wv * MW + d], a2[d]);
    }
    const long o = (((long)b * AH + h) * nsplit + sp) * T + tid;
#pragma unroll
    for (int d = 0; d < AD; ++d) part_acc[o * AD + d] = a2[d];
    part_ml[o * 2] = m2; part_ml[o * 2 + 1] = l2;
  }
}

template <int HD, int HC>
__global__ void extract_attn_reduce_kernel(const float* __restrict__ part_acc, const float* __restrict__ part_ml, int T, int nsplit, int heads,
                                           float* __restrict__ out, float* __restrict__ lse) {
  // grid (B * heads), block T threads (<=128): thread = token
  AD_DIMS;
  const int bh = blockIdx.x, b = bh / AH, h = bh % AH, t = threadIdx.x;
  if (t >= T) return;
  float mx = -1.0e30f;
  for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, part_ml[(((long)bh * nsplit + s) * T + t) * 2]);
  float l = 0.f, acc[AD];
#pragma unroll
  for (int d = 0; d < AD; ++d) acc[d] = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const long o = ((long)bh * nsplit + s) * T + t;
    const float w = __expf(part_ml[o * 2] - mx);
    l += w * part_ml[o * 2 + 1];
#pragma unroll
    for (int d = 0; d < AD; ++d) acc[d] = fmaf(w, part_acc[o * AD + d], acc[d]);
  }
  const float inv = 1.0f / l;
#pragma unroll
  for (int d = 0; d < AD; ++d) out[((long)b * T + t) * AE + h * AD + d] = acc[d] * inv;
  lse[((long)b * T + t) * AH + h] = mx + __logf(l);
}

// backward on MFMA: workgroup = 4 waves = ETILES x 128 keys of one (pass, head); wave = 32 keys (key = lane & 31).
// Phase 1: S[t,key] = Q . K^T and dP[t,key] = dO . V^T, a chain of HD / 16 32x32x16 MFMAs per 32-token block each, with -lse[t] and
// -delta[t] as the initial accumulators (rows of the accumulators are tokens); p = exp(S'), ds = p dP';
// dK^T[d,key] += Q^T . dS and dV^T[d,key] += dO^T . P with dS / P taken from the accumulators (Q^T, dO^T from
// transposed fp16 LDS images); ds and k go to LDS transposed.  Phase 2: dq[t,d] += sum_keys ds[key,t] k[key,d] (wave w:
// token block w); one atomic per (token, dim) per workgroup at the end.  q (pre-scaled by 1/sqrt(HD)) and dout are rounded to
// fp16 for the MFMA, as in the forward.  LDS at T = 128: 60 KiB at HD = 16 (two workgroups per CU), 80 KiB at 32, 121 KiB at 64 (one).
constexpr int EBK = 128, ETILES = 4;
static_assert(EBK == IBR, "rowtile_product and RSTR serve both backward kernels");
template <int HD>
struct ExtractBwdLds {      // floats, then halves
  int T, TB = tok_blocks(T);
  int nls = 0;                                    // [TB]  -lse (natural log) ; big negative past T
  int ndl = nls + TMAX;                           // [TB]  -delta
  int qsh = 2 * (ndl + TMAX);                     // [TB][KP]   Q rows (scaled)
  int dosh = qsh + TB * AdDim<HD>::KP;            // [TB][KP]   dO rows
  int qT = dosh + TB * AdDim<HD>::KP;             // [HD][TPV]  Q^T
  int doT = qT + HD * AdDim<HD>::TPV;             // [HD][TPV]  dO^T
  int dssT = doT + HD * AdDim<HD>::TPV;           // [T][RSTR]
  int kT = dssT + T * RSTR;                       // [HD][RSTR]
  int end = kT + HD * RSTR;
  constexpr size_t bytes() const { return sizeof(h16) * (size_t)end; }
};
// DET (deterministic mode): dq is the partial workspace [gridDim.x][B][T][E], slot = blockIdx.x (the key block), plain stores.
template <int HD, int HC, bool DET = false>
__global__ __launch_bounds__(256) void extract_attn_bwd_kernel(const float* __restrict__ q, const h16* __restrict__ kv,
                                                               const float* __restrict__ out, const float* __restrict__ lse,
                                                               const float* __restrict__ dout, int T, int L, int heads, float* __restrict__ dq,
                                                               h16* __restrict__ dkv) {
  AD_DIMS;
  AD_LANE;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ntb = (T + 31) / 32, TB = ntb * 32;
  const ExtractBwdLds<HD> lds{T};
  float *nls = smem + lds.nls, *ndl = smem + lds.ndl;
  h16* sh = reinterpret_cast<h16*>(smem);
  h16 *qsh = sh + lds.qsh, *dosh = sh + lds.dosh, *qT = sh + lds.qT, *doT = sh + lds.doT, *dssT = sh + lds.dssT, *kT = sh + lds.kT;
  const int h = blockIdx.y, b = blockIdx.z;
  const long tok0 = (long)b * T * AE + h * AD;
  stage_token_rows<HD, true>(tid, T, TB, AE, 1, tok_op(q + tok0, qsh, qT), tok_op(dout + tok0, dosh, doT));
  for (int t = tid; t < TB; t += 256) {
    float d = 0.f, l = 1.0e30f;
    if (t < T) {
      l = lse[((long)b * T + t) * AH + h];
      for (int e = 0; e < AD; ++e) d = fmaf(dout[((long)b * T + t) * AE + h * AD + e], out[((long)b * T + t) * AE + h * AD + e], d);
    }
    nls[t] = -l; ndl[t] = -d;
  }
  f32x16 accq[NA];                  // phase 2: token block `wave`, dims 32 j + lane
  zero(accq);
  const h16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  __syncthreads();
  for (int tile = 0; tile < ETILES; ++tile) {
    const int k0 = (blockIdx.x * ETILES + tile) * EBK;
    if (k0 >= L) break;             // uniform
    const int kl = wave * 32 + l31;
    const int key = k0 + kl;
    const bool valid = key < L;
    const h16* kvrow = kv + ((long)b * L + (valid ? key : 0)) * (2 * AE) + h * AD + 8 * hh;
    h16x8 kf[NC], vf[NC];                                     // B operands: K^T[d = 16 c + 8 hh + j][key], V^T likewise
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      kf[c] = valid ? ldg8(kvrow + 16 * c) : zero8;
      vf[c] = valid ? ldg8(kvrow + AE + 16 * c) : zero8;
#pragma unroll
      for (int e = 0; e < 8; ++e) kT[(16 * c + 8 * hh + e) * RSTR + kl] = kf[c][e];
    }
    f32x16 dka[NA], dva[NA];
    zero(dka);
    zero(dva);
#pragma unroll
    for (int tb = 0; tb < TMAX / 32; ++tb) {
      if (tb < ntb) {
        f32x16 sc = acc_from_rows(nls + tb * 32, hh), dpv = acc_from_rows(ndl + tb * 32, hh);      // accumulator rows are tokens
        score_chain<HD>(qsh, tb * 32 + l31, hh, kf, sc);
        score_chain<HD>(dosh, tb * 32 + l31, hh, vf, dpv);
        h16x8 pf[2], dsf[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int t = tb * 32 + acc_row(i, hh);
          const float pv = valid ? __expf(sc[i]) : 0.f;       // rows past T carry -1e30 -> 0
          const float ds = pv * dpv[i];
          pf[i >> 3][i & 7] = (h16)pv;
          dsf[i >> 3][i & 7] = (h16)ds;
          if (t < T) dssT[t * RSTR + kl] = (h16)(ds * ASCALE);
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
          for (int j = 0; j < NA; ++j) {
            const int tok = tb * 32 + 16 * s2 + 4 * hh;
            dka[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tr_frag<HD>(qT, j, drow, tok), dsf[s2], dka[j], 0, 0, 0);
            dva[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tr_frag<HD>(doT, j, drow, tok), pf[s2], dva[j], 0, 0, 0);
          }
        }
      }
    }
    if (valid) {      // the d x key accumulators (qsh already carries the scale)
      h16* dst = dkv + ((long)b * L + key) * (2 * AE) + h * AD;
      store_dim_tile<HD>(dst, dka, hh);
      store_dim_tile<HD>(dst + AE, dva, hh);
    }
    __syncthreads();
    if (wave < ntb) rowtile_product<HD>(dssT, min(wave * 32 + l31, T - 1), kT, drow, hh, accq);      // uniform per wave
    __syncthreads();
  }
  if (wave < ntb) flush_token_dim<HD, DET>(dq + flush_pass<DET>(b) * T * AE + h * AD, accq, wave, T, AE, hh, l31);
}

// ---------------------------------------------------------------- token self-attention -----------
// grid (heads, B), 512 threads: four threads per query token (sub = tid & 3), all T <= 128 tokens in ONE sweep.  K, V and the
// T x T score matrix live in LDS: the scores are written once, normalised in place, and leave as probs [B, heads, T, T] (saved
// for the backward) in one pass.  (The first form -- a thread per query looping over the keys with the score row in GLOBAL
// memory, written and re-read three times -- ran 24 us for 36 workgroups of 65 tokens; the step launches it between dependent
// token-side products, so its latency is exposed.  256 threads = 64 tokens per sweep: 13 us at T = 65, the 65th token costs a
// whole second sweep.)  Templated on the head dim HD: a thread of a token's four owns HD / 4 consecutive dims in the output sweeps.
// K, V and the scores take 16 T HD + 4 T S1 bytes (T = 128: 83 KiB at 16, 99 KiB at 32, 131 KiB at 64): the forward fits at every T.
MT_DEVINL f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// Score rows of the forward: T entries padded to a multiple of four, row stride S1 = 4 x odd >= that (sixteen tokens of a wave then start
// on sixteen different 16-byte bank groups), so that the value sweep reads FOUR probabilities with one 16-byte read -- every LDS read of
// that loop is in the 8 / 16-byte banking class (common.h: no counted lgkmcnt wait may span both classes).
__host__ __device__ constexpr int mha_t4(int T) { return (T + 3) & ~3; }
__host__ __device__ constexpr int mha_s1(int T) { return ((mha_t4(T) >> 2) & 1) ? mha_t4(T) : mha_t4(T) + 4; }
// DROP (nn.MultiheadAttention(dropout = p) in train(): dropout on the softmax, adapter_modules.py:42-52): P~ = P o m / (1 - p), m the
// element-dropout keep mask of drop.site at linear index ((b heads + h) T + i) T + j -- the mask mt_dropout_f32 draws over the flat
// [B heads T T] tensor.  The workgroup's T x T keep flags live in LDS as a BIT image, built once before the first barrier: byte x holds the
// elements of linear index 8 (base / 8 + x) .. + 7 (base = the head's first element; two Philox calls, each yielding four consecutive
// elements), so element (i, j) is bit (base & 7) + i T + j.  Writers store bytes, readers load 4-byte words: one banking class.
// mha_keep_bytes(T): the image's LDS, a multiple of four that covers the word of the last bit (2052 bytes at T = 128).
__host__ __device__ constexpr int mha_keep_bytes(int T) { return (((T * T + 14) >> 3) + 3) & ~3; }
MT_DEVINL uint32_t lds_u32(const uint32_t* p) { return *reinterpret_cast<const volatile uint32_t*>(p); }
MT_DEVINL void mha_keep_image(uint32_t* mb, int T, uint64_t base, const DropArgs& d, int tid) {
  uint8_t* mb8 = reinterpret_cast<uint8_t*>(mb);
  const uint64_t g0 = base >> 3;
  const int nb = (int)(((base & 7) + (uint64_t)T * T + 7) >> 3);
  const uint32_t thr = drop_threshold(d.p);
  for (int x = tid; x < nb; x += 512) {
    const uint64_t idx4 = (g0 + x) * 2;
    mb8[x] = (uint8_t)(drop_keep4(d, idx4, thr) | (drop_keep4(d, idx4 + 1, thr) << 4));
  }
}
MT_DEVINL bool mha_keep(const uint32_t* mb, int bit) { return (lds_u32(mb + (bit >> 5)) >> (bit & 31)) & 1u; }
// x o m / (1 - p) for the element at `bit` of the keep image (keep = 1 / (1 - p)): a dropped entry is SELECTED to 0, never multiplied
// by it (0 x inf, 0 x nan stay out)
MT_DEVINL float mha_drop_sel(const uint32_t* mb, int bit, float x, float keep) { return mha_keep(mb, bit) ? x * keep : 0.f; }
// Staging of forward and backward: rows 0 .. T - 1 of the head's slice (src[n] + o0 + t E) of N fp32 operands go to the LDS images
// img[n] [.][HD] as 16-byte copies; rows T .. NT - 1 of the image zpad are zeroed (NT = T and the literal nullptr: no such rows).
template <int HD, int N, class Z>
MT_DEVINL void mha_stage(int tid, int T, int NT, long o0, int E, const float* const (&src)[N], float* const (&img)[N], Z zpad) {
  constexpr int C4 = HD / 4;      // 16-byte chunks per row
  for (int i = tid; i < NT * C4; i += 512) {
    const int tt = i / C4, c = (i % C4) * 4;
    if (std::is_same_v<Z, std::nullptr_t> || tt < T) {
      const long o = o0 + (long)tt * E + c;
#pragma unroll
      for (int n = 0; n < N; ++n) *reinterpret_cast<f32x4*>(img[n] + tt * HD + c) = ld4(src[n] + o);
    } else if constexpr (!std::is_same_v<Z, std::nullptr_t>) {
      *reinterpret_cast<f32x4*>(zpad + tt * HD + c) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
}
template <int HD, bool DROP>
struct TokenFwdLds {      // floats
  int T, T4 = mha_t4(T), S1 = mha_s1(T);
  int ks = 0;                   // [T][HD]
  int vs = ks + T * HD;         // [T4][HD], rows T .. T4 - 1 zero
  int ss = vs + T4 * HD;        // [T][S1], entries T .. T4 - 1 of a row zero
  int mb = ss + T * S1;         // DROP: the keep-bit image, mha_keep_bytes(T)
  constexpr size_t bytes() const { return sizeof(float) * (size_t)mb + (DROP ? mha_keep_bytes(T) : 0); }
};
template <int HD, bool DROP = false>
__global__ __launch_bounds__(512) void token_mha_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            int T, int E, int heads, float* __restrict__ out, float* __restrict__ probs,
                                                            DropArgs drop) {
  constexpr int AD = HD, C4 = HD / 4, DS = HD / 4;      // C4: 16-byte chunks per row; DS: dims a thread owns in the value sweep
  constexpr float ASCALE = AdDim<HD>::SCALE;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TokenFwdLds<HD, DROP> lds{T};
  const int T4 = lds.T4, S1 = lds.S1;
  float *ks = smem + lds.ks, *vs = smem + lds.vs, *ss = smem + lds.ss;
  uint32_t* mb = reinterpret_cast<uint32_t*>(smem + lds.mb);
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, sub = tid & 3;
  const uint64_t mbase = ((uint64_t)b * heads + h) * T * T;
  if constexpr (DROP) mha_keep_image(mb, T, mbase, drop, tid);
  mha_stage<HD>(tid, T, T4, (long)b * T * E + h * AD, E, {k, v}, {ks, vs}, vs);
  const int t = tid >> 2;
  const bool act = t < T;
  float qv[AD];
  if (act) {
    const float* qr = q + ((long)b * T + t) * E + h * AD;
#pragma unroll
    for (int c = 0; c < C4; ++c) {
      const f32x4 x = ld4(qr + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) qv[4 * c + e] = x[e] * ASCALE;
    }
  }
  __syncthreads();
  if (act) {
    float mx = -1.0e30f;
    for (int j = sub; j < T; j += 4) {
      const float* kr = ks + j * AD;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < AD; ++d) s = fmaf(qv[d], kr[d], s);
      ss[t * S1 + j] = s;
      mx = fmaxf(mx, s);
    }
    if (T + sub < T4) ss[t * S1 + T + sub] = 0.f;      // (the row's padding: at most one entry per thread)
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    float l = 0.f;
    for (int j = sub; j < T; j += 4) { const float p = __expf(ss[t * S1 + j] - mx); ss[t * S1 + j] = p; l += p; }
    l += __shfl_xor(l, 1, 64);
    l += __shfl_xor(l, 2, 64);
    const float inv = 1.0f / l;
    float* pr = probs + (((long)b * heads + h) * T + t) * T;
    if constexpr (DROP) {      // probs keeps P (the backward and the attention maps read it), the value sweep sees P~
      const float keep = 1.f / (1.f - drop.p);
      const int bit0 = (int)(mbase & 7) + t * T;
      for (int j = sub; j < T; j += 4) {
        const float p = ss[t * S1 + j] * inv;
        pr[j] = p;
        ss[t * S1 + j] = mha_drop_sel(mb, bit0 + j, p, keep);
      }
    } else {
      for (int j = sub; j < T; j += 4) { const float p = ss[t * S1 + j] * inv; ss[t * S1 + j] = p; pr[j] = p; }
    }
  }
  __syncthreads();          // a row's four writers -> its four readers
  if (act) {
    // value sweep, four keys per step: one 16-byte read of the row's probabilities, four 16-byte value rows (all one banking class)
    f32x4 acc[DS / 4];
#pragma unroll
    for (int x = 0; x < DS / 4; ++x) acc[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < T4; j += 4) {
      const f32x4 p4 = ld4(ss + t * S1 + j);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int x = 0; x < DS / 4; ++x) acc[x] += p4[u] * ld4(vs + (j + u) * AD + DS * sub + 4 * x);
    }
#pragma unroll
    for (int x = 0; x < DS / 4; ++x) *reinterpret_cast<f32x4*>(out + ((long)b * T + t) * E + h * AD + DS * sub + 4 * x) = acc[x];
  }
}

// dq / dk / dv of the above from the saved probs: dP = dO V^T, dS = P (dP - rowsum(P dP)) scale, dQ = dS K, dK = dS^T Q, dV = P^T dO.
// Q, K, V, dO and dS in LDS -- and P too while both T x T images fit; four threads per token, each owning HD / 4 consecutive head
// dimensions in the output sweeps.  FORM picks what lives in LDS (16 T HD bytes of operands + 4 T (T + 1) per T x T image, 160 KiB):
//   0  Q, K, V, dO, dS, P      T <= 127 at HD = 16, <= 114 at 32, <= 92 at 64
//   1  Q, K, V, dO, dS         P read from global memory: every T <= 128 at 16 and 32, T <= 111 at 64
//   2  V, dO, dS               P, Q and K read from global memory (L2-resident: T x HD floats per head): the rest, HD = 64 and T > 111
// DROP (the forward's P~ = P o m / (1 - p); probs holds P): dV = P~^T dO, dP = (dO V^T) o m / (1 - p), delta and dS from P and that dP -- a
// dropped probability still receives -P delta.  The keep-bit image of the forward (mha_keep_image, regenerated from (rng, site, index))
// sits behind the images above: + mha_keep_bytes(T), so the DROP instantiations change form one token earlier where the sum was
// within 2 KiB of the limit:
//   0  T <= 126 at HD = 16, <= 113 at 32, <= 92 at 64        1  every T <= 128 at 16 and 32, T <= 110 at 64        2  the rest
// (All these limits are TokenBwdLds<HD, FORM, DROP>(T).bytes() <= LDS_MAX: the launcher takes the first FORM that fits.)
template <int HD, int FORM, bool DROP>
struct TokenBwdLds {      // floats
  int T;
  int qs = 0;                                       // [T][HD]     (Q and K: not in FORM 2)
  int ks = qs + T * HD;
  int vs = FORM == 2 ? 0 : ks + T * HD;
  int dos = vs + T * HD;
  int dss = dos + T * HD;                           // [T][T + 1]  dS (already scaled)
  int pls = dss + T * (T + 1);                      // [T][T + 1]  P (FORM 0 only)
  int mb = FORM == 0 ? pls + T * (T + 1) : pls;     // DROP: the keep-bit image, mha_keep_bytes(T)
  constexpr size_t bytes() const { return sizeof(float) * (size_t)mb + (DROP ? mha_keep_bytes(T) : 0); }
};
template <int HD, int FORM, bool DROP = false>
__global__ __launch_bounds__(512) void token_mha_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ probs, const float* __restrict__ dout, int T, int E,
                                                            int heads, float* __restrict__ dq, float* __restrict__ dk, float* __restrict__ dv,
                                                            DropArgs drop) {
  constexpr int AD = HD, DS = HD / 4;
  constexpr float ASCALE = AdDim<HD>::SCALE;
  constexpr bool PL = FORM == 0, GQK = FORM == 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TokenBwdLds<HD, FORM, DROP> lds{T};
  float *qs = smem + lds.qs, *ks = smem + lds.ks, *vs = smem + lds.vs, *dos = smem + lds.dos, *dss = smem + lds.dss, *pls = smem + lds.pls;
  uint32_t* mb = reinterpret_cast<uint32_t*>(smem + lds.mb);
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, sub = tid & 3, S1 = T + 1;
  const float* pbase = probs + ((long)b * heads + h) * T * T;
  const uint64_t mbase = ((uint64_t)b * heads + h) * T * T;
  const float keep = DROP ? 1.f / (1.f - drop.p) : 1.f;
  if constexpr (DROP) mha_keep_image(mb, T, mbase, drop, tid);
  const long o0 = (long)b * T * E + h * AD;
  if constexpr (GQK) mha_stage<HD>(tid, T, T, o0, E, {v, dout}, {vs, dos}, nullptr);
  else mha_stage<HD>(tid, T, T, o0, E, {q, k, v, dout}, {qs, ks, vs, dos}, nullptr);
  if (PL)
    for (int i = tid; i < T * T; i += 512) pls[(i / T) * S1 + i % T] = pbase[i];
  __syncthreads();
  const int t = tid >> 2;
  const bool act = t < T;
  const float* pr = PL ? pls + t * S1 : pbase + (long)t * T;      // row t of P
  const long pst = PL ? S1 : T;
  const float* pc = PL ? pls + t : pbase + t;                      // column t of P
  if (act) {          // a thread writes and re-reads only its own entries (j = sub mod 4) here
    float dov[AD];
#pragma unroll
    for (int d = 0; d < AD; ++d) dov[d] = dos[t * AD + d];
    // One banking class of LDS reads per loop (lds_f32, common.h): dP from the 16-byte value rows first, then delta from the 4-byte
    // probabilities and the thread's own dP entries.
    for (int j = sub; j < T; j += 4) {
      const float* vr = vs + j * AD;
      float dp = 0.f;
#pragma unroll
      for (int d = 0; d < AD; ++d) dp = fmaf(dov[d], vr[d], dp);
      dss[t * S1 + j] = dp;
    }
    float delta = 0.f;
    if constexpr (DROP) {      // dP = dP~ o m / (1 - p), written back over the thread's own entries (4-byte class: mask words, P, dP)
      const int bit0 = (int)(mbase & 7) + t * T;
      for (int j = sub; j < T; j += 4) {
        const float dp = mha_drop_sel(mb, bit0 + j, lds_f32(&dss[t * S1 + j]), keep);
        dss[t * S1 + j] = dp;
        delta = fmaf(lds_f32(&pr[j]), dp, delta);
      }
    } else {
      for (int j = sub; j < T; j += 4) delta = fmaf(lds_f32(&pr[j]), lds_f32(&dss[t * S1 + j]), delta);
    }
    delta += __shfl_xor(delta, 1, 64);
    delta += __shfl_xor(delta, 2, 64);
    for (int j = sub; j < T; j += 4) dss[t * S1 + j] = lds_f32(&pr[j]) * (lds_f32(&dss[t * S1 + j]) - delta) * ASCALE;
  }
  __syncthreads();
  if (act) {          // dQ: thread (query t, dims DS sub ..);  dK, dV: thread (key t, dims DS sub ..)
    f32x4 aq[DS / 4], ak[DS / 4], av[DS / 4];
#pragma unroll
    for (int x = 0; x < DS / 4; ++x) aq[x] = ak[x] = av[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* kr = GQK ? k + ((long)b * T) * E + h * AD + DS * sub : ks + DS * sub;      // row j of K / Q: + j * rst
    const float* qr = GQK ? q + ((long)b * T) * E + h * AD + DS * sub : qs + DS * sub;
    const long rst = GQK ? E : AD;
    for (int j = 0; j < T; ++j) {      // (4-byte LDS reads only, as in the forward's value sweep)
      const float dsq = lds_f32(&dss[t * S1 + j]);
#pragma unroll
      for (int x = 0; x < DS / 4; ++x) aq[x] += dsq * lds_f32x4_by_dword(kr + j * rst + 4 * x);
      const float dsk = lds_f32(&dss[j * S1 + t]);
#pragma unroll
      for (int x = 0; x < DS / 4; ++x) ak[x] += dsk * lds_f32x4_by_dword(qr + j * rst + 4 * x);
      float pv = lds_f32(&pc[j * pst]);
      if constexpr (DROP) pv = mha_drop_sel(mb, (int)(mbase & 7) + j * T + t, pv, keep);      // P~[j][t]
#pragma unroll
      for (int x = 0; x < DS / 4; ++x) av[x] += pv * lds_f32x4_by_dword(dos + j * AD + DS * sub + 4 * x);
    }
    const long o = ((long)b * T + t) * E + h * AD + DS * sub;
#pragma unroll
    for (int x = 0; x < DS / 4; ++x) {
      *reinterpret_cast<f32x4*>(dq + o + 4 * x) = aq[x];
      *reinterpret_cast<f32x4*>(dk + o + 4 * x) = ak[x];
      *reinterpret_cast<f32x4*>(dv + o + 4 * x) = av[x];
    }
  }
}

// ---------------------------------------------------------------- attention maps (forward only) ---
// The head-averaged softmax of each adapter attention (nn.MultiheadAttention's `need_weights` output), recomputed in one streaming
// pass from what the forward already keeps: the fp16 operands and the row log-sum-exp.  The scores are rounded exactly as the
// forward rounds them -- through the same stage_token_rows / scaled_h16 / score_chain -- so every row of every head sums to one
// against the saved LSE.
constexpr int PBR = 128;          // keys (extractor) / patch rows (injector) per workgroup: 4 waves x 32

// Extractor: w[b, t, l] = 1/heads sum_h exp(s_bthl - lse_bth), s = fp16(q / sqrt(HD)) . fp16(k) (extract_attn_fwd's rounding).
// grid (ceil(L / 128), B); wave = 32 keys (key = lane & 31).  Per head a chain of HD / 16 32x32x16 MFMAs per 32-token block with
// -lse as the initial accumulator (extract_attn_bwd phase 1); the exp is summed over the heads in registers and every element is
// stored once (a store instruction writes two 128-byte rows).  LDS: -lse [G][TB] and fp16(q / sqrt(HD)) [G][TB][KP], all reads 16
// bytes wide, for a GROUP of G heads at a time: the launcher picks the largest G whose image stays within PROBS_LDS = 80 KiB, so
// that two workgroups (8 waves) share a CU in every form -- all 12 heads at once at 12 x 16 (78 KiB at T = 128, as before the
// template), 3 passes of 4 heads at 9 x 64 rather than a 162 KiB image of all nine or fewer tokens per workgroup.
constexpr int PROBS_LDS = 80 * 1024;
// heads per LDS image of the attention-map kernels: all of them when that fits PROBS_LDS, else the largest group that does
inline int probs_group(int heads, size_t per_head) {
  const int g = (int)((size_t)PROBS_LDS / per_head);
  return g < 1 ? 1 : g > heads ? heads : g;
}
template <int HD>
struct ExtractProbsLds {
  int T, G, TB = tok_blocks(T);
  int nls = 0;                      // floats: [G][TB]      -lse; -1e30 past T
  int qsh = 2 * (nls + G * TB);     // halves: [G][TB][KP]  q / sqrt(HD) (fp16); zero past T
  constexpr size_t bytes() const { return sizeof(h16) * ((size_t)qsh + (size_t)G * TB * AdDim<HD>::KP); }
  constexpr size_t per_head() const { return bytes() / G; }
};
template <int HD, int HC>
__global__ __launch_bounds__(256) void extract_attn_probs_kernel(const float* __restrict__ q, const h16* __restrict__ kv,
                                                                 const float* __restrict__ lse, int T, int L, int heads, int hgroup,
                                                                 float* __restrict__ w) {
  AD_DIMS;
  AD_LANE;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ntb = (T + 31) / 32, TB = ntb * 32;
  const int G = HC ? HC : hgroup;                         // heads per LDS image
  const ExtractProbsLds<HD> lds{T, G};
  float* nls = smem + lds.nls;
  h16* qsh = reinterpret_cast<h16*>(smem) + lds.qsh;
  const int b = blockIdx.y;
  const int key = blockIdx.x * PBR + wave * 32 + l31;
  const bool valid = key < L;
  const h16* row = kv + ((long)b * L + (valid ? key : 0)) * (2 * AE) + 8 * hh;
  f32x16 acc[TMAX / 32];
  zero(acc);
  for (int h0 = 0; h0 < AH; h0 += G) {
    const int gh = min(G, AH - h0);
    if (h0) __syncthreads();          // the previous group's image has been read by every wave
    stage_token_rows<HD, true>(tid, T, TB, AE, gh, tok_op(q + (long)b * T * AE + h0 * AD, qsh, nullptr));
    for (int i = tid; i < TB * gh; i += 256) {
      const int t = i / gh, h = i % gh;
      nls[h * TB + t] = t < T ? -lse[((long)b * T + t) * AH + h0 + h] : -1.0e30f;
    }
    __syncthreads();
    for (int h = 0; h < gh; ++h) {
      h16x8 kf[NC];                   // B operands: K^T[d = 16 c + 8 hh + j][key]
      row_frags(row + (h0 + h) * AD, valid, kf);
#pragma unroll
      for (int tb = 0; tb < TMAX / 32; ++tb) {
        if (tb < ntb) {
          f32x16 sc = acc_from_rows(nls + h * TB + tb * 32, hh);      // accumulator rows are tokens
          score_chain<HD>(qsh, h * TB + tb * 32 + l31, hh, kf, sc);
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[tb][i] += __expf(sc[i]);
        }
      }
    }
  }
  if (valid) {
    const float inv = 1.0f / (float)AH;
#pragma unroll
    for (int tb = 0; tb < TMAX / 32; ++tb) {
      if (tb < ntb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int t = tb * 32 + acc_row(i, hh);
          if (t < T) w[((long)b * T + t) * L + key] = acc[tb][i] * inv;
        }
      }
    }
  }
}

// Injector: w[m, t] = 1/heads sum_h exp(s_mht / sqrt(HD) - lse_mh), s = fp16(k) . q (inject_attn_fwd's rounding; its lse is natural-log).
// grid (ceil(rows_per_pass / 128), B); wave = 32 patch rows (row = lane & 31).  Per head S^T = K . Q^T, a chain of HD / 16 32x32x16 MFMAs
// per 32-token block (K rows from an fp16 LDS image of a group of G heads, 16-byte reads; G as above: the image or the 65 KiB output
// tile, whichever is larger, stays within 80 KiB -- two workgroups per CU in every form).  The [128 rows][T] tile then goes through LDS
// (4-byte writes, a barrier, 4-byte reads; odd row stride) and leaves as one contiguous, coalesced run of the [M, T] output.
template <int HD>
struct InjectProbsLds {
  int T, G, TB = tok_blocks(T), S = T | 1;      // S: floats per row of the output tile (odd)
  int ksh = 0;      // halves: [G][TB][KP]  fp16(k); zero past T
  int osh = 0;      // floats: [128][S]     the output tile, over the K image once every wave is done with it
  constexpr size_t per_head() const { return sizeof(h16) * (size_t)TB * AdDim<HD>::KP; }
  constexpr size_t bytes() const { return per_head() * G > sizeof(float) * PBR * S ? per_head() * G : sizeof(float) * PBR * S; }
};
template <int HD, int HC>
__global__ __launch_bounds__(256) void inject_attn_probs_kernel(const h16* __restrict__ q, int rows_per_pass, const float* __restrict__ k,
                                                                const float* __restrict__ lse, int T, int heads, int hgroup,
                                                                float* __restrict__ w) {
  AD_DIMS;
  AD_LANE;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ntb = (T + 31) / 32, TB = ntb * 32;
  const int G = HC ? HC : hgroup;                         // heads per LDS image
  const InjectProbsLds<HD> lds{T, G};
  h16* ksh = reinterpret_cast<h16*>(smem) + lds.ksh;
  const int b = blockIdx.y;
  const int r0 = blockIdx.x * PBR, rl = wave * 32 + l31;
  const bool valid = r0 + rl < rows_per_pass;
  const long m = (long)b * rows_per_pass + (valid ? r0 + rl : 0);
  f32x16 acc[TMAX / 32];
  zero(acc);
  for (int h0 = 0; h0 < AH; h0 += G) {
    const int gh = min(G, AH - h0);
    if (h0) __syncthreads();          // the previous group's image has been read by every wave
    stage_token_rows<HD>(tid, T, TB, AE, gh, tok_op(k + (long)b * T * AE + h0 * AD, ksh, nullptr));
    __syncthreads();
    for (int h = 0; h < gh; ++h) {
      h16x8 qf[NC];                   // B operands: Q^T[d = 16 c + 8 hh + j][row]
      row_frags(q + m * AE + (h0 + h) * AD + 8 * hh, valid, qf);
      const float nl = valid ? -lse[m * AH + h0 + h] : 0.f;
#pragma unroll
      for (int tb = 0; tb < TMAX / 32; ++tb) {
        if (tb < ntb) {
          f32x16 sc;
          zero(sc);
          score_chain<HD>(ksh, h * TB + tb * 32 + l31, hh, qf, sc);
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[tb][i] += __expf(fmaf(sc[i], ASCALE, nl));
        }
      }
    }
  }
  __syncthreads();                  // every wave is done with the K image: its storage takes the output tile
  const int S = lds.S;
  float* osh = smem + lds.osh;      // [128][S]
  const float inv = 1.0f / (float)AH;
  if (valid) {
#pragma unroll
    for (int tb = 0; tb < TMAX / 32; ++tb) {
      if (tb < ntb) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {      // accumulator rows are tokens, column = the lane's row
          const int t = tb * 32 + acc_row(i, hh);
          if (t < T) osh[rl * S + t] = acc[tb][i] * inv;
        }
      }
    }
  }
  __syncthreads();
  const int n = min(PBR, rows_per_pass - r0) * T;
  float* dst = w + ((long)b * rows_per_pass + r0) * T;
  for (int e = tid; e < n; e += 256) dst[e] = osh[(e / T) * S + e % T];
}

// Prompt self-attention: out[b, i, j] = mean over the heads of token_mha_fwd's probs [B, heads, T, T].
__global__ void token_probs_mean_kernel(const float* __restrict__ probs, int B, int heads, int T, float* __restrict__ out) {
  const long n = (long)T * T;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)B * n) return;
  const long b = e / n, r = e % n;
  float s = 0.f;
  for (int h = 0; h < heads; ++h) s += probs[(b * heads + h) * n + r];
  out[e] = s / (float)heads;
}

// ---------------------------------------------------------------- launchers ----------------------
// One launcher per kernel, templated like it; AD_DISPATCH (AD_SELECT: without the return) picks the instantiation: <16, 12> for the shipped 12 x 16 (the head count a
// compile-time constant, as before the template), <HD, 0> otherwise.
#define AD_SELECT(rc, heads, hd, CALL)                      \
  do {                                                      \
    if ((hd) == 16 && (heads) == 12) rc = CALL(16, 12);     \
    else if ((hd) == 16) rc = CALL(16, 0);                  \
    else if ((hd) == 32) rc = CALL(32, 0);                  \
    else if ((hd) == 64) rc = CALL(64, 0);                  \
    else rc = MT_ERR_UNSUPPORTED;                           \
  } while (0)
// (a launcher with a deterministic form defines AD_CALL(HD, HC, DET) and selects through these two)
#define AD_BASE(HD, HC) AD_CALL(HD, HC, false)
#define AD_DET(HD, HC) AD_CALL(HD, HC, true)
#define AD_DISPATCH(heads, hd, CALL)                        \
  do {                                                      \
    int rc__;                                               \
    AD_SELECT(rc__, heads, hd, CALL);                       \
    return rc__;                                            \
  } while (0)

// Every launch of this file: K with `shm` bytes of dynamic LDS (its layout's bytes(); more than LDS_MAX: unsupported).  A kernel that takes
// dynamic LDS is opted into LDS_MAX once per instantiation (one static per K).
template <auto K, class... Args>
int ad_launch(dim3 grid, int block, size_t shm, hipStream_t stream, Args... args) {
  if (shm > (size_t)LDS_MAX) return MT_ERR_UNSUPPORTED;
  static bool attr_set = false;
  if (shm && !attr_set) {
    (void)hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    attr_set = true;
  }
  hipLaunchKernelGGL(K, grid, dim3(block), shm, stream, args...);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

template <int HD, int HC>
int launch_inject_fwd(const h16* q, int rows_per_pass, int B, const float* k, const float* v, int T, int heads, h16* a, float* lse,
                      hipStream_t stream) {
  return ad_launch<inject_attn_fwd_kernel<HD, HC>>(dim3(cdiv(rows_per_pass, 128), heads, B), 256, 0, stream, q, rows_per_pass, k, v, T, heads, a,
                                                   lse);
}

template <int HD, int HC, bool DET = false>
int launch_inject_bwd(const h16* q, const h16* a, const float* lse, const h16* da, int rows_per_pass, int B, const float* k, const float* v,
                      int T, int heads, h16* dq, float* dk, float* dv, hipStream_t stream) {
  return ad_launch<inject_attn_bwd_kernel<HD, HC, DET>>(dim3(cdiv(rows_per_pass, IBR * ITILES), heads, B), 256, InjectBwdLds<HD>{T}.bytes(), stream,
                                                        q, a, lse, da, rows_per_pass, k, v, T, heads, dq, dk, dv);
}

template <int HD, int HC>
int launch_extract_fwd(const float* q, const h16* kv, int B, int T, int L, int heads, int kps, float* out, float* lse, float* part_acc,
                       float* part_ml, int nsplit, hipStream_t stream) {
  // (HD = 16: static LDS; beyond, the V blocks and the merge image [4][T][HD + 2] are dynamic)
  const size_t shm = HD == 16 ? 0 : ExtractFwdLds<HD>{T}.bytes();
  if (int rc = ad_launch<extract_attn_fwd_kernel<HD, HC>>(dim3(nsplit, heads, B), EFT, shm, stream, q, kv, T, L, heads, kps, part_acc, part_ml))
    return rc;
  return ad_launch<extract_attn_reduce_kernel<HD, HC>>(dim3(B * heads), TMAX, 0, stream, (const float*)part_acc, (const float*)part_ml, T, nsplit,
                                                       heads, out, lse);
}

template <int HD, int HC, bool DET = false>
int launch_extract_bwd(const float* q, const h16* kv, const float* out, const float* lse, const float* dout, int B, int T, int L, int heads,
                       float* dq, h16* dkv, hipStream_t stream) {
  return ad_launch<extract_attn_bwd_kernel<HD, HC, DET>>(dim3(cdiv(L, EBK * ETILES), heads, B), 256, ExtractBwdLds<HD>{T}.bytes(), stream, q, kv, out,
                                                         lse, dout, T, L, heads, dq, dkv);
}

template <int HD, int HC>
int launch_extract_probs(const float* q, const h16* kv, const float* lse, int B, int T, int L, int heads, float* w, hipStream_t stream) {
  const int G = HC ? HC : probs_group(heads, ExtractProbsLds<HD>{T, 1}.per_head());
  return ad_launch<extract_attn_probs_kernel<HD, HC>>(dim3(cdiv(L, PBR), B), 256, ExtractProbsLds<HD>{T, G}.bytes(), stream, q, kv, lse, T, L, heads,
                                                      G, w);
}

template <int HD, int HC>
int launch_inject_probs(const h16* q, int rows_per_pass, int B, const float* k, const float* lse, int T, int heads, float* w,
                        hipStream_t stream) {
  const int G = HC ? HC : probs_group(heads, InjectProbsLds<HD>{T, 1}.per_head());
  return ad_launch<inject_attn_probs_kernel<HD, HC>>(dim3(cdiv(rows_per_pass, PBR), B), 256, InjectProbsLds<HD>{T, G}.bytes(), stream, q,
                                                     rows_per_pass, k, lse, T, heads, G, w);
}

// d: the softmax dropout (make_drop of the entry's MtDropout); inactive = the DROP = false kernel, which never reads it
template <int HD, bool DROP>
int launch_token_fwd_drop(const float* q, const float* k, const float* v, int B, int T, int E, int heads, float* out, float* probs,
                          const DropArgs& d, hipStream_t stream) {
  return ad_launch<token_mha_fwd_kernel<HD, DROP>>(dim3(heads, B), 512, TokenFwdLds<HD, DROP>{T}.bytes(), stream, q, k, v, T, E, heads, out, probs, d);
}

template <int HD, int FORM, bool DROP>
int launch_token_bwd_form(const float* q, const float* k, const float* v, const float* probs, const float* dout, int B, int T, int E,
                          int heads, float* dq, float* dk, float* dv, const DropArgs& d, hipStream_t stream) {
  return ad_launch<token_mha_bwd_kernel<HD, FORM, DROP>>(dim3(heads, B), 512, TokenBwdLds<HD, FORM, DROP>{T}.bytes(), stream, q, k, v, probs, dout, T,
                                                         E, heads, dq, dk, dv, d);
}
// the first FORM whose images fit at this T (the T limits of the kernel's comment); FORM 2 fits at every T <= TMAX
template <int HD, bool DROP>
int launch_token_bwd_drop(const float* q, const float* k, const float* v, const float* probs, const float* dout, int B, int T, int E,
                          int heads, float* dq, float* dk, float* dv, const DropArgs& d, hipStream_t stream) {
  static_assert(TokenBwdLds<HD, 2, DROP>{TMAX}.bytes() <= (size_t)LDS_MAX, "token backward: FORM 2 at TMAX");
  int rc = launch_token_bwd_form<HD, 0, DROP>(q, k, v, probs, dout, B, T, E, heads, dq, dk, dv, d, stream);
  if (rc == MT_ERR_UNSUPPORTED) rc = launch_token_bwd_form<HD, 1, DROP>(q, k, v, probs, dout, B, T, E, heads, dq, dk, dv, d, stream);
  if (rc == MT_ERR_UNSUPPORTED) rc = launch_token_bwd_form<HD, 2, DROP>(q, k, v, probs, dout, B, T, E, heads, dq, dk, dv, d, stream);
  return rc;
}

// the shape predicates of the entry points
inline bool ad_heads_ok(int heads, int head_dim) { return heads >= 1 && head_dim >= 1 && heads <= 1024; }
inline bool ad_head_dim_ok(int head_dim) { return head_dim == 16 || head_dim == 32 || head_dim == 64; }
inline bool inject_shape_ok(int M, int rows_per_pass, int T, int heads, int head_dim) {
  return !(M <= 0 || rows_per_pass <= 0 || M % rows_per_pass || T < 1 || T > TMAX || !ad_heads_ok(heads, head_dim));
}
inline bool extract_shape_ok(int B, int T, int L, int heads, int head_dim) {
  return !(B < 1 || T < 1 || T > TMAX || L < 1 || !ad_heads_ok(heads, head_dim));
}

}  // namespace

extern "C" int mt_inject_attn_fwd_hd(const mt_half* q, int M, int rows_per_pass, const float* k, const float* v, int T, int heads,
                                     int head_dim, mt_half* a, float* lse, mt_stream_t stream) {
  if (!q || !k || !v || !a || !inject_shape_ok(M, rows_per_pass, T, heads, head_dim)) return MT_ERR_BAD_ARG;
#define AD_CALL(HD, HC) \
  launch_inject_fwd<HD, HC>((const h16*)q, rows_per_pass, M / rows_per_pass, k, v, T, heads, (h16*)a, lse, (hipStream_t)stream)
  AD_DISPATCH(heads, head_dim, AD_CALL);
#undef AD_CALL
}

extern "C" int mt_inject_attn_fwd(const mt_half* q, int M, int rows_per_pass, const float* k, const float* v, int T,
                                  mt_half* a, float* lse, mt_stream_t stream) {
  return mt_inject_attn_fwd_hd(q, M, rows_per_pass, k, v, T, 12, 16, a, lse, stream);
}

// partials = dk slots [row blocks][B][T][E], then dv slots likewise; row blocks = cdiv(rows_per_pass, 512), E = heads * head_dim.
// Rows t >= T of a slot do not exist.
extern "C" long mt_inject_attn_bwd_hd_det_elems(int M, int rows_per_pass, int T, int heads, int head_dim) {
  if (!inject_shape_ok(M, rows_per_pass, T, heads, head_dim) || !ad_head_dim_ok(head_dim)) return MT_ERR_BAD_ARG;
  return 2L * cdiv(rows_per_pass, IBR * ITILES) * (M / rows_per_pass) * T * heads * head_dim;
}

// opt->partials: the deterministic form (det_reduce.hip) -- the kernel's dk / dv targets are the partial slots, two reduces follow
extern "C" int mt_inject_attn_bwd_hd(const mt_half* q, const mt_half* a, const float* lse, const mt_half* da, int M, int rows_per_pass,
                                     const float* k, const float* v, int T, int heads, int head_dim, mt_half* dq, float* dk, float* dv,
                                     const MtLaunchOpts* opt, mt_stream_t stream) {
  if (int rc = mt_opts_check(opt, MT_OPT_PARTIALS)) return rc;
  float* partials = mt_opt_partials(opt);
  if (!q || !a || !lse || !da || !k || !v || !dq || !dk || !dv || !inject_shape_ok(M, rows_per_pass, T, heads, head_dim))
    return MT_ERR_BAD_ARG;
  const int B = M / rows_per_pass, slots = cdiv(rows_per_pass, IBR * ITILES), E = heads * head_dim;
  const long slot = (long)B * T * E;
  if (partials) {
    const long need = mt_inject_attn_bwd_hd_det_elems(M, rows_per_pass, T, heads, head_dim);
    if (need < 0 || opt->partials_elems < need) return MT_ERR_BAD_ARG;
  }
  float* pk = partials ? partials : dk;
  float* pv = partials ? partials + slots * slot : dv;
  hipStream_t s = (hipStream_t)stream;
  int rc;
#define AD_CALL(HD, HC, DET)                                                                                                            \
  launch_inject_bwd<HD, HC, DET>((const h16*)q, (const h16*)a, lse, (const h16*)da, rows_per_pass, B, k, v, T, heads, (h16*)dq, pk, pv, s)
  if (!partials) AD_SELECT(rc, heads, head_dim, AD_BASE);
  else AD_SELECT(rc, heads, head_dim, AD_DET);
#undef AD_CALL
  if (rc != MT_OK || !partials) return rc;
  rc = mt_det_reduce_launch(pk, slots, B * T, E, slot, dk, E, s);
  if (rc != MT_OK) return rc;
  return mt_det_reduce_launch(pv, slots, B * T, E, slot, dv, E, s);
}

extern "C" int mt_inject_attn_bwd(const mt_half* q, const mt_half* a, const float* lse, const mt_half* da, int M,
                                  int rows_per_pass, const float* k, const float* v, int T, mt_half* dq, float* dk,
                                  float* dv, mt_stream_t stream) {
  return mt_inject_attn_bwd_hd(q, a, lse, da, M, rows_per_pass, k, v, T, 12, 16, dq, dk, dv, nullptr, stream);
}

extern "C" int mt_extract_attn_fwd_hd(const float* q, const mt_half* kv, int B, int T, int L, int heads, int head_dim, float* out,
                                      float* lse, float* part_acc, float* part_ml, int nsplit, mt_stream_t stream) {
  if (!q || !kv || !out || !lse || !part_acc || !part_ml || nsplit < 1 || !extract_shape_ok(B, T, L, heads, head_dim))
    return MT_ERR_BAD_ARG;
  const int kps = cdiv(cdiv(L, nsplit), EKT) * EKT;
  if ((long)kps * (nsplit - 1) >= L && nsplit > 1) return MT_ERR_BAD_ARG;   // every split must own >= 1 key
#define AD_CALL(HD, HC) \
  launch_extract_fwd<HD, HC>(q, (const h16*)kv, B, T, L, heads, kps, out, lse, part_acc, part_ml, nsplit, (hipStream_t)stream)
  AD_DISPATCH(heads, head_dim, AD_CALL);
#undef AD_CALL
}

extern "C" int mt_extract_attn_fwd(const float* q, const mt_half* kv, int B, int T, int L, float* out, float* lse,
                                   float* part_acc, float* part_ml, int nsplit, mt_stream_t stream) {
  return mt_extract_attn_fwd_hd(q, kv, B, T, L, 12, 16, out, lse, part_acc, part_ml, nsplit, stream);
}

// partials = dq slots [key blocks][B][T][E], key blocks = cdiv(L, 512)
extern "C" long mt_extract_attn_bwd_hd_det_elems(int B, int T, int L, int heads, int head_dim) {
  if (!extract_shape_ok(B, T, L, heads, head_dim) || !ad_head_dim_ok(head_dim)) return MT_ERR_BAD_ARG;
  return (long)cdiv(L, EBK * ETILES) * B * T * heads * head_dim;
}

// opt->partials: the deterministic form -- the kernel's dq target is the partial slots, one reduce follows
extern "C" int mt_extract_attn_bwd_hd(const float* q, const mt_half* kv, const float* out, const float* lse, const float* dout, int B,
                                      int T, int L, int heads, int head_dim, float* dq, mt_half* dkv, const MtLaunchOpts* opt,
                                      mt_stream_t stream) {
  if (int rc = mt_opts_check(opt, MT_OPT_PARTIALS)) return rc;
  float* partials = mt_opt_partials(opt);
  if (!q || !kv || !out || !lse || !dout || !dq || !dkv || !extract_shape_ok(B, T, L, heads, head_dim)) return MT_ERR_BAD_ARG;
  if (partials) {
    const long need = mt_extract_attn_bwd_hd_det_elems(B, T, L, heads, head_dim);
    if (need < 0 || opt->partials_elems < need) return MT_ERR_BAD_ARG;
  }
  float* pq = partials ? partials : dq;
  hipStream_t s = (hipStream_t)stream;
  int rc;
#define AD_CALL(HD, HC, DET) launch_extract_bwd<HD, HC, DET>(q, (const h16*)kv, out, lse, dout, B, T, L, heads, pq, (h16*)dkv, s)
  if (!partials) AD_SELECT(rc, heads, head_dim, AD_BASE);
  else AD_SELECT(rc, heads, head_dim, AD_DET);
#undef AD_CALL
  if (rc != MT_OK || !partials) return rc;
  const int E = heads * head_dim;
  return mt_det_reduce_launch(partials, cdiv(L, EBK * ETILES), B * T, E, (long)B * T * E, dq, E, s);
}

extern "C" int mt_extract_attn_bwd(const float* q, const mt_half* kv, const float* out, const float* lse,
                                   const float* dout, int B, int T, int L, float* dq, mt_half* dkv, mt_stream_t stream) {
  return mt_extract_attn_bwd_hd(q, kv, out, lse, dout, B, T, L, 12, 16, dq, dkv, nullptr, stream);
}

static bool mha_ptrs_ok(const float* const* ps, int n, int E) {
  for (int i = 0; i < n; ++i)
    if (!ps[i] || ((uintptr_t)ps[i] & 15)) return false;
  return (E & 3) == 0;
}
// the shapes of the prompt self-attention entries, and its softmax dropout: element dropout only (no DropPath at this site), p in [0, 1)
static bool mha_shape_ok(int B, int T, int E, int heads, const MtDropout* drop) {
  return !(B < 1 || T < 1 || T > TMAX || heads < 1 || E < 1 || E % heads) &&
         (!drop || (drop->p >= 0.f && drop->p < 1.f && drop->path_p == 0.f));
}
// one instantiation per head dim E / heads in 16 / 32 / 64 and per form of the dropout d (active or not): CALL(HD, DROP) is the launcher's call
#define MHA_DISPATCH(E, heads, d, CALL)                                             \
  do {                                                                              \
    const int hd__ = (E) / (heads);                                                 \
    if (hd__ == 16) return (d).active() ? CALL(16, true) : CALL(16, false);         \
    if (hd__ == 32) return (d).active() ? CALL(32, true) : CALL(32, false);         \
    if (hd__ == 64) return (d).active() ? CALL(64, true) : CALL(64, false);         \
    return MT_ERR_UNSUPPORTED;                                                      \
  } while (0)
extern "C" int mt_token_mha_fwd_drop(const float* q, const float* k, const float* v, int B, int T, int E, int heads, float* out,
                                     float* probs, const MtDropout* drop, mt_stream_t stream) {
  const float* ps[] = {q, k, v, out};
  if (!mha_ptrs_ok(ps, 4, E) || !probs || !mha_shape_ok(B, T, E, heads, drop)) return MT_ERR_BAD_ARG;
  const DropArgs d = make_drop(drop);
#define MHA_CALL(HD, DROP) launch_token_fwd_drop<HD, DROP>(q, k, v, B, T, E, heads, out, probs, d, (hipStream_t)stream)
  MHA_DISPATCH(E, heads, d, MHA_CALL);
#undef MHA_CALL
}
extern "C" int mt_token_mha_fwd(const float* q, const float* k, const float* v, int B, int T, int E, int heads,
                                float* out, float* probs, mt_stream_t stream) {
  return mt_token_mha_fwd_drop(q, k, v, B, T, E, heads, out, probs, nullptr, stream);
}

extern "C" int mt_token_mha_bwd_drop(const float* q, const float* k, const float* v, const float* probs, const float* dout, int B, int T,
                                     int E, int heads, float* dq, float* dk, float* dv, const MtDropout* drop, mt_stream_t stream) {
  const float* ps[] = {q, k, v, dout, dq, dk, dv};
  if (!mha_ptrs_ok(ps, 7, E) || !probs || !mha_shape_ok(B, T, E, heads, drop)) return MT_ERR_BAD_ARG;
  const DropArgs d = make_drop(drop);
#define MHA_CALL(HD, DROP) launch_token_bwd_drop<HD, DROP>(q, k, v, probs, dout, B, T, E, heads, dq, dk, dv, d, (hipStream_t)stream)
  MHA_DISPATCH(E, heads, d, MHA_CALL);
#undef MHA_CALL
}
extern "C" int mt_token_mha_bwd(const float* q, const float* k, const float* v, const float* probs, const float* dout,
                                int B, int T, int E, int heads, float* dq, float* dk, float* dv, mt_stream_t stream) {
  return mt_token_mha_bwd_drop(q, k, v, probs, dout, B, T, E, heads, dq, dk, dv, nullptr, stream);
}

extern "C" int mt_extract_attn_probs_hd(const float* q, const mt_half* kv, const float* lse, int B, int T, int L, int heads, int head_dim,
                                        float* w, mt_stream_t stream) {
  if (!q || !kv || !lse || !w || !extract_shape_ok(B, T, L, heads, head_dim)) return MT_ERR_BAD_ARG;
#define AD_CALL(HD, HC) launch_extract_probs<HD, HC>(q, (const h16*)kv, lse, B, T, L, heads, w, (hipStream_t)stream)
  AD_DISPATCH(heads, head_dim, AD_CALL);
#undef AD_CALL
}

extern "C" int mt_extract_attn_probs(const float* q, const mt_half* kv, const float* lse, int B, int T, int L, float* w,
                                     mt_stream_t stream) {
  return mt_extract_attn_probs_hd(q, kv, lse, B, T, L, 12, 16, w, stream);
}

extern "C" int mt_inject_attn_probs_hd(const mt_half* q, int M, int rows_per_pass, const float* k, const float* lse, int T, int heads,
                                       int head_dim, float* w, mt_stream_t stream) {
  if (!q || !k || !lse || !w || !inject_shape_ok(M, rows_per_pass, T, heads, head_dim)) return MT_ERR_BAD_ARG;
#define AD_CALL(HD, HC) \
  launch_inject_probs<HD, HC>((const h16*)q, rows_per_pass, M / rows_per_pass, k, lse, T, heads, (float*)w, (hipStream_t)stream)
  AD_DISPATCH(heads, head_dim, AD_CALL);
#undef AD_CALL
}

extern "C" int mt_inject_attn_probs(const mt_half* q, int M, int rows_per_pass, const float* k, const float* lse, int T, float* w,
                                    mt_stream_t stream) {
  return mt_inject_attn_probs_hd(q, M, rows_per_pass, k, lse, T, 12, 16, w, stream);
}

extern "C" int mt_token_probs_mean(const float* probs, int B, int heads, int T, float* out, mt_stream_t stream) {
  if (!probs || !out || B < 1 || heads < 1 || T < 1 || T > TMAX) return MT_ERR_BAD_ARG;
  const long n = (long)B * T * T;
  hipLaunchKernelGGL(token_probs_mean_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, probs, B, heads, T, out);
  MT_CHECK_LAUNCH();
  return MT_OK;
}
