// LayerNorm forward/backward (one wave per row, fp32 statistics) and the elementwise helpers.
// HBM-bound: every row is read once with 8/16-byte vector loads and written once.
#include <type_traits>

#include "common.h"

namespace {

// ---------------------------------------------------------------- vector load and store -----------
template <typename T> struct Vec4;
template <> struct Vec4<float> {
  static MT_DEVINL f32x4 load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  static MT_DEVINL void store(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
};
template <> struct Vec4<h16> {
  static MT_DEVINL f32x4 load(const h16* p) {
    h16x4 v = *reinterpret_cast<const h16x4*>(p);
    return (f32x4){(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  }
  static MT_DEVINL void store(h16* p, f32x4 v) {
    *reinterpret_cast<h16x4*>(p) = (h16x4){(h16)v[0], (h16)v[1], (h16)v[2], (h16)v[3]};
  }
};

// ---------------------------------------------------------------- row stages ----------------------
// The one-wave-per-row kernels (256 threads = 4 waves = 4 rows in flight): lane l owns the columns c * 256 + l * 4 .. + 3 of chunk c,
// NC = D / 256 chunks per row.  Every kernel below states its row arithmetic through these; the order of the additions is theirs.

// A per-column vector (gamma, beta) into the lane's registers: r[c] = the lane's four columns of chunk c.  A lane always owns the same
// columns, so the vector stays in registers across rows.
template <int NC>
MT_DEVINL void load_cols(const float* p, int lane, f32x4 (&r)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) r[c] = Vec4<float>::load(p + c * 256 + lane * 4);
}

// Two-pass statistics of one row.  v: the lane's values; s: the lane's own sum of them, added c ascending, within a chunk
// ((v0 + v1) + v2) + v3.  mean = wave_sum(s) / D; then the centred second moment, q += d * d over c then e, summed over the wave
// the same way; rstd = rsqrt(q / D + eps).  Every lane gets both.
template <int NC>
MT_DEVINL void row_stats(const f32x4 (&v)[NC], float s, float eps, float& mean, float& rstd) {
  constexpr int D = NC * 256;
  mean = wave_sum(s) * (1.0f / D);
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float d = v[c][e] - mean; q += d * d; }
  rstd = rsqrtf(wave_sum(q) * (1.0f / D) + eps);
}

// Normalise and affine of the lane's four columns of one chunk (the expression is contracted as it is written: keep its shape)
MT_DEVINL f32x4 norm_affine(f32x4 v, float mean, float rstd, f32x4 w, f32x4 b) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (v[e] - mean) * rstd * w[e] + b[e];
  return o;
}

// Saved statistics of row m: stats[2 m] = mean, stats[2 m + 1] = rstd.  One lane of the row stores; every lane may load.
MT_DEVINL void store_stats(float* stats, int m, float mean, float rstd) { stats[2 * (long)m] = mean; stats[2 * (long)m + 1] = rstd; }
MT_DEVINL void load_stats(const float* stats, int m, float& mean, float& rstd) { mean = stats[2 * (long)m]; rstd = stats[2 * (long)m + 1]; }

// Column sums over the workgroup's four waves through LDS, `red[wave][col]` (floats only or doubles only per array: one banking
// class, common.h).  put_cols: a lane writes its accumulators acc[c][e] to `row` = its wave's row of LDS, at its own columns.  `row`
// MUST point into a `__shared__` array: the cast names the LDS address space (through a generic pointer the compiler arranges the
// callers' address arithmetic and loop guards another way), and a pointer to anything else is undefined behaviour behind it.
// After a barrier, sum_waves gives column i as ((wave 0 + wave 1) + wave 2) + wave 3; thread t takes the columns i = t, t + 256, ...
template <int NC, typename T, typename A>
MT_DEVINL void put_cols(T* row, int lane, const A (&acc)[NC]) {
  auto* lds = (__attribute__((address_space(3))) T*)row;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) lds[c * 256 + lane * 4 + e] = acc[c][e];
}
template <typename T, int D>
MT_DEVINL T sum_waves(const T (&red)[4][D], int i) { return red[0][i] + red[1][i] + red[2][i] + red[3][i]; }

// ---------------------------------------------------------------- forward -------------------------
struct LnFwdArgs {
  const void* x; long ldx; RowMap xmap;
  const float* w; const float* b; const float* add_rows; int add_period;
  void* y; long ldy; RowMap ymap;
  float* stats; int M;
  float eps;
  const int* live; int live_rows;      // ln_gelu_fwd_kernel: only the rows of the passes [live[0], live[1]) (live_rows rows each); nullptr = all
};

template <int D, typename InT, typename OutT, bool GELU>
__global__ __launch_bounds__(256) void ln_fwd_kernel(LnFwdArgs a) {
  constexpr int NC = D / 256;   // 4-element chunks per lane
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 wr[NC], br[NC];
  load_cols(a.w, lane, wr);
  load_cols(a.b, lane, br);
  for (int m = blockIdx.x * 4 + wave; m < a.M; m += gridDim.x * 4) {
    const InT* x = reinterpret_cast<const InT*>(a.x) + a.xmap.map(m) * a.ldx;
    f32x4 v[NC];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      v[c] = Vec4<InT>::load(x + c * 256 + lane * 4);
      if (GELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[c][e] = gelu_erf(v[c][e]);
      }
      s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
    }
    float mean, rstd;
    row_stats(v, s, a.eps, mean, rstd);
    OutT* y = reinterpret_cast<OutT*>(a.y) + a.ymap.map(m) * a.ldy;
    const float* add = a.add_rows ? a.add_rows + (long)(m % a.add_period) * D : nullptr;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 256 + lane * 4;
      f32x4 o = norm_affine(v[c], mean, rstd, wr[c], br[c]);
      if (add) { const f32x4 p = Vec4<float>::load(add + col); o += p; }
      Vec4<OutT>::store(y + col, o);
    }
    if (a.stats && lane == 0) store_stats(a.stats, m, mean, rstd);
  }
}

// h = x + drop(branch) ; y = LN(h) * w + b.  The residual add of a backbone sub-layer (branch = fp16 output of the
// out_proj / fc2 GEMM, Dropout + DropPath as in the GEMM's BIAS_RESID epilogue: same counters, same masks) rides on the
// LayerNorm that reads the sum anyway: the GEMM keeps a plain fp16 epilogue (MFMA-bound) and the fp32 residual stream
// is read and written by this HBM-bound pass only.
struct AddLnArgs {
  const float* x; const h16* branch; DropArgs drop;
  const float* w; const float* b;
  float* h; h16* y; float* stats; int M;
  float eps;
};

template <int D>
__global__ __launch_bounds__(256) void add_ln_fwd_kernel(AddLnArgs a) {
  constexpr int NC = D / 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 wr[NC], br[NC];
  load_cols(a.w, lane, wr);
  load_cols(a.b, lane, br);
  const bool dropping = a.drop.active();
  for (int m = blockIdx.x * 4 + wave; m < a.M; m += gridDim.x * 4) {
    const float* x = a.x + (long)m * D;
    const h16* bp = a.branch + (long)m * D;
    f32x4 v[NC], bv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      v[c] = Vec4<float>::load(x + c * 256 + lane * 4);
      bv[c] = Vec4<h16>::load(bp + c * 256 + lane * 4);
    }
    const float pf = dropping ? drop_path_factor(a.drop, m / a.drop.rows_per_pass) : 1.f;
    float s = 0.f;
    float* hrow = a.h + (long)m * D;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 256 + lane * 4;
      // (a dropped pass -- wave-uniform -- is selected to 0, not multiplied by it: its branch rows may never have been written)
      if (dropping) bv[c] = pf != 0.f ? bv[c] * drop_elem4(a.drop, ((uint64_t)m * D + col) >> 2, pf) : (f32x4){0.f, 0.f, 0.f, 0.f};
      v[c] += bv[c];
      Vec4<float>::store(hrow + col, v[c]);
      s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
    }
    float mean, rstd;
    row_stats(v, s, a.eps, mean, rstd);
    h16* y = a.y + (long)m * D;
#pragma unroll
    for (int c = 0; c < NC; ++c) Vec4<h16>::store(y + c * 256 + lane * 4, norm_affine(v[c], mean, rstd, wr[c], br[c]));
    if (lane == 0) store_stats(a.stats, m, mean, rstd);
  }
}

// ---------------------------------------------------------------- pooled read-out -------------------
// out[b, :] = LN_post( 1 / (r1 - r0) * sum_{r in [r0, r1)} LN_pre( x[b, r, :] ) )  (mt_layernorm_pool_fwd, include/modaltune_hip.h).
// Stage 1, grid (G, B): workgroup g of pass b owns the rows r0 + [g * POOL_WG_ROWS, (g + 1) * POOL_WG_ROWS) of the range; wave w walks
// the rows w, w + 4, ... of that share in ascending order -- LN_pre by the row stages above (one wave per row, fp32 mean, centred second
// moment), then the row is added to the lane's twelve DOUBLE column accumulators.  The four waves are added in ascending order through
// LDS (doubles only: one LDS banking class, common.h).  G == 1: the workgroup finishes the pass itself; else it stores its D sums to
// its own slot of the workspace and stage 2, one workgroup per pass, adds the G slots in ascending order.  Which rows a lane adds, and
// in which order, is a function of (r1 - r0, D) alone; no atomic executes.
constexpr int POOL_WG_ROWS = 64, POOL_D = 768;

struct LnPoolArgs {
  const float* x; long ldx; int rows_per_pass, r0, n;      // n = r1 - r0
  const float* pre_w; const float* pre_b; float pre_eps;
  const float* post_w; const float* post_b; float post_eps;
  float* out; double* partials; int G;
};

// sum over the workgroup, every thread gets it; `red`: 4 doubles of LDS.  Two barriers: `red` may be reused right after.
MT_DEVINL float pool_block_sum(float v, double* red) {
  const float w = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (double)w;
  __syncthreads();
  const float s = (float)red[0] + (float)red[1] + (float)red[2] + (float)red[3];
  __syncthreads();
  return s;
}

// colsum: the D column sums of pass b in LDS (complete, barrier passed).  Thread t owns the columns t, t + 256, t + 512 -- not the
// layout of the row stages, so this LayerNorm is written out here: the mean is rounded to fp32 once, LN_post (optional) takes the
// statistics of the fp32 vector the way row_stats does, over the workgroup.
MT_DEVINL void pool_finish(const LnPoolArgs& a, int b, const double* colsum, double* red) {
  constexpr int D = POOL_D, NJ = D / 256;
  const double inv_n = 1.0 / (double)a.n;
  float p[NJ];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) { p[j] = (float)(colsum[threadIdx.x + 256 * j] * inv_n); s += p[j]; }
  float* out = a.out + (long)b * D;
  if (!a.post_w) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) out[threadIdx.x + 256 * j] = p[j];
    return;
  }
  const float mean = pool_block_sum(s, red) * (1.0f / D);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) { const float d = p[j] - mean; q += d * d; }
  const float rstd = rsqrtf(pool_block_sum(q, red) * (1.0f / D) + a.post_eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = threadIdx.x + 256 * j;
    out[col] = (p[j] - mean) * rstd * a.post_w[col] + a.post_b[col];
  }
}

template <bool PRE>
__global__ __launch_bounds__(256) void ln_pool_rows_kernel(LnPoolArgs a) {
  constexpr int D = POOL_D, NC = D / 256;
  __shared__ double acc_lds[4][D];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y, g = blockIdx.x;
  f32x4 wr[NC], br[NC];
  if (PRE) {
    load_cols(a.pre_w, lane, wr);
    load_cols(a.pre_b, lane, br);
  }
  double acc[NC][4];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[c][e] = 0.0;
  const int i_end = min(a.n, (g + 1) * POOL_WG_ROWS);
  for (int i = g * POOL_WG_ROWS + wave; i < i_end; i += 4) {
    const float* x = a.x + ((long)b * a.rows_per_pass + a.r0 + i) * a.ldx;
    f32x4 v[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) v[c] = Vec4<float>::load(x + c * 256 + lane * 4);
    if (PRE) {
      float s = 0.f, mean, rstd;
#pragma unroll
      for (int c = 0; c < NC; ++c) s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
      row_stats(v, s, a.pre_eps, mean, rstd);
#pragma unroll
      for (int c = 0; c < NC; ++c) v[c] = norm_affine(v[c], mean, rstd, wr[c], br[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[c][e] += (double)v[c][e];
  }
  put_cols(acc_lds[wave], lane, acc);
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += 256) {
    const double t = sum_waves(acc_lds, i);
    if (a.G > 1) a.partials[((long)b * a.G + g) * D + i] = t;
    else acc_lds[0][i] = t;          // (column i is read and written by this thread alone)
  }
  if (a.G > 1) return;               // (uniform over the grid)
  __syncthreads();
  pool_finish(a, b, acc_lds[0], red);
}

__global__ __launch_bounds__(256) void ln_pool_final_kernel(LnPoolArgs a) {
  constexpr int D = POOL_D;
  __shared__ double colsum[D];
  __shared__ double red[4];
  const int b = blockIdx.x;
  const double* slot = a.partials + (long)b * a.G * D;
  for (int i = threadIdx.x; i < D; i += 256) {
    double t = slot[i];
    for (int g = 1; g < a.G; ++g) t += slot[(long)g * D + i];
    colsum[i] = t;
  }
  __syncthreads();
  pool_finish(a, b, colsum, red);
}

// ---------------------------------------------------------------- backward ------------------------
struct LnBwdArgs {
  const void* dy; long lddy; RowMap dymap;
  const void* x; long ldx; RowMap xmap;
  const float* w; const float* stats;
  void* dx; long lddx; RowMap dxmap; int accumulate;
  float* dw; float* db; h16* dx16; DropArgs drop16; int M;
  // live table entry of the residual branch this LayerNorm closes, live_rows rows per pass (nullptr = every pass is live).
  // ln_bwd_kernel: dy of a row outside the live passes counts as zero (its bytes are stale); ln_gelu_bwd_kernel walks the live rows only
  const int* live; int live_rows;
};

// DET (deterministic mode, det_reduce.hip): a.dw is the partial workspace [gridDim.x][2][D]; workgroup blockIdx.x stores its dw | db
// sums to slot blockIdx.x with plain stores
// LIVE (a.live != nullptr; the launcher picks): without it the kernel is what it was before the live table existed -- a null check of
// a.live at the top cost a serialized kernel-argument fetch per wave, 5 % of this two-rows-per-wave kernel inside the step.
template <int D, typename DyT, typename InT, typename DxT, bool GELU, bool PARAM, bool DET = false, bool LIVE = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(LnBwdArgs a) {
  constexpr int NC = D / 256;
  constexpr int NP = PARAM ? NC : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 gw[NP], gb[NP];
#pragma unroll
  for (int c = 0; c < NP; ++c) { gw[c] = (f32x4){0.f, 0.f, 0.f, 0.f}; gb[c] = gw[c]; }
  f32x4 wr[NC];
  load_cols(a.w, lane, wr);
  for (int m = blockIdx.x * 4 + wave; m < a.M; m += gridDim.x * 4) {
    const DyT* dy = reinterpret_cast<const DyT*>(a.dy) + a.dymap.map(m) * a.lddy;
    const InT* x = reinterpret_cast<const InT*>(a.x) + a.xmap.map(m) * a.ldx;
    float mean, rstd;
    load_stats(a.stats, m, mean, rstd);
    f32x4 xh[NC], g[NC], raw[GELU ? NC : 1];
    float s1 = 0.f, s2 = 0.f;
    // LIVE: dy of a row outside the live passes is masked to +0 bit by bit behind an UNCONDITIONAL load (a `dead ? 0 : load` select
    // makes hipcc branch around every load and wait for each one separately: 7 - 25 % on this kernel inside the step).  The table is read
    // in the loop, behind the row's first loads (the compiler barrier keeps it there): read in front of the loop, every wave would wait
    // for it before it issues anything.
    uint32_t keep = 0xFFFFFFFFu;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 256 + lane * 4;
      f32x4 xv = Vec4<InT>::load(x + col);
      if (GELU) {
        raw[c] = xv;
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[e] = gelu_erf(xv[e]);
      }
      f32x4 d = Vec4<DyT>::load(dy + col);
      if constexpr (LIVE) {
        if (c == 0) {
          asm volatile("" ::: "memory");
          const RowRange lr = live_rows_of(a.live, a.live_rows, a.M);      // (clamped like every other reader of the table)
          keep = (m >= lr.first && m < lr.end) ? 0xFFFFFFFFu : 0u;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = __uint_as_float(__float_as_uint(d[e]) & keep);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xh[c][e] = (xv[e] - mean) * rstd;
        g[c][e] = d[e] * wr[c][e];
        s1 += g[c][e];
        s2 += g[c][e] * xh[c][e];
      }
      if (PARAM) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { gw[c][e] += d[e] * xh[c][e]; gb[c][e] += d[e]; }
      }
    }
    const float c1 = wave_sum(s1) * (1.0f / D), c2 = wave_sum(s2) * (1.0f / D);
    DxT* dx = reinterpret_cast<DxT*>(a.dx) + a.dxmap.map(m) * a.lddx;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 256 + lane * 4;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = rstd * (g[c][e] - c1 - xh[c][e] * c2);
        if (GELU) o[e] *= gelu_erf_grad(raw[c][e]);
      }
      if (a.accumulate) { const f32x4 old = Vec4<DxT>::load(dx + col); o += old; }
      Vec4<DxT>::store(dx + col, o);
      if (a.dx16) {
        if (a.drop16.active()) o *= drop_scale4(a.drop16, ((uint64_t)m * D + col) >> 2, m);
        Vec4<h16>::store(a.dx16 + (long)m * D + col, o);
      }
    }
  }
  if (PARAM) {
    __shared__ float red[2][4][D];
    // Not put_cols(red[0]..) then put_cols(red[1]..): two calls would change the LDS store opcodes (ds_write_b128 instead of the
    // ds_write2_b32 of this interleaved dw | db loop), so the loop is kept as it was (profiles/norm_stages.txt).
#pragma unroll
    for (int c = 0; c < NP; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        red[0][wave][c * 256 + lane * 4 + e] = gw[c][e];
        red[1][wave][c * 256 + lane * 4 + e] = gb[c][e];
      }
    __syncthreads();
    for (int i = threadIdx.x; i < D; i += 256) {
      const float sw = sum_waves(red[0], i), sb = sum_waves(red[1], i);
      if constexpr (DET) {
        float* slot = a.dw + (long)blockIdx.x * (2 * D);
        slot[i] = sw;
        slot[D + i] = sb;
      } else {
        atomicAdd(&a.dw[i], sw);
        atomicAdd(&a.db[i], sb);
      }
    }
  }
}

// ---------------------------------------------------------------- FFN sub-LayerNorm ---------------
// y = LN(gelu(a1)) over D = 3072 (feedforward_network.py:136-139) and its backward, fp16 in / fp16 out.  These two
// launches stream 0.37 / 0.55 GB per layer and were co-bound by the VALU (erf twice per element, scalar fp32 ops, the
// affine vectors re-read per row): here a lane owns 8 consecutive columns per chunk (16-byte loads/stores), keeps
// gamma/beta in registers across rows, evaluates erf ONCE for both gelu and gelu', and does the arithmetic with packed
// fp32 instructions (v_pk_fma/mul/add_f32).  Another column layout than the row stages above, and statistics that cross a wave pair
// or triple through LDS with barrier counts of their own: of the row stages only the statistics store is shared.
MT_DEVINL f32x2 pk_fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
MT_DEVINL f32x2 splat2(float v) { return (f32x2){v, v}; }

// gelu(x) and d gelu / dx for two values; A&S 7.1.26 erf as in common.h (|err| <= 1.5e-7), its constants from there
template <bool WANT_GRAD>
MT_DEVINL void gelu_pair(f32x2 x, f32x2& g, f32x2& dg) {
  const f32x2 ax = {fabsf(x[0]), fabsf(x[1])};
  const f32x2 z = ax * splat2(MT_RSQRT2);
  const f32x2 den = pk_fma2(z, splat2(MT_ERF_P), splat2(1.0f));
  const f32x2 t = {__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
  f32x2 poly = pk_fma2(t, splat2(MT_ERF_A5), splat2(MT_ERF_A4));
  poly = pk_fma2(poly, t, splat2(MT_ERF_A3));
  poly = pk_fma2(poly, t, splat2(MT_ERF_A2));
  poly = pk_fma2(poly, t, splat2(MT_ERF_A1));
  poly = poly * t;
  const f32x2 ea = z * z * splat2(-MT_LOG2E);
  const f32x2 e = {__builtin_amdgcn_exp2f(ea[0]), __builtin_amdgcn_exp2f(ea[1])};
  const f32x2 r = pk_fma2(-poly, e, splat2(1.0f));                 // erf(|x| / sqrt 2)
  const f32x2 er = {copysignf(r[0], x[0]), copysignf(r[1], x[1])};
  const f32x2 h = pk_fma2(er, splat2(0.5f), splat2(0.5f));          // Phi(x)
  g = x * h;
  if (WANT_GRAD) dg = pk_fma2(x * splat2(MT_RSQRT_2PI), e, h);   // Phi(x) + x phi(x)
}

MT_DEVINL void cvt8(h16x8 v, f32x2 (&o)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (f32x2){(float)v[2 * i], (float)v[2 * i + 1]};
}
MT_DEVINL h16x8 pack8(const f32x2 (&o)[4]) {
  h16x8 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[2 * i] = (h16)o[i][0]; v[2 * i + 1] = (h16)o[i][1]; }
  return v;
}
MT_DEVINL void ldf8(const float* p, f32x2 (&o)[4]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
  o[0] = (f32x2){a[0], a[1]}; o[1] = (f32x2){a[2], a[3]}; o[2] = (f32x2){b[0], b[1]}; o[3] = (f32x2){b[2], b[3]};
}

// Two waves per row (a lane owns D / 128 columns in chunks of 8): ~100 VGPRs, 4-5 waves per SIMD of loads in flight.
// Row statistics cross the wave pair through LDS.
template <int D, bool LIVE = false>
__global__ __launch_bounds__(256) void ln_gelu_fwd_kernel(LnFwdArgs a) {
  constexpr int NC = D / 1024;   // 8-element chunks per lane
  __shared__ float red[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = wave & 1, rsel = wave >> 1;
  const int col0 = half * (D / 2) + lane * 8;
  f32x2 wr[NC][4], br[NC][4];
#pragma unroll
  for (int c = 0; c < NC; ++c) { ldf8(a.w + col0 + c * 512, wr[c]); ldf8(a.b + col0 + c * 512, br[c]); }
  const RowRange lr = live_rows_of(LIVE ? a.live : nullptr, a.live_rows, a.M);      // (uniform over the workgroup: the barriers below stay aligned)
  for (int base = lr.first + blockIdx.x * 2; base < lr.end; base += gridDim.x * 2) {
    const int m = base + rsel;
    const bool valid = m < lr.end;
    const int mc = valid ? m : lr.end - 1;
    const h16* x = reinterpret_cast<const h16*>(a.x) + a.xmap.map(mc) * a.ldx;
    h16x8 raw[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) raw[c] = ldg8(x + col0 + c * 512);
    f32x2 v[NC][4];
    f32x2 s2 = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      f32x2 xv[4];
      cvt8(raw[c], xv);
#pragma unroll
      for (int i = 0; i < 4; ++i) { f32x2 dg; gelu_pair<false>(xv[i], v[c][i], dg); s2 += v[c][i]; }
    }
    const float ps = wave_sum(s2[0] + s2[1]);
    if (lane == 0) red[0][wave] = ps;
    __syncthreads();
    const float mean = (red[0][2 * rsel] + red[0][2 * rsel + 1]) * (1.0f / D);
    f32x2 q2 = {0.f, 0.f};
    const f32x2 nm = splat2(-mean);
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) { v[c][i] += nm; q2 = pk_fma2(v[c][i], v[c][i], q2); }
    const float pq = wave_sum(q2[0] + q2[1]);
    if (lane == 0) red[1][wave] = pq;
    __syncthreads();
    const float rstd = rsqrtf((red[1][2 * rsel] + red[1][2 * rsel + 1]) * (1.0f / D) + a.eps);
    if (valid) {
      h16* y = reinterpret_cast<h16*>(a.y) + a.ymap.map(m) * a.ldy;
      const f32x2 rs = splat2(rstd);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        f32x2 o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = pk_fma2(v[c][i] * rs, wr[c][i], br[c][i]);
        stg8(y + col0 + c * 512, pack8(o));
      }
      if (a.stats && lane == 0 && half == 0) store_stats(a.stats, m, mean, rstd);
    }
  }
}

// backward: WPR waves per row (a lane owns D / (64 WPR) columns in chunks of 8), one row per workgroup iteration
template <int D, int WPR, bool LIVE = false>
__global__ __launch_bounds__(64 * WPR) void ln_gelu_bwd_kernel(LnBwdArgs a) {
  constexpr int NC = D / (512 * WPR);
  static_assert(NC * 512 * WPR == D, "row must split into 8-element chunks over the waves");
  __shared__ float red[2][2][WPR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col0 = wave * (D / WPR) + lane * 8;
  f32x2 wr[NC][4];
#pragma unroll
  for (int c = 0; c < NC; ++c) ldf8(a.w + col0 + c * 512, wr[c]);
  int it = 0;
  const RowRange lr = live_rows_of(LIVE ? a.live : nullptr, a.live_rows, a.M);      // (uniform over the workgroup: one barrier per row, as before)
  for (int m = lr.first + blockIdx.x; m < lr.end; m += gridDim.x, it ^= 1) {
    const h16* dy = reinterpret_cast<const h16*>(a.dy) + a.dymap.map(m) * a.lddy;
    const h16* x = reinterpret_cast<const h16*>(a.x) + a.xmap.map(m) * a.ldx;
    h16x8 rx[NC], rd[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { rx[c] = ldg8(x + col0 + c * 512); rd[c] = ldg8(dy + col0 + c * 512); }
    float mean, rstd;
    load_stats(a.stats, m, mean, rstd);
    const f32x2 rs = splat2(rstd), nmr = splat2(-mean * rstd);
    f32x2 xh[NC][4], g[NC][4], dgl[NC][4];
    f32x2 s1 = {0.f, 0.f}, s2 = {0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      f32x2 xv[4], dv[4];
      cvt8(rx[c], xv); cvt8(rd[c], dv);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        f32x2 gl;
        gelu_pair<true>(xv[i], gl, dgl[c][i]);
        xh[c][i] = pk_fma2(gl, rs, nmr);
        g[c][i] = dv[i] * wr[c][i];
        s1 += g[c][i];
        s2 = pk_fma2(g[c][i], xh[c][i], s2);
      }
    }
    const float p1 = wave_sum(s1[0] + s1[1]), p2 = wave_sum(s2[0] + s2[1]);
    if (lane == 0) { red[it][0][wave] = p1; red[it][1][wave] = p2; }      // double-buffered: one barrier per row
    __syncthreads();
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < WPR; ++w2) { c1 += red[it][0][w2]; c2 += red[it][1][w2]; }
    c1 *= (1.0f / D); c2 *= (1.0f / D);
    h16* dx = reinterpret_cast<h16*>(a.dx) + a.dxmap.map(m) * a.lddx;
    const f32x2 nc1 = splat2(-c1), nc2 = splat2(-c2);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      f32x2 o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (pk_fma2(xh[c][i], nc2, g[c][i]) + nc1) * (dgl[c][i] * rs);
      if (a.accumulate) {
        f32x2 old[4];
        cvt8(ldg8(dx + col0 + c * 512), old);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] += old[i];
      }
      stg8(dx + col0 + c * 512, pack8(o));
    }
  }
}

// ---------------------------------------------------------------- injector residual backward ------
// y = (1+g) x + g * proj  (A.1), with proj = out(a) recomputed in fp16:
//   dx (+)= (1+g) dy ; dproj = g * dy (fp16, feeds the dX/dW GEMMs) ; dgamma += sum_m dy * (x + proj)
struct InjBwdArgs {
  const float* dy; long lddy; RowMap dymap;
  const float* x; long ldx; RowMap xmap;
  const h16* proj; const float* gamma;
  float* dx; long lddx; RowMap dxmap; int dx_accumulate;
  h16* dproj; float* dgamma; int M;
};
// DET (deterministic mode): a.dgamma is the partial workspace [gridDim.x][D], slot = blockIdx.x, plain stores
template <int D, bool DET = false>
__global__ __launch_bounds__(256) void inject_resid_bwd_kernel(InjBwdArgs a) {
  constexpr int NC = D / 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 gg[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) gg[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int m = blockIdx.x * 4 + wave; m < a.M; m += gridDim.x * 4) {
    const float* dy = a.dy + a.dymap.map(m) * a.lddy;
    const float* x = a.x + a.xmap.map(m) * a.ldx;
    const h16* pr = a.proj + (long)m * D;
    float* dx = a.dx + a.dxmap.map(m) * a.lddx;
    h16* dp = a.dproj + (long)m * D;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = c * 256 + lane * 4;
      const f32x4 d = Vec4<float>::load(dy + col), xv = Vec4<float>::load(x + col), p = Vec4<h16>::load(pr + col);
      const f32x4 gm = Vec4<float>::load(a.gamma + col);
      f32x4 o, q;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (1.0f + gm[e]) * d[e];
        q[e] = gm[e] * d[e];
        gg[c][e] += d[e] * (xv[e] + p[e]);
      }
      if (a.dx_accumulate) o += Vec4<float>::load(dx + col);
      Vec4<float>::store(dx + col, o);
      Vec4<h16>::store(dp + col, q);
    }
  }
  __shared__ float red[4][D];
  put_cols(red[wave], lane, gg);
  __syncthreads();
  for (int i = threadIdx.x; i < D; i += 256) {
    if constexpr (DET) a.dgamma[(long)blockIdx.x * D + i] = sum_waves(red, i);
    else atomicAdd(&a.dgamma[i], sum_waves(red, i));
  }
}

// ---------------------------------------------------------------- elementwise ---------------------
__global__ void cast_drop_f32_f16_kernel(const float* x, h16* y, long n, DropArgs d, int D) {    // n % 4 == 0, D % 4 == 0
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (; i < n; i += stride) {
    f32x4 v = Vec4<float>::load(x + i);
    v *= drop_scale4(d, (uint64_t)i >> 2, (int)(i / D));
    Vec4<h16>::store(y + i, v);
  }
}
// y(m,:) = drop(x(xmap(m),:)), dense fp32 y
__global__ void dropout_f32_kernel(const float* x, long ldx, RowMap xmap, float* y, int M, int D, DropArgs d) {
  const int per_row = D / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)M * per_row; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / per_row), c = (int)(i % per_row) * 4;
    f32x4 v = Vec4<float>::load(x + xmap.map(m) * ldx + c);
    v *= drop_scale4(d, ((uint64_t)m * D + c) >> 2, m);
    Vec4<float>::store(y + (long)m * D + c, v);
  }
}
__global__ void droppath_rows_kernel(float* x, int M, int D, DropArgs d) {
  const int per_row = D / 4;
  DropArgs dd = d;
  dd.p = 0.f;                           // path factor only
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)M * per_row; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / per_row), c = (int)(i % per_row) * 4;
    f32x4 v = Vec4<float>::load(x + (long)m * D + c);
    v *= drop_scale4(dd, 0, m);
    Vec4<float>::store(x + (long)m * D + c, v);
  }
}
// live table (include/modaltune_hip.h: mt_droppath_live): thread i evaluates the B draws of site i and stores their hull
struct LiveSites { int n; unsigned site[MT_LIVE_SITES_MAX]; float p[MT_LIVE_SITES_MAX]; };
__global__ void droppath_live_kernel(LiveSites ls, int B, const uint32_t* rng, int* table) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ls.n) return;
  DropArgs d;
  d.rng = rng; d.site = 0; d.p = 0.f; d.path_site = ls.site[i]; d.path_p = ls.p[i]; d.rows_per_pass = 1;
  int b0 = 0, b1 = 0;
  for (int b = 0; b < B; ++b)
    if (drop_path_factor(d, b) != 0.f) {
      if (b1 == 0) b0 = b;
      b1 = b + 1;
    }
  table[2 * i] = b0; table[2 * i + 1] = b1;
}

__global__ void rng_advance_kernel(uint32_t* rng) { if (threadIdx.x == 0 && blockIdx.x == 0) rng[2] += 1u; }

__global__ void cast_f32_f16_kernel(const float* x, h16* y, long n) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (; i + 3 < n; i += stride) Vec4<h16>::store(y + i, Vec4<float>::load(x + i));
  if (i < n && i + 3 >= n) for (long j = i; j < n; ++j) y[j] = (h16)x[j];
}
__global__ void cast_f16_f32_kernel(const h16* x, float* y, long n) {
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (; i + 3 < n; i += stride) Vec4<float>::store(y + i, Vec4<h16>::load(x + i));
  if (i < n && i + 3 >= n) for (long j = i; j < n; ++j) y[j] = (float)x[j];
}
__global__ void act_fwd_kernel(const float* x, float* y, long n, int act) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = x[i];
    y[i] = act == MT_ACT_RELU ? fmaxf(v, 0.f) : act == MT_ACT_GELU ? gelu_erf(v) : act == MT_ACT_ELU ? (v > 0.f ? v : expm1f(v)) : v;
  }
}
__global__ void act_bwd_kernel(const float* x, const float* dy, float* dx, long n, int act) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = x[i];
    float d = 1.f;
    if (act == MT_ACT_RELU) d = v > 0.f ? 1.f : 0.f;
    else if (act == MT_ACT_GELU) d = gelu_erf_grad(v);
    else if (act == MT_ACT_ELU) d = v > 0.f ? 1.f : __expf(v);
    dx[i] = dy[i] * d;
  }
}
__global__ void axpy_kernel(const float* a, const float* b, float alpha, float* y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = a[i] + alpha * b[i];
}
__global__ void axpy_bcast_kernel(const float* a, const float* b, float alpha, float* y, long n, long period) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = a[i] + alpha * b[i % period];
}
// out[i] += sum_r x[r * period + i], r ascending: the adjoint of axpy_bcast (period % 4 == 0, 16-byte aligned)
__global__ void fold_rows_kernel(const float* __restrict__ x, int reps, long period, float* __restrict__ out) {
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < period; i += (long)gridDim.x * blockDim.x * 4) {
    f32x4 s = *reinterpret_cast<const f32x4*>(x + i);
    for (int r = 1; r < reps; ++r) s += *reinterpret_cast<const f32x4*>(x + r * period + i);
    *reinterpret_cast<f32x4*>(out + i) += s;
  }
}
__global__ void copy_rows_kernel(const float* src, long lds, RowMap smap, float* dst, long ldd, RowMap dmap, int M,
                                 int D, int accumulate) {
  const int per_row = D / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)M * per_row; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / per_row), c = (int)(i % per_row) * 4;
    f32x4 v = Vec4<float>::load(src + smap.map(m) * lds + c);
    float* d = dst + dmap.map(m) * ldd + c;
    if (accumulate) v += Vec4<float>::load(d);
    Vec4<float>::store(d, v);
  }
}

// ---------------------------------------------------------------- weight packers ------------------
// fp32 [R, C] -> fp16 [R, C] (transpose = 0) or fp16 [C, R] (transpose = 1), 32x32 tiles through LDS
__global__ __launch_bounds__(256) void pack_f16_kernel(const float* __restrict__ src, int R, int C, h16* __restrict__ dst, int transpose) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    tile[ty + 8 * i][tx] = (r < R && c < C) ? src[(long)r * C + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (transpose) {
      const int c = c0 + ty + 8 * i, r = r0 + tx;
      if (r < R && c < C) dst[(long)c * R + r] = (h16)tile[tx][ty + 8 * i];
    } else {
      const int r = r0 + ty + 8 * i, c = c0 + tx;
      if (r < R && c < C) dst[(long)r * C + c] = (h16)tile[ty + 8 * i][tx];
    }
  }
}

// grouped form: blockIdx.x = item (8 int64 per record, see mt_pack_weights_f16), blockIdx.y strides over its 32x32 tiles;
// one pass writes both the as-stored and the transposed fp16 copy
__global__ __launch_bounds__(256) void pack_group_kernel(const long long* __restrict__ items) {
  __shared__ float tile[32][33];
  const long long* it = items + (long)blockIdx.x * 8;
  const float* src = reinterpret_cast<const float*>(it[0]);
  h16* dst = reinterpret_cast<h16*>(it[1]);
  h16* dst_t = reinterpret_cast<h16*>(it[2]);
  const int R = (int)it[3], C = (int)it[4], roff = (int)it[5];
  const long ld = it[6], ld_t = it[7];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int tiles_c = (C + 31) / 32, tiles = ((R + 31) / 32) * tiles_c;
  for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
    const int r0 = (t / tiles_c) * 32, c0 = (t % tiles_c) * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + ty + 8 * i, c = c0 + tx;
      const float v = (r < R && c < C) ? src[(long)r * C + c] : 0.f;
      tile[ty + 8 * i][tx] = v;
      if (dst && r < R && c < C) dst[(long)(roff + r) * ld + c] = (h16)v;
    }
    __syncthreads();
    if (dst_t) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (r < R && c < C) dst_t[(long)c * ld_t + roff + r] = (h16)tile[tx][ty + 8 * i];
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- grids and dispatch --------------
// Every launcher of this file ends here: launch, check, status.
template <typename K, typename... Args>
int launch(K kernel, dim3 grid, dim3 block, hipStream_t s, const Args&... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

// Workgroups per launch.  Whatever sizes a partial workspace asks the function that the launch asks.
int ew_grid(long n) { return (int)max(1L, min((n + 1023) / 1024, 4096L)); }
int ln_grid(int M) { return max(1, min(cdiv(M, 4), 4096)); }       // one wave per row, four rows per workgroup
int ln_param_grid(int M) { return min(ln_grid(M), 512); }          // PARAM / DET forms of ln_bwd_kernel: workgroups = partial slots [2][D]
int inj_grid(int M) { return min(cdiv(M, 4), 512); }               // inject_resid_bwd_kernel: workgroups = partial slots [D]
int ln_gelu_grid(int M) { return max(1, min(cdiv(M, 2), 8192)); }  // packed forward: two rows per workgroup
int ln_gelu_bwd_grid(int M) { return min(M, 16384); }              // packed backward: one row per workgroup
int ln_pool_groups(int n) { return cdiv(n, POOL_WG_ROWS); }

// The widths the LayerNorm kernels are built for: f(std::integral_constant<int, D>) at a supported D, MT_ERR_UNSUPPORTED otherwise.
template <typename F>
int with_ln_width(int D, F&& f) {
  switch (D) {
    case 256: return f(std::integral_constant<int, 256>{});
    case 768: return f(std::integral_constant<int, 768>{});
    case 2304: return f(std::integral_constant<int, 2304>{});
    case 3072: return f(std::integral_constant<int, 3072>{});
    default: return MT_ERR_UNSUPPORTED;
  }
}
bool ln_width_ok(int D) { return with_ln_width(D, [](auto) { return (int)MT_OK; }) == MT_OK; }

// live / live_rows of the options (MT_OPT_LIVE); a table without its rows per pass is malformed
struct LiveOpt {
  const int* live; int rows;
  bool malformed() const { return live && rows < 1; }
};
LiveOpt live_opt(const MtLaunchOpts* o) { return {mt_opt_live(o), o ? o->live_rows : 0}; }

// The packed pair takes D % 1024 == 0 (the `if constexpr` at its callers: no other width instantiates it), fp16 throughout, 16-byte
// rows -- and what is listed here; the packed form alone walks a live range.
bool ln_gelu_fwd_ok(const LnFwdArgs& a, int in_dt, int out_dt, int gelu) {
  return gelu && in_dt == MT_OUT_F16 && out_dt == MT_OUT_F16 && !a.add_rows && !(a.ldx & 7) && !(a.ldy & 7);
}
bool ln_gelu_bwd_ok(const LnBwdArgs& a, bool dyh, bool inh, bool dxh) {      // (asked under gelu)
  return dyh && inh && dxh && !a.dw && !(a.lddy & 7) && !(a.ldx & 7) && !(a.lddx & 7);
}

template <int D, typename InT, typename OutT>
int ln_fwd_dispatch(const LnFwdArgs& a, int gelu, hipStream_t s) {
  return launch(gelu ? ln_fwd_kernel<D, InT, OutT, true> : ln_fwd_kernel<D, InT, OutT, false>, dim3(ln_grid(a.M)), dim3(256), s, a);
}
template <int D>
int ln_fwd_types(const LnFwdArgs& a, int in_dt, int out_dt, int gelu, hipStream_t s) {
  if constexpr (D % 1024 == 0) {
    if (ln_gelu_fwd_ok(a, in_dt, out_dt, gelu))
      return launch(a.live ? ln_gelu_fwd_kernel<D, true> : ln_gelu_fwd_kernel<D>, dim3(ln_gelu_grid(a.M)), dim3(256), s, a);
  }
  if (a.live) return MT_ERR_UNSUPPORTED;      // (only the form above walks a live range)
  if (in_dt == MT_OUT_F32 && out_dt == MT_OUT_F16) return ln_fwd_dispatch<D, float, h16>(a, gelu, s);
  if (in_dt == MT_OUT_F32 && out_dt == MT_OUT_F32) return ln_fwd_dispatch<D, float, float>(a, gelu, s);
  if (in_dt == MT_OUT_F16 && out_dt == MT_OUT_F16) return ln_fwd_dispatch<D, h16, h16>(a, gelu, s);
  return MT_ERR_UNSUPPORTED;
}

template <int D, typename DyT, typename InT, typename DxT, bool GELU>
int ln_bwd_launch(const LnBwdArgs& a, hipStream_t s, bool det) {
  // dw / db exist for the trainable norms: the token side (fp32 dy) and the adapters' 768-wide norms over the patch rows
  constexpr bool HAS_PARAM = (!GELU && sizeof(DyT) == 4) || (D <= 768 && !GELU);
  const dim3 block(256);
  if (a.dw) {
    if constexpr (HAS_PARAM) {
      return launch(det ? ln_bwd_kernel<D, DyT, InT, DxT, GELU, true, true> : ln_bwd_kernel<D, DyT, InT, DxT, GELU, true>,
                    dim3(ln_param_grid(a.M)), block, s, a);
    } else {
      return MT_ERR_UNSUPPORTED;
    }
  }
  return launch(a.live ? ln_bwd_kernel<D, DyT, InT, DxT, GELU, false, false, true> : ln_bwd_kernel<D, DyT, InT, DxT, GELU, false>,
                dim3(ln_grid(a.M)), block, s, a);
}

template <int D>
int ln_bwd_types(const LnBwdArgs& a, int dy_dt, int in_dt, int dx_dt, int gelu, hipStream_t s, bool det) {
  const bool dyh = dy_dt == MT_OUT_F16, inh = in_dt == MT_OUT_F16, dxh = dx_dt == MT_OUT_F16;
  if (gelu) {
    if constexpr (D % 1024 == 0) {
      if (ln_gelu_bwd_ok(a, dyh, inh, dxh)) {
        constexpr int WPR = (D % 1536 == 0) ? 3 : 2;        // 3072 -> three waves per row (16 columns per lane)
        return launch(a.live ? ln_gelu_bwd_kernel<D, WPR, true> : ln_gelu_bwd_kernel<D, WPR>, dim3(ln_gelu_bwd_grid(a.M)), dim3(64 * WPR),
                      s, a);
      }
    }
    if (a.live) return MT_ERR_UNSUPPORTED;      // (a GELU input means a LayerNorm INSIDE a branch: only the form above walks a live range)
    if (dyh && inh && dxh) return ln_bwd_launch<D, h16, h16, h16, true>(a, s, det);
    return MT_ERR_UNSUPPORTED;
  }
  if (dyh && !inh && !dxh) return ln_bwd_launch<D, h16, float, float, false>(a, s, det);
  if (dyh && !inh && dxh) return ln_bwd_launch<D, h16, float, h16, false>(a, s, det);
  if (!dyh && !inh && !dxh) return ln_bwd_launch<D, float, float, float, false>(a, s, det);
  return MT_ERR_UNSUPPORTED;
}

}  // namespace

// ---------------------------------------------------------------- C entry points ------------------
extern "C" int mt_layernorm_fwd(const void* x, long ldx, const MtRowMap* xmap, int in_dtype, int gelu_in,
                                const float* w, const float* b, const float* add_rows, int add_period, void* y,
                                long ldy, const MtRowMap* ymap, int out_dtype, float* stats, int M, int D,
                                const MtLaunchOpts* opt, mt_stream_t stream) {
  if (int rc = mt_opts_check(opt, MT_OPT_EPS | MT_OPT_LIVE)) return rc;
  const LiveOpt lv = live_opt(opt);
  if (!x || !y || !w || !b || M <= 0 || (ldx & 3) || (ldy & 3) || lv.malformed()) return MT_ERR_BAD_ARG;
  const LnFwdArgs a{x, ldx, make_rowmap(xmap), w, b, add_rows, add_period > 0 ? add_period : 1, y, ldy, make_rowmap(ymap), stats, M,
                    mt_opt_eps(opt), lv.live, lv.rows};
  return with_ln_width(D, [&](auto d) { return ln_fwd_types<d()>(a, in_dtype, out_dtype, gelu_in, (hipStream_t)stream); });
}

extern "C" int mt_add_layernorm_fwd(const float* x, const mt_half* branch, const MtDropout* drop, const float* w,
                                    const float* b, float* h, mt_half* y, float* stats, int M, int D, const MtLaunchOpts* opt,
                                    mt_stream_t stream) {
  if (int rc = mt_opts_check(opt, MT_OPT_EPS)) return rc;
  if (!x || !branch || !w || !b || !h || !y || !stats || M <= 0 || h == x) return MT_ERR_BAD_ARG;
  if (D != 768) return MT_ERR_UNSUPPORTED;
  const AddLnArgs a{x, (const h16*)branch, make_drop(drop), w, b, h, (h16*)y, stats, M, mt_opt_eps(opt)};
  return launch(add_ln_fwd_kernel<768>, dim3(ln_grid(M)), dim3(256), (hipStream_t)stream, a);
}

extern "C" long mt_layernorm_pool_partials_elems(int B, int rows, int D) {
  if (B < 1 || rows < 1 || D != POOL_D) return MT_ERR_BAD_ARG;
  const int G = ln_pool_groups(rows);
  return G > 1 ? (long)B * G * D : 0;
}

extern "C" int mt_layernorm_pool_fwd(const float* x, long ldx, int B, int rows_per_pass, int r0, int r1, const float* pre_w,
                                     const float* pre_b, float pre_eps, const float* post_w, const float* post_b, float post_eps,
                                     float* out, double* partials, long partials_elems, int D, mt_stream_t stream) {
  if (!x || !out || B < 1 || B > 65535 || rows_per_pass < 1 || r0 < 0 || r1 <= r0 || r1 > rows_per_pass || ldx < D || (ldx & 3) ||
      ((uintptr_t)x & 15) || ((uintptr_t)pre_w & 15) || ((uintptr_t)pre_b & 15) || (!pre_w) != (!pre_b) ||
      (!post_w) != (!post_b) || !(pre_eps >= 0.f) || !(post_eps >= 0.f) || partials_elems < 0)
    return MT_ERR_BAD_ARG;
  if (D != POOL_D) return MT_ERR_UNSUPPORTED;
  const int n = r1 - r0, G = ln_pool_groups(n);
  if (G > 1 && (!partials || ((uintptr_t)partials & 7) || partials_elems < mt_layernorm_pool_partials_elems(B, n, D))) return MT_ERR_BAD_ARG;
  const LnPoolArgs a{x, ldx, rows_per_pass, r0, n, pre_w, pre_b, pre_eps != 0.f ? pre_eps : 1e-5f, post_w, post_b,
                     post_eps != 0.f ? post_eps : 1e-5f, out, partials, G};
  hipStream_t s = (hipStream_t)stream;
  const int rc = launch(pre_w ? ln_pool_rows_kernel<true> : ln_pool_rows_kernel<false>, dim3(G, B), dim3(256), s, a);
  if (rc != MT_OK || G == 1) return rc;
  return launch(ln_pool_final_kernel, dim3(B), dim3(256), s, a);
}

extern "C" long mt_layernorm_bwd_det_elems(int M, int D) {
  if (M <= 0 || !ln_width_ok(D)) return MT_ERR_BAD_ARG;
  return (long)ln_param_grid(M) * 2 * D;
}

// opt->partials: the deterministic form (det_reduce.hip), partials = [slots][2][D] for dw | db, slots = workgroups of the PARAM form
extern "C" int mt_layernorm_bwd(const void* dy, long lddy, const MtRowMap* dymap, int dy_dtype, const void* x,
                                long ldx, const MtRowMap* xmap, int in_dtype, int gelu_in, const float* w,
                                const float* stats, void* dx, long lddx, const MtRowMap* dxmap, int dx_dtype,
                                int accumulate, float* dw, float* db, mt_half* dx_f16, const MtDropout* dx_f16_drop, int M,
                                int D, const MtLaunchOpts* opt, mt_stream_t stream) {
  if (int rc = mt_opts_check(opt, MT_OPT_LIVE | MT_OPT_PARTIALS)) return rc;
  const LiveOpt lv = live_opt(opt);
  float* partials = mt_opt_partials(opt);
  if (lv.live && partials) return MT_ERR_UNSUPPORTED;
  if (!dy || !x || !w || !stats || !dx || M <= 0 || (!dw) != (!db) || (partials && !dw) || lv.malformed() ||
      (lddy & 3) || (ldx & 3) || (lddx & 3))      // (8- and 16-byte vector accesses per row, as in mt_layernorm_fwd)
    return MT_ERR_BAD_ARG;
  if (dx_f16 && gelu_in) return MT_ERR_UNSUPPORTED;
  if (lv.live && dw) return MT_ERR_UNSUPPORTED;      // (dw / db of a trainable norm sum over every row: its forms take no table)
  if (partials) {
    const long need = mt_layernorm_bwd_det_elems(M, D);
    if (need < 0) return MT_ERR_UNSUPPORTED;
    if (opt->partials_elems < need) return MT_ERR_BAD_ARG;
  }
  const LnBwdArgs a{dy, lddy, make_rowmap(dymap), x, ldx, make_rowmap(xmap), w, stats, dx, lddx, make_rowmap(dxmap), accumulate,
                    partials ? partials : dw, partials ? partials + D : db, (h16*)dx_f16, make_drop(dx_f16 ? dx_f16_drop : nullptr), M,
                    lv.live, lv.rows};
  hipStream_t s = (hipStream_t)stream;
  const bool det = partials != nullptr;
  int rc = with_ln_width(D, [&](auto d) { return ln_bwd_types<d()>(a, dy_dtype, in_dtype, dx_dtype, gelu_in, s, det); });
  if (rc != MT_OK || !det) return rc;
  const int slots = ln_param_grid(M);
  rc = mt_det_reduce_launch(partials, slots, 1, D, 2L * D, dw, D, s);
  if (rc != MT_OK) return rc;
  return mt_det_reduce_launch(partials + D, slots, 1, D, 2L * D, db, D, s);
}

extern "C" long mt_inject_resid_bwd_det_elems(int M, int D) {
  if (M <= 0 || D != 768) return MT_ERR_BAD_ARG;
  return (long)inj_grid(M) * D;
}

// opt->partials: the deterministic form, partials = [slots][D], slots = workgroups
extern "C" int mt_inject_resid_bwd(const float* dy, long lddy, const MtRowMap* dymap, const float* x, long ldx,
                                   const MtRowMap* xmap, const mt_half* proj, const float* gamma, float* dx, long lddx,
                                   const MtRowMap* dxmap, int dx_accumulate, mt_half* dproj, float* dgamma, int M,
                                   int D, const MtLaunchOpts* opt, mt_stream_t stream) {
  if (int rc = mt_opts_check(opt, MT_OPT_PARTIALS)) return rc;
  float* partials = mt_opt_partials(opt);
  if (!dy || !x || !proj || !gamma || !dx || !dproj || !dgamma || M <= 0 || D != 768 || (lddy & 3) || (ldx & 3) || (lddx & 3) ||
      (partials && opt->partials_elems < mt_inject_resid_bwd_det_elems(M, D)))
    return MT_ERR_BAD_ARG;
  const InjBwdArgs a{dy, lddy, make_rowmap(dymap), x, ldx, make_rowmap(xmap), (const h16*)proj, gamma, dx, lddx,
                     make_rowmap(dxmap), dx_accumulate, (h16*)dproj, partials ? partials : dgamma, M};
  hipStream_t s = (hipStream_t)stream;
  const int slots = inj_grid(M);
  const int rc = launch(partials ? inject_resid_bwd_kernel<768, true> : inject_resid_bwd_kernel<768>, dim3(slots), dim3(256), s, a);
  if (rc != MT_OK || !partials) return rc;
  return mt_det_reduce_launch(partials, slots, 1, D, D, dgamma, D, s);
}

extern "C" int mt_cast_f32_to_f16(const float* x, mt_half* y, long n, const MtDropout* drop, int D, mt_stream_t stream) {
  if (!x || !y || n <= 0) return MT_ERR_BAD_ARG;
  const DropArgs d = make_drop(drop);
  const dim3 grid(ew_grid(n / 4 + 1)), block(256);
  if (!d.active()) return launch(cast_f32_f16_kernel, grid, block, (hipStream_t)stream, x, (h16*)y, n);
  if ((n & 3) || D <= 0 || (D & 3)) return MT_ERR_BAD_ARG;
  return launch(cast_drop_f32_f16_kernel, grid, block, (hipStream_t)stream, x, (h16*)y, n, d, D);
}
extern "C" int mt_cast_f16_to_f32(const mt_half* x, float* y, long n, mt_stream_t stream) {
  if (!x || !y || n <= 0) return MT_ERR_BAD_ARG;
  return launch(cast_f16_f32_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), (hipStream_t)stream, (const h16*)x, y, n);
}
extern "C" int mt_rng_advance(unsigned* rng, mt_stream_t stream) {
  if (!rng) return MT_ERR_BAD_ARG;
  return launch(rng_advance_kernel, dim3(1), dim3(64), (hipStream_t)stream, rng);
}
extern "C" int mt_droppath_live(const unsigned* path_sites, const float* path_ps, int n, int B, const unsigned* rng, int* table,
                                mt_stream_t stream) {
  if (!path_sites || !path_ps || !rng || !table || n < 1 || n > MT_LIVE_SITES_MAX || B < 1) return MT_ERR_BAD_ARG;
  LiveSites ls;
  ls.n = n;
  for (int i = 0; i < MT_LIVE_SITES_MAX; ++i) { ls.site[i] = i < n ? path_sites[i] : 0u; ls.p[i] = i < n ? path_ps[i] : 0.f; }
  return launch(droppath_live_kernel, dim3(1), dim3(MT_LIVE_SITES_MAX), (hipStream_t)stream, ls, B, rng, table);
}
extern "C" int mt_dropout_f32(const float* x, long ldx, const MtRowMap* xmap, float* y, int M, int D, const MtDropout* drop,
                              mt_stream_t stream) {
  if (!x || !y || M <= 0 || D <= 0 || (D & 3) || (ldx & 3)) return MT_ERR_BAD_ARG;
  return launch(dropout_f32_kernel, dim3(ew_grid((long)M * D / 4 + 1)), dim3(256), (hipStream_t)stream, x, ldx, make_rowmap(xmap), y, M, D,
                make_drop(drop));
}
extern "C" int mt_droppath_rows_f32(float* x, int M, int D, const MtDropout* drop, mt_stream_t stream) {
  if (!x || M <= 0 || D <= 0 || (D & 3)) return MT_ERR_BAD_ARG;
  const DropArgs d = make_drop(drop);
  if (!d.active() || d.path_p <= 0.f) return MT_OK;
  return launch(droppath_rows_kernel, dim3(ew_grid((long)M * D / 4 + 1)), dim3(256), (hipStream_t)stream, x, M, D, d);
}
extern "C" int mt_pack_weight_f16(const float* src, int R, int C, mt_half* dst, int transpose, mt_stream_t stream) {
  if (!src || !dst || R <= 0 || C <= 0) return MT_ERR_BAD_ARG;
  return launch(pack_f16_kernel, dim3(cdiv(C, 32), cdiv(R, 32)), dim3(256), (hipStream_t)stream, src, R, C, (h16*)dst, transpose);
}
extern "C" int mt_pack_weights_f16(const long long* items, int n_items, mt_stream_t stream) {
  if (!items || n_items <= 0) return MT_ERR_BAD_ARG;
  return launch(pack_group_kernel, dim3(n_items, 48), dim3(256), (hipStream_t)stream, items);
}
extern "C" int mt_act_fwd(const float* x, float* y, long n, int act, mt_stream_t stream) {
  if (!x || !y || n <= 0) return MT_ERR_BAD_ARG;
  return launch(act_fwd_kernel, dim3(ew_grid(n)), dim3(256), (hipStream_t)stream, x, y, n, act);
}
extern "C" int mt_act_bwd(const float* x, const float* dy, float* dx, long n, int act, mt_stream_t stream) {
  if (!x || !dy || !dx || n <= 0) return MT_ERR_BAD_ARG;
  return launch(act_bwd_kernel, dim3(ew_grid(n)), dim3(256), (hipStream_t)stream, x, dy, dx, n, act);
}
extern "C" int mt_axpy(const float* a, const float* b, float alpha, float* y, long n, mt_stream_t stream) {
  if (!a || !b || !y || n <= 0) return MT_ERR_BAD_ARG;
  return launch(axpy_kernel, dim3(ew_grid(n)), dim3(256), (hipStream_t)stream, a, b, alpha, y, n);
}
extern "C" int mt_axpy_bcast(const float* a, const float* b, float alpha, float* y, long n, long period, mt_stream_t stream) {
  if (!a || !b || !y || n <= 0 || period <= 0) return MT_ERR_BAD_ARG;
  return launch(axpy_bcast_kernel, dim3(ew_grid(n)), dim3(256), (hipStream_t)stream, a, b, alpha, y, n, period);
}
extern "C" int mt_fold_rows(const float* x, int reps, long period, float* out, mt_stream_t stream) {
  if (!x || !out || reps < 1 || period <= 0 || (period & 3) || ((uintptr_t)x & 15) || ((uintptr_t)out & 15)) return MT_ERR_BAD_ARG;
  return launch(fold_rows_kernel, dim3(ew_grid(period / 4)), dim3(256), (hipStream_t)stream, x, reps, period, out);
}
extern "C" int mt_copy_rows_f32(const float* src, long lds, const MtRowMap* smap, float* dst, long ldd,
                                const MtRowMap* dmap, int M, int D, int accumulate, mt_stream_t stream) {
  if (!src || !dst || M <= 0 || D <= 0 || (D & 3) || (lds & 3) || (ldd & 3)) return MT_ERR_BAD_ARG;
  return launch(copy_rows_kernel, dim3(ew_grid((long)M * D / 4)), dim3(256), (hipStream_t)stream, src, lds, make_rowmap(smap), dst, ldd,
                make_rowmap(dmap), M, D, accumulate);
}
