// Grouped pathway networks of the gene encoder (gene_encoder.py:97-131,194-207): for each of G pathways
//   z_i = ELU(W2_i ELU(W1_i g_i + b1_i) + b2_i),  W1_i [latent, n_i], W2_i [latent, latent], g_i [n_i]
// With the real grouping (G = 331, n_i = 1..199, 24 M parameters) the reference runs 662 tiny nn.Linear modules; here
// ONE launch per direction walks all pathways: workgroup = pathway, thread = output unit, weights streamed through LDS
// in 32-column chunks with coalesced loads.  HBM-bound on the weights (forward reads them once; backward reads W2 once
// and read-modify-writes the gradient slots).  Parameters are addressed by element offsets into the flat fp32
// parameter / gradient buffers (the per-pathway tensors keep their reference state_dict names and order).
#include "common.h"

namespace {

constexpr int GL = 256;      // latent width = workgroup size
constexpr int GC = 32;       // chunk width

MT_DEVINL float elu(float v) { return v > 0.f ? v : expm1f(v); }
MT_DEVINL float elu_grad(float pre) { return pre > 0.f ? 1.f : __expf(pre); }

struct GeneArgs {
  const float* params; float* grads;
  const long* offs;      // [G][4]: w1, b1, w2, b2 (element offsets)
  const int* sizes;      // [G]
  const long* goff;      // [G] offset of g_i in `genes`
  const float* genes;
  float* a1; float* a2;  // pre-activations (saved): a1 [G][latent] (the same in every pass), a2 [G][P][latent]
  float* z;              // [G][P][latent] forward output (pathway-major: the mixer's group axis stays outermost)
  const float* dz;       // [G][P][latent]
  DropArgs adrop;        // nn.AlphaDropout after each ELU (gene_encoder.py:178-181): sites adrop.site, adrop.site + 1
  int G, P;              // P task passes: one forward call of the reference each, so each draws its own masks
};
constexpr int GP_MAX = 4;
// the launch's pass count (1 .. GP_MAX: the entry points check) onto the kernels' template argument
#define GENE_LAUNCH(kernel, passes, grid, stream, args)                                                    \
  do {                                                                                                     \
    switch (passes) {                                                                                      \
      case 1: hipLaunchKernelGGL(kernel<1>, dim3(grid), dim3(GL), 0, stream, args); break;                 \
      case 2: hipLaunchKernelGGL(kernel<2>, dim3(grid), dim3(GL), 0, stream, args); break;                 \
      case 3: hipLaunchKernelGGL(kernel<3>, dim3(grid), dim3(GL), 0, stream, args); break;                 \
      default: hipLaunchKernelGGL(kernel<4>, dim3(grid), dim3(GL), 0, stream, args); break;                \
    }                                                                                                      \
  } while (0)

// AlphaDropout(p): kept values pass, dropped ones become alpha' = -selu_scale * selu_alpha; then the affine (a, b) that
// restores zero mean / unit variance (torch.nn.functional.alpha_dropout)
constexpr float ALPHA_P = -1.7580993408473766f;
struct AlphaAff { float a, b; };
MT_DEVINL AlphaAff alpha_affine(float p) {
  const float a = rsqrtf((1.f - p) * (1.f + p * ALPHA_P * ALPHA_P));
  return AlphaAff{a, -a * ALPHA_P * p};
}
// The AlphaDropout of one launch.  Pass p draws its own masks: element index (i P + p) 256 + j of pathway i, unit j, at site `site`
// after the first ELU and `site + 1` after the second -- an index of the pathway and P, never of the grid.
struct AlphaDrop {
  DropArgs d; bool on; AlphaAff af;
  MT_DEVINL explicit AlphaDrop(const DropArgs& d_) : d(d_), on(d_.active() && d_.p > 0.f), af(alpha_affine(d_.p)) {}
  MT_DEVINL bool keep(int layer, uint64_t idx) const { return !on || drop_keep1(d, d.site + layer, idx); }
  MT_DEVINL float apply(bool kept, float v) const { return on ? fmaf(af.a, kept ? v : ALPHA_P, af.b) : v; }
  MT_DEVINL float grad(bool kept) const { return on ? (kept ? af.a : 0.f) : 1.f; }
};

// ---- The stages of the pathway networks, each stated ONCE and called by every kernel that runs it.  Every accumulation below has one
// chain -- bias first, k (or r) ascending, one fmaf per term -- so kernels that share a stage give the same bits: the kernels that share a
// pathway among workgroups against the workgroup-per-pathway ones (a model does not change with the number of pathways it is grouped
// into; tests/test_kernels_gpu.py: test_gene_snn_families_same_bits -- one exception, the da1 sum of gene_snn_bwd_split_kernel), and the
// points forward at alpha = 1 / alpha = 0 against the plain forward.  Every LDS read of the loops is in the 4-byte class (lds_f32,
// common.h).  The backward functions switch the compiler's fp contraction off: there a `+=` IS an add of rounded terms and every fused
// multiply-add is written fmaf -- which of the two a sum gets is not left to the optimiser, kernel by kernel.

// acc_v[j] += sum_{k < n} W[j][k] x_v[k] (thread j; the caller seeds acc with the bias) for NX input vectors at once: W, row-major with
// row stride ld, is streamed through LDS ONCE for all of them in 32-column chunks, x_v in LDS
template <int NX>
MT_DEVINL void gemv_rows(const float* __restrict__ W, int ld, int n, const float (*xs)[GL], float (*Ws)[GC + 1], float (&acc)[NX]) {
  const int j = threadIdx.x;
  for (int k0 = 0; k0 < n; k0 += GC) {
    const int kc = min(GC, n - k0);
    __syncthreads();
    for (int t = j; t < GL * GC; t += GL) {       // 8 rows of 32 columns per step: 128-B coalesced row segments
      const int r = t / GC, c = t - r * GC;
      Ws[r][c] = c < kc ? W[(long)r * ld + k0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int c = 0; c < GC; ++c) {
      const float w = lds_f32(&Ws[j][c]);
#pragma unroll
      for (int v = 0; v < NX; ++v) acc[v] = fmaf(w, (k0 + c < n) ? lds_f32(&xs[v][k0 + c]) : 0.f, acc[v]);
    }
  }
}

// First layer: acc_v[j] += sum_k W1[j][k] x_v[k] for NX input vectors of n elements in global memory, a null vector being zeros.  n can
// exceed the LDS vector: the input is walked in pieces of GL, the rows of W1 restricted to a piece.  Uses xs[0 .. NX).
template <int NX>
MT_DEVINL void first_layer(const float* W1, int n, const float* const (&x)[NX], float (*xs)[GL], float (*Ws)[GC + 1], float (&acc)[NX]) {
  const int j = threadIdx.x;
  for (int p0 = 0; p0 < n; p0 += GL) {
    const int pn = min(GL, n - p0);
    __syncthreads();
    if (j < pn) {
#pragma unroll
      for (int v = 0; v < NX; ++v) xs[v][j] = x[v] ? x[v][p0 + j] : 0.f;
    }
    __syncthreads();
    gemv_rows<NX>(W1 + p0, n, pn, xs, Ws, acc);
  }
}

// h1_p[j] = AlphaDropout(ELU(pre1[j])) of every pass into LDS (the first layer is the same in every pass: the input is data)
template <int P>
MT_DEVINL void stage_h1(const AlphaDrop& ad, int i, float pre1, float (*xs)[GL]) {
  const int j = threadIdx.x;
  const float e1 = elu(pre1);
#pragma unroll
  for (int p = 0; p < P; ++p) xs[p][j] = ad.apply(ad.keep(0, ((uint64_t)i * P + p) * GL + j), e1);
}

// Second-layer epilogue of row `row` of pathway i: a2 saved, z = AlphaDropout(ELU(a2))
template <int P>
MT_DEVINL void store_second_layer(const AlphaDrop& ad, int i, int row, const float (&acc2)[P], float* a2, float* z) {
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const long e = ((long)i * P + p) * GL + row;
    a2[e] = acc2[p];
    z[e] = ad.apply(ad.keep(1, (uint64_t)e), elu(acc2[p]));
  }
}

// Backward prologue (thread j of pathway i): both masks regenerated; da2_p = dz_p * mask2_p * elu'(a2_p) and h1_p into LDS, the first
// mask's factor into g1; returns db2[j] = sum_p da2_p[j]: the ROUNDED da2_p that went to LDS, p ascending, plain adds
template <int P>
MT_DEVINL float bwd_prologue(const GeneArgs& a, const AlphaDrop& ad, int i, float pre1, float (*da2s)[GL], float (*h1s)[GL], float (&g1)[P]) {
#pragma clang fp contract(off)
  const int j = threadIdx.x;
  float db2 = 0.f;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const long e = ((long)i * P + p) * GL + j;
    const float pre2 = a.a2[e];
    const bool keep1 = ad.keep(0, (uint64_t)e), keep2 = ad.keep(1, (uint64_t)e);
    g1[p] = ad.grad(keep1);
    const float da2 = a.dz[e] * ad.grad(keep2) * elu_grad(pre2);
    da2s[p][j] = da2;
    h1s[p][j] = ad.apply(keep1, elu(pre1));
    db2 += da2;
  }
  return db2;
}

// dW2[r][c] += sum_p da2_p[r] h1_p[c] for rows [row_begin, row_end): one wave per row, 16-byte accesses
template <int P>
MT_DEVINL void dw2_rows(float* dW2, int row_begin, int row_end, const float (*da2s)[GL], const float (*h1s)[GL]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = row_begin + wave; r < row_end; r += 4) {
    float* dst = dW2 + (long)r * GL + lane * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(dst);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const float d = lds_f32(&da2s[p][r]);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaf(d, lds_f32(&h1s[p][lane * 4 + e]), v[e]);
    }
    *reinterpret_cast<f32x4*>(dst) = v;
  }
}

// dh1_p[k] = sum_r W2[r][k] da2_p[r] (thread k), r ascending from 0: W2 streamed ONCE for all passes, 32 rows at a time, coalesced
template <int P>
MT_DEVINL void w2t_stream(const float* W2, const float (*da2s)[GL], float (*Ws)[GL + 1], float (&dh1)[P]) {
  const int j = threadIdx.x;
#pragma unroll
  for (int p = 0; p < P; ++p) dh1[p] = 0.f;
  for (int r0 = 0; r0 < GL; r0 += GC) {
    __syncthreads();
    for (int t = j; t < GC * GL; t += GL) {
      const int r = t / GL, c = t - r * GL;
      Ws[r][c] = W2[(long)(r0 + r) * GL + c];
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < GC; ++r) {
      const float w = lds_f32(&Ws[r][j]);
#pragma unroll
      for (int p = 0; p < P; ++p) dh1[p] = fmaf(w, lds_f32(&da2s[p][r0 + r]), dh1[p]);
    }
  }
}

template <int P>
__global__ __launch_bounds__(GL) void gene_snn_fwd_kernel(GeneArgs a) {
  __shared__ float Ws[GL][GC + 1];
  __shared__ float xs[P][GL];
  const int i = blockIdx.x, j = threadIdx.x;
  const int n = a.sizes[i];
  const long* o = a.offs + 4L * i;
  const AlphaDrop ad(a.adrop);
  const float* const x[1] = {a.genes + a.goff[i]};
  float acc[1] = {a.params[o[1] + j]};
  first_layer<1>(a.params + o[0], n, x, xs, Ws, acc);
  a.a1[(long)i * GL + j] = acc[0];
  __syncthreads();
  stage_h1<P>(ad, i, acc[0], xs);
  float acc2[P];
#pragma unroll
  for (int p = 0; p < P; ++p) acc2[p] = a.params[o[3] + j];
  gemv_rows<P>(a.params + o[2], GL, GL, xs, Ws, acc2);
  store_second_layer<P>(ad, i, j, acc2, a.a2, a.z);
}

template <int P>
__global__ __launch_bounds__(GL) void gene_snn_bwd_kernel(GeneArgs a) {
#pragma clang fp contract(off)
  __shared__ float Ws[GC][GL + 1];   // 32 rows x 256 columns of W2
  __shared__ float da2s[P][GL], h1s[P][GL], da1s[GL];
  const int i = blockIdx.x, j = threadIdx.x;
  const int n = a.sizes[i];
  const long* o = a.offs + 4L * i;
  const float pre1 = a.a1[(long)i * GL + j];
  const AlphaDrop ad(a.adrop);
  float g1[P], dh1[P];
  const float db2 = bwd_prologue<P>(a, ad, i, pre1, da2s, h1s, g1);
  a.grads[o[3] + j] += db2;
  __syncthreads();
  dw2_rows<P>(a.grads + o[2], 0, GL, da2s, h1s);
  w2t_stream<P>(a.params + o[2], da2s, Ws, dh1);
  // the first layer's input is the same in every pass: da1 = (sum_p dh1_p * mask_p) * elu'(pre1), the sum over rounded products
  float s1 = 0.f;
#pragma unroll
  for (int p = 0; p < P; ++p) s1 += dh1[p] * g1[p];
  const float eg1 = elu_grad(pre1);
  a.grads[o[1] + j] = fmaf(eg1, s1, a.grads[o[1] + j]);
  da1s[j] = eg1 * s1;
  __syncthreads();
  // dW1[r][k] += da1[r] g[k]: rows of n floats (4-byte accesses: the slots are only 4-byte aligned inside a row)
  const float* g = a.genes + a.goff[i];
  for (long t = j; t < (long)GL * n; t += GL) {
    const int r = (int)(t / n), k = (int)(t - (long)r * n);
    a.grads[o[0] + t] = fmaf(lds_f32(&da1s[r]), g[k], a.grads[o[0] + t]);
  }
}

// ---- few pathways (the 6-pathway configuration of the headline bench): a workgroup per pathway leaves the chip to 6 workgroups that
// each pull a 256 KB W2 through one CU (fwd 37 us, bwd 83 us inside the step).  Here GS workgroups share a pathway by INDEX RANGES that
// need no reduction across workgroups: forward = GR = 256 / GS rows of the second layer each (the small first layer is recomputed by
// all of them); backward = rows [GR s, GR s + GR) of dW2 / db2 and COLUMNS [GR s, ...) of W2^T da2, hence of da1, db1 and the rows of dW1.
constexpr int GS = 8, GR = GL / GS;      // 8 workgroups x 32 rows / columns

template <int P>
__global__ __launch_bounds__(GL) void gene_snn_fwd_split_kernel(GeneArgs a) {
  __shared__ float Ws[GL][GC + 1];
  __shared__ float xs[P][GL];
  const int i = blockIdx.x / GS, sp = blockIdx.x % GS, j = threadIdx.x;
  const int n = a.sizes[i];
  const long* o = a.offs + 4L * i;
  const AlphaDrop ad(a.adrop);
  const float* const x[1] = {a.genes + a.goff[i]};
  float acc[1] = {a.params[o[1] + j]};
  first_layer<1>(a.params + o[0], n, x, xs, Ws, acc);
  if (sp == 0) a.a1[(long)i * GL + j] = acc[0];
  __syncthreads();
  stage_h1<P>(ad, i, acc[0], xs);
  __syncthreads();
  // second layer, rows [GR sp, GR sp + GR): the rows are staged in LDS by all threads (8 per row: a wave reads 8 rows x 1 KB,
  // contiguous), then ONE thread per row runs the chain of gemv_rows (bias first, k = 0 .. 255 ascending): the same bits
  float (*Wl)[GL + 1] = reinterpret_cast<float (*)[GL + 1]>(&Ws[0][0]);      // [GR][GL + 1] in the chunk buffer (8 224 of its 8 448 floats)
  {
    const int r = j >> 3, part = j & 7;
    const float* wr = a.params + o[2] + (long)(GR * sp + r) * GL + part * 32;
#pragma unroll
    for (int c = 0; c < 32; c += 4) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) Wl[r][part * 32 + c + e] = w4[e];
    }
  }
  __syncthreads();
  if (j < GR) {
    const int r = GR * sp + j;
    float a2[P];
#pragma unroll
    for (int p = 0; p < P; ++p) a2[p] = a.params[o[3] + r];
#pragma unroll 8
    for (int k = 0; k < GL; ++k) {
      const float w = lds_f32(&Wl[j][k]);
#pragma unroll
      for (int p = 0; p < P; ++p) a2[p] = fmaf(w, lds_f32(&xs[p][k]), a2[p]);
    }
    store_second_layer<P>(ad, i, r, a2, a.a2, a.z);
  }
}

template <int P>
__global__ __launch_bounds__(GL) void gene_snn_bwd_split_kernel(GeneArgs a) {
#pragma clang fp contract(off)
  __shared__ float da2s[P][GL], h1s[P][GL], Wc[GL][GR + 1], da1s[GR];
  const int i = blockIdx.x / GS, sp = blockIdx.x % GS, j = threadIdx.x;
  const int n = a.sizes[i];
  const long* o = a.offs + 4L * i;
  const float pre1 = a.a1[(long)i * GL + j];
  const AlphaDrop ad(a.adrop);
  float g1[P];      // (unit j's, unused: the columns of this workgroup draw theirs below)
  const float db2 = bwd_prologue<P>(a, ad, i, pre1, da2s, h1s, g1);
  if (j / GR == sp) a.grads[o[3] + j] += db2;
  __syncthreads();
  dw2_rows<P>(a.grads + o[2], GR * sp, GR * sp + GR, da2s, h1s);
  // dh1_p[k] = sum_r W2[r][k] da2_p[r] for the columns k in [GR sp, GR sp + GR): the 256 x GR block of W2 is staged in LDS (each
  // row's 128 bytes by 8 threads), then one thread per column runs the chain of w2t_stream (r = 0 .. 255 ascending): the same bits
  {
    const int part = j & 7;
    for (int r = j >> 3; r < GL; r += GL / 8) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(a.params + o[2] + (long)r * GL + GR * sp + part * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) Wc[r][part * 4 + e] = w4[e];
    }
  }
  __syncthreads();
  if (j < GR) {
    const int k = GR * sp + j;
    float dh1[P];
#pragma unroll
    for (int p = 0; p < P; ++p) dh1[p] = 0.f;
#pragma unroll 8
    for (int r = 0; r < GL; ++r) {
      const float w = lds_f32(&Wc[r][j]);
#pragma unroll
      for (int p = 0; p < P; ++p) dh1[p] = fmaf(w, lds_f32(&da2s[p][r]), dh1[p]);
    }
    // da1 as in gene_snn_bwd_kernel, but the sum over the passes is ONE fmaf chain here: under AlphaDropout (mask factors other than 1)
    // db1 and dW1 of the two kernels differ in the last bits; every other tensor, and these two without dropout, have the same bits
    float s1 = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) s1 = fmaf(dh1[p], ad.grad(ad.keep(0, (uint64_t)(((long)i * P + p) * GL + k))), s1);
    const float eg1 = elu_grad(a.a1[(long)i * GL + k]);
    a.grads[o[1] + k] = fmaf(eg1, s1, a.grads[o[1] + k]);
    da1s[j] = eg1 * s1;
  }
  __syncthreads();
  // dW1 rows [GR sp, GR sp + GR): dW1[r][c] += da1[r] g[c]
  const float* g = a.genes + a.goff[i];
  for (long t = j; t < (long)GR * n; t += GL) {
    const int r = (int)(t / n), c = (int)(t - (long)r * n);
    float* dst = a.grads + o[0] + ((long)GR * sp + r) * n + c;
    *dst = fmaf(lds_f32(&da1s[r]), g[c], *dst);
  }
}

// below this many pathways a pathway is shared by GS workgroups (a workgroup per pathway fills the chip from a few hundred on)
#ifndef MT_GENE_SPLIT_BELOW
#define MT_GENE_SPLIT_BELOW 64
#endif
constexpr int GENE_SPLIT_BELOW = MT_GENE_SPLIT_BELOW;

}  // namespace

extern "C" int mt_gene_snn_fwd(const float* params, const long* offs, const int* sizes, const long* goff, const float* genes,
                               int G, int latent, int passes, float* a1, float* a2, float* z, const MtDropout* alpha_drop,
                               mt_stream_t stream) {
  if (!params || !offs || !sizes || !goff || !genes || !a1 || !a2 || !z || G < 1 || passes < 1) return MT_ERR_BAD_ARG;
  if (latent != GL || passes > GP_MAX) return MT_ERR_UNSUPPORTED;
  GeneArgs a{params, nullptr, offs, sizes, goff, genes, a1, a2, z, nullptr, make_drop(alpha_drop), G, passes};
  hipStream_t s = (hipStream_t)stream;
  if (G < GENE_SPLIT_BELOW) GENE_LAUNCH(gene_snn_fwd_split_kernel, passes, G * GS, s, a);
  else GENE_LAUNCH(gene_snn_fwd_kernel, passes, G, s, a);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_gene_snn_bwd(const float* params, float* grads, const long* offs, const int* sizes, const long* goff,
                               const float* genes, int G, int latent, int passes, const float* a1, const float* a2,
                               const float* dz, const MtDropout* alpha_drop, mt_stream_t stream) {
  if (!params || !grads || !offs || !sizes || !goff || !genes || !a1 || !a2 || !dz || G < 1 || passes < 1) return MT_ERR_BAD_ARG;
  if (latent != GL || passes > GP_MAX) return MT_ERR_UNSUPPORTED;
  GeneArgs a{params, grads, offs, sizes, goff, genes, const_cast<float*>(a1), const_cast<float*>(a2), nullptr, dz,
             make_drop(alpha_drop), G, passes};
  hipStream_t s = (hipStream_t)stream;
  if (G < GENE_SPLIT_BELOW) GENE_LAUNCH(gene_snn_bwd_split_kernel, passes, G * GS, s, a);
  else GENE_LAUNCH(gene_snn_bwd_kernel, passes, G, s, a);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

// ---- Integrated Gradients over the gene inputs (attribution.py): the pass axis carries P quadrature points of the straight path
// g_p = baseline + alpha_p (genes - baseline) instead of P dropout draws.  Forward = the networks at all P points with the weights
// streamed once; backward = the INPUT gradient only (no parameter-gradient slot is touched); finalize = (genes - baseline) * dF/dgenes
// and its per-pathway sums.  One workgroup per pathway throughout: these launches sit beside a full backbone pass.
namespace {

struct GenePointArgs {
  const float* params;
  const long* offs; const int* sizes; const long* goff;      // as GeneArgs
  const float* genes; const float* baseline;                 // baseline may be null (= zeros)
  const float* alphas;                                       // [P] device: position of each point on the path
  const float* weights;                                      // [P] device: quadrature weight of each point (backward)
  const float* unscale;                                      // device scalar or null (= 1): undoes the caller's gradient scaling
  float* a1; float* a2; float* z;                            // [G][P][latent] each: the first layer differs per point here
  const float* dz;                                           // [G][P][latent]
  float* dgenes;                                             // [total]
  int G, accumulate;
};

template <int P>
__global__ __launch_bounds__(GL) void gene_snn_fwd_points_kernel(GenePointArgs a) {
  __shared__ float Ws[GL][GC + 1];
  __shared__ float xs[P < 2 ? 2 : P][GL];      // first layer: row 0 = genes, row 1 = baseline; second layer: h1 of point p
  const int i = blockIdx.x, j = threadIdx.x;
  const int n = a.sizes[i];
  const long* o = a.offs + 4L * i;
  // The first layer is affine in alpha: b1 + W1 genes and b1 + W1 baseline are formed ONCE (each by the chain of first_layer, so
  // alpha = 1 / alpha = 0 reproduce the bits of gene_snn_fwd_kernel) and combined per point below
  const float* const x[2] = {a.genes + a.goff[i], a.baseline ? a.baseline + a.goff[i] : nullptr};
  const float b1 = a.params[o[1] + j];
  float acc[2] = {b1, b1};
  first_layer<2>(a.params + o[0], n, x, xs, Ws, acc);
  __syncthreads();
  float acc2[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const float al = a.alphas[p];
    const float pre1 = fmaf(al, acc[0], (1.f - al) * acc[1]);      // exact at alpha = 0 and alpha = 1
    a.a1[((long)i * P + p) * GL + j] = pre1;
    xs[p][j] = elu(pre1);
    acc2[p] = a.params[o[3] + j];
  }
  gemv_rows<P>(a.params + o[2], GL, GL, xs, Ws, acc2);
  store_second_layer<P>(AlphaDrop(DropArgs{}), i, j, acc2, a.a2, a.z);      // (no dropout on the path)
}

template <int P>
__global__ __launch_bounds__(GL) void gene_snn_bwd_input_kernel(GenePointArgs a) {
#pragma clang fp contract(off)
  __shared__ float Ws[GC][GL + 1];   // 32 rows x 256 columns of W2
  __shared__ float da2s[P][GL], ss[GL];
  const int i = blockIdx.x, j = threadIdx.x;
  const int n = a.sizes[i];
  const long* o = a.offs + 4L * i;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const long e = ((long)i * P + p) * GL + j;
    da2s[p][j] = a.dz[e] * elu_grad(a.a2[e]);
  }
  float dh1[P];
  w2t_stream<P>(a.params + o[2], da2s, Ws, dh1);
  // s[k] = sum_p w_p da1_p[k], p ascending: the input gradient is linear in da1, so the quadrature sum is taken before W1^T
  float s = 0.f;
#pragma unroll
  for (int p = 0; p < P; ++p) s = fmaf(a.weights[p], dh1[p] * elu_grad(a.a1[((long)i * P + p) * GL + j]), s);
  ss[j] = s;
  __syncthreads();
  // dgenes[k] (+)= unscale * sum_r W1[r][k] s[r]: ONE thread per input k (coalesced along the rows of W1), r ascending -- no atomics,
  // every element has one writer and one summation order
  const float us = a.unscale ? a.unscale[0] : 1.f;
  float* dg = a.dgenes + a.goff[i];
  const float* W1 = a.params + o[0];
  for (int k = j; k < n; k += GL) {
    float acc = 0.f;
#pragma unroll 8
    for (int r = 0; r < GL; ++r) acc = fmaf(W1[(long)r * n + k], lds_f32(&ss[r]), acc);
    acc *= us;
    dg[k] = a.accumulate ? dg[k] + acc : acc;
  }
}

struct IgFinalArgs {
  const float* genes; const float* baseline; const float* dgenes;
  const int* sizes; const long* goff;
  float* attr; float* pathway;
};

// attr = (genes - baseline) * dgenes; pathway[i] = sum of its attr: per thread k ascending in steps of 256, then the wave butterfly,
// then the four wave sums in order -- a fixed order
__global__ __launch_bounds__(GL) void ig_finalize_kernel(IgFinalArgs a) {
  __shared__ float part[GL / MT_WAVE];
  const int i = blockIdx.x, j = threadIdx.x;
  const int n = a.sizes[i];
  const long g0 = a.goff[i];
  float sum = 0.f;
  for (int k = j; k < n; k += GL) {
    const float d = a.genes[g0 + k] - (a.baseline ? a.baseline[g0 + k] : 0.f);
    const float v = d * a.dgenes[g0 + k];
    a.attr[g0 + k] = v;
    sum += v;
  }
  sum = wave_sum(sum);
  if ((j & (MT_WAVE - 1)) == 0) part[j / MT_WAVE] = sum;
  __syncthreads();
  if (j == 0) a.pathway[i] = ((lds_f32(&part[0]) + lds_f32(&part[1])) + lds_f32(&part[2])) + lds_f32(&part[3]);
}

}  // namespace

extern "C" int mt_gene_snn_fwd_points(const float* params, const long* offs, const int* sizes, const long* goff, const float* genes,
                                      const float* baseline, const float* alphas, int G, int latent, int points, float* a1, float* a2,
                                      float* z, mt_stream_t stream) {
  if (!params || !offs || !sizes || !goff || !genes || !alphas || !a1 || !a2 || !z || G < 1 || points < 1) return MT_ERR_BAD_ARG;
  if (latent != GL || points > GP_MAX) return MT_ERR_UNSUPPORTED;
  GenePointArgs a{params, offs, sizes, goff, genes, baseline, alphas, nullptr, nullptr, a1, a2, z, nullptr, nullptr, G, 0};
  hipStream_t s = (hipStream_t)stream;
  GENE_LAUNCH(gene_snn_fwd_points_kernel, points, G, s, a);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_gene_snn_bwd_input(const float* params, const long* offs, const int* sizes, const long* goff, int G, int latent,
                                     int points, const float* a1, const float* a2, const float* dz, const float* weights,
                                     const float* unscale, float* dgenes, int accumulate, mt_stream_t stream) {
  if (!params || !offs || !sizes || !goff || !a1 || !a2 || !dz || !weights || !dgenes || G < 1 || points < 1) return MT_ERR_BAD_ARG;
  if (latent != GL || points > GP_MAX) return MT_ERR_UNSUPPORTED;
  GenePointArgs a{params, offs, sizes, goff, nullptr, nullptr, nullptr, weights, unscale, const_cast<float*>(a1), const_cast<float*>(a2),
                  nullptr, dz, dgenes, G, accumulate != 0};
  hipStream_t s = (hipStream_t)stream;
  GENE_LAUNCH(gene_snn_bwd_input_kernel, points, G, s, a);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_ig_finalize(const float* genes, const float* baseline, const float* dgenes, const int* sizes, const long* goff, int G,
                              float* attr, float* pathway, mt_stream_t stream) {
  if (!genes || !dgenes || !sizes || !goff || !attr || !pathway || G < 1) return MT_ERR_BAD_ARG;
  IgFinalArgs a{genes, baseline, dgenes, sizes, goff, attr, pathway};
  hipLaunchKernelGGL(ig_finalize_kernel, dim3(G), dim3(GL), 0, (hipStream_t)stream, a);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

// ---- Integrated Gradients over the PATCH embeddings (attribution.py, inputs = "patches" / "both").  The patch embedding is affine in
// the input features, so the straight path x(alpha) = base + alpha (x - base) is the straight path between the two EMBEDDED bags, and
// sum_c IG[l][c] = <e_x[l] - e_base[l], integral dF/dx0[l]>: one interpolation in the embedding space per pass and one weighted row dot
// of the activation gradient -- no GEMM back to the input channels.  Both kernels are HBM-bound streams: 16-byte accesses, no LDS, no
// atomics.
namespace {

struct PatchPointArgs {
  const float* ex; const float* eb;      // [L][D]: the embedded input and the embedded baseline
  const float* alphas;                   // [B] device (forward)
  const float* weights;                  // [B] device (accumulate)
  const float* unscale;                  // device scalar or null (= 1)
  float* x0p;                            // [B][L][D]
  const float* dh;                       // [B][N][D]: row 0 of every pass is the cls row
  float* acc;                            // [L]
  int B, L, D, N;
};

MT_DEVINL float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// x0p[b][l] = eb[l] + alpha_b (ex[l] - eb[l]): one thread per 16 bytes of a row, ex / eb read ONCE for all B passes.  alpha = 0 / 1
// SELECT eb / ex (their bits: the endpoint passes are the plain forward at the baseline / at the input)
__global__ __launch_bounds__(GL) void patch_points_fwd_kernel(PatchPointArgs a) {
  const long e = ((long)blockIdx.x * GL + threadIdx.x) * 4;
  const long n = (long)a.L * a.D;
  if (e >= n) return;
  const float4 x = ld4(a.ex + e), b = ld4(a.eb + e);
  for (int p = 0; p < a.B; ++p) {
    const float al = a.alphas[p];
    float4 o;
    if (al == 0.f) o = b;
    else if (al == 1.f) o = x;
    else o = make_float4(fmaf(al, x.x - b.x, b.x), fmaf(al, x.y - b.y, b.y), fmaf(al, x.z - b.z, b.z), fmaf(al, x.w - b.w, b.w));
    *reinterpret_cast<float4*>(a.x0p + (long)p * n + e) = o;
  }
}

// acc[l] += unscale * sum_b w_b <dh[b][1 + l], ex[l] - eb[l]>: one wave per patch row.  A lane forms its share of every live pass's
// dot (columns ascending; the difference is formed once per column for all passes), sums the passes with their weights (b ascending),
// and wave_sum joins the 64 lane sums: one writer per acc[l], one order.  A pass with w_b == 0 is NOT read (the endpoint and padding
// slots of a quadrature); neither is any cls row.
__global__ __launch_bounds__(GL) void patch_ig_accumulate_kernel(PatchPointArgs a) {
  const int lane = threadIdx.x & (MT_WAVE - 1);
  const long l = (long)blockIdx.x * (GL / MT_WAVE) + threadIdx.x / MT_WAVE;
  if (l >= a.L) return;                  // (whole waves leave: wave_sum below sees full waves only)
  float w[GP_MAX], part[GP_MAX];
#pragma unroll
  for (int p = 0; p < GP_MAX; ++p) {
    w[p] = p < a.B ? a.weights[p] : 0.f;
    part[p] = 0.f;
  }
  const float* ex = a.ex + l * a.D;
  const float* eb = a.eb + l * a.D;
  for (int c = lane * 4; c < a.D; c += MT_WAVE * 4) {
    const float4 x = ld4(ex + c), b = ld4(eb + c);
    const float4 d = make_float4(x.x - b.x, x.y - b.y, x.z - b.z, x.w - b.w);
#pragma unroll
    for (int p = 0; p < GP_MAX; ++p) {
      if (w[p] == 0.f) continue;         // (wave-uniform)
      const float4 g = ld4(a.dh + ((long)p * a.N + 1 + l) * a.D + c);
      part[p] = fmaf(g.w, d.w, fmaf(g.z, d.z, fmaf(g.y, d.y, fmaf(g.x, d.x, part[p]))));
    }
  }
  float s = 0.f;
#pragma unroll
  for (int p = 0; p < GP_MAX; ++p)
    if (w[p] != 0.f) s = fmaf(w[p], part[p], s);
  s = wave_sum(s);
  if (lane == 0) a.acc[l] += (a.unscale ? a.unscale[0] : 1.f) * s;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mt_patch_points_fwd(const float* ex, const float* eb, const float* alphas, int B, int L, int D, float* x0p,
                                   mt_stream_t stream) {
  if (!ex || !eb || !alphas || !x0p || B < 1 || L < 1 || D < 4 || (D & 3)) return MT_ERR_BAD_ARG;
  if (!aligned16(ex) || !aligned16(eb) || !aligned16(x0p)) return MT_ERR_BAD_ARG;
  if (B > GP_MAX) return MT_ERR_UNSUPPORTED;
  const long blocks = ((long)L * D / 4 + GL - 1) / GL;
  if (blocks > 0x7fffffffL) return MT_ERR_UNSUPPORTED;
  PatchPointArgs a{ex, eb, alphas, nullptr, nullptr, x0p, nullptr, nullptr, B, L, D, 0};
  hipLaunchKernelGGL(patch_points_fwd_kernel, dim3((unsigned)blocks), dim3(GL), 0, (hipStream_t)stream, a);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_patch_ig_accumulate(const float* dh, int N, const float* ex, const float* eb, const float* weights,
                                      const float* unscale, int B, int L, int D, float* acc, mt_stream_t stream) {
  if (!dh || !ex || !eb || !weights || !acc || B < 1 || L < 1 || N < L + 1 || D < 4 || (D & 3)) return MT_ERR_BAD_ARG;
  if (!aligned16(dh) || !aligned16(ex) || !aligned16(eb)) return MT_ERR_BAD_ARG;
  if (B > GP_MAX) return MT_ERR_UNSUPPORTED;
  PatchPointArgs a{ex, eb, nullptr, weights, unscale, nullptr, dh, acc, B, L, D, N};
  hipLaunchKernelGGL(patch_ig_accumulate_kernel, dim3(cdiv(L, GL / MT_WAVE)), dim3(GL), 0, (hipStream_t)stream, a);
  MT_CHECK_LAUNCH();
  return MT_OK;
}
