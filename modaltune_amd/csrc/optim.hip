// Distillation loss head, fused AdamW with GradScaler semantics, and library metadata.
#include "common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// One workgroup: R <= 8 rows of O <= 1024 logits.  train_modaltune.py:225-233:
//   z = logit / ||logit||; loss = 10 * sum_r sum_j p_rj (log p_rj - log_softmax(z_r)_j), p = softmax(target_r)
// d loss / d z_rj = 10 * (softmax(z_r)_j - p_rj)   (sum_j p_rj = 1);  d/d logit = (dz - z (z . dz)) / ||logit||
__global__ __launch_bounds__(256) void distill_loss_kernel(const float* __restrict__ logits, const float* __restrict__ target, int R, int O,
                                                           float loss_scale_host, const float* __restrict__ scale_dev,
                                                           float* __restrict__ loss, float* __restrict__ dlogits) {
  const float loss_scale = loss_scale_host * (scale_dev ? *scale_dev : 1.0f);
  __shared__ float red[256];
  __shared__ float bc[4];
  const int tid = threadIdx.x;
  auto block_sum = [&](float v) {
    red[tid] = v; __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const float r = red[0]; __syncthreads(); return r;
  };
  auto block_max = [&](float v) {
    red[tid] = v; __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]); __syncthreads(); }
    const float r = red[0]; __syncthreads(); return r;
  };
  float total = 0.f;
  for (int r = 0; r < R; ++r) {
    const float* lg = logits + (long)r * O;
    const float* tg = target + (long)r * O;
    float ss = 0.f;
    for (int j = tid; j < O; j += 256) ss += lg[j] * lg[j];
    const float nrm = sqrtf(block_sum(ss));
    float zm = -1.0e30f, tm = -1.0e30f;
    for (int j = tid; j < O; j += 256) { zm = fmaxf(zm, lg[j] / nrm); tm = fmaxf(tm, tg[j]); }
    zm = block_max(zm); tm = block_max(tm);
    float ze = 0.f, te = 0.f;
    for (int j = tid; j < O; j += 256) { ze += expf(lg[j] / nrm - zm); te += expf(tg[j] - tm); }
    ze = block_sum(ze); te = block_sum(te);
    const float zl = zm + logf(ze), tl = tm + logf(te);
    float part = 0.f, zdz = 0.f;
    for (int j = tid; j < O; j += 256) {
      const float z = lg[j] / nrm;
      const float logq = z - zl, logp = tg[j] - tl, p = expf(logp);
      part += p * (logp - logq);
      const float dz = 10.0f * (expf(logq) - p);
      zdz += z * dz;
    }
    part = block_sum(part); zdz = block_sum(zdz);
    total += 10.0f * part;
    for (int j = tid; j < O; j += 256) {
      const float z = lg[j] / nrm;
      const float dz = 10.0f * (expf(z - zl) - expf(tg[j] - tl));
      dlogits[(long)r * O + j] = loss_scale * (dz - z * zdz) / nrm;
    }
  }
  if (tid == 0) *loss = total;
  (void)bc;
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                             float lr, float b1, float b2, float omb1, float omb2, float eps, double wd, float decay, float bc1, float bc2s,
                             double b1d, double b2d, float grad_mult, const float* __restrict__ scale, const int* __restrict__ found_inf,
                             const int* __restrict__ step_dev, const float* __restrict__ lr_dev) {
  if (found_inf && *found_inf) return;       // GradScaler.step: skip the whole update when a grad is inf/nan
  // the schedule's current learning rate lives on the device (graph replays read it); 1 - lr * wd in double, as torch forms it
  if (lr_dev) { lr = *lr_dev; decay = (float)(1.0 - (double)lr * wd); }
  if (step_dev) {                            // optimiser step count lives on the device (skipped steps do not count)
    // bias corrections in DOUBLE, as torch's Python arithmetic forms them (1 - beta ** step): powf in fp32 is ~1e-5 off in the first
    // steps, where 1 - beta2 ** step is itself ~1e-3 (two pows per thread against >= 32 elements of 28 bytes each: not measurable)
    const double st = (double)(*step_dev + 1);
    bc1 = (float)(1.0 - pow(b1d, st));
    bc2s = (float)sqrt(1.0 - pow(b2d, st));
  }
  const float inv_scale = grad_mult * (scale ? 1.0f / *scale : 1.0f);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float gi = g[i] * inv_scale;
    float pi = p[i] * decay;
    const float mi = b1 * m[i] + omb1 * gi;                 // (omb = 1 - beta formed in double on the host, as torch does)
    const float vi = b2 * v[i] + omb2 * gi * gi;
    pi -= (lr / bc1) * mi / (sqrtf(vi) / bc2s + eps);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

// adamw_kernel with PARAMETER GROUPS: the flat buffer is a run of segments (tensors of one group that lie next to each other), a
// segment's group supplies lr_mult and weight_decay; everything else -- betas, eps, bias corrections, grad_mult / *scale, the found_inf
// skip -- is shared.  Per element the arithmetic is adamw_kernel's, expression for expression (adamw_elem below).
//   lr_g = (float)((double)lr_f32 * lr_mult)  (rounded once: lr_mult == 1.0 gives the base bits),  decay_g = (float)(1 - (double)lr_g * wd_g)
// Indices are ABSOLUTE (index_base + i: pieces of one buffer compose as in checksum64_partials_kernel).  Segment ends are multiples of
// 4 and a float4 starts on an absolute multiple of 4, so a vector never straddles two segments: one lookup per vector at most.  Every
// workgroup owns a CONTIGUOUS range of vectors (whole 256-vector rows); a thread walks it in steps of 256 vectors, two vectors in flight, finds the segment of its first vector by
// one binary search and from then on only moves forward, keeping the segment's end and its two values in registers -- a vector
// inside the same segment costs one compare, no memory read.  The group table travels as kernel arguments (no upload).  Workgroup 0
// takes the `head` scalars in front of the first vector and the tail behind the last (grad_sumsq_partials_kernel's form).  No LDS, no
// atomics.
constexpr int ADAMG_THREADS = 256, ADAMG_MAX_WGS = 8192, ADAMG_MAX_GROUPS = MT_ADAM_MAX_GROUPS;
static_assert((ADAMG_MAX_GROUPS & (ADAMG_MAX_GROUPS - 1)) == 0, "group ids are masked into the table");
struct AdamGroupTab { double lr_mult[ADAMG_MAX_GROUPS]; double wd[ADAMG_MAX_GROUPS]; };

struct AdamShared { float b1, b2, omb1, omb2, eps, bc1, bc2s, inv_scale; };

// adamw_kernel's loop body is written as plain expressions and compiled under the build's default -ffp-contract=fast, which fuses ONE
// of them: m = fma(1 - beta1, g, beta1 * m); the two products of v are rounded and then added, p * decay and the quotient are
// rounded and then subtracted.  Which expressions a compiler fuses depends on the code around them (the float4 form fused v as
// well), so the roundings are spelled out here: contraction off, the one FMA explicit.  tests/test_adamw_groups_gpu.py holds the two
// kernels to the same bits.
MT_DEVINL void adamw_elem(float& p, float g, float& m, float& v, float lr, float decay, const AdamShared& c) {
#pragma clang fp contract(off)
  const float gi = g * c.inv_scale;
  float pi = p * decay;
  const float mi = fmaf(c.omb1, gi, c.b1 * m);
  const float vi = c.b2 * v + (c.omb2 * gi) * gi;
  const float step = (lr / c.bc1) * mi;
  const float den = sqrtf(vi) / c.bc2s + c.eps;
  pi = pi - step / den;
  p = pi; m = mi; v = vi;
}

// Exponential moving average of the parameters, inside the AdamW launch (EMA = true): one more flat buffer `ema`, indexed like `p`,
// moved towards the NEW parameter by the launch's one weight w = 1 - decay_t.  Three fp32 operations, each rounded once, no FMA -- the
// difference form: a tensor held still whose average equals it (d = 0) keeps every bit, which decay * e + (1 - decay) * p would not.
MT_DEVINL void ema_elem(float& e, float p_new, float w) {
#pragma clang fp contract(off)
  const float d = p_new - e;
  const float t = w * d;
  e = e + t;
}

// w of optimiser step t (1-based), in double, on the host (step_count) and on the device (*step_dev + 1) alike:
//   decay_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay,   w = (float)(1 - decay_t)
__host__ __device__ inline float ema_weight(double decay, int warmup, double t) {
  double d = decay;
  if (warmup) { const double r = (1.0 + t) / (10.0 + t); d = r < d ? r : d; }
  return (float)(1.0 - d);
}

template <bool EMA>
MT_DEVINL f32x4 ema_load(const f32x4* __restrict__ ev, long i) {
  if constexpr (EMA) return ev[i];
  else return f32x4{0.f, 0.f, 0.f, 0.f};
}

// the segment of absolute index a: the first s with a < seg_end[s] (an index behind the last end stays in the last segment)
MT_DEVINL int adamg_find(const int* __restrict__ seg_end, int nseg, long a) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a < (long)seg_end[mid]) hi = mid; else lo = mid + 1;
  }
  return lo;
}

MT_DEVINL void adamg_values(const AdamGroupTab& tab, const unsigned char* __restrict__ seg_group, int s, float lr, float& lr_g,
                            float& decay_g) {
  const int gid = (int)seg_group[s] & (ADAMG_MAX_GROUPS - 1);
  lr_g = (float)((double)lr * tab.lr_mult[gid]);
  decay_g = (float)(1.0 - (double)lr_g * tab.wd[gid]);
}

template <bool EMA>
__global__ __launch_bounds__(ADAMG_THREADS) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                     float* __restrict__ v, long n, long base, int head, long nvec, long per,
                                                                     const int* __restrict__ seg_end,
                                                                     const unsigned char* __restrict__ seg_group, int nseg,
                                                                     AdamGroupTab tab, float lr, float b1, float b2, float omb1, float omb2,
                                                                     float eps, float bc1, float bc2s, double b1d, double b2d, float grad_mult,
                                                                     const float* __restrict__ scale, const int* __restrict__ found_inf,
                                                                     const int* __restrict__ step_dev, const float* __restrict__ lr_dev,
                                                                     float* __restrict__ ema, float ema_w, double ema_decay,
                                                                     int ema_warmup) {
  if (found_inf && *found_inf) return;       // (EMA: a skipped step moves nothing and does not count)
  if (lr_dev) lr = *lr_dev;
  if (step_dev) {                            // (adamw_kernel: the bias corrections in double from the device's step count)
    const double st = (double)(*step_dev + 1);
    bc1 = (float)(1.0 - pow(b1d, st));
    bc2s = (float)sqrt(1.0 - pow(b2d, st));
    if constexpr (EMA) ema_w = ema_weight(ema_decay, ema_warmup, st);
  }
  const AdamShared c = {b1, b2, omb1, omb2, eps, bc1, bc2s, grad_mult * (scale ? 1.0f / *scale : 1.0f)};
  const int tid = threadIdx.x;
  const long vbase = base + head;            // absolute index of the first element of vector 0 (a multiple of 4: the launcher checked)
  f32x4* __restrict__ pv = reinterpret_cast<f32x4*>(p + head);
  const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
  f32x4* __restrict__ mv = reinterpret_cast<f32x4*>(m + head);
  f32x4* __restrict__ vv = reinterpret_cast<f32x4*>(v + head);
  f32x4* __restrict__ ev = reinterpret_cast<f32x4*>(ema + head);      // (EMA = false: never dereferenced)
  const long v0 = (long)blockIdx.x * per, v1 = v0 + per < nvec ? v0 + per : nvec;      // (per: a multiple of the workgroup size)
  long i = v0 + tid;
  if (i < v1) {
    int s = adamg_find(seg_end, nseg, vbase + 4 * i);
    long end = (long)seg_end[s];
    float lr_g, decay_g;
    adamg_values(tab, seg_group, s, lr, lr_g, decay_g);
    auto update = [&](long iv, f32x4 p4, f32x4 g4, f32x4 m4, f32x4 v4, f32x4 e4) {
      const long a = vbase + 4 * iv;
      if (a >= end && s + 1 < nseg) {        // (forward only; behind the last end: the last segment)
        do { ++s; end = (long)seg_end[s]; } while (a >= end && s + 1 < nseg);
        adamg_values(tab, seg_group, s, lr, lr_g, decay_g);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p4[e], me = m4[e], ve = v4[e];
        adamw_elem(pe, g4[e], me, ve, lr_g, decay_g, c);
        p4[e] = pe; m4[e] = me; v4[e] = ve;
        if constexpr (EMA) { float ee = e4[e]; ema_elem(ee, pe, ema_w); e4[e] = ee; }
      }
      pv[iv] = p4; mv[iv] = m4; vv[iv] = v4;
      if constexpr (EMA) ev[iv] = e4;
    };
    for (; i + ADAMG_THREADS < v1; i += 2 * ADAMG_THREADS) {      // two vectors per thread: eight 16-byte loads in flight (EMA: ten)
      const long k = i + ADAMG_THREADS;
      const f32x4 pa = pv[i], ga = gv[i], ma = mv[i], va = vv[i], pb = pv[k], gb = gv[k], mb = mv[k], vb = vv[k];
      const f32x4 ea = ema_load<EMA>(ev, i), eb = ema_load<EMA>(ev, k);
      update(i, pa, ga, ma, va, ea);
      update(k, pb, gb, mb, vb, eb);
    }
    if (i < v1) update(i, pv[i], gv[i], mv[i], vv[i], ema_load<EMA>(ev, i));
  }
  if (blockIdx.x == 0) {
    const long tail0 = head + 4 * nvec;
    long j = -1;
    if (tid < head) j = tid;
    else if (tid >= 4 && tail0 + (tid - 4) < n) j = tail0 + (tid - 4);      // (head <= 3, n - tail0 <= 3: threads 0..2 and 4..6)
    if (j >= 0) {
      float lr_g, decay_g;
      adamg_values(tab, seg_group, adamg_find(seg_end, nseg, base + j), lr, lr_g, decay_g);
      adamw_elem(p[j], g[j], m[j], v[j], lr_g, decay_g, c);
      if constexpr (EMA) ema_elem(ema[j], p[j], ema_w);
    }
  }
}

// a[i] <-> b[i] over two fp32 buffers that do not overlap, moved as 32-bit PATTERNS (NaN payloads, -0.0 survive).  Both 4-byte aligned:
// when they sit alike in their 16-byte lines everything between the `head` scalars in front of the first boundary and the tail behind
// the last whole vector goes as 16-byte loads and stores (grad_sumsq_partials_kernel's form, two vectors of each buffer in flight); else
// the launcher hands over nvec = 0 and every word goes through the scalar loop.  A grid-stride loop over a fixed cap of workgroups.
constexpr int SWAP_THREADS = 256, SWAP_MAX_WGS = 2048;

__global__ __launch_bounds__(SWAP_THREADS) void swap_f32_kernel(unsigned* __restrict__ a, unsigned* __restrict__ b, long n, int head,
                                                                long nvec) {
  u32x4* __restrict__ av = reinterpret_cast<u32x4*>(a + head);
  u32x4* __restrict__ bv = reinterpret_cast<u32x4*>(b + head);
  const long stride = (long)gridDim.x * SWAP_THREADS, first = (long)blockIdx.x * SWAP_THREADS + threadIdx.x;
  long v = first;
  for (; v + stride < nvec; v += 2 * stride) {
    const u32x4 a0 = av[v], b0 = bv[v], a1 = av[v + stride], b1 = bv[v + stride];
    av[v] = b0; bv[v] = a0; av[v + stride] = b1; bv[v + stride] = a1;
  }
  if (v < nvec) { const u32x4 a0 = av[v], b0 = bv[v]; av[v] = b0; bv[v] = a0; }
  const long tail0 = head + 4 * nvec, loose = head + (n - tail0);      // the words outside the vectors: [0, head) and [tail0, n)
  for (long j = first; j < loose; j += stride) {
    const long i = j < head ? j : tail0 + (j - head);
    const unsigned x = a[i], y = b[i];
    a[i] = y; b[i] = x;
  }
}

__global__ void check_finite_kernel(const float* __restrict__ g, long n, int* __restrict__ found_inf) {
  bool bad = false;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    bad |= !isfinite(g[i]);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(found_inf, 1);
}

// Sum of squares of the flat gradient, stage 1: workgroup b stores the double sum of its grid-stride share into partials[b] (a plain
// store into its own slot: the workspace needs no initialisation, nothing is added with atomics).  Squares and sums are double from
// the first element: finite fp32 inputs cannot overflow (2^24 * FLT_MAX^2 < 2^281) and the result does not depend on fp32 association.
// `g` is 4-byte aligned: workgroup 0 takes the `head` scalars in front of the first 16-byte boundary and the `tail` scalars behind the
// last whole float4; everything between is read as float4, four loads in flight per thread.  The cross-wave step goes through LDS
// as doubles only (one LDS banking class, common.h).
constexpr int SUMSQ_THREADS = 256, SUMSQ_UNROLL = 4, SUMSQ_MAX_WGS = 2048;
constexpr long SUMSQ_WG_ELEMS = (long)SUMSQ_THREADS * SUMSQ_UNROLL * 4;      // elements of one workgroup before the grid stride

MT_DEVINL double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
MT_DEVINL double sq4(f32x4 x) {
  const double a = (double)x[0], b = (double)x[1], c = (double)x[2], d = (double)x[3];
  return fma(a, a, fma(b, b, fma(c, c, d * d)));
}

__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_partials_kernel(const float* __restrict__ g, long n, int head, long nvec,
                                                                            double* __restrict__ partials) {
  __shared__ double red[SUMSQ_THREADS / MT_WAVE];
  const int tid = threadIdx.x;
  const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
  const long stride = (long)gridDim.x * SUMSQ_THREADS;
  double acc = 0.0;
  long v = (long)blockIdx.x * SUMSQ_THREADS + tid;
  for (; v + 3 * stride < nvec; v += 4 * stride) {
    const f32x4 x0 = gv[v], x1 = gv[v + stride], x2 = gv[v + 2 * stride], x3 = gv[v + 3 * stride];
    acc += (sq4(x0) + sq4(x1)) + (sq4(x2) + sq4(x3));
  }
  for (; v < nvec; v += stride) acc += sq4(gv[v]);
  if (blockIdx.x == 0) {
    const long tail0 = head + 4 * nvec;
    if (tid < head) { const double x = (double)g[tid]; acc = fma(x, x, acc); }
    if (tail0 + tid < n) { const double x = (double)g[tail0 + tid]; acc = fma(x, x, acc); }      // (n - tail0 <= 3)
  }
  acc = wave_sum_f64(acc);
  if ((tid & (MT_WAVE - 1)) == 0) red[tid / MT_WAVE] = acc;
  __syncthreads();
  if (tid == 0) {
    double s = red[0];
#pragma unroll
    for (int w = 1; w < SUMSQ_THREADS / MT_WAVE; ++w) s += red[w];
    partials[blockIdx.x] = s;
  }
}

// Stage 2, one workgroup: thread t adds the slots [t * per, (t + 1) * per) in ascending order, thread 0 adds the 256 thread sums in
// ascending order.  A sum of squares is non-finite exactly when an element was (inf^2 = +inf, squares never cancel): that is the flag,
// ORed like mt_check_finite's and never cleared.
__global__ __launch_bounds__(SUMSQ_THREADS) void grad_sumsq_final_kernel(const double* __restrict__ partials, int nparts,
                                                                         double* __restrict__ sumsq, int* __restrict__ found_inf) {
  __shared__ double red[SUMSQ_THREADS];
  const int tid = threadIdx.x, per = (nparts + SUMSQ_THREADS - 1) / SUMSQ_THREADS;
  double s = 0.0;
  for (int i = tid * per; i < min(nparts, (tid + 1) * per); ++i) s += partials[i];
  red[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int i = 1; i < SUMSQ_THREADS; ++i) t += red[i];
    sumsq[0] = t;
    if (found_inf && !isfinite(t)) atomicOr(found_inf, 1);
  }
}

// Exact 64-bit checksum of a buffer of 32-bit words (the replica canary and the checkpoint seal):
//   out[0] = sum_i mix(index_base + i) * (word_i + 1)  mod 2^64,   mix(j) = splitmix64(j) | 1
// Unsigned integer sums are associative: any grid, any reduction order, the same value -- so the two stages take the form of
// grad_sumsq_partials / final_kernel above (own slot per workgroup, plain stores, no atomics, no initialised workspace) without their
// ordering rules.  The multiplier is odd (a single-word change always moves the sum) and depends on the position (swapped words move
// it); the + 1 makes runs of zeros of different lengths differ; index_base makes pieces compose.  The cross-wave step goes through LDS
// as 8-byte words only (one LDS banking class, common.h).

MT_DEVINL u64 cs_mix(u64 j) {
  u64 z = j + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (z ^ (z >> 31)) | 1ull;
}
MT_DEVINL u64 cs_term(u64 j, unsigned w) { return cs_mix(j) * ((u64)w + 1ull); }
MT_DEVINL u64 cs4(u64 j, u32x4 x) { return (cs_term(j, x[0]) + cs_term(j + 1, x[1])) + (cs_term(j + 2, x[2]) + cs_term(j + 3, x[3])); }
MT_DEVINL u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(SUMSQ_THREADS) void checksum64_partials_kernel(const unsigned* __restrict__ d, long n, u64 base, int head,
                                                                            long nvec, u64* __restrict__ partials) {
  __shared__ u64 red[SUMSQ_THREADS / MT_WAVE];
  const int tid = threadIdx.x;
  const u32x4* __restrict__ dv = reinterpret_cast<const u32x4*>(d + head);
  const long stride = (long)gridDim.x * SUMSQ_THREADS;
  const u64 vbase = base + (u64)head;       // index of the first word of vector 0
  u64 acc = 0;
  long v = (long)blockIdx.x * SUMSQ_THREADS + tid;
  for (; v + 3 * stride < nvec; v += 4 * stride) {
    const u32x4 x0 = dv[v], x1 = dv[v + stride], x2 = dv[v + 2 * stride], x3 = dv[v + 3 * stride];
    acc += (cs4(vbase + 4 * (u64)v, x0) + cs4(vbase + 4 * (u64)(v + stride), x1)) +
           (cs4(vbase + 4 * (u64)(v + 2 * stride), x2) + cs4(vbase + 4 * (u64)(v + 3 * stride), x3));
  }
  for (; v < nvec; v += stride) acc += cs4(vbase + 4 * (u64)v, dv[v]);
  if (blockIdx.x == 0) {
    const long tail0 = head + 4 * nvec;
    if (tid < head) acc += cs_term(base + (u64)tid, d[tid]);
    if (tail0 + tid < n) acc += cs_term(base + (u64)(tail0 + tid), d[tail0 + tid]);      // (n - tail0 <= 3)
  }
  acc = wave_sum_u64(acc);
  if ((tid & (MT_WAVE - 1)) == 0) red[tid / MT_WAVE] = acc;
  __syncthreads();
  if (tid == 0) {
    u64 s = red[0];
#pragma unroll
    for (int w = 1; w < SUMSQ_THREADS / MT_WAVE; ++w) s += red[w];
    partials[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(SUMSQ_THREADS) void checksum64_final_kernel(const u64* __restrict__ partials, int nparts,
                                                                         u64* __restrict__ out) {
  __shared__ u64 red[SUMSQ_THREADS];
  const int tid = threadIdx.x, per = (nparts + SUMSQ_THREADS - 1) / SUMSQ_THREADS;
  u64 s = 0;
  for (int i = tid * per; i < min(nparts, (tid + 1) * per); ++i) s += partials[i];
  red[tid] = s;
  __syncthreads();
  if (tid == 0) {
    u64 t = red[0];
    for (int i = 1; i < SUMSQ_THREADS; ++i) t += red[i];
    out[0] = t;
  }
}

// torch.nn.utils.clip_grad_norm_'s coefficient on the device, one thread, double throughout, each output rounded once:
//   out[0] = total_norm = sqrt(sum of the slots, ascending) * grad_mult / *scale
//   out[1] = coef = min(1, max_norm / (total_norm + 1e-6));   out[2] = *scale / coef: the `scale` mt_adamw_step then divides by
// coef == 1 (also: max_norm = +inf, a set found_inf, a non-finite sum) leaves out[2] = *scale bit for bit; a finite gradient whose norm
// overflows fp32 gives total_norm = +inf and coef = 0 (out[2] = +inf: AdamW sees g * 0), as torch does.
__global__ void grad_clip_coef_kernel(const double* __restrict__ sumsq, int nsums, double grad_mult, const float* __restrict__ scale,
                                      double max_norm, const int* __restrict__ found_inf, float* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  double S = sumsq[0];
  for (int i = 1; i < nsums; ++i) S += sumsq[i];
  const float sc = scale ? *scale : 1.0f;
  const double norm = sqrt(S) * grad_mult / (double)sc;
  const float normf = (float)norm;
  float coef = 1.0f, eff = sc;
  if (isfinite(S) && !(found_inf && *found_inf) && !isinf(max_norm)) {
    if (isinf(normf)) { coef = 0.0f; eff = __builtin_inff(); }
    else {
      const double c = fmin(1.0, max_norm / (norm + 1e-6));
      coef = (float)c;
      if (coef != 1.0f) eff = (float)((double)sc / c);
    }
  }
  out[0] = normf; out[1] = coef; out[2] = eff;
}

// y[r] = x[r] / ||x[r]||_2 : one workgroup per row (text / ||text||, TM:213)
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int O) {
  __shared__ float red[256];
  const float* xr = x + (long)blockIdx.x * O;
  float s = 0.f;
  for (int j = threadIdx.x; j < O; j += 256) s += xr[j] * xr[j];
  red[threadIdx.x] = s; __syncthreads();
  for (int k = 128; k > 0; k >>= 1) { if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k]; __syncthreads(); }
  const float inv = 1.0f / sqrtf(red[0]);
  for (int j = threadIdx.x; j < O; j += 256) y[(long)blockIdx.x * O + j] = xr[j] * inv;
}

// torch.cuda.amp.GradScaler.update (TM:107,237): backoff 0.5 on overflow, x2 after `interval` clean steps.  As in
// torch._amp_update_scale_, a growth whose product is not finite keeps the old scale (the tracker still restarts).
__global__ void scaler_update_kernel(float* scale, int* tracker, int* found_inf, int* step_dev, float growth, float backoff, int interval) {
  if (threadIdx.x || blockIdx.x) return;
  if (*found_inf) { *scale *= backoff; *tracker = 0; }
  else {
    if (step_dev) ++(*step_dev);
    if (++(*tracker) >= interval) {
      const float grown = *scale * growth;
      if (isfinite(grown)) *scale = grown;
      *tracker = 0;
    }
  }
  *found_inf = 0;
}


// s[0] = target / max|x| (1 when the maximum is 0 or not finite), s[1] = 1 / s[0]: the device-side loss-scale of the
// nn.Module bridge (no host read-back of the incoming gradient's range).  One workgroup; n is a few hundred.
// s[0] is CLAMPED to [2^-126, 2^126]: a maximum below ~target / FLT_MAX (a nearly converged loss) would make target / max|x|
// +inf and s[1] zero (0 * inf = NaN gradients); at the clamp the factor is a power of two, both s[0] and s[1] are normal
// numbers and scaling by them is exact.  So s[0] and s[1] are finite and positive for every input.
__global__ __launch_bounds__(256) void absmax_scale_kernel(const float* __restrict__ x, long n, float target, float* __restrict__ s) {
  __shared__ float red[256];
  float m = 0.f;
  bool bad = false;
  for (long i = threadIdx.x; i < n; i += 256) { const float v = fabsf(x[i]); bad |= !(v <= 3.0e38f); m = fmaxf(m, v); }
  red[threadIdx.x] = bad ? __builtin_inff() : m; __syncthreads();
  for (int k = 128; k > 0; k >>= 1) { if (threadIdx.x < k) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + k]); __syncthreads(); }
  if (threadIdx.x == 0) {
    const float a = red[0];
    const float sc = (a > 0.f && a <= 3.0e38f) ? fminf(fmaxf(target / a, 0x1p-126f), 0x1p126f) : 1.0f;
    s[0] = sc; s[1] = 1.0f / sc;
  }
}

// y = a + (*alpha) * b (a may be null: y = (*alpha) * b).  In place, y == b (optim.clip_grad_norm_: g *= coef) or y == a, is
// supported: a thread reads index i of its inputs before it writes index i and touches no other index -- so `a`, `b` and `y` carry no
// __restrict__.
__global__ void axpy_dev_kernel(const float* a, const float* b, const float* __restrict__ alpha, float* y, long n) {
  const float al = *alpha;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = (a ? a[i] : 0.f) + al * b[i];
}

// grid cell of every patch: row = floor(coords[:, 0] / tile), col = floor(coords[:, 1] / tile) (slide_encoder.py:209-211);
// cells outside [0, ngrids) are clamped and reported through *err (checked by the host when it next synchronises)
__global__ void coords_to_grid_kernel(const float* __restrict__ coords, int L, float tile, int ngrids, int* __restrict__ prow,
                                      int* __restrict__ pcol, int* __restrict__ err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  const float fr = floorf(coords[2 * i] / tile), fc = floorf(coords[2 * i + 1] / tile);
  // (int) of a NaN / out-of-range float is unspecified: test the floats (NaN fails every comparison -> bad)
  const bool bad = !(fr >= 0.f && fc >= 0.f && fr < (float)ngrids && fc < (float)ngrids);
  const int r = bad ? 0 : (int)fr, c = bad ? 0 : (int)fc;
  prow[i] = min(max(r, 0), ngrids - 1);
  pcol[i] = min(max(c, 0), ngrids - 1);
  if (bad && err) atomicOr(err, 1);
}

// dst(idx[m], :) (+)= src(m, :): rows scattered by index (TITAN feature gridding: index_add of the patch features into
// their grid cells, titan_adapter.py:318-320); atomics because several patches may fall into one cell
__global__ void scatter_rows_kernel(const float* __restrict__ src, const int* __restrict__ src_idx, const int* __restrict__ idx,
                                    float* __restrict__ dst, int M, int D, int accumulate) {
  const long n = (long)M * D;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / D), d = (int)(i - (long)m * D);
    const float v = src[(long)(src_idx ? src_idx[m] : m) * D + d];
    float* p = dst + (long)idx[m] * D + d;
    if (accumulate) atomicAdd(p, v);
    else *p = v;
  }
}

// out[m] = max_d |x(m, d)|: one wave per row
__global__ __launch_bounds__(256) void row_absmax_kernel(const float* __restrict__ x, float* __restrict__ out, int M, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long m = (long)blockIdx.x * 4 + wave; m < M; m += (long)gridDim.x * 4) {
    float v = 0.f;
    for (int d = lane; d < D; d += 64) v = fmaxf(v, fabsf(x[m * D + d]));
    v = wave_max(v);
    if (lane == 0) out[m] = v;
  }
}

// Bare MFMA loop (bench.py: the chip's own fp16 MFMA rate next to the vendor peak): every wave issues
// `iters` x 4 independent v_mfma_f32_32x32x16_f16 on pseudo-random register operands (the clock the chip holds depends on the
// data: all-zero operands read ~19 % high, MI355X_MICROARCH.md "DVFS give-back"), 4 waves per workgroup = one per SIMD.
__global__ __launch_bounds__(256) void mfma_probe_kernel(float* __restrict__ sink, int iters) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  h16x8 a, b;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    unsigned h = (t * 9781u + e * 6271u) * 2654435761u;
    a[e] = (h16)(((int)(h >> 20) & 1023) * (1.0f / 1024.0f) - 0.5f);
    b[e] = (h16)(((int)(h >> 8) & 1023) * (1.0f / 1024.0f) - 0.5f);
  }
  f32x16 c0, c1, c2, c3;
#pragma unroll
  for (int i = 0; i < 16; ++i) { c0[i] = 0.f; c1[i] = 0.f; c2[i] = 0.f; c3[i] = 0.f; }
  for (int it = 0; it < iters; ++it) {
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(b, a, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, a, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f32_32x32x16_f16(b, b, c3, 0, 0, 0);
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += c0[i] + c1[i] + c2[i] + c3[i];
  if (s == 123.456f) sink[0] = s;      // (keeps the chains alive; practically never taken)
}

}  // namespace

extern "C" int mt_l2norm_rows(const float* x, float* y, int R, int O, mt_stream_t stream) {
  if (!x || !y || R < 1 || O < 1) return MT_ERR_BAD_ARG;
  hipLaunchKernelGGL(l2norm_rows_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, x, y, O);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_scaler_update(float* scale, int* growth_tracker, int* found_inf, int* step_dev, float growth,
                                float backoff, int interval, mt_stream_t stream) {
  if (!scale || !growth_tracker || !found_inf || interval < 1) return MT_ERR_BAD_ARG;
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale, growth_tracker, found_inf, step_dev,
                     growth, backoff, interval);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_distill_loss(const float* logits, const float* target, int R, int O, float loss_scale,
                               const float* scale_dev, float* loss, float* dlogits, mt_stream_t stream) {
  if (!logits || !target || !loss || !dlogits || R < 1 || O < 1) return MT_ERR_BAD_ARG;
  hipLaunchKernelGGL(distill_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, target, R, O, loss_scale, scale_dev,
                     loss, dlogits);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_adamw_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                             double eps, double weight_decay, int step_count, const int* step_dev, float grad_mult,
                             const float* scale, int* found_inf, const float* lr_dev, mt_stream_t stream) {
  if (!p || !g || !m || !v || n <= 0 || (step_count < 1 && !step_dev)) return MT_ERR_BAD_ARG;
  if (step_count < 1) step_count = 1;
  const float bc1 = (float)(1.0 - pow(beta1, (double)step_count));
  const float bc2s = (float)sqrt(1.0 - pow(beta2, (double)step_count));
  const int grid = (int)((n + 1023) / 1024 > 4096 ? 4096 : (n + 1023) / 1024);
  hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, (float)lr, (float)beta1, (float)beta2,
                     (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, weight_decay, (float)(1.0 - lr * weight_decay), bc1, bc2s,
                     beta1, beta2, grad_mult, scale, (const int*)found_inf, step_dev, lr_dev);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

// the one body of mt_adamw_step_groups and mt_adamw_step_groups_ema (ema == NULL: the EMA = false instantiation)
static int adamw_groups_launch(float* p, const float* g, float* m, float* v, long n, long index_base, const int* seg_end,
                               const unsigned char* seg_group, int nseg, const MtAdamGroup* groups, int ngroups, double lr, double beta1,
                               double beta2, double eps, int step_count, const int* step_dev, float grad_mult, const float* scale,
                               int* found_inf, const float* lr_dev, float* ema, double ema_decay, int ema_warmup, mt_stream_t stream) {
  if (!p || !g || !m || !v || !seg_end || !seg_group || !groups || nseg < 1 || n < 1 || index_base < 0 || (step_count < 1 && !step_dev))
    return MT_ERR_BAD_ARG;
  if (ema && !(ema_decay >= 0.0 && ema_decay < 1.0)) return MT_ERR_BAD_ARG;
  if (ngroups < 1 || ngroups > MT_ADAM_MAX_GROUPS) return MT_ERR_UNSUPPORTED;
  // a float4 starts on an absolute multiple of 4 AND on a 16-byte address, in all buffers: the piece must lie in its buffer as
  // index_base says (p = flat + index_base with a 16-byte aligned flat)
  const uintptr_t want = (uintptr_t)(index_base & 3);
  for (const void* q : {(const void*)p, (const void*)g, (const void*)m, (const void*)v, (const void*)(ema ? ema : p)})
    if (((uintptr_t)q & 3) || (((uintptr_t)q >> 2) & 3) != want) return MT_ERR_BAD_ARG;
  if (ema)      // the average is a buffer of its own: [ema, ema + n) meets none of the other four
    for (const float* q : {(const float*)p, g, (const float*)m, (const float*)v})
      if ((uintptr_t)ema < (uintptr_t)(q + n) && (uintptr_t)q < (uintptr_t)(ema + n)) return MT_ERR_BAD_ARG;
  AdamGroupTab tab;
  for (int i = 0; i < MT_ADAM_MAX_GROUPS; ++i) {
    tab.lr_mult[i] = groups[i < ngroups ? i : 0].lr_mult;
    tab.wd[i] = groups[i < ngroups ? i : 0].weight_decay;
  }
  if (step_count < 1) step_count = 1;
  const float bc1 = (float)(1.0 - pow(beta1, (double)step_count));
  const float bc2s = (float)sqrt(1.0 - pow(beta2, (double)step_count));
  const float ema_w = ema ? ema_weight(ema_decay, ema_warmup, (double)step_count) : 0.f;
  long head = (long)((4 - (index_base & 3)) & 3);
  if (head > n) head = n;
  const long nvec = (n - head) / 4;
  // a workgroup's contiguous range: a whole number of workgroup-wide rows (no partly idle last row), at least two (the loop's two
  // vectors in flight), and as many more as the cap on the workgroups asks for; the grid covers nvec with ranges of that size
  long rows = (nvec + (long)ADAMG_THREADS * ADAMG_MAX_WGS - 1) / ((long)ADAMG_THREADS * ADAMG_MAX_WGS);
  if (rows < 2) rows = 2;
  const long per = rows * ADAMG_THREADS;
  const int grid = (int)(nvec > 0 ? (nvec + per - 1) / per : 1);
  hipLaunchKernelGGL(ema ? adamw_groups_kernel<true> : adamw_groups_kernel<false>, dim3(grid), dim3(ADAMG_THREADS), 0, (hipStream_t)stream,
                     p, g, m, v, n, index_base, (int)head, nvec, per, seg_end, seg_group, nseg, tab, (float)lr, (float)beta1, (float)beta2,
                     (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, bc1, bc2s, beta1, beta2, grad_mult, scale,
                     (const int*)found_inf, step_dev, lr_dev, ema, ema_w, ema_decay, ema_warmup);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_adamw_step_groups(float* p, const float* g, float* m, float* v, long n, long index_base, const int* seg_end,
                                    const unsigned char* seg_group, int nseg, const MtAdamGroup* groups, int ngroups, double lr,
                                    double beta1, double beta2, double eps, int step_count, const int* step_dev, float grad_mult,
                                    const float* scale, int* found_inf, const float* lr_dev, mt_stream_t stream) {
  return adamw_groups_launch(p, g, m, v, n, index_base, seg_end, seg_group, nseg, groups, ngroups, lr, beta1, beta2, eps, step_count,
                             step_dev, grad_mult, scale, found_inf, lr_dev, nullptr, 0.0, 0, stream);
}

extern "C" int mt_adamw_step_groups_ema(float* p, const float* g, float* m, float* v, long n, long index_base, const int* seg_end,
                                        const unsigned char* seg_group, int nseg, const MtAdamGroup* groups, int ngroups, double lr,
                                        double beta1, double beta2, double eps, int step_count, const int* step_dev, float grad_mult,
                                        const float* scale, int* found_inf, const float* lr_dev, float* ema, double ema_decay,
                                        int ema_warmup, mt_stream_t stream) {
  return adamw_groups_launch(p, g, m, v, n, index_base, seg_end, seg_group, nseg, groups, ngroups, lr, beta1, beta2, eps, step_count,
                             step_dev, grad_mult, scale, found_inf, lr_dev, ema, ema_decay, ema_warmup, stream);
}

extern "C" int mt_swap_f32(float* a, float* b, long n, mt_stream_t stream) {
  if (!a || !b || n <= 0) return MT_ERR_BAD_ARG;
  if (((uintptr_t)a & 3) || ((uintptr_t)b & 3)) return MT_ERR_BAD_ARG;
  if ((uintptr_t)a < (uintptr_t)(b + n) && (uintptr_t)b < (uintptr_t)(a + n)) return MT_ERR_BAD_ARG;      // (overlapping ranges)
  long head = 0, nvec = 0;
  if ((((uintptr_t)a ^ (uintptr_t)b) & 15) == 0) {      // alike in their 16-byte lines: the vector form
    head = (long)(((16 - ((uintptr_t)a & 15)) & 15) / 4);
    if (head > n) head = n;
    nvec = (n - head) / 4;
  }
  const long work = nvec > 0 ? (nvec + 1) / 2 : n;      // threads that have something to do
  const long wgs = (work + SWAP_THREADS - 1) / SWAP_THREADS;
  hipLaunchKernelGGL(swap_f32_kernel, dim3((int)(wgs > SWAP_MAX_WGS ? SWAP_MAX_WGS : wgs)), dim3(SWAP_THREADS), 0, (hipStream_t)stream,
                     (unsigned*)a, (unsigned*)b, n, (int)head, nvec);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_check_finite(const float* g, long n, int* found_inf, mt_stream_t stream) {
  if (!g || !found_inf || n <= 0) return MT_ERR_BAD_ARG;
  const int grid = (int)((n + 1023) / 1024 > 2048 ? 2048 : (n + 1023) / 1024);
  hipLaunchKernelGGL(check_finite_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n, found_inf);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

// stage-1 workgroups = slots of the workspace: a pure function of n
extern "C" long mt_grad_sumsq_partials_elems(long n) {
  if (n <= 0) return MT_ERR_BAD_ARG;
  const long wgs = (n + SUMSQ_WG_ELEMS - 1) / SUMSQ_WG_ELEMS;
  return wgs > SUMSQ_MAX_WGS ? SUMSQ_MAX_WGS : wgs;
}

extern "C" int mt_grad_sumsq(const float* g, long n, double* partials, long partials_elems, double* sumsq, int* found_inf,
                             mt_stream_t stream) {
  if (!g || !partials || !sumsq || n <= 0) return MT_ERR_BAD_ARG;
  if (((uintptr_t)g & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)sumsq & 7)) return MT_ERR_BAD_ARG;
  const int grid = (int)mt_grad_sumsq_partials_elems(n);
  if (partials_elems < grid) return MT_ERR_BAD_ARG;
  long head = (long)(((16 - ((uintptr_t)g & 15)) & 15) / 4);
  if (head > n) head = n;
  const long nvec = (n - head) / 4;
  hipLaunchKernelGGL(grad_sumsq_partials_kernel, dim3(grid), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, g, n, (int)head, nvec, partials);
  MT_CHECK_LAUNCH();
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, (const double*)partials, grid, sumsq,
                     found_inf);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

// stage-1 workgroups = slots of the workspace: a pure function of nwords
extern "C" long mt_checksum64_partials_elems(long nwords) {
  if (nwords <= 0) return MT_ERR_BAD_ARG;
  const long wgs = (nwords + SUMSQ_WG_ELEMS - 1) / SUMSQ_WG_ELEMS;
  return wgs > SUMSQ_MAX_WGS ? SUMSQ_MAX_WGS : wgs;
}

extern "C" int mt_checksum64(const void* data, long nwords, long index_base, unsigned long long* partials, long partials_elems,
                             unsigned long long* out, mt_stream_t stream) {
  if (!data || !partials || !out || nwords <= 0 || index_base < 0) return MT_ERR_BAD_ARG;
  if (((uintptr_t)data & 3) || ((uintptr_t)partials & 7) || ((uintptr_t)out & 7)) return MT_ERR_BAD_ARG;
  const int grid = (int)mt_checksum64_partials_elems(nwords);
  if (partials_elems < grid) return MT_ERR_BAD_ARG;
  long head = (long)(((16 - ((uintptr_t)data & 15)) & 15) / 4);
  if (head > nwords) head = nwords;
  const long nvec = (nwords - head) / 4;
  hipLaunchKernelGGL(checksum64_partials_kernel, dim3(grid), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, (const unsigned*)data, nwords,
                     (u64)index_base, (int)head, nvec, partials);
  MT_CHECK_LAUNCH();
  hipLaunchKernelGGL(checksum64_final_kernel, dim3(1), dim3(SUMSQ_THREADS), 0, (hipStream_t)stream, (const u64*)partials, grid, out);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_grad_clip_coef(const double* sumsq, int nsums, double grad_mult, const float* scale, double max_norm,
                                 const int* found_inf, float* out, mt_stream_t stream) {
  if (!sumsq || !out || nsums < 1 || !(max_norm >= 0.0) || !(grad_mult > 0.0)) return MT_ERR_BAD_ARG;
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq, nsums, grad_mult, scale, max_norm,
                     found_inf, out);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_absmax_scale(const float* x, long n, float target, float* s, mt_stream_t stream) {
  if (!x || !s || n <= 0 || !(target > 0.f)) return MT_ERR_BAD_ARG;
  hipLaunchKernelGGL(absmax_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, n, target, s);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_axpy_dev(const float* a, const float* b, const float* alpha, float* y, long n, mt_stream_t stream) {
  if (!b || !alpha || !y || n <= 0) return MT_ERR_BAD_ARG;
  const int grid = (int)((n + 1023) / 1024 > 4096 ? 4096 : (n + 1023) / 1024);
  hipLaunchKernelGGL(axpy_dev_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, alpha, y, n);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_mfma_probe(float* sink, int workgroups, int iters, mt_stream_t stream) {
  if (!sink || workgroups < 1 || iters < 1) return MT_ERR_BAD_ARG;
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(workgroups), dim3(256), 0, (hipStream_t)stream, sink, iters);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_coords_to_grid(const float* coords, int L, float tile, int ngrids, int* prow, int* pcol, int* err,
                                 mt_stream_t stream) {
  if (!coords || !prow || !pcol || L < 1 || !(tile > 0.f) || ngrids < 1) return MT_ERR_BAD_ARG;
  hipLaunchKernelGGL(coords_to_grid_kernel, dim3((L + 255) / 256), dim3(256), 0, (hipStream_t)stream, coords, L, tile, ngrids, prow,
                     pcol, err);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_scatter_rows_f32(const float* src, const int* src_idx, const int* idx, float* dst, int M, int D, int accumulate,
                                   mt_stream_t stream) {
  if (!src || !idx || !dst || M < 1 || D < 1) return MT_ERR_BAD_ARG;
  const long n = (long)M * D;
  const int grid = (int)((n + 255) / 256 > 8192 ? 8192 : (n + 255) / 256);
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, src_idx, idx, dst, M, D, accumulate);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_row_absmax_f32(const float* x, float* out, int M, int D, mt_stream_t stream) {
  if (!x || !out || M < 1 || D < 1) return MT_ERR_BAD_ARG;
  hipLaunchKernelGGL(row_absmax_kernel, dim3((M + 3) / 4 > 4096 ? 4096 : (M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, out, M, D);
  MT_CHECK_LAUNCH();
  return MT_OK;
}

extern "C" int mt_version(void) { return 360; }      // (3.0: MtLaunchOpts, 3.1: the _drop forms of mt_token_mha_*, 3.2: mt_patch_points_fwd / mt_patch_ig_accumulate, 3.3: mt_checksum64, 3.4: mt_adamw_step_groups, 3.5: mt_adamw_step_groups_ema / mt_swap_f32, 3.6: mt_layernorm_pool_fwd; the binary itself is identified by mt_build_id(), not by this number)

extern "C" const char* mt_status_string(int status) {
  switch (status) {
    case MT_OK: return "ok";
    case MT_ERR_BAD_ARG: return "bad argument (shape / alignment / null pointer)";
    case MT_ERR_LAUNCH: return "kernel launch failed";
    case MT_ERR_UNSUPPORTED: return "unsupported configuration";
    default: return "unknown status";
  }
}
