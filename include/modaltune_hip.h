/* modaltune_hip — C ABI of the MI355X-native Modal-Adapter hot path.
 *
 * The reference (martellab-sri/ModalTune) is pure Python/PyTorch and has no FFI layer; its drop-in
 * boundary is the nn.Module surface.  This header is the native boundary underneath
 * that surface: one `extern "C"` launcher per fused op and direction, plain device pointers and sizes,
 * no torch types.  Each entry cites the reference code whose arithmetic it replaces
 * (paths relative to the reference root; abbreviations as in SURVEY.md).
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless stated; the caller owns every buffer (no hidden hipMalloc)
 *   - `mt_half` = IEEE fp16 storage (the reference's AMP dtype, TM:216); accumulation is fp32 everywhere
 *   - activations are row-major [rows, cols]; token buffers are [B*N, C] with pass b at rows [b*N, (b+1)*N)
 *   - every launcher enqueues on `stream` (a hipStream_t) and returns immediately: 0 or a negative MtStatus
 *   - no exception crosses this boundary; nothing here synchronises the device
 */
#ifndef MODALTUNE_HIP_H
#define MODALTUNE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mt_stream_t;     /* hipStream_t */
typedef uint16_t mt_half;      /* IEEE binary16 bit pattern */

typedef enum {
  MT_OK = 0,
  MT_ERR_BAD_ARG = -1,         /* shape/alignment the kernels do not support */
  MT_ERR_LAUNCH = -2,          /* hipGetLastError() != hipSuccess after the launch */
  MT_ERR_UNSUPPORTED = -3
} MtStatus;

/* logical row m -> physical row (m / seg_rows) * seg_stride + row0 + m % seg_rows; seg_rows <= 0: identity.
 * Lets the adapter ops address "the patch rows of a [B, N, C] token buffer" without the torch.cat / slice
 * copies of AM:492,501-510, and broadcast one slide to the 3 task passes (seg_stride = 0). */
typedef struct { int seg_rows, seg_stride, row0; } MtRowMap;

/* The optional inputs of a launcher, passed as `const MtLaunchOpts* opt` directly in front of `stream`.  opt == NULL or a zeroed struct: the
 * default form.  Each launcher that takes one says which fields it honours; a set field it does not honour -- or a combination it does
 * not serve -- returns MT_ERR_UNSUPPORTED, it is never ignored.  The options are checked before anything else. */
typedef struct {
  float eps;             /* LayerNorm forward epsilon; 0 = the reference's 1e-5 (negative / NaN: MT_ERR_BAD_ARG) */
  const int* live;       /* one entry {b0, b1} of a DropPath live table (device; mt_droppath_live), or NULL: every pass */
  int live_rows;         /* rows per pass, for launchers without a plan (GEMM, LayerNorm); the dilated-attention
                            launchers take it from the plan and ignore it */
  float* partials;       /* deterministic form: the caller's partial workspace (sized by mt_<name>_det_elems), or NULL: default form */
  long partials_elems;
  int grid_wgs;          /* mix kernels, tests and tools only: number of workgroups, 0 = default */
} MtLaunchOpts;

/* major * 100 + minor * 10.  3.0: the optional inputs of a launcher travel in MtLaunchOpts; the suffixed twin entries (_eps, _det, _grid,
 * _live) of 2.x are gone, so a 2.x caller does not link against this library.  3.1: + mt_token_mha_fwd_drop / _bwd_drop.  3.2: + mt_patch_points_fwd / mt_patch_ig_accumulate.
 * 3.3: + mt_checksum64.  3.4: + mt_adamw_step_groups.  3.5: + mt_adamw_step_groups_ema, mt_swap_f32.  3.6: + mt_layernorm_pool_fwd. */
int mt_version(void);
const char* mt_status_string(int status);
/* Build provenance: sha256 (hex) over the kernel sources, this header and the compiler flags the library was built from
 * (modaltune_amd/_build_id.py: tree_build_id); `build()` rebuilds when it differs from the tree's. */
const char* mt_build_id(void);

/* ---------------------------------------------------------------- GEMMs ---------------------------- */
enum { MT_EPI_BIAS = 0,        /* C = acc + bias                                   (nn.Linear)            */
       MT_EPI_BIAS_RESID = 1,  /* C = resid + acc + bias                           (ENC:149-154,169-172)  */
       MT_EPI_INJECT = 2,      /* C = (1+g[n]) * resid + g[n] * (acc + bias)       (AM:231,362; A.1)      */
       MT_EPI_POSEMB = 3,      /* C = acc + bias + sincos(col|row)                 (LVA:232-237)          */
       MT_EPI_QKV_HM = 4 };    /* C = acc + bias, written head-major [N/48][M][48] (fp16): the q|k|v layout the
                                  dilated-attention kernels read (DA:169-175 "b l (h d) -> (b h) l d")          */
enum { MT_OUT_F16 = 0, MT_OUT_F32 = 1 };

/* Train-mode stochastic ops (nn.Dropout, timm DropPath: ENC:149-152,169-170, FFN:142, ENC:339, AM:319-327) as
 * counter-based masks: nothing is stored, the backward regenerates the mask of a site from (seed, step, site, element
 * index) with Philox4x32 (7 rounds).  rng: device uint32[4] = {seed_lo, seed_hi, step, reserved}; mt_rng_advance
 * increments `step` once per train step (inside the captured graph).  Element dropout: element (m, n) of a dense [M, D]
 * activation is kept when its random word >= p * 2^32 and scaled by 1/(1-p).  DropPath: one Bernoulli per (path_site,
 * pass), pass = m / rows_per_pass; a dropped pass is zeroed, a kept one scaled by 1/(1-path_p).  rng == NULL or both
 * probabilities 0: identity. */
typedef struct {
  const unsigned* rng;
  unsigned site;
  float p;
  unsigned path_site;
  float path_p;
  int rows_per_pass;
} MtDropout;
int mt_rng_advance(unsigned* rng, mt_stream_t stream);
/* y(m,:) = drop(x(xmap(m),:)) for a dense fp32 y [M, D] (Encoder.prepare_forward's input dropout, ENC:339: one mask
 * per task pass over the shared patch embedding) */
int mt_dropout_f32(const float* x, long ldx, const MtRowMap* xmap, float* y, int M, int D, const MtDropout* drop,
                   mt_stream_t stream);
/* in place on rows: x(m,:) *= DropPath factor of pass m / rows_per_pass (token-side residual branches) */
int mt_droppath_rows_f32(float* x, int M, int D, const MtDropout* drop, mt_stream_t stream);

/* DropPath live table.  A residual branch whose DropPath draw is 0 for a task pass contributes exact zeros for that pass, forward
 * and backward, so the kernels of the branch may leave the pass out.  mt_droppath_live evaluates the draw of every (site, pass) ON
 * THE DEVICE -- the host never sees it, a captured graph replays with whatever the rng holds -- and stores, per site i, table[2 i],
 * table[2 i + 1] = {b0, b1}: the contiguous hull of the live passes (first live pass, last live pass + 1; {0, 0} when none is live;
 * {0, B} for path_p = 0).  A hull is the exact live set for B <= 2; a dead pass inside it (B = 3, only the middle one dropped) is
 * computed as if live and discarded by the DropPath factor, as without a table.  path_sites / path_ps: HOST arrays of n <=
 * MT_LIVE_SITES_MAX entries (MtDropout.path_site / .path_p of the branches); rng as in MtDropout; table: device int[2 n].  Launch it
 * after the step's mt_rng_advance and before the first consumer; forward and backward read the same table.
 * The launchers that honour MtLaunchOpts.live take one site's {b0, b1} (device): work of the passes outside [b0, b1) is not
 * done and its outputs keep whatever bytes they held -- the consumers of a branch select a dropped pass to 0 and never multiply it
 * (mt_add_layernorm_fwd, the BIAS_RESID epilogue), and mt_layernorm_bwd with a table counts its dy as zero.  live == NULL: every pass
 * is live.  Correctness never depends on a pass having been left out. */
#define MT_LIVE_SITES_MAX 64
int mt_droppath_live(const unsigned* path_sites, const float* path_ps, int n, int B, const unsigned* rng, int* table,
                     mt_stream_t stream);

typedef struct {
  const float* bias;           /* [N] or NULL */
  const float* resid;          /* fp32 [*, ldr] (BIAS_RESID, INJECT) */
  long ldr;
  MtRowMap rmap;
  const float* colscale;       /* gamma [N] (INJECT) */
  const float* pos_table;      /* [ngrids, N/2] 1-D sin-cos table (POSEMB), pos_embed.py:62-81 */
  const int* pos_row;          /* [M] grid row index  floor(coords[:,0]/256), SE:209-211 */
  const int* pos_col;          /* [M] grid col index */
  MtDropout drop;              /* BIAS_RESID: C = resid + drop(acc + bias)  (ENC:149-154: dropout, DropPath, + residual) */
} MtGemmEpilogue;

/* C[M,N] = epilogue(A[M,K] @ W[N,K]^T); A, W fp16; fp32 accumulate on MFMA.  K % 64 == 0, lda % 8 == 0.
 * Replaces every big-M nn.Linear on the path: PatchEmbed.proj (SE:52-56), q/k/v/out_proj (DA:169-171,260),
 * fc1/fc2 (FFN:134,140), adapter q_proj/output_proj/k|v projections (AM:154-164,221-231), and — with a
 * pre-transposed weight — the activation-gradient (dX) GEMMs of the frozen backbone. */
/* opt: live.  With a table the product runs over the rows of the live passes only (live_rows rows per pass): M_eff = (b1 - b0) * live_rows
 * rows starting at row b0 * live_rows are computed, in row tiles laid from that row on, and stored; every other row of C keeps its bytes.
 * A row's result does not depend on where the tiles lie, and whatever in an epilogue depends on the row (the head-major row of
 * MT_EPI_QKV_HM, row maps) takes the global row: kept rows keep their bits.  For MT_EPI_BIAS and MT_EPI_QKV_HM (the products inside a
 * residual branch); the epilogues that carry the residual stream (BIAS_RESID, INJECT, POSEMB) run over every row: MT_ERR_UNSUPPORTED
 * with a table. */
int mt_gemm_nt_f16(const mt_half* A, long lda, const MtRowMap* amap, const mt_half* W, int M, int N, int K,
                   int epilogue, const MtGemmEpilogue* epi, void* C, long ldc, const MtRowMap* cmap, int out_dtype,
                   const MtLaunchOpts* opt, mt_stream_t stream);

/* C[N1,N2] (fp32) += sum_m A[m,N1] * B[m,N2] over M rows (split over workgroups, fp32 atomics): the weight
 * gradient of a big-M nn.Linear (autograd of AM:154-164 etc.).  N1 % 64 == 0, N2 % 64 == 0.
 * colsum (fp32 [N1], or NULL): colsum[n] += sum_m A[m,n] on the same pass -- the bias gradient of that nn.Linear.
 * opt: partials (the deterministic forms at the end of this header; ldc >= N2 then). */
int mt_gemm_tn_f16(const mt_half* A, long lda, const MtRowMap* amap, const mt_half* B, long ldb, const MtRowMap* bmap,
                   int M, int N1, int N2, float* C, long ldc, float* colsum, const MtLaunchOpts* opt, mt_stream_t stream);

/* out[n] (fp32) += sum_m A[m,n]: bias gradient of a big-M nn.Linear.  N % 8 == 0, lda % 8 == 0 (16-byte loads).  opt: partials. */
int mt_colsum_f16(const mt_half* A, long lda, const MtRowMap* amap, int M, int N, float* out, const MtLaunchOpts* opt,
                  mt_stream_t stream);

/* Generic small strided fp32 GEMM for the token-side ops (T <= 66 rows; gene encoder GE:194-223, prompt
 * self-attention projections AM:81-94, extractor FFN AM:284-287, fusion head LVA:343-347), forward and
 * backward:  C(m,n) = act(sum_k A(m,k) B(n,k) + bias[n]) [+ C(m,n) if accumulate].
 * Element (i,j) of X is X[i*xs0 + j*xs1].  batch: pointer offsets a_bs/b_bs/c_bs per batch index.
 * rowsum (fp32 [M], or NULL; batch must be 1): rowsum[m] += sum_k A(m,k) -- the bias gradient riding on the
 * dW = dy^T x product of an nn.Linear backward. */
enum { MT_ACT_NONE = 0, MT_ACT_RELU = 1, MT_ACT_GELU = 2, MT_ACT_ELU = 3 };
int mt_sgemm_small(const float* A, long as0, long as1, long a_bs, const float* B, long bs0, long bs1, long b_bs,
                   const float* bias, int bias_on_m, float* C, long cs0, long cs1, long c_bs, int M, int N, int K,
                   int batch, int act, int accumulate, float* rowsum, mt_stream_t stream);

/* Up to MT_SGEMM_MAX independent small products in ONE launch, each with the nn.Linear forward / backward fused around it
 * (the token side is a chain of ~5 us launches; what it costs is their number):
 *   forward   C = resid + drop_c(act(A B^T + bias)) [+ C];  pre_out (or NULL) receives A B^T + bias, the value the
 *             backward differentiates -- nn.Linear + activation + nn.Dropout + residual add of GE:184-192, AM:284-287;
 *   backward  A'(m,k) = drop_a(A(m,k)) * act'(a_aux(m,k)) is formed as the dy operand is loaded (a_aux = the saved
 *             pre_out, a_drop = the forward's c_drop): dX = A' W and dW = A'^T x (+ rowsum = db) of one nn.Linear share a launch.
 * pre_out / resid are addressed like C, a_aux like A.  The masks are element dropout of a DENSE tensor: the mask index
 * is the element offset from C / from A.  DropPath of the branch (path_p > 0: one Bernoulli per task pass of rows_per_pass
 * rows, AM:319,327) rides on the same specs: in c_drop the pass is (row m of C) / rows_per_pass; in a_drop it is
 * (element offset in A / a_ld) / rows_per_pass with a_ld = the row length of the dense dy tensor (required then).
 * resid_scale: the residual enters as resid_scale * resid (0 is read as 1; `query + (tgt + f(.))` with tgt == query is
 * 2 * query + f(.), AM:231,324).  Products of one launch must not write what another reads or writes.  mt_sgemm_small is the
 * one-product, no-fusion form of this entry. */
#define MT_SGEMM_MAX 3
typedef struct {
  const float* A; long as0, as1, a_bs;
  const float* B; long bs0, bs1, b_bs;
  const float* bias; int bias_on_m;
  float* C; long cs0, cs1, c_bs;
  int M, N, K, batch, act, accumulate;
  float* rowsum;
  float* pre_out;
  const float* resid;
  MtDropout c_drop;
  const float* a_aux; int a_act;
  MtDropout a_drop;
  float resid_scale; int a_ld;
} MtSgemm;
int mt_sgemm_multi(const MtSgemm* probs, int n, mt_stream_t stream);

/* ------------------------------------------------------------- LayerNorm --------------------------- */
/* y = LN(f(x)) * w + b over the last dim D, one wave per row; stats (mean, rstd) saved per row.
 * f = identity or erf-GELU computed in fp32 (FFN:136 forces the activation to fp32, then FFN:138 ffn_layernorm).
 * in_dtype/out_dtype: MT_OUT_F16 / MT_OUT_F32.  D in {256, 768, 2304, 3072}.  `add_rows` (fp32 [add_period, D],
 * or NULL) is added AFTER the affine: LN(c) + pe as in AM:218,227 (with_pos_embed on normed memory).
 * opt: eps, live.  eps: the default is the reference's 1e-5 (ENC / AM / GE LayerNorms); the TITAN ViT's LayerNorms carry their own, e.g.
 * timm's 1e-6 (the backward needs none: it reads the saved rstd).  live (live_rows rows per pass): only the rows of the live passes, for
 * the fp16 GELU form (D = 3072: the FFN's sub-LayerNorm, a LayerNorm INSIDE a branch); every other form with a table:
 * MT_ERR_UNSUPPORTED.  Rows are read and written with 8- and 16-byte vector accesses: ldx % 4 == 0 and ldy % 4 == 0, else MT_ERR_BAD_ARG. */
int mt_layernorm_fwd(const void* x, long ldx, const MtRowMap* xmap, int in_dtype, int gelu_in, const float* w,
                     const float* b, const float* add_rows, int add_period, void* y, long ldy, const MtRowMap* ymap,
                     int out_dtype, float* stats, int M, int D, const MtLaunchOpts* opt, mt_stream_t stream);
/* h = x + drop(branch) ; y = fp16(LN(h) * w + b): the residual add of a backbone sub-layer (ENC:95-97,121-123 --
 * x = residual stream fp32 [M, D], branch = fp16 output of the out_proj / fc2 GEMM, drop = that branch's Dropout +
 * DropPath, same counters as the BIAS_RESID GEMM epilogue) riding on the LayerNorm that consumes the sum.
 * h (fp32, != x) receives the new residual stream, stats the (mean, rstd) rows.  D = 768.  opt: eps. */
int mt_add_layernorm_fwd(const float* x, const mt_half* branch, const MtDropout* drop, const float* w, const float* b,
                         float* h, mt_half* y, float* stats, int M, int D, const MtLaunchOpts* opt, mt_stream_t stream);

/* Pooled read-out of the plain slide encoder, LayerNorm on either side of a row mean:
 *   out[b, :] = LN_post( 1 / (r1 - r0) * sum_{r in [r0, r1)} LN_pre( x[b, r, :] ) )
 * x fp32 [B][rows_per_pass][D] with row stride ldx >= D (ldx % 4 == 0, 16-byte aligned), [r0, r1) a row range inside every pass, out
 * fp32 [B, D].  LN_pre (pre_w, pre_b: both or neither; pre_eps) and LN_post (post_w, post_b: both or neither; post_eps) are each
 * optional; an eps of 0 is the reference's 1e-5, a negative or NaN one MT_ERR_BAD_ARG.  The two epsilons are plain arguments -- one
 * MtLaunchOpts.eps could not carry both, and nothing else of MtLaunchOpts applies -- so this entry takes no options pointer.
 * D = 768 (else MT_ERR_UNSUPPORTED).  The four read-outs of LongNetViT.forward
 * (gigapath/slide_encoder.py:277-285) over Encoder.layer_forward's two results are this one launch:
 *   encoder_out (torchscale/architecture/encoder.py:425-426, SE:279-285)  cls:  rows [0, 1), pre = encoder.layer_norm, post = norm
 *                                                                          pool: rows [1, N), pre = encoder.layer_norm, post = norm
 *   encoder_states (ENC:400-422; all_layer_embed, no encoder.layer_norm)   cls:  rows [0, 1), post = norm;  pool: rows [1, N), post = norm
 * `norm` carries eps 1e-6 (SE:368-377), encoder.layer_norm the encoder's 1e-5.
 * The selected rows are read once and nothing outside [r0, r1) is read.  Precision: the row statistics are those of mt_layernorm_fwd
 * (fp32 mean, centred second moment, one wave per row); each normalised row is added to DOUBLE column sums, waves and workgroups are
 * added in double too, and the mean is rounded to fp32 once -- so against fp64 the pooled vector carries the error of one fp32
 * LayerNorm row (averaged, not accumulated, over the rows) and LN_post adds that of one more fp32 LayerNorm.  The summation order is a
 * function of (r1 - r0, D) alone and no floating-point atomic executes: the same input gives the same bits.
 * Workspace: ranges of more than 64 rows are split over workgroups (64 rows each); every workgroup stores its column sums to its own
 * slot of `partials` (device doubles, 8-byte aligned, at least mt_layernorm_pool_partials_elems(B, r1 - r0, D) of them, no
 * initialisation needed) and one workgroup per pass adds the slots in ascending order.  A short workspace: MT_ERR_BAD_ARG before any
 * launch; partials may be NULL where the query returns 0. */
int mt_layernorm_pool_fwd(const float* x, long ldx, int B, int rows_per_pass, int r0, int r1, const float* pre_w, const float* pre_b,
                          float pre_eps, const float* post_w, const float* post_b, float post_eps, float* out, double* partials,
                          long partials_elems, int D, mt_stream_t stream);
/* host arithmetic: the doubles mt_layernorm_pool_fwd needs for B passes of `rows` = r1 - r0 rows (0: one workgroup per pass, no
 * workspace); negative MtStatus for B < 1, rows < 1 or a width it does not serve */
long mt_layernorm_pool_partials_elems(int B, int rows, int D);

/* dx (+)= LN backward.  dy fp16 or fp32 [M,D]; x as in forward (gelu_in: also backprop through the GELU).
 * dx_dtype F32 with accumulate=1 adds into the fp32 residual-gradient stream (ENC:137-154 backward);
 * dw/db (fp32 [D], atomically accumulated) may be NULL for frozen norms (selective backward).
 * dx_f16 (dense fp16 [M,D], or NULL): a second, half-precision copy of the final dx -- the operand of the next dX GEMM
 * of the frozen layer below, written here instead of by a separate cast pass over the fp32 stream; dx_f16_drop (or
 * NULL): the dropout / DropPath mask of the residual branch that GEMM differentiates, applied to the copy only.
 * opt: live, partials (not both: MT_ERR_UNSUPPORTED).  live = the table entry of the residual branch this LayerNorm closes (live_rows
 * rows per pass): dy of a row outside the live passes counts as ZERO whatever its bytes are -- then an accumulating dx passes through
 * unchanged and dx_f16 is still written, which is what exact-zero dy rows give.  The fp16 GELU form (the FFN's sub-LayerNorm) instead
 * walks the live rows only and leaves the other rows of dx untouched; the other GELU forms and a trainable norm (dw / db) take no
 * table: MT_ERR_UNSUPPORTED.  partials: the deterministic form (end of this header), dw and db required.
 * lddy, ldx and lddx are multiples of 4 elements as in the forward (vector accesses per row), else MT_ERR_BAD_ARG. */
int mt_layernorm_bwd(const void* dy, long lddy, const MtRowMap* dymap, int dy_dtype, const void* x, long ldx,
                     const MtRowMap* xmap, int in_dtype, int gelu_in, const float* w, const float* stats, void* dx,
                     long lddx, const MtRowMap* dxmap, int dx_dtype, int accumulate, float* dw, float* db,
                     mt_half* dx_f16, const MtDropout* dx_f16_drop, int M, int D, const MtLaunchOpts* opt, mt_stream_t stream);

/* ------------------------------------------------------- dilated attention ------------------------- */
#define MT_MAX_BRANCHES 8
#define MT_QK_SCALE_LOG2 0.20823509396846288f     /* 48^-1/2 * log2(e) */
typedef struct {
  int nbranch;
  int N;                              /* tokens per pass (L + 1) */
  int B;                              /* task passes batched */
  int seg[MT_MAX_BRANCHES];           /* s = min(segment_length, N)                  DA:96-98   */
  int ratio[MT_MAX_BRANCHES];         /* dilation r                                  DA:213     */
  int nseg[MT_MAX_BRANCHES];          /* ceil(N / s)                                            */
  int n[MT_MAX_BRANCHES];             /* sparse length ceil(s / r) incl. zero padding DA:22-37  */
  int qlimit[MT_MAX_BRANCHES];        /* 0, or: only the first qlimit sparse entries of every (segment, head) act as QUERIES
                                       * (all n act as keys) -- the sequence-parallel form of DA:61-111, where a rank's
                                       * queries attend over the keys gathered from the ranks of its segment            */
} MtDilatedPlan;

/* qkv: fp16 HEAD-MAJOR [3][16][B*N][48] (q' | k | v; MT_EPI_QKV_HM writes it).  The q slab holds
 * q' = MT_QK_SCALE_LOG2 * q with MT_QK_SCALE_LOG2 = 48^-1/2 * log2(e): the caller bakes the softmax scale (MHA:109-119
 * scaling = head_dim^-0.5; in log2 units because the kernels exponentiate with v_exp_f32 = 2^x) into the q rows of the
 * frozen q_proj weight and bias before rounding them to fp16, so no kernel multiplies by it and q is rounded once.
 * For every branch, every (segment, head): O_b = softmax(Q K^T / sqrt(48)) V over the head's dilated positions, zero-padded rows acting as keys with
 * logit 0 / value 0 (DA:98-101,24-28).  o_br: fp16 [nbranch][B*N, 768]; lse_br: fp32 [nbranch][B*N, 16]
 * (natural log).  (position, head) pairs a branch does not visit are left untouched.  DA:212-253, MHA:109-119.
 * opt: live -- workgroups of the passes outside [live[0], live[1]) exit before they touch anything. */
int mt_dilated_attn_fwd(const mt_half* qkv, const MtDilatedPlan* plan, mt_half* o_br, float* lse_br, const MtLaunchOpts* opt,
                        mt_stream_t stream);

/* Branch mix + inner_attn_ln: w_b = softmax_b(lse_b) per (position, head) (constant in backward, DA:132-137),
 * mixed = sum_b w_b O_b, y = LN(mixed) (DA:257-258).  Writes y fp16 [B*N,768], LN stats, and
 * lse_tot = logsumexp_b(lse_b) fp32 [B*N,16] for the backward.
 * opt (both mix launchers): live -- the rows of the live passes only; grid_wgs (tests and tools only; the results do not depend on it)
 * > 0 = that many workgroups, capped at what the rows need. */
int mt_dilated_mix_ln_fwd(const mt_half* o_br, const float* lse_br, const MtDilatedPlan* plan, const float* ln_w,
                          const float* ln_b, mt_half* y, float* stats, float* lse_tot, const MtLaunchOpts* opt, mt_stream_t stream);

/* Backward of mix + inner_attn_ln: given dy (fp16, gradient wrt the LN output) recomputes mixed, writes
 * dmixed fp16 HEAD-MAJOR [16][B*N][48] and delta_br[b][row][head] = sum_d dmixed * O_b (fp32). */
int mt_dilated_mix_ln_bwd(const mt_half* dy, const mt_half* o_br, const float* lse_br, const float* lse_tot,
                          const MtDilatedPlan* plan, const float* ln_w, const float* stats, mt_half* dmixed,
                          float* delta_br, const MtLaunchOpts* opt, mt_stream_t stream);

/* Flash-style backward of all branches: dqkv fp16 [B*N, 2304] (overwritten) from qkv, dmixed, lse_tot, delta_br.  The q
 * columns of dqkv are the gradient with respect to the PRE-SCALED q' (what the dX GEMM through the scaled q_proj cache needs).
 * P~ = exp(s - lse_tot) (= w_b P_b), dS = P~ (dmixed V^T - delta_b), dQ = dS K, dK = dS^T Q, dV = P~^T dmixed.
 * Two launches cover all branches (a dK/dV kernel with key = lane, a dQ kernel with query = lane); each writes its
 * per-branch result once into `workspace` (fp16, mt_dilated_attn_bwd_workspace_bytes) and a combine kernel sums the
 * branches that visit a (position, head) into the dense fp16 gradient: no atomics, bitwise reproducible. */
long mt_dilated_attn_bwd_workspace_bytes(const MtDilatedPlan* plan);
enum { MT_ATTN_BWD_KV = 1, MT_ATTN_BWD_Q = 2, MT_ATTN_BWD_COMBINE = 4, MT_ATTN_BWD_ALL = 7 };   /* `phases` mask */
int mt_dilated_attn_bwd(const mt_half* qkv, const mt_half* dmixed, const float* lse_tot, const float* delta_br,
                        const MtDilatedPlan* plan, void* workspace, mt_half* dqkv, int phases, mt_stream_t stream);
/* The same backward with the dense (ratio 1) branch written IN PLACE: the two kernels store that branch straight into dqkv (its
 * workspace slot and the dqkv row have the same address arithmetic; its workspace region is left untouched) and the combine
 * adds the sparse branches only where they cover a (position, head), in the same order and precision as the form above, so
 * equal inputs give equal dqkv.  KV and Q phases must both have run on dqkv before COMBINE, and COMBINE runs once.  The
 * workspace keeps its size.  What mt_longnet_layer_bwd uses; a plan without a ratio-1 branch takes the workspace form.
 * opt: live -- the live passes only (all three phases; a plan without a ratio-1 branch runs the workspace-form combine over every row:
 * the dqkv rows of a dropped pass then hold undefined values, which no consumer reads). */
int mt_dilated_attn_bwd_inplace(const mt_half* qkv, const mt_half* dmixed, const float* lse_tot, const float* delta_br,
                                const MtDilatedPlan* plan, void* workspace, mt_half* dqkv, int phases, const MtLaunchOpts* opt,
                                mt_stream_t stream);

/* ------------------------------------------------- dense attention with 2-D ALiBi (TITAN blocks) ---- */
/* The attention of the TITAN slide encoder's ViT blocks (titan_adapter.py:253-293 `get_alibi`, :359-361,394
 * `blocks.modules_list[i](x, attn_bias, bg_mask)`; adapter_modules.py:526-558): H heads of 64 over one sequence of N tokens
 * per pass (cls + the slide's foreground cells), softmax(q k^T / 8 + bias) v with bias[h, i, j] = -slope_h * euclidean distance
 * of the tokens' grid cells (0 to and from cls).  The distance is head-independent: ONE fp16 [N, N] table per slide
 * (mt_alibi_dist), stored in the order the kernels' accumulator registers consume it, replaces the reference's [H, N, N] fp32
 * bias; the kernels read it straight into registers and apply the slope with one fused multiply-add per score.
 * qkv: fp16 TOKEN-MAJOR [B*N, 3*H*64] (q' | k | v) as the qkv GEMM writes it, q' = MT_DENSE_QK_SCALE_LOG2 * q (the caller
 * bakes 64^-1/2 log2(e) into the q rows of the frozen qkv weight / bias).  o: fp16 [B*N, H*64]; lse: fp32 [B*N, H] (natural
 * log, bias included). */
#define MT_DENSE_QK_SCALE_LOG2 0.18033688011112042f     /* 64^-1/2 * log2(e) */
typedef struct {
  int N;                 /* tokens per pass */
  int B;                 /* task passes batched */
  int H;                 /* heads (head dim 64) */
  const mt_half* dist;   /* distance table of mt_alibi_dist (mt_alibi_dist_halves(N) halves), or NULL: no bias */
  const float* nslope;   /* [H]: -slope_h * log2(e) (with dist) */
} MtDensePlan;
/* table[...] = euclidean distance between the grid cells of tokens i and j (token 0 = cls: zero row and column), from
 * cells[i - 1] = (row, col) of token i's cell, rounded to fp16 (relative 2^-12: a bias error below 2.5e-4 of the bias), in
 * blocks of 32 x 64 tokens laid out as four 16-byte pieces per lane of a wave (csrc/dense_attn.hip: DistRegs).  Symmetric, so
 * one table serves the query-in-lane and the key-in-lane kernels.  mt_alibi_dist_halves(N) = its size in fp16 elements
 * (N^2 rounded up to whole blocks: 34 MB at N = 4097). */
long mt_alibi_dist_halves(int N);
int mt_alibi_dist(const int* cells, int N, mt_half* table, mt_stream_t stream);
int mt_dense_attn_fwd(const mt_half* qkv, const MtDensePlan* plan, mt_half* o, float* lse, mt_stream_t stream);
/* dqkv fp16 [B*N, 3*H*64] (overwritten; q columns = gradient of the pre-scaled q') from qkv, o, dO (fp16 [B*N, H*64]) and lse.
 * delta: fp32 [B*N, H] workspace (sum_d dO * O, written by the DELTA phase).  The bias carries no gradient.  Every output
 * element is written exactly once: no atomics, no combine pass. */
enum { MT_DENSE_BWD_DELTA = 1, MT_DENSE_BWD_KV = 2, MT_DENSE_BWD_Q = 4, MT_DENSE_BWD_ALL = 7 };
int mt_dense_attn_bwd(const mt_half* qkv, const mt_half* o, const mt_half* d_o, const float* lse, const MtDensePlan* plan,
                      float* delta, mt_half* dqkv, int phases, mt_stream_t stream);

/* y = gelu(x) (erf form, nn.GELU) / dx = dy * gelu'(x) on fp16 vectors, n % 8 == 0: the ViT block's MLP activation */
int mt_gelu_f16_fwd(const mt_half* x, mt_half* y, long n, mt_stream_t stream);
int mt_gelu_f16_bwd(const mt_half* x, const mt_half* dy, mt_half* dx, long n, mt_stream_t stream);

/* Attentional pooling core (TA:401-402 `forward_attn_pool`): nq learned queries attend over the N tokens of every pass, keys
 * split over workgroups (flash-decoding form).  q fp32 [nq, E] (projected; frozen, so no dq); kv fp16 [B*N, 2E] (k | v
 * projected); out fp32 [B, nq, E]; scores fp32 [B, heads, nq, N] (raw scaled logits, saved) and lse fp32 [B, heads, nq]: the
 * backward recomputes p = exp(score - lse); workspace: mt_pool_attn_workspace_floats() floats.
 * backward: dkv fp16 [B*N, 2E] (overwritten) from scores, lse, out and dout (fp32 [B, nq, E]). */
long mt_pool_attn_workspace_floats(int B, int N, int heads, int nq);
int mt_pool_attn_fwd(const float* q, const mt_half* kv, int B, int N, int E, int heads, int nq, float* out, float* scores,
                     float* lse, float* workspace, mt_stream_t stream);
int mt_pool_attn_bwd(const float* q, const mt_half* kv, const float* scores, const float* lse, const float* out,
                     const float* dout, int B, int N, int E, int heads, int nq, mt_half* dkv, mt_stream_t stream);

/* ------------------------------------------------- composite launchers: one backbone layer per call ---- */
/* The launch list of ONE frozen backbone layer behind one entry point per direction (mt_lnqkv_fwd, mt_dilated_attn_*,
 * mt_mix_ln_outproj_*, mt_ffn_* as one sequence): the host makes 2 calls per layer and step instead of ~20.
 * `steps`: bit i selects the i-th launch of the entry's list (the enums below, in launch order); MT_LAYER_ALL enqueues the whole
 * list.  A tool that wants HIP events around every kernel issues the bits one call at a time: the buffers then hold the same bits
 * as after one MT_LAYER_ALL call.  A step whose condition does not hold (the cast when dh16_valid is set) is skipped whether
 * selected or not; which variant a step takes (pend_x, defer, dh16_valid, feeds_lower) never depends on `steps`.
 * LongNet EncoderLayer (ENC:121-175; DA:146-262; FFN:132-143), D = 768, F = ffn width.  Weights: fp32 LayerNorm affines and
 * biases, fp16 [N, K] weight caches (q rows of w_qkv / b_qkv pre-scaled by MT_QK_SCALE_LOG2) and their transposes for the dX GEMMs.
 * Buffers: saved per layer (hin, hmid fp32 [M, D]; qkv fp16 head-major; o_br fp16 [nbranch, M, D]; lse_br fp32 [nbranch, M, 16];
 * lse_tot fp32 [M, 16]; a1 fp16 [M, F]; st1 / stin / st2 / stf fp32 [M, 2]) and transients shared by all layers.
 * forward: pend_x / pend_branch / pend_drop: the residual stream, fp16 fc2 branch and its dropout of the layer BELOW whose add is
 * still outstanding (hin is then written here) or NULL; defer != 0: leave this layer's fc2 add to the layer above (br16 holds the
 * branch, `out` is not written).  backward: dh (fp32 [M, D]) in / out; dh16_valid: the layer above left fp16(dh) in dh16;
 * feeds_lower: leave fp16(dh) (masked with drop_lower_ffn) for the layer below.
 * live_attn / live_ffn (one pass = plan->N rows): the kernels inside a branch -- its GEMMs, attention, mix, combine,
 * the FFN's sub-LayerNorm -- leave the dropped passes of the branch out, forward and backward; the kernels that carry the residual
 * stream (the add + LayerNorm forward, the LayerNorm backward, the cast, the BIAS_RESID product) run over all rows. */
typedef struct {
  const float *ln1_w, *ln1_b, *inner_ln_w, *inner_ln_b, *ln2_w, *ln2_b, *ffn_ln_w, *ffn_ln_b;
  const float *b_qkv, *b_out, *b_fc1, *b_fc2;
  const mt_half *w_qkv, *w_out, *w_fc1, *w_fc2;
  const mt_half *wt_qkv, *wt_out, *wt_fc1, *wt_fc2;
} MtLongNetLayerWeights;
typedef struct {
  float *hin, *hmid; mt_half *qkv, *o_br; float *lse_br, *lse_tot; mt_half* a1; float *st1, *stin, *st2, *stf;
  mt_half *u16, *br16, *t16;
  float* dh; mt_half *dy16, *dh16, *dt16, *da1, *dmixed, *dqkv16; float* delta; void* attn_ws;
  const int *live_attn, *live_ffn;   /* live table entries (mt_droppath_live) of the layer's attention / FFN branch, or NULL: all passes */
} MtLongNetLayerBuffers;
enum { MT_LAYER_ALL = 0x7fffffff };
/* forward, in launch order: self_attn_layer_norm (mt_layernorm_fwd; with pend_x: mt_add_layernorm_fwd, which also writes hin) ->
 * QKV GEMM (head-major) -> mt_dilated_attn_fwd -> mt_dilated_mix_ln_fwd -> out_proj GEMM -> final_layer_norm
 * (mt_add_layernorm_fwd: hmid = hin + drop(branch)) -> fc1 GEMM -> ffn_layernorm of gelu(a1) -> fc2 GEMM (+ hmid into `out`;
 * with defer: the plain branch into br16). */
enum { MT_LNF_LN1 = 1 << 0, MT_LNF_QKV = 1 << 1, MT_LNF_ATTN = 1 << 2, MT_LNF_MIX = 1 << 3, MT_LNF_OUT = 1 << 4, MT_LNF_LN2 = 1 << 5,
       MT_LNF_FC1 = 1 << 6, MT_LNF_FFN_LN = 1 << 7, MT_LNF_FC2 = 1 << 8 };
int mt_longnet_layer_fwd(const MtLongNetLayerWeights* w, const MtLongNetLayerBuffers* b, const MtDilatedPlan* plan, int M, int D, int F,
                         const float* pend_x, const mt_half* pend_branch, const MtDropout* pend_drop, int defer, float* out,
                         const MtDropout* drop_attn, const MtDropout* drop_ffn, int steps, mt_stream_t stream);
/* backward, in launch order: fp16(drop(dh)) (only without dh16_valid) -> fc2 dX GEMM -> ffn_layernorm backward -> fc1 dX GEMM ->
 * final_layer_norm backward (dh +=, fp16 copy in dh16) -> out_proj dX GEMM -> mt_dilated_mix_ln_bwd -> mt_dilated_attn_bwd (its
 * three `phases` are the bits MT_ATTN_BWD_* << MT_LNB_ATTN_SHIFT: one call with the selected ones) -> QKV dX GEMM ->
 * self_attn_layer_norm backward (dh +=; with feeds_lower also dh16). */
enum { MT_LNB_CAST = 1 << 0, MT_LNB_FC2 = 1 << 1, MT_LNB_FFN_LN = 1 << 2, MT_LNB_FC1 = 1 << 3, MT_LNB_LN2 = 1 << 4, MT_LNB_OUT = 1 << 5,
       MT_LNB_MIX = 1 << 6, MT_LNB_ATTN_SHIFT = 7, MT_LNB_QKV = 1 << 10, MT_LNB_LN1 = 1 << 11 };
int mt_longnet_layer_bwd(const MtLongNetLayerWeights* w, const MtLongNetLayerBuffers* b, const MtDilatedPlan* plan, int M, int D, int F,
                         int dh16_valid, int feeds_lower, const MtDropout* drop_attn, const MtDropout* drop_ffn,
                         const MtDropout* drop_lower_ffn, int steps, mt_stream_t stream);
/* Dense pre-norm ViT block of the TITAN configuration (TA:359-361: x + proj(attn(LN(x))), then + fc2(gelu(fc1(LN(.)))); layer scale
 * folded into w_proj / w_fc2 by the caller): qkv fp16 TOKEN-major [M, 3D], o16 fp16 [M, D], lse fp32 [M, H], a1 fp16 [M, F]. */
typedef struct {
  const float *n1_w, *n1_b, *n2_w, *n2_b; float n1_eps, n2_eps;
  const float *b_qkv, *b_proj, *b_fc1, *b_fc2;
  const mt_half *w_qkv, *w_proj, *w_fc1, *w_fc2;
  const mt_half *wt_qkv, *wt_proj, *wt_fc1, *wt_fc2;
} MtVitBlockWeights;
typedef struct {
  float *hin, *hmid; mt_half *qkv, *o16; float* lse; mt_half* a1; float *st1, *st2;
  mt_half *u16, *br16, *t16;
  float* dh; mt_half *dy16, *dh16, *dt16, *da1, *dqkv16; float* delta;
} MtVitBlockBuffers;
/* forward, in launch order: norm1 (mt_layernorm_fwd with n1_eps; with pend_x: mt_add_layernorm_fwd, which also writes hin) -> QKV GEMM ->
 * mt_dense_attn_fwd -> proj GEMM -> norm2 (mt_add_layernorm_fwd with n2_eps: hmid = hin + branch) -> fc1 GEMM -> mt_gelu_f16_fwd ->
 * fc2 GEMM (+ hmid into `out`; with defer: the plain branch into br16). */
enum { MT_VBF_LN1 = 1 << 0, MT_VBF_QKV = 1 << 1, MT_VBF_ATTN = 1 << 2, MT_VBF_PROJ = 1 << 3, MT_VBF_LN2 = 1 << 4, MT_VBF_FC1 = 1 << 5,
       MT_VBF_GELU = 1 << 6, MT_VBF_FC2 = 1 << 7 };
int mt_vit_block_fwd(const MtVitBlockWeights* w, const MtVitBlockBuffers* b, const MtDensePlan* plan, int M, int D, int F,
                     const float* pend_x, const mt_half* pend_branch, int defer, float* out, int steps, mt_stream_t stream);
/* backward, in launch order: fp16(dh) (only without dh16_valid) -> fc2 dX GEMM -> mt_gelu_f16_bwd -> fc1 dX GEMM -> norm2 backward
 * (dh +=, fp16 copy in dh16) -> proj dX GEMM -> mt_dense_attn_bwd (its three `phases` are the bits MT_DENSE_BWD_* <<
 * MT_VBB_ATTN_SHIFT: one call with the selected ones) -> QKV dX GEMM -> norm1 backward (dh +=; with feeds_lower also dh16). */
enum { MT_VBB_CAST = 1 << 0, MT_VBB_FC2 = 1 << 1, MT_VBB_GELU = 1 << 2, MT_VBB_FC1 = 1 << 3, MT_VBB_LN2 = 1 << 4, MT_VBB_PROJ = 1 << 5,
       MT_VBB_ATTN_SHIFT = 6, MT_VBB_QKV = 1 << 9, MT_VBB_LN1 = 1 << 10 };
int mt_vit_block_bwd(const MtVitBlockWeights* w, const MtVitBlockBuffers* b, const MtDensePlan* plan, int M, int D, int F,
                     int dh16_valid, int feeds_lower, int steps, mt_stream_t stream);

/* ------------------------------------------------------------ adapter ops -------------------------- */
/* Injector attention core (AM:225-229 inside AM:359-369): for each of M patch rows and 12 heads (dim 16):
 * a = softmax(q k^T / 4) v over the T modal tokens of the row's pass.  q fp16 [M,192]; k,v fp32 [B,T,192];
 * lse fp32 [M,12] (log-sum-exp of the scaled logits, saved for the backward; may be NULL for inference). */
int mt_inject_attn_fwd(const mt_half* q, int M, int rows_per_pass, const float* k, const float* v, int T,
                       mt_half* a, float* lse, mt_stream_t stream);
/* backward (a, lse from the forward): dq fp16 [M,192]; dk, dv fp32 [B,T,192] accumulated with atomics (pre-zeroed
 * by the caller).  The reductions over the patch rows run on MFMA. */
int mt_inject_attn_bwd(const mt_half* q, const mt_half* a, const float* lse, const mt_half* da, int M,
                       int rows_per_pass, const float* k, const float* v, int T, mt_half* dq, float* dk, float* dv,
                       mt_stream_t stream);

/* Extractor attention core (AM:225-229 inside AM:321-335): T token queries attend over the L patch rows of their
 * pass.  q fp32 [B,T,192]; kv fp16 [B*L, 384] (k | v).  Split over L (flash-decoding style): part_* are
 * workspaces of nsplit partials; out fp32 [B,T,192]; lse fp32 [B,T,12]. */
int mt_extract_attn_fwd(const float* q, const mt_half* kv, int B, int T, int L, float* out, float* lse,
                        float* part_acc, float* part_ml, int nsplit, mt_stream_t stream);
/* backward: dq fp32 [B,T,192] (atomics, pre-zeroed), dkv fp16 [B*L,384] */
int mt_extract_attn_bwd(const float* q, const mt_half* kv, const float* out, const float* lse, const float* dout,
                        int B, int T, int L, float* dq, mt_half* dkv, mt_stream_t stream);

/* Width-aware forms of the four cores above: `heads` heads of dim `head_dim` (16, 32 or 64; anything else returns
 * MT_ERR_UNSUPPORTED), E = heads * head_dim wherever 192 stands above (kv [B*L, 2E]), lse [M,heads] / [B,T,heads], the
 * extractor partials part_acc [B*heads*nsplit*T*head_dim] and part_ml [B*heads*nsplit*T*2] floats.  The entry points above
 * are these with (12, 16) (and opt = NULL).  The two backward forms take opt: partials (the deterministic forms, end of this header). */
int mt_inject_attn_fwd_hd(const mt_half* q, int M, int rows_per_pass, const float* k, const float* v, int T, int heads,
                          int head_dim, mt_half* a, float* lse, mt_stream_t stream);
int mt_inject_attn_bwd_hd(const mt_half* q, const mt_half* a, const float* lse, const mt_half* da, int M,
                          int rows_per_pass, const float* k, const float* v, int T, int heads, int head_dim, mt_half* dq,
                          float* dk, float* dv, const MtLaunchOpts* opt, mt_stream_t stream);
int mt_extract_attn_fwd_hd(const float* q, const mt_half* kv, int B, int T, int L, int heads, int head_dim, float* out,
                           float* lse, float* part_acc, float* part_ml, int nsplit, mt_stream_t stream);
int mt_extract_attn_bwd_hd(const float* q, const mt_half* kv, const float* out, const float* lse, const float* dout,
                           int B, int T, int L, int heads, int head_dim, float* dq, mt_half* dkv, const MtLaunchOpts* opt,
                           mt_stream_t stream);

/* Pathway networks of the gene encoder, all G pathways in one launch (gene_encoder.py:97-131,194-207: per pathway
 * SNN_Block(n_i -> latent), SNN_Block(latent -> latent), ELU, AlphaDropout off):
 *   z[i] = ELU(W2_i ELU(W1_i g_i + b1_i) + b2_i).
 * params / grads: the flat fp32 parameter / gradient buffers; offs [G][4] = element offsets of (W1_i [latent, n_i],
 * b1_i, W2_i [latent, latent], b2_i) (W2 offsets multiples of 4); sizes [G] = n_i; goff [G] = offset of g_i in the
 * concatenated `genes` vector; latent must be 256.  passes P (1..4): the reference calls the model once per task, so in
 * train mode every task pass draws its own AlphaDropout masks; the weights are streamed once for all passes.
 * z, a2 (second pre-activation, saved) are [G, P, latent] (pathway-major: the mixer's group axis stays outermost); a1 (first
 * pre-activation: the same in every pass) [G, latent].  alpha_drop (or NULL): train-mode nn.AlphaDropout(p) after each ELU, sites
 * alpha_drop->site and site + 1; the mask index of pathway i, pass p, unit j is (i P + p) latent + j. */
int mt_gene_snn_fwd(const float* params, const long* offs, const int* sizes, const long* goff, const float* genes, int G,
                    int latent, int passes, float* a1, float* a2, float* z, const MtDropout* alpha_drop, mt_stream_t stream);
/* backward: grads (+)= dW1, db1, dW2, db2 for every pathway, summed over the passes, given dz [G, P, latent] (no input
 * gradient: genes are data) */
int mt_gene_snn_bwd(const float* params, float* grads, const long* offs, const int* sizes, const long* goff,
                    const float* genes, int G, int latent, int passes, const float* a1, const float* a2, const float* dz,
                    const MtDropout* alpha_drop, mt_stream_t stream);

/* Integrated Gradients over the gene inputs (modaltune_amd/attribution.py): the pass axis carries `points` (1..4) quadrature points
 * of the straight path, point p seeing the input baseline + alphas[p] (genes - baseline); baseline NULL = zeros; alphas [points] is
 * read on the DEVICE.  No dropout (IG is defined with the stochastic layers off).  The weights are streamed once for all points: the
 * first layer is affine in alpha, so b1 + W1 genes and b1 + W1 baseline are formed once (in mt_gene_snn_fwd's summation order) and
 * point p takes alpha_p of the first and (1 - alpha_p) of the second -- alpha = 1 and alpha = 0 give mt_gene_snn_fwd's bits at genes
 * and at baseline.  a1, a2, z are [G, points, latent] (a1 differs per point here).  One workgroup per pathway, any n_i >= 1. */
int mt_gene_snn_fwd_points(const float* params, const long* offs, const int* sizes, const long* goff, const float* genes,
                           const float* baseline, const float* alphas, int G, int latent, int points, float* a1, float* a2, float* z,
                           mt_stream_t stream);
/* The INPUT gradient of the pathway networks at those points, summed with the quadrature weights (weights [points], device):
 *   dgenes[goff_i + k] (+)= unscale * sum_r W1_i[r][k] * sum_p weights[p] * elu'(a1_p[r]) * (W2_i^T (dz_p * elu'(a2_p)))[r]
 * unscale: device scalar or NULL (= 1), the reciprocal of the caller's gradient scale; accumulate != 0: += into dgenes [sum n_i].
 * Writes NO parameter gradient.  Every output element has one writer thread and one summation order (p ascending, then r
 * ascending): no atomics, bit-reproducible by construction. */
int mt_gene_snn_bwd_input(const float* params, const long* offs, const int* sizes, const long* goff, int G, int latent, int points,
                          const float* a1, const float* a2, const float* dz, const float* weights, const float* unscale,
                          float* dgenes, int accumulate, mt_stream_t stream);
/* attr = (genes - baseline) * dgenes (all [sum n_i]; baseline NULL = zeros) and pathway[i] = sum_k attr[goff_i + k] in a fixed
 * order (the same bits on every call). */
int mt_ig_finalize(const float* genes, const float* baseline, const float* dgenes, const int* sizes, const long* goff, int G,
                   float* attr, float* pathway, mt_stream_t stream);

/* Integrated Gradients over the PATCH embeddings.  The patch embedding is affine in the input features, so the straight path between a
 * baseline bag and the slide is the straight path between their embeddings ex, eb [L, D] (fp32, D % 4 == 0, 16-byte aligned):
 *   x0p[b L + l, :] = eb[l, :] + alphas[b] (ex[l, :] - eb[l, :])        1 <= B <= 4 passes, alphas [B] read on the DEVICE, any L >= 1
 * alphas[b] == 0 stores eb's bits and alphas[b] == 1 stores ex's (selected, not computed): those passes are the plain forward.
 * ex and eb are read once for all B passes. */
int mt_patch_points_fwd(const float* ex, const float* eb, const float* alphas, int B, int L, int D, float* x0p, mt_stream_t stream);
/* The per-patch attribution from the activation gradient dh [B, N, D] (N >= L + 1: row 0 of every pass is the cls row, never read):
 *   acc[l] += unscale * sum_b weights[b] <dh[b N + 1 + l, :], ex[l, :] - eb[l, :]>
 * weights [B] on the device; a pass with weights[b] == 0 is SKIPPED (its rows may hold anything); unscale: device scalar or NULL (= 1).
 * One wave per patch row, b ascending, the lane sums joined by a butterfly: one writer per acc[l] and one summation order, no
 * atomics -- the same bits on every call. */
int mt_patch_ig_accumulate(const float* dh, int N, const float* ex, const float* eb, const float* weights, const float* unscale, int B,
                           int L, int D, float* acc, mt_stream_t stream);

/* Small dense multi-head attention over tokens (prompt self-attention AM:87): q,k,v fp32 [B,T,E], heads h; the head dim
 * E / h must be 16, 32 or 64 (MT_ERR_UNSUPPORTED otherwise). */
int mt_token_mha_fwd(const float* q, const float* k, const float* v, int B, int T, int E, int heads, float* out,
                     float* probs, mt_stream_t stream);
int mt_token_mha_bwd(const float* q, const float* k, const float* v, const float* probs, const float* dout, int B,
                     int T, int E, int heads, float* dq, float* dk, float* dv, mt_stream_t stream);
/* The same with nn.MultiheadAttention(dropout = p) in train() (AM:42-52; the prompt_dropout key): the softmax probabilities are dropped
 * before the value product, out = (P o m / (1 - p)) V.  m is the element-dropout keep mask of drop->site over the flat [B, heads, T, T]
 * tensor -- element (b, h, i, j) has linear index ((b heads + h) T + i) T + j, so mt_dropout_f32 over one row of B heads T T ones
 * (rounded up to a multiple of 4) with the same MtDropout returns exactly m / (1 - p).  probs keeps the PRE-dropout softmax (the
 * attention maps and the backward read it); the backward regenerates m: dV = P~^T dO, dP = (dO V^T) o m / (1 - p), then delta and dS
 * from P and that dP.  drop NULL, rng NULL or p == 0: the entries above, bit for bit.  p outside [0, 1) or path_p != 0 (there is no
 * DropPath at this site): MT_ERR_BAD_ARG. */
int mt_token_mha_fwd_drop(const float* q, const float* k, const float* v, int B, int T, int E, int heads, float* out,
                          float* probs, const MtDropout* drop, mt_stream_t stream);
int mt_token_mha_bwd_drop(const float* q, const float* k, const float* v, const float* probs, const float* dout, int B,
                          int T, int E, int heads, float* dq, float* dk, float* dv, const MtDropout* drop, mt_stream_t stream);

/* Attention maps of the adapter attentions (forward only): the head-averaged softmax that nn.MultiheadAttention returns with
 * need_weights=True, recomputed from the operands and the LSE the forward kept -- the scores are rounded as the forward rounds
 * them, so each head's rows sum to 1 against that LSE.
 * Extractor: q fp32 [B,T,192], kv fp16 [B*L,384], lse [B,T,12] of mt_extract_attn_fwd -> w fp32 [B,T,L]. */
int mt_extract_attn_probs(const float* q, const mt_half* kv, const float* lse, int B, int T, int L, float* w, mt_stream_t stream);
/* Injector: q fp16 [M,192], k fp32 [B,T,192], lse [M,12] of mt_inject_attn_fwd -> w fp32 [M,T] (M = B * rows_per_pass). */
int mt_inject_attn_probs(const mt_half* q, int M, int rows_per_pass, const float* k, const float* lse, int T, float* w,
                         mt_stream_t stream);
/* The two above for `heads` heads of dim `head_dim` (16 / 32 / 64), E = heads * head_dim, lse [.., heads]. */
int mt_extract_attn_probs_hd(const float* q, const mt_half* kv, const float* lse, int B, int T, int L, int heads,
                             int head_dim, float* w, mt_stream_t stream);
int mt_inject_attn_probs_hd(const mt_half* q, int M, int rows_per_pass, const float* k, const float* lse, int T, int heads,
                            int head_dim, float* w, mt_stream_t stream);
/* Prompt self-attention: out fp32 [B,T,T] = mean over the heads of mt_token_mha_fwd's probs [B,heads,T,T]. */
int mt_token_probs_mean(const float* probs, int B, int heads, int T, float* out, mt_stream_t stream);

/* ------------------------------------------------------------ elementwise -------------------------- */
/* y = fp16(x); with `drop` (rows of D elements): y = fp16(drop(x)) -- the masked gradient of a dropped residual branch */
int mt_cast_f32_to_f16(const float* x, mt_half* y, long n, const MtDropout* drop, int D, mt_stream_t stream);
int mt_cast_f16_to_f32(const mt_half* x, float* y, long n, mt_stream_t stream);
/* Derived fp16 weight cache of an fp32 nn.Linear weight [R, C]: as stored (forward, W[N,K]) or transposed
 * (the dX GEMM's W^T[K,N]); re-run for trainable weights after every optimiser step (SURVEY §8b ownership). */
int mt_pack_weight_f16(const float* src, int R, int C, mt_half* dst, int transpose, mt_stream_t stream);
/* The same for a whole list of weights in ONE launch (the per-step refresh of every trainable big-M weight).
 * `items` is a DEVICE array of n_items records of 8 int64 each:
 *   { src fp32 [rows, cols] , dst fp16 (or 0) , dst_t fp16 (or 0) , rows , cols , row_off , ld , ld_t }
 * dst[(row_off + r) * ld + c] = dst_t[c * ld_t + row_off + r] = fp16(src[r * cols + c]); row_off / ld_t place the rows
 * of one source inside a cache that concatenates several (the fused K|V projection). */
int mt_pack_weights_f16(const long long* items, int n_items, mt_stream_t stream);
/* y = act(x) / dx = dy * act'(x) on fp32 vectors (ELU GE:178, GELU GE:187, ReLU AM:286) */
int mt_act_fwd(const float* x, float* y, long n, int act, mt_stream_t stream);
int mt_act_bwd(const float* x, const float* dy, float* dx, long n, int act, mt_stream_t stream);
/* y[i] = a[i] + alpha * b[i] */
int mt_axpy(const float* a, const float* b, float alpha, float* y, long n, mt_stream_t stream);
/* y[i] = a[i] + alpha * b[i % period]: a [period] row block broadcast over the batch (with_pos_embed, AM:64-65) */
int mt_axpy_bcast(const float* a, const float* b, float alpha, float* y, long n, long period, mt_stream_t stream);
/* out[i] += sum_r x[r * period + i] (r ascending): the gradient of the broadcast operand of mt_axpy_bcast and of the rows
 * mt_layernorm_fwd adds per period (d level / position embeddings summed over the task passes, AM:64-65); period % 4 == 0,
 * 16-byte aligned pointers */
int mt_fold_rows(const float* x, int reps, long period, float* out, mt_stream_t stream);
/* strided row copies between fp32 buffers: dst(map(m), :) (+)= src(map(m), :) */
int mt_copy_rows_f32(const float* src, long lds, const MtRowMap* smap, float* dst, long ldd, const MtRowMap* dmap,
                     int M, int D, int accumulate, mt_stream_t stream);
/* Injector residual-path backward (A.1): dres(m,:) += (1 + g) * dy(m,:) for the patch rows; also reduces
 * dgamma[n] += sum_m dy(m,n) * (x(m,n) + proj(m,n)) where proj = a @ Wo^T + bo is recomputed by the caller as
 * fp16 `proj`.  opt: partials.  lddy, ldx, lddx % 4 == 0 (16-byte vector accesses per row), else MT_ERR_BAD_ARG. */
int mt_inject_resid_bwd(const float* dy, long lddy, const MtRowMap* dymap, const float* x, long ldx,
                        const MtRowMap* xmap, const mt_half* proj, const float* gamma, float* dx, long lddx,
                        const MtRowMap* dxmap, int dx_accumulate, mt_half* dproj, float* dgamma, int M, int D,
                        const MtLaunchOpts* opt, mt_stream_t stream);

/* ---------------------------------------------------------- head, loss, optimiser ------------------ */
/* y[r,:] = x[r,:] / ||x[r,:]||_2 for R contiguous rows of O (projected text rows, TM:213) */
int mt_l2norm_rows(const float* x, float* y, int R, int O, mt_stream_t stream);
/* logits [R,O] -> L2-normalise rows, log_softmax, KL(sum) against softmax(target rows) * 10 (TM:225-233).
 * Writes loss (1 float) and dlogits [R,O] scaled by `loss_scale` (GradScaler semantics, TM:107,235). */
int mt_distill_loss(const float* logits, const float* target, int R, int O, float loss_scale,
                    const float* scale_dev /* device scalar multiplied into loss_scale, or NULL */, float* loss,
                    float* dlogits, mt_stream_t stream);

/* Fused multi-tensor AdamW over one flat fp32 parameter/gradient buffer (torch.optim.AdamW, TM:145-149) with
 * GradScaler.step semantics (TM:235-237): grads are divided by *scale; if any is non-finite the update is
 * skipped and *found_inf is set.  step_count is 1-based. */
int mt_adamw_step(float* p, const float* g, float* m, float* v, long n, double lr, double beta1, double beta2,
                  double eps, double weight_decay /* doubles: torch forms 1 - beta, lr * weight_decay and the bias corrections in
                  double before they meet the fp32 tensors (1 - 0.999f is 4.7e-5 off 0.001) */, int step_count, const int* step_dev /* device count of completed
                  steps (overrides step_count - 1) or NULL */, float grad_mult /* e.g. 1/world_size */,
                  const float* scale, int* found_inf, const float* lr_dev /* device scalar: the schedule's current
                  learning rate (overrides lr; a captured graph replays with whatever it holds -- the reference steps
                  GradualWarmupScheduler + CosineAnnealingLR every epoch, TM:151-154,242) or NULL */, mt_stream_t stream);
/* mt_adamw_step with PARAMETER GROUPS: the flat buffer is a run of segments (neighbouring tensors of one group), and a segment's group
 * supplies two values; betas, eps, the bias corrections, grad_mult / *scale and the found_inf skip are shared.  Per element the
 * arithmetic is mt_adamw_step's with
 *   lr_g    = (float)((double)lr_f32 * lr_mult)           lr_f32 = *lr_dev or (float)lr; rounded once: lr_mult == 1.0 gives the base bits
 *   decay_g = (float)(1.0 - (double)lr_g * weight_decay)
 * so one launch equals mt_adamw_step over every segment alone with lr = lr_g and the group's weight_decay, bit for bit.
 * `p` is the piece [index_base, index_base + n) of a 16-byte aligned flat buffer (pieces compose, as in mt_checksum64): p, g, m, v are
 * 4-byte aligned and lie in their buffers as index_base says (address / 4 = index_base mod 4), else MT_ERR_BAD_ARG.  Segment s covers the
 * ABSOLUTE indices [seg_end[s - 1], seg_end[s]), seg_end[-1] = 0; the ends are ascending multiples of 4 (slot padding lies inside a
 * segment and stays +0), the last one at or behind index_base + n.  seg_end / seg_group are DEVICE tables of nseg entries, group ids
 * < ngroups; `groups` is a HOST array of ngroups entries that travels as kernel arguments.  ngroups outside 1 .. MT_ADAM_MAX_GROUPS:
 * MT_ERR_UNSUPPORTED.  lr_mult = 0 with weight_decay = 0 holds a group's parameter bits still while its moments keep updating. */
#define MT_ADAM_MAX_GROUPS 16
typedef struct { double lr_mult; double weight_decay; } MtAdamGroup;
int mt_adamw_step_groups(float* p, const float* g, float* m, float* v, long n, long index_base, const int* seg_end,
                         const unsigned char* seg_group, int nseg, const MtAdamGroup* groups, int ngroups, double lr, double beta1,
                         double beta2, double eps, int step_count, const int* step_dev, float grad_mult, const float* scale,
                         int* found_inf, const float* lr_dev, mt_stream_t stream);
/* mt_adamw_step_groups that also keeps an EXPONENTIAL MOVING AVERAGE of the parameters, in the same launch: `ema` is one more flat fp32
 * buffer laid out and indexed like `p` (the same piece of its own 16-byte aligned buffer, overlapping none of p, g, m, v: else
 * MT_ERR_BAD_ARG).  Behind the AdamW update of an element, with p_new its new parameter and contraction off:
 *   d = p_new - e;   t = w * d;   e = e + t          three fp32 operations, each rounded once, no FMA
 * so an element held still (lr_mult = 0, weight_decay = 0) whose average equals it keeps every bit.  w is one value per launch, formed
 * in double from the 1-based optimiser step t = *step_dev + 1 (step_dev NULL: step_count):
 *   decay_t = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay;   w = (float)(1.0 - decay_t)
 * A set *found_inf skips the average with the update.  p, m and v get mt_adamw_step_groups's bits.  ema == NULL: mt_adamw_step_groups
 * itself (ema_decay and ema_warmup are not read); otherwise ema_decay outside [0, 1): MT_ERR_BAD_ARG. */
int mt_adamw_step_groups_ema(float* p, const float* g, float* m, float* v, long n, long index_base, const int* seg_end,
                             const unsigned char* seg_group, int nseg, const MtAdamGroup* groups, int ngroups, double lr, double beta1,
                             double beta2, double eps, int step_count, const int* step_dev, float grad_mult, const float* scale,
                             int* found_inf, const float* lr_dev, float* ema, double ema_decay, int ema_warmup, mt_stream_t stream);
/* a[i] <-> b[i] for i < n: two fp32 buffers exchanged as 32-bit patterns (NaN payloads and -0.0 survive).  Both 4-byte aligned, any
 * n >= 1; the ranges must not overlap (MT_ERR_BAD_ARG, as for a null pointer or n <= 0).  16-byte loads and stores when a and b sit
 * alike in their 16-byte lines, 4-byte ones otherwise. */
int mt_swap_f32(float* a, float* b, long n, mt_stream_t stream);
/* GradScaler.update on device (TM:237): *found_inf ? scale *= backoff : (every `interval` clean steps scale *= growth,
 * unless the product is not finite: then the scale stays, as in torch._amp_update_scale_); *found_inf is cleared */
int mt_scaler_update(float* scale, int* growth_tracker, int* found_inf, int* step_dev /* ++ on a clean step, or NULL */,
                     float growth, float backoff, int interval, mt_stream_t stream);
int mt_check_finite(const float* g, long n, int* found_inf, mt_stream_t stream);
/* Global-norm clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) without a host read-back.
 * mt_grad_sumsq: sumsq[0] = sum of g[i]^2 over n floats (g 4-byte aligned, any n >= 1), squared and summed in DOUBLE from the first
 * element: finite inputs never overflow and the same input gives the same bits.  Two launches, no floating-point atomics: every
 * stage-1 workgroup stores its sum into its own slot of `partials` (device doubles, at least mt_grad_sumsq_partials_elems(n) of them,
 * no initialisation needed), one workgroup adds the slots in ascending order.  *found_inf (device int, or NULL) is ORed with 1 when an
 * element is not finite -- mt_check_finite's rule (+-FLT_MAX and subnormals are finite; never cleared here) -- so at a step that
 * clips this launch stands in for mt_check_finite. */
int mt_grad_sumsq(const float* g, long n, double* partials, long partials_elems, double* sumsq, int* found_inf, mt_stream_t stream);
/* host arithmetic: the slots mt_grad_sumsq needs for n elements (non-decreasing in n); negative for n <= 0 */
long mt_grad_sumsq_partials_elems(long n);
/* One thread, double arithmetic, each output rounded once to fp32: S = sumsq[0] + ... + sumsq[nsums - 1] (ascending);
 *   out[0] = total_norm = sqrt(S) * grad_mult / *scale (scale NULL: 1): the norm of the unscaled, averaged gradient
 *   out[1] = coef = min(1, max_norm / (total_norm + 1e-6))
 *   out[2] = *scale / coef: hand `out + 2` to mt_adamw_step as its `scale` and it applies g * grad_mult * coef / *scale
 * coef == 1 leaves out[2] = *scale bit for bit (an unclipped step is today's arithmetic); so do max_norm = +inf (report the norm
 * only), a set *found_inf (device int or NULL; the step is skipped anyway) and a non-finite S.  A finite gradient whose norm
 * overflows fp32: total_norm = +inf, coef = 0, out[2] = +inf (the update sees a zero gradient, as with torch). */
int mt_grad_clip_coef(const double* sumsq, int nsums, double grad_mult, const float* scale, double max_norm, const int* found_inf,
                      float* out, mt_stream_t stream);

/* Exact 64-bit checksum of `nwords` 32-bit words (data 4-byte aligned, any nwords >= 1), formed on the device:
 *   out[0] = sum_{i < nwords} mix(index_base + i) * (word_i + 1)  mod 2^64,   mix(j) = splitmix64(j) | 1
 *   (z = j + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31)
 * Unsigned 64-bit arithmetic throughout, so every reduction order gives the same value and pieces compose:
 * cs(a) = cs(a[:k]) + cs(a[k:], index_base = k).  An odd, position-dependent multiplier: any single-word change and any swap of two
 * unequal words moves the sum; the + 1 tells zero-filled ranges of different lengths apart.  Two launches in the form of mt_grad_sumsq,
 * no atomics: every stage-1 workgroup stores into its own slot of `partials` (device 8-byte words, at least
 * mt_checksum64_partials_elems(nwords) of them, no initialisation needed), one workgroup adds the slots.  index_base >= 0. */
int mt_checksum64(const void* data, long nwords, long index_base, unsigned long long* partials, long partials_elems,
                  unsigned long long* out, mt_stream_t stream);
/* host arithmetic: the slots mt_checksum64 needs for nwords words (non-decreasing in nwords); negative for nwords <= 0 */
long mt_checksum64_partials_elems(long nwords);

/* Measurement aid (bench.py, SURVEY §8d "the builder's own MFMA micro-benchmark peak"): `workgroups` x 4 waves each issue
 * iters x 4 independent v_mfma_f32_32x32x16_f16 on non-trivial register operands = workgroups * 4 * iters * 4 * 32768 FLOP. */
int mt_mfma_probe(float* sink, int workgroups, int iters, mt_stream_t stream);

/* ---------------------------------------------------------- module bridge / input boundary --------- */
/* s[0] = target / max|x|, s[1] = 1 / s[0] (both 1 when the maximum is 0 or not finite): device-side rescale of the
 * gradient torch hands to the nn.Module bridge (loss.backward(), TM:235) into the fp16 range of the activation-gradient
 * stream, without a host read-back.  s[0] is clamped to [2^-126, 2^126] (a maximum below ~target / FLT_MAX would otherwise
 * give s[0] = inf, s[1] = 0): s[0] and s[1] are finite, positive normal numbers for every input. */
int mt_absmax_scale(const float* x, long n, float target, float* s, mt_stream_t stream);
/* y[i] = a[i] + (*alpha) * b[i] with alpha a DEVICE scalar (a may be NULL: y = (*alpha) * b); y may be a or b (in place) */
int mt_axpy_dev(const float* a, const float* b, const float* alpha, float* y, long n, mt_stream_t stream);
/* LongNetViT.coords_to_pos (SE:198-211) on the device: prow[i] = floor(coords[i][0] / tile), pcol[i] = floor(coords[i][1]
 * / tile) for fp32 coords [L, 2]; cells outside [0, ngrids) are clamped and *err (device int, or NULL) is OR-ed with 1 --
 * the host raises when it next looks (the reference would index out of bounds, SE:116-120,237). */
int mt_coords_to_grid(const float* coords, int L, float tile, int ngrids, int* prow, int* pcol, int* err,
                      mt_stream_t stream);
/* TITAN feature gridding on the device (titan_adapter.py:295-327 `preprocess_features` + the background drop of
 * `prepare_forward_features`, TA:282-291) WITHOUT materialising the H x W grid: the tokens of a slide are its occupied cells
 * in row-major order, each the sum of its patches' features in patch order (what index_add_ produces on the CPU, bitwise
 * reproducible: no atomics, no sort -- O(L^2) integer compares through LDS).
 *   mt_titan_grid         cells[i] = floor((coords[i] - min coords) / patch) (fp32 coords [L, 2]); dims (device int[2]) = {H, W};
 *                         *err |= 1 for non-finite / out-of-range coordinates
 *   mt_titan_cell_sums    first[i] / next[i]: chain of the patches of one cell in patch order; sums[i, :] (fp32 [L, C]) = the cell's
 *                         summed features for its first patch; nz[i] = any(sum != 0) (the reference's bg_mask, TA:326)
 *   mt_titan_token_order  pos[i] = token index (without cls) of the cell patch i owns, or -1; cells_tok[pos] = (row, col);
 *                         *count = number of tokens
 *   mt_titan_gather_tokens x16[pos[i], :] = fp16(sums[i, :]): the A operand of the patch-embedding GEMM */
int mt_titan_grid(const float* coords, int L, float patch, int* cells, int* dims, int* err, mt_stream_t stream);
int mt_titan_cell_sums(const float* feat, long ldf, const int* cells, int L, int C, int* first, int* next, float* sums, int* nz,
                       mt_stream_t stream);
int mt_titan_token_order(const int* cells, const int* first, const int* nz, int L, int* pos, int* cells_tok, int* count,
                         mt_stream_t stream);
int mt_titan_gather_tokens(const float* sums, const int* pos, int L, int C, mt_half* x16, mt_stream_t stream);
/* The same index_add as one strided scatter (host-computed indices): the bring-your-own-backbone path of modaltune_amd/titan.py,
 * which must hand the backbone module the dense [1, C, H, W] grid its own `prepare_forward_features` expects.
 * dst(idx[m], :) (+)= src(src_idx[m], :) for fp32 rows of D (src_idx NULL = identity); the caller launches one pass per
 * occurrence rank of a cell, so the cells of a pass are distinct.
 * mt_row_absmax_f32: out[m] = max_d |x(m, d)| (the background mask is "any feature of the cell != 0", TA:326). */
int mt_scatter_rows_f32(const float* src, const int* src_idx, const int* idx, float* dst, int M, int D, int accumulate,
                        mt_stream_t stream);
int mt_row_absmax_f32(const float* x, float* out, int M, int D, mt_stream_t stream);

/* ------------------------------------------------------- deterministic forms ------------------------ */
/* The six launchers above that accumulate a trainable-parameter gradient with fp32 atomics (in whatever order their workgroups
 * retire) have a bit-reproducible form, selected by MtLaunchOpts.partials: no atomic, global or LDS, executes.  Every workgroup stores
 * its partial result with plain stores to its own slot of `partials` (a pure function of its block index), then ONE reduce kernel
 * (csrc/det_reduce.hip) adds the slots in ascending order and adds the sum to the destination -- the `+=` of the default forms is kept,
 * and every output that is not reduced across workgroups (dx, dx_f16, dproj, the patch-side dq, dkv) has the default form's bits.
 * `partials`: the caller's fp32 workspace (16-byte aligned) of `partials_elems` floats, at least what the `_det_elems` query of the same
 * shape returns (host arithmetic only; a negative MtStatus for a shape the form rejects).  A short workspace returns MT_ERR_BAD_ARG
 * before any launch.  The workspace needs no initialisation: no slot is read that was not written by the same call.  Like everything
 * here: no allocation, no synchronisation; two calls in flight need two workspaces.
 *   mt_gemm_tn_f16         slots = the row ranges of the M-split that hold rows; [slots][N1][N2], then [slots][N1] with colsum
 *   mt_colsum_f16          [cdiv(M, 256)][N]
 *   mt_layernorm_bwd       dw and db required; [min(cdiv(M, 4), 512)][2][D]
 *   mt_inject_resid_bwd    [min(cdiv(M, 4), 512)][D]
 *   mt_inject_attn_bwd_hd  [cdiv(rows_per_pass, 512)][B][T][E] for dk, then the same for dv
 *   mt_extract_attn_bwd_hd [cdiv(L, 512)][B][T][E] */
long mt_gemm_tn_f16_det_elems(int M, int N1, int N2, int with_colsum);
long mt_colsum_f16_det_elems(int M, int N);
long mt_layernorm_bwd_det_elems(int M, int D);
long mt_inject_resid_bwd_det_elems(int M, int D);
long mt_inject_attn_bwd_hd_det_elems(int M, int rows_per_pass, int T, int heads, int head_dim);
long mt_extract_attn_bwd_hd_det_elems(int B, int T, int L, int heads, int head_dim);

#ifdef __cplusplus
}
#endif
#endif /* MODALTUNE_HIP_H */
