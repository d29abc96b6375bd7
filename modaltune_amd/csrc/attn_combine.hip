// Dilated attention (LongNet), backward: the combine pass over the per-branch compact gradients.
// (see attn.hip for the reference semantics and the forward; split out so that the translation unit can carry its own
// LLVM scheduling strategy -- attn_common.h)
#include "attn_common.h"

namespace {

// Sum the per-branch compact gradients into the dense fp16 dqkv [B*N, 2304] that feeds the dX GEMM.
// 192 threads per token row: thread -> 12 consecutive columns of one (q|k|v, head).  The workspace is token-major
// (attn_common.h: ws_slot): the heads a branch covers at a token are one contiguous run in the source AND in the dense row, so
// the threads of a wave read consecutive addresses.
__global__ __launch_bounds__(192) void dilated_attn_bwd_combine_kernel(const h16* __restrict__ ws, Plan p, h16* __restrict__ dqkv) {
  const long M = (long)p.B * p.N;
  const int t = threadIdx.x;
  const int col = t * 12, which = col / DM, h = (col % DM) / HD, d0 = col % HD;
  for (long m = blockIdx.x; m < M; m += gridDim.x) {
    const int pos = (int)(m % p.N);
    float acc[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) acc[e] = 0.f;
#pragma unroll
    for (int br = 0; br < MT_MAX_BRANCHES; ++br) {
      if (br < p.nbranch) {
        const int dr = p.ratio[br], sg = p.seg[br], hb = H / dr;
        const int j = pos / sg, loc = pos - j * sg;
        if (loc % dr == h / hb) {
          const h16* src = ws + p.ws_off[br] + ((m * 3 + which) * hb + (h % hb)) * HD + d0;
          const h16x4 a0 = *reinterpret_cast<const h16x4*>(src), a1 = *reinterpret_cast<const h16x4*>(src + 4),
                      a2 = *reinterpret_cast<const h16x4*>(src + 8);
#pragma unroll
          for (int e = 0; e < 4; ++e) { acc[e] += (float)a0[e]; acc[4 + e] += (float)a1[e]; acc[8 + e] += (float)a2[e]; }
        }
      }
    }
    h16* dst = dqkv + m * QKV_LD + col;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const h16x4 o = {(h16)acc[4 * k], (h16)acc[4 * k + 1], (h16)acc[4 * k + 2], (h16)acc[4 * k + 3]};
      *reinterpret_cast<h16x4*>(dst + 4 * k) = o;
    }
  }
}

// In-place form: the dQ and dK/dV kernels wrote the dense branch (ratio 1) straight into dqkv (attn_common.h: DenseDst), so a
// (token, head) that no sparse branch covers -- (1/2)(3/4)(7/8)(15/16) = 38 % of them with the shipped table -- is final already
// and is neither read nor written here.  Everywhere else the sum is the workspace form's, operand for operand: fp32 from +0,
// ascending branch index (the dense value, read back from dqkv, at ITS index), rounded once.
// One wave per token row, so the branch geometry (segment, residue, covered head run) is wave-uniform and lives in SGPRs; a lane
// owns the 16-byte pieces (8 halves: a piece never straddles a head, 48 = 6 x 8) it * 64 + lane of the row's 288.  A branch
// covers the heads [res * hb, res * hb + hb): one subtract and one unsigned compare per lane and branch, and its source run for
// one `which` is contiguous, so the piece's address is a scalar row base plus which * hb * 48 + (piece % 96) * 8 -- for the dense
// branch (hb = 16, base = the dqkv row) that is the piece itself.  No branch around any load (hipcc would wait for each one
// separately): a lane whose piece a branch does not cover loads the first 16 bytes of the workspace instead, one line that
// stays in cache, and the value is dropped with a select; adding the +0 it leaves changes no bit of a sum that starts at +0.
constexpr int CMB_PIECES = QKV_LD / 8;      // 288
constexpr int CMB_GRID_MAX = 2048;          // 8 workgroups of four row-waves per CU; a wave walks rows grid * 4 apart
template <int NB>
__global__ __launch_bounds__(256) void dilated_attn_bwd_combine_inplace_kernel(const h16* __restrict__ ws, Plan p, int db, h16* dqkv) {
  const long M = (long)p.B * p.N;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const LivePasses lp = live_passes(p);      // rows of the live passes only (the others' gradients are never read)
  const long m_end = min(M, (long)lp.b1 * p.N);
  for (long m = (long)lp.b0 * p.N + (long)blockIdx.x * 4 + wave; m < m_end; m += (long)gridDim.x * 4) {
    const int pos = (int)((unsigned)m % (unsigned)p.N);      // (M < 2^31: checked by the caller)
    h16* row = dqkv + m * QKV_LD;
    int lo[NB], hbs[NB], str[NB];
    const h16* src[NB];
#pragma unroll
    for (int br = 0; br < NB; ++br) {
      const bool sparse = br < p.nbranch && br != db;
      const int dr = sparse ? p.ratio[br] : 1, sg = sparse ? p.seg[br] : 1, hb = H / dr;
      const int loc = pos % sg;
      lo[br] = (loc % dr) * hb;
      hbs[br] = sparse ? hb : 0;      // 0: covers no head by itself (a branch the plan does not have; the dense one: see `any`)
      str[br] = hb * HD;
      src[br] = br == db ? row : ws + (sparse ? p.ws_off[br] + (m * 3 * hb - lo[br]) * HD : 0);
    }
#pragma unroll 1      // (unrolled, hipcc keeps every iteration's piece geometry live across the row loop: 107 VGPRs instead of 63)
    for (int it = 0; it < (CMB_PIECES + 63) / 64; ++it) {
      const int piece = it * 64 + lane;
      const int which = piece / (DM / 8), hp = piece - which * (DM / 8), h = hp / 6;
      bool cov[NB], any = false;
#pragma unroll
      for (int br = 0; br < NB; ++br) {
        cov[br] = piece < CMB_PIECES && (unsigned)(h - lo[br]) < (unsigned)hbs[br];
        any |= cov[br];
      }
      h16x8 v[NB];
#pragma unroll
      for (int br = 0; br < NB; ++br) {
        if (br == db) cov[br] = any;      // the dense value takes part wherever a sparse branch does
        const h16* a = cov[br] ? src[br] + (which * str[br] + hp * 8) : ws;
        v[br] = *reinterpret_cast<const h16x8*>(a);
      }
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
      for (int br = 0; br < NB; ++br) {
        const h16x8 x = sel8(cov[br], v[br]);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)x[e];
      }
      if (any) {
        h16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (h16)acc[e];
        *reinterpret_cast<h16x8*>(row + piece * 8) = o;
      }
    }
  }
}

}  // namespace

void mt_attn::launch_bwd_combine(const void* ws, const MtDilatedPlan* plan, mt_half* dqkv, hipStream_t s) {
  const Plan p = make_plan(plan, 128);
  const long M = (long)p.B * p.N;
  hipLaunchKernelGGL(dilated_attn_bwd_combine_kernel, dim3((int)min(M, 16384L)), dim3(192), 0, s, (const h16*)ws, p, (h16*)dqkv);
}

void mt_attn::launch_bwd_combine_inplace(const void* ws, const MtDilatedPlan* plan, mt_half* dqkv, const int* live, hipStream_t s) {
  const Plan p = make_plan(plan, 128, live);
  const long M = (long)p.B * p.N;
  const int db = dense_branch_host(plan);
  const dim3 grid((int)min((M + 3) / 4, (long)CMB_GRID_MAX));
  if (p.nbranch <= 5)
    hipLaunchKernelGGL(dilated_attn_bwd_combine_inplace_kernel<5>, grid, dim3(256), 0, s, (const h16*)ws, p, db, (h16*)dqkv);
  else
    hipLaunchKernelGGL(dilated_attn_bwd_combine_inplace_kernel<MT_MAX_BRANCHES>, grid, dim3(256), 0, s, (const h16*)ws, p, db, (h16*)dqkv);
}
