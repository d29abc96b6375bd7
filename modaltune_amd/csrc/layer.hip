// Composite launchers: the launch list of one frozen backbone layer / block, forward and backward, behind ONE C-ABI call each
// (SURVEY §8b lists `mt_lnqkv_fwd`, `mt_dilated_attn_fwd/bwd`, `mt_mix_ln_outproj_fwd/bwd`, `mt_ffn_fwd/bwd` as the per-layer
// surface; these entries enqueue that whole sequence).  Host code only: every kernel is launched through the per-op extern "C"
// entry points.  These four lists are the ONLY statement of a layer's schedule: Python makes one call per layer and direction (9 + 11
// ctypes hops per LongNet layer and step saved, 36 layers' worth per step: the eager schedule of short bags is bound by exactly
// that), and a timed pass (modaltune_amd/ops.py, TIMER) walks the same list one `steps` bit per call (include/modaltune_hip.h).
#include "common.h"

namespace {

MtGemmEpilogue epi_bias(const float* bias) {
  MtGemmEpilogue e{};
  e.bias = bias;
  return e;
}
MtLaunchOpts live_opts(const int* live, int live_rows) {      // a branch's live table entry (or NULL: every pass), one pass = live_rows rows
  MtLaunchOpts o{};
  o.live = live; o.live_rows = live_rows;
  return o;
}
MtLaunchOpts eps_opts(float eps) {
  MtLaunchOpts o{};
  o.eps = eps;
  return o;
}
#define MT_TRY(call)              \
  do {                            \
    const int st__ = (call);      \
    if (st__ != MT_OK) return st__; \
  } while (0)
#define MT_STEP(bits, call) \
  do { if (steps & (bits)) MT_TRY(call); } while (0)      // one launch of a list: enqueued when the caller's `steps` selects it

}  // namespace

// ---------------------------------------------------------------- LongNet EncoderLayer (ENC:121-175, DA:146-262, FFN:132-143)
extern "C" int mt_longnet_layer_fwd(const MtLongNetLayerWeights* w, const MtLongNetLayerBuffers* b, const MtDilatedPlan* plan, int M,
                                    int D, int F, const float* pend_x, const mt_half* pend_branch, const MtDropout* pend_drop, int defer,
                                    float* out, const MtDropout* drop_attn, const MtDropout* drop_ffn, int steps, mt_stream_t s) {
  if (!w || !b || !plan || M < 1 || D != 768 || (!defer && !out)) return MT_ERR_BAD_ARG;
  const MtLaunchOpts la = live_opts(b->live_attn, plan->N), lf = live_opts(b->live_ffn, plan->N);
  // self_attn_layer_norm (pre-norm); with an outstanding fc2 add of the layer below: hin = x + drop(branch) on the same pass
  if (!pend_x)
    MT_STEP(MT_LNF_LN1, mt_layernorm_fwd(b->hin, D, nullptr, MT_OUT_F32, 0, w->ln1_w, w->ln1_b, nullptr, 0, b->u16, D, nullptr, MT_OUT_F16, b->st1, M, D, nullptr, s));
  else
    MT_STEP(MT_LNF_LN1, mt_add_layernorm_fwd(pend_x, pend_branch, pend_drop, w->ln1_w, w->ln1_b, b->hin, b->u16, b->st1, M, D, nullptr, s));
  MtGemmEpilogue e = epi_bias(w->b_qkv);
  MT_STEP(MT_LNF_QKV, mt_gemm_nt_f16(b->u16, D, nullptr, w->w_qkv, M, 3 * D, D, MT_EPI_QKV_HM, &e, b->qkv, 3 * D, nullptr, MT_OUT_F16, &la, s));
  MT_STEP(MT_LNF_ATTN, mt_dilated_attn_fwd(b->qkv, plan, b->o_br, b->lse_br, &la, s));
  MT_STEP(MT_LNF_MIX, mt_dilated_mix_ln_fwd(b->o_br, b->lse_br, plan, w->inner_ln_w, w->inner_ln_b, b->u16, b->stin, b->lse_tot, &la, s));
  e = epi_bias(w->b_out);
  MT_STEP(MT_LNF_OUT, mt_gemm_nt_f16(b->u16, D, nullptr, w->w_out, M, D, D, MT_EPI_BIAS, &e, b->br16, D, nullptr, MT_OUT_F16, &la, s));
  MT_STEP(MT_LNF_LN2, mt_add_layernorm_fwd(b->hin, b->br16, drop_attn, w->ln2_w, w->ln2_b, b->hmid, b->u16, b->st2, M, D, nullptr, s));
  e = epi_bias(w->b_fc1);
  MT_STEP(MT_LNF_FC1, mt_gemm_nt_f16(b->u16, D, nullptr, w->w_fc1, M, F, D, MT_EPI_BIAS, &e, b->a1, F, nullptr, MT_OUT_F16, &lf, s));
  MT_STEP(MT_LNF_FFN_LN,
          mt_layernorm_fwd(b->a1, F, nullptr, MT_OUT_F16, 1, w->ffn_ln_w, w->ffn_ln_b, nullptr, 0, b->t16, F, nullptr, MT_OUT_F16, b->stf, M, F,
                                &lf, s));
  e = epi_bias(w->b_fc2);
  if (defer) {
    MT_STEP(MT_LNF_FC2, mt_gemm_nt_f16(b->t16, F, nullptr, w->w_fc2, M, D, F, MT_EPI_BIAS, &e, b->br16, D, nullptr, MT_OUT_F16, &lf, s));
  } else {      // (the BIAS_RESID form carries the residual stream: every row, the epilogue selects a dropped pass to 0)
    e.resid = b->hmid; e.ldr = D;
    if (drop_ffn) e.drop = *drop_ffn;
    MT_STEP(MT_LNF_FC2, mt_gemm_nt_f16(b->t16, F, nullptr, w->w_fc2, M, D, F, MT_EPI_BIAS_RESID, &e, out, D, nullptr, MT_OUT_F32, nullptr, s));
  }
  return MT_OK;
}

extern "C" int mt_longnet_layer_bwd(const MtLongNetLayerWeights* w, const MtLongNetLayerBuffers* b, const MtDilatedPlan* plan, int M,
                                    int D, int F, int dh16_valid, int feeds_lower, const MtDropout* drop_attn, const MtDropout* drop_ffn,
                                    const MtDropout* drop_lower_ffn, int steps, mt_stream_t s) {
  if (!w || !b || !plan || M < 1 || D != 768) return MT_ERR_BAD_ARG;
  const MtLaunchOpts la = live_opts(b->live_attn, plan->N), lf = live_opts(b->live_ffn, plan->N);
  const MtGemmEpilogue none{};
  const mt_half* src16 = b->dh16;
  if (!dh16_valid) {      // gradient of the (dropped) FFN branch output
    MT_STEP(MT_LNB_CAST, mt_cast_f32_to_f16(b->dh, b->dy16, (long)M * D, drop_ffn, D, s));
    src16 = b->dy16;
  }
  MT_STEP(MT_LNB_FC2, mt_gemm_nt_f16(src16, D, nullptr, w->wt_fc2, M, F, D, MT_EPI_BIAS, &none, b->dt16, F, nullptr, MT_OUT_F16, &lf, s));
  // (the live_* entries: the kernels of a branch -- its GEMMs included -- leave its dropped passes out; the LayerNorm backward that closes
  // the branch reads their stale dy as zero)
  MT_STEP(MT_LNB_FFN_LN, mt_layernorm_bwd(b->dt16, F, nullptr, MT_OUT_F16, b->a1, F, nullptr, MT_OUT_F16, 1, w->ffn_ln_w, b->stf, b->da1, F,
                                               nullptr, MT_OUT_F16, 0, nullptr, nullptr, nullptr, nullptr, M, F, &lf, s));
  MT_STEP(MT_LNB_FC1, mt_gemm_nt_f16(b->da1, F, nullptr, w->wt_fc1, M, D, F, MT_EPI_BIAS, &none, b->dy16, D, nullptr, MT_OUT_F16, &lf, s));
  MT_STEP(MT_LNB_LN2, mt_layernorm_bwd(b->dy16, D, nullptr, MT_OUT_F16, b->hmid, D, nullptr, MT_OUT_F32, 0, w->ln2_w, b->st2, b->dh, D, nullptr,
                                            MT_OUT_F32, 1, nullptr, nullptr, b->dh16, drop_attn, M, D, &lf, s));
  MT_STEP(MT_LNB_OUT, mt_gemm_nt_f16(b->dh16, D, nullptr, w->wt_out, M, D, D, MT_EPI_BIAS, &none, b->u16, D, nullptr, MT_OUT_F16, &la, s));
  MT_STEP(MT_LNB_MIX, mt_dilated_mix_ln_bwd(b->u16, b->o_br, b->lse_br, b->lse_tot, plan, w->inner_ln_w, b->stin, b->dmixed, b->delta,
                                                 &la, s));
  MT_STEP(MT_ATTN_BWD_ALL << MT_LNB_ATTN_SHIFT, mt_dilated_attn_bwd_inplace(b->qkv, b->dmixed, b->lse_tot, b->delta, plan, b->attn_ws, b->dqkv16,
                                                                         (steps >> MT_LNB_ATTN_SHIFT) & MT_ATTN_BWD_ALL, &la, s));
  MT_STEP(MT_LNB_QKV, mt_gemm_nt_f16(b->dqkv16, 3 * D, nullptr, w->wt_qkv, M, D, 3 * D, MT_EPI_BIAS, &none, b->dy16, D, nullptr, MT_OUT_F16, &la, s));
  MT_STEP(MT_LNB_LN1, mt_layernorm_bwd(b->dy16, D, nullptr, MT_OUT_F16, b->hin, D, nullptr, MT_OUT_F32, 0, w->ln1_w, b->st1, b->dh, D, nullptr,
                                            MT_OUT_F32, 1, nullptr, nullptr, feeds_lower ? b->dh16 : nullptr,
                                            feeds_lower ? drop_lower_ffn : nullptr, M, D, &la, s));
  return MT_OK;
}

// ---------------------------------------------------------------- dense pre-norm ViT block (TITAN configuration, TA:359-361)
extern "C" int mt_vit_block_fwd(const MtVitBlockWeights* w, const MtVitBlockBuffers* b, const MtDensePlan* plan, int M, int D, int F,
                                const float* pend_x, const mt_half* pend_branch, int defer, float* out, int steps, mt_stream_t s) {
  if (!w || !b || !plan || M < 1 || D != 768 || (!defer && !out)) return MT_ERR_BAD_ARG;
  if (!(w->n1_eps > 0.f) || !(w->n2_eps > 0.f)) return MT_ERR_BAD_ARG;      // (0 in MtLaunchOpts would mean the default)
  const MtLaunchOpts e1 = eps_opts(w->n1_eps), e2 = eps_opts(w->n2_eps);
  if (!pend_x)
    MT_STEP(MT_VBF_LN1, mt_layernorm_fwd(b->hin, D, nullptr, MT_OUT_F32, 0, w->n1_w, w->n1_b, nullptr, 0, b->u16, D, nullptr, MT_OUT_F16, b->st1,
                                             M, D, &e1, s));
  else
    MT_STEP(MT_VBF_LN1, mt_add_layernorm_fwd(pend_x, pend_branch, nullptr, w->n1_w, w->n1_b, b->hin, b->u16, b->st1, M, D, &e1, s));
  MtGemmEpilogue e = epi_bias(w->b_qkv);
  MT_STEP(MT_VBF_QKV, mt_gemm_nt_f16(b->u16, D, nullptr, w->w_qkv, M, 3 * D, D, MT_EPI_BIAS, &e, b->qkv, 3 * D, nullptr, MT_OUT_F16, nullptr, s));
  MT_STEP(MT_VBF_ATTN, mt_dense_attn_fwd(b->qkv, plan, b->o16, b->lse, s));
  e = epi_bias(w->b_proj);
  MT_STEP(MT_VBF_PROJ, mt_gemm_nt_f16(b->o16, D, nullptr, w->w_proj, M, D, D, MT_EPI_BIAS, &e, b->br16, D, nullptr, MT_OUT_F16, nullptr, s));
  MT_STEP(MT_VBF_LN2, mt_add_layernorm_fwd(b->hin, b->br16, nullptr, w->n2_w, w->n2_b, b->hmid, b->u16, b->st2, M, D, &e2, s));
  e = epi_bias(w->b_fc1);
  MT_STEP(MT_VBF_FC1, mt_gemm_nt_f16(b->u16, D, nullptr, w->w_fc1, M, F, D, MT_EPI_BIAS, &e, b->a1, F, nullptr, MT_OUT_F16, nullptr, s));
  MT_STEP(MT_VBF_GELU, mt_gelu_f16_fwd(b->a1, b->t16, (long)M * F, s));
  e = epi_bias(w->b_fc2);
  if (defer) {
    MT_STEP(MT_VBF_FC2, mt_gemm_nt_f16(b->t16, F, nullptr, w->w_fc2, M, D, F, MT_EPI_BIAS, &e, b->br16, D, nullptr, MT_OUT_F16, nullptr, s));
  } else {
    e.resid = b->hmid; e.ldr = D;
    MT_STEP(MT_VBF_FC2, mt_gemm_nt_f16(b->t16, F, nullptr, w->w_fc2, M, D, F, MT_EPI_BIAS_RESID, &e, out, D, nullptr, MT_OUT_F32, nullptr, s));
  }
  return MT_OK;
}

extern "C" int mt_vit_block_bwd(const MtVitBlockWeights* w, const MtVitBlockBuffers* b, const MtDensePlan* plan, int M, int D, int F,
                                int dh16_valid, int feeds_lower, int steps, mt_stream_t s) {
  if (!w || !b || !plan || M < 1 || D != 768) return MT_ERR_BAD_ARG;
  const MtGemmEpilogue none{};
  const mt_half* src16 = b->dh16;
  if (!dh16_valid) {
    MT_STEP(MT_VBB_CAST, mt_cast_f32_to_f16(b->dh, b->dy16, (long)M * D, nullptr, 0, s));
    src16 = b->dy16;
  }
  MT_STEP(MT_VBB_FC2, mt_gemm_nt_f16(src16, D, nullptr, w->wt_fc2, M, F, D, MT_EPI_BIAS, &none, b->dt16, F, nullptr, MT_OUT_F16, nullptr, s));
  MT_STEP(MT_VBB_GELU, mt_gelu_f16_bwd(b->a1, b->dt16, b->da1, (long)M * F, s));
  MT_STEP(MT_VBB_FC1, mt_gemm_nt_f16(b->da1, F, nullptr, w->wt_fc1, M, D, F, MT_EPI_BIAS, &none, b->dy16, D, nullptr, MT_OUT_F16, nullptr, s));
  MT_STEP(MT_VBB_LN2, mt_layernorm_bwd(b->dy16, D, nullptr, MT_OUT_F16, b->hmid, D, nullptr, MT_OUT_F32, 0, w->n2_w, b->st2, b->dh, D, nullptr,
                                       MT_OUT_F32, 1, nullptr, nullptr, b->dh16, nullptr, M, D, nullptr, s));
  MT_STEP(MT_VBB_PROJ, mt_gemm_nt_f16(b->dh16, D, nullptr, w->wt_proj, M, D, D, MT_EPI_BIAS, &none, b->u16, D, nullptr, MT_OUT_F16, nullptr, s));
  MT_STEP(MT_DENSE_BWD_ALL << MT_VBB_ATTN_SHIFT, mt_dense_attn_bwd(b->qkv, b->o16, b->u16, b->lse, plan, b->delta, b->dqkv16,
                                                                   (steps >> MT_VBB_ATTN_SHIFT) & MT_DENSE_BWD_ALL, s));
  MT_STEP(MT_VBB_QKV, mt_gemm_nt_f16(b->dqkv16, 3 * D, nullptr, w->wt_qkv, M, D, 3 * D, MT_EPI_BIAS, &none, b->dy16, D, nullptr, MT_OUT_F16, nullptr, s));
  MT_STEP(MT_VBB_LN1, mt_layernorm_bwd(b->dy16, D, nullptr, MT_OUT_F16, b->hin, D, nullptr, MT_OUT_F32, 0, w->n1_w, b->st1, b->dh, D, nullptr,
                                       MT_OUT_F32, 1, nullptr, nullptr, feeds_lower ? b->dh16 : nullptr, nullptr, M, D, nullptr, s));
  return MT_OK;
}
