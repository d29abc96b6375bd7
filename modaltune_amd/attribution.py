"""Integrated Gradients over the gene inputs (the reference's README Figure 3, second half: "the top pathways influencing risk") and
over the patch embeddings of the slide (which patches move a task's embedding along a probe direction, and how much of
F(x, genes) - F(baseline) each modality carries).

IG_t[k] = (genes[k] - baseline[k]) * integral_0^1 dF_t/dgenes[k] (baseline + a (genes - baseline)) da  for the scalar
F_t = <target_t, logits_t> on the raw logits of task t -- what the reference's linear probes (LogReg / Cox coefficients on the
embeddings) compute.  Every gradient evaluation is a full forward and activation-gradient backward through the frozen backbone (the
Injector feeds the gene tokens into every patch row), so the quadrature points ride on the engine's PASS axis: one engine pass
evaluates `points_per_pass` points, the pathway weights are streamed once for all of them (mt_gene_snn_fwd_points), and the input
gradient is written by a kernel that touches no parameter-gradient slot (mt_gene_snn_bwd_input).

The patch side needs no gradient at the 1536 input channels: the patch embedding is affine, x0_l = W x_l + b + pos_l, and F depends on
x only through x0, so on the straight path x(a) = base + a (x - base) the embedded rows are e_base,l + a (e_x,l - e_base,l) (b and pos
cancel in the difference) and the per-patch attribution is

    sum_c IG[l, c] = < e_x,l - e_base,l , integral_0^1 dF/dx0_l (a) da >

-- both bags are embedded once (Engine.prepare_shared), the points are interpolated per pass in the embedding space
(mt_patch_points_fwd) and the gradient that the backward leaves at block 0's input becomes a weighted row dot (mt_patch_ig_accumulate).

The reference side is a captum loop over a model whose gene tensors require grad; here it is one call:

    res = model.integrated_gradients(x, coords, genes, target=w)          # or IntegratedGradients(engine)(...)
    bars = top_pathways(res, pathway_names, task=0, k=10)
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .engine import Engine, F32, GenePoints, PatchPoints, flatten_genes

INPUTS = ("genes", "patches", "both")


class IntegratedGradients:
    """Midpoint rule with `steps` points a_k = (k + 1/2) / steps, weights 1 / steps, `points_per_pass` of them per engine pass
    (ceil((steps + 2) / points_per_pass) passes per task: two weight-0 slots carry a = 0 and a = 1, so F(baseline) and F(genes) come
    out of the same passes; spare slots carry weight 0).

    inputs: which modality walks the path -- "genes" (the patches stay at the slide's), "patches" (the genes stay at their values; the
    baseline bag is `patch_baseline`, zeros by default) or "both" (one straight path through both).  With patches on the path the result
    has `patches` [tasks, L] (the attribution of each patch, summed over its input channels) and `patches_total` [tasks];
    `convergence_delta` is the sum of the attributions of every modality on the path minus `delta`.

    A call leaves the engine as it found it: the adapters' weight gradients that the backward still computes go into a scratch
    gradient set of this object's own, tape and workspace are the call's own, no Dropout / DropPath site runs and none of their
    counters moves, and `engine.generation` stays -- graphs that a TrainStep or an EmbeddingExtractor captured on the engine replay
    afterwards as before.  Nothing inside the loop waits for the device; ONE finiteness check at the end reads a flag back."""

    def __init__(self, engine: Engine, task_ids: Sequence[int] = (0, 1, 2), steps: int = 64, points_per_pass: int = 3,
                 inputs: str = "genes"):
        engine.refuse("integrated_gradients")
        if inputs not in INPUTS:
            raise ValueError(f"inputs must be one of {INPUTS}, got {inputs!r}")
        if inputs != "genes" and engine.cfg.first_interaction_layer != 0:
            raise NotImplementedError("Integrated Gradients over the patches: first_interaction_layer > 0 is not supported (the layers in "
                                      "front of the first interaction run forward-only)")
        self.inputs = inputs
        steps, P = int(steps), int(points_per_pass)
        if steps < 1:
            raise ValueError(f"steps must be >= 1, got {steps}")
        if not 1 <= P <= ops.GENE_POINTS_MAX:
            raise ValueError(f"points_per_pass must be 1..{ops.GENE_POINTS_MAX}, got {P}")
        cfg = engine.cfg
        self.task_ids = tuple(int(t) for t in task_ids) if cfg.is_multi else (0,)
        nt = max(1, int(cfg.multi_task))
        if not self.task_ids or any(not 0 <= t < nt for t in self.task_ids):
            raise ValueError(f"task_ids {tuple(task_ids)} outside 0..{nt - 1}")
        self.engine, self.steps, self.points_per_pass = engine, steps, P
        dev = engine.device
        # slots: [a = 0 (weight 0), a = 1 (weight 0), the midpoints, padding (a = 0, weight 0)] in passes of P
        self.passes = -(-(steps + 2) // P)
        al = np.zeros(self.passes * P, dtype=np.float32)
        w = np.zeros(self.passes * P, dtype=np.float32)
        al[1] = 1.0
        al[2:2 + steps] = ((np.arange(steps, dtype=np.float64) + 0.5) / steps).astype(np.float32)
        w[2:2 + steps] = np.float32(1.0 / steps)
        self._alphas = torch.from_numpy(al).to(dev).view(self.passes, P)
        self._weights = torch.from_numpy(w).to(dev).view(self.passes, P)
        self._onehots = [torch.eye(nt, dtype=F32, device=dev)[t:t + 1].repeat(P, 1).contiguous() if cfg.is_multi
                         else torch.zeros(P, 1, dtype=F32, device=dev) for t in self.task_ids]
        self._scratch = None          # (flat, views): where the adapters' weight gradients of the IG passes go
        self._found_inf = torch.zeros(1, dtype=torch.int32, device=dev)

    # ------------------------------------------------------------------ argument checks (before any launch)
    def _target(self, target) -> torch.Tensor:
        eng, nT = self.engine, len(self.task_ids)
        O = int(eng.cfg.output_dim)
        if not torch.is_tensor(target):
            target = torch.as_tensor(np.asarray(target, dtype=np.float32))
        if tuple(target.shape) == (O,):
            target = target.reshape(1, O).expand(nT, O)
        if tuple(target.shape) != (nT, O):
            raise ValueError(f"target: expected [{nT}, {O}] or [{O}], got {tuple(target.shape)}")
        return target.to(eng.device, F32).contiguous()

    def _flat(self, v, what: str) -> torch.Tensor:
        eng = self.engine
        flat = flatten_genes(v).to(eng.device, F32).contiguous()
        if flat.numel() != eng._gene_total:
            raise ValueError(f"{what}: expected {eng._gene_total} gene values in {len(eng.group_sizes)} groups, got {flat.numel()}")
        return flat

    def _patch_baseline(self, x, patch_baseline) -> torch.Tensor:
        C = int(self.engine.cfg.in_chans)
        if not torch.is_tensor(x) or x.shape[-1] != C or x.numel() < C:
            raise ValueError(f"x: expected a tensor [L, {C}], got {tuple(x.shape) if torch.is_tensor(x) else type(x)}")
        L = x.numel() // C
        if patch_baseline is None:
            return torch.zeros(L, C, dtype=x.dtype, device=x.device)
        if not torch.is_tensor(patch_baseline):
            patch_baseline = torch.as_tensor(np.asarray(patch_baseline, dtype=np.float32))
        if patch_baseline.shape[-1] != C or patch_baseline.numel() != L * C:
            raise ValueError(f"patch_baseline: expected [{L}, {C}], got {tuple(patch_baseline.shape)}")
        return patch_baseline.reshape(L, C)

    def __call__(self, x, coords, genes, target, baseline=None, clinical=None, patch_baseline=None) -> Dict[str, torch.Tensor]:
        eng, P, nT = self.engine, self.points_per_pass, len(self.task_ids)
        dev, G, n = eng.device, len(eng.group_sizes), eng._gene_total
        on_genes, on_patches = self.inputs != "patches", self.inputs != "genes"
        if on_patches:
            patch_baseline = self._patch_baseline(x, patch_baseline)
        elif patch_baseline is not None:
            raise ValueError('patch_baseline: the patches are not on the path (inputs="patches" or "both")')
        if baseline is not None and not on_genes:
            raise ValueError('baseline: the genes are not on the path (inputs="genes" or "both")')
        if not torch.is_tensor(genes) and len(genes) != G:
            raise ValueError(f"expected {G} gene groups, got {len(genes)}")
        target = self._target(target)
        gflat = self._flat(genes, "genes")
        base = None if baseline is None else self._flat(baseline, "baseline")
        if eng.cfg.clinical and clinical is None:
            raise ValueError("this model variant needs `clinical` features [1, clinfeat_dim]")
        O = int(target.shape[1])
        st = eng.store
        if self._scratch is None:
            self._scratch = st.new_grad_set()
        self._scratch[0].zero_()
        dgenes = torch.zeros(nT, n, dtype=F32, device=dev)
        fvals = torch.empty(nT, self.passes * P, dtype=F32, device=dev)
        scale = torch.empty(nT, 2, dtype=F32, device=dev)
        seed = torch.empty(P, O, dtype=F32, device=dev)
        attr = torch.empty(nT, n, dtype=F32, device=dev)
        pathway = torch.empty(nT, G, dtype=F32, device=dev)
        # the task-independent patch embedding: once per call, in buffers of its own, read by every pass.  (Each pass gets its own
        # dict around it: a fresh call parks its workspace lease there, and a lease held for the whole call would keep one workspace
        # per pass alive.)
        share: dict = {}
        eng.prepare_shared(x, coords, share)
        share_b: dict = {}
        if on_patches:                # the embedded baseline bag: once per call, too
            eng.prepare_shared(patch_baseline, coords, share_b)
            L = int(share["x0"].shape[0])
            dpatch = torch.zeros(nT, L, dtype=F32, device=dev)
        old = st.use_grad_set(*self._scratch)
        hook, eng.grad_ready_hook = eng.grad_ready_hook, None          # (a TrainStep sharing the engine must not see these passes)
        try:
            for ti in range(nT):
                # the fp16 activation-gradient stream wants a seed of max |.| = 2^10: scaled on the device as the module bridge does it,
                # the reciprocal goes to the input-gradient kernel
                ops.absmax_scale(target[ti], scale[ti], 1024.0)
                for p in range(P):
                    ops.axpy_dev(None, target[ti], scale[ti, 0:1], seed[p])
                for q in range(self.passes):
                    pts = GenePoints(base, self._alphas[q], self._weights[q], dgenes[ti], unscale=scale[ti, 1:2]) if on_genes else None
                    ppts = PatchPoints(share_b["x0"], self._alphas[q], self._weights[q], dpatch[ti], unscale=scale[ti, 1:2]) \
                        if on_patches else None
                    logits = eng.forward(x, coords, gflat, self._onehots[ti], need_grad=True, fresh=True, clinical=clinical,
                                         share={"x0": share["x0"]},
                                         points=pts, stochastic=False, patch_points=ppts)
                    call = eng.last_call
                    # F_t at the P points of this pass: logits [P, O] . target_t
                    ops.sgemm(logits, (O, 1), target[ti], (O, 1), fvals[ti, q * P:(q + 1) * P], (1, 1), P, 1, O)
                    eng.backward(seed.clone(), call=call)          # (the tape may hand the seed's storage on as a gradient)
                    del call, logits
                if on_genes:
                    ops.ig_finalize(gflat, base, dgenes[ti], eng._gene_sizes, eng._gene_goff, G, attr[ti], pathway[ti])
        finally:
            eng.grad_ready_hook = hook
            st.use_grad_set(*old)
            share.clear()
            share_b.clear()
        self._found_inf.zero_()
        if on_genes:
            ops.check_finite(attr, attr.numel(), self._found_inf)
        if on_patches:
            ops.check_finite(dpatch, dpatch.numel(), self._found_inf)
        ops.check_finite(fvals, fvals.numel(), self._found_inf)
        if int(self._found_inf) != 0:          # the call's one host sync
            raise RuntimeError("Integrated Gradients: non-finite attribution or logit (an overflow of the fp16 activation-gradient stream, "
                               "or non-finite inputs)")
        f_base, f_in = fvals[:, 0].clone(), fvals[:, 1].clone()
        delta = f_in - f_base
        if not on_patches:
            return {"attributions": attr, "offsets": eng._gene_goff.clone(), "pathway": pathway, "f_input": f_in, "f_baseline": f_base,
                    "delta": delta, "convergence_delta": pathway.sum(1) - delta, "steps": self.steps}
        total = dpatch.sum(1)         # (one reduction kernel over a fixed shape: a fixed order)
        res = {"patches": dpatch, "patches_total": total, "f_input": f_in, "f_baseline": f_base, "delta": delta, "steps": self.steps}
        if on_genes:
            res.update(attributions=attr, offsets=eng._gene_goff.clone(), pathway=pathway)
            res["convergence_delta"] = (pathway.sum(1) + total) - delta
        else:
            res["convergence_delta"] = total - delta
        return res


def top_pathways(result: Dict[str, torch.Tensor], names: Sequence[str], task: int, k: int = 10) -> List[Tuple[str, float]]:
    """The `k` pathways with the largest |attribution| for row `task` of `result["pathway"]`, as (name, value) sorted by |value|,
    largest first: the bars of the reference's "top 10 pathways" figure."""
    vals = result["pathway"][task].detach().cpu().numpy().astype(np.float64)
    if len(names) != vals.shape[0]:
        raise ValueError(f"{len(names)} names for {vals.shape[0]} pathways")
    order = np.argsort(-np.abs(vals), kind="stable")[:max(0, int(k))]
    return [(str(names[i]), float(vals[i])) for i in order]
