"""Eval / embedding-extraction pass: the forward kernels of the train step without the backward.

Reference: train_modaltune.py:156-179 (`multitask_forward`: one model call per task id, concatenated) and
train_modaltune.py:252-327 (`get_features`: eval mode, no_grad, logits [3, 256] per case for train / val / test,
stacked on the host for the CPU-side probes).  Here the task passes of a slide are ONE batched engine call (B = len
(task_ids)) with need_grad = False (no activations are saved), optionally replayed from a captured hipGraph.
The probes themselves (sklearn LogisticRegression / lifelines Cox, TM:329-458) are host code and out of scope.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import pass_groups
from .config import attention_sites, coords_to_rowcol
from .engine import Engine, F32, flatten_genes
from .graph_cache import GraphCache


def multitask_forward(model, task_ids: Optional[Sequence[int]] = None, num_tasks: Optional[int] = None, **kwargs) -> torch.Tensor:
    """Drop-in for the trainer's `multitask_forward` (TM:156-179): logits [len(task_ids), output_dim].
    kwargs as the reference passes them: x, coords, genes, clinical."""
    if not model.is_multi:
        return model(**kwargs)
    num_tasks = num_tasks or model.cfg.multi_task
    if task_ids is None:
        task_ids = range(num_tasks)
    onehots = torch.eye(num_tasks, dtype=F32)[list(task_ids)]
    return model.forward_tasks(kwargs["x"], kwargs["coords"], kwargs["genes"], onehots, clinical=kwargs.get("clinical"))


class EmbeddingExtractor:
    """Forward-only pass over slides with static buffers + hipGraph replay per bag geometry (graph_cache.py: captured once it has
    come back `capture_after` times, up to `graph_cache_size` of them).  TITAN configuration: the gridding and its one host read-back
    (the token count) run eagerly into static buffers, the capture starts at the token gather and is keyed on (patches, TOKENS) -- as
    TrainStep.step_graphed does.

    attention: None (default: logits only), True (every site of config.attention_sites) or a list of site names -- the reference's
    module paths of the adapter attentions.  With a request, a call returns (logits, {site: map}): the head-averaged attention
    weights that a forward hook on those nn.MultiheadAttention modules reads as output[1] in the reference, computed by the same
    forward (batched, two pass groups or graph replay alike) right behind each attention core.  Not for TITAN models."""

    graph_cache_size = property(lambda o: o._cache.size, lambda o, v: setattr(o._cache, "size", int(v)))
    capture_after = property(lambda o: o._cache.capture_after, lambda o, v: setattr(o._cache, "capture_after", int(v)))

    def __init__(self, engine: Engine, task_ids: Sequence[int] = (0, 1, 2), graphed: bool = True, graph_cache_size: int = 8,
                 capture_after: int = 1, attention=None):
        self.engine, self.dev, self.graphed = engine, engine.device, graphed
        self.sites: Optional[Tuple[str, ...]] = None
        if attention is not None and attention is not False:
            engine.attention_map_shapes(1, 1)                   # (raises NotImplementedError for an engine that refuses them)
            every = attention_sites(engine.cfg)
            self.sites = tuple(every) if attention is True else tuple(attention)
            bad = [s for s in self.sites if s not in every]
            if bad or not self.sites:
                raise ValueError(f"unknown attention site(s) {bad}; this model has {every}")
        nt = max(1, engine.cfg.multi_task)
        self.onehots = torch.eye(nt, dtype=F32, device=self.dev)[list(task_ids)].contiguous()
        self._cache = GraphCache(graph_cache_size, capture_after)      # key -> SimpleNamespace(graph, out, generation)
        self._static_key = None
        self.graph_replays = 0
        self.patch_size_lv0 = 1024          # TITAN configuration only (titan_adapter.py:335)
        self.split_passes = pass_groups.split_mode() != "off"
        self.split_min_patches = pass_groups.SPLIT_MIN_PATCHES
        self._pg = pass_groups.PassGroups(engine, grad_sets=False, tapes=True)

    @property
    def _streams(self):
        return self._pg.streams or None       # (None until the first bag that ran as groups)

    def _forward_groups(self, B: int, L: int) -> torch.Tensor:
        """The forward of a long bag as two concurrent pass groups (pass_groups.py): the patch embedding once in front of the fork,
        own workspace and tape per group, logits joined behind it."""
        eng, pg = self.engine, self._pg
        groups = pass_groups.group_bounds(B)
        pg.ensure(len(groups))
        share = {}
        eng.slide_prologue(None, None, share, groups[0][1], staged_rows=L, patch_size_lv0=self.patch_size_lv0, need_grad=False)
        out = torch.empty(B, eng.cfg.output_dim, dtype=F32, device=self.dev)
        maps = eng.new_attention_maps(self.sites, B, L) if self.sites else None      # (each group writes its rows)
        pg.fork(len(groups))
        for gi, (lo, hi) in enumerate(groups):
            with pg.group(gi):
                lg = eng.forward_slide(None, None, self._sgenes, self.onehots[lo:hi], staged_rows=L, patch_size_lv0=self.patch_size_lv0,
                                       need_grad=False, clinical=self._sclin, share=share, tape=pg.tapes[gi], site_group=gi + 1,
                                       attn_maps={s: w[lo:hi] for s, w in maps.items()} if maps else None)
                out[lo:hi].copy_(lg)
        pg.join()
        return (out, maps) if maps else out

    def _forward_batched(self, B: int, L: int):
        eng = self.engine
        maps = eng.new_attention_maps(self.sites, B, L) if self.sites else None
        lg = eng.forward_slide(None, None, self._sgenes, self.onehots, staged_rows=L, patch_size_lv0=self.patch_size_lv0, need_grad=False,
                               clinical=self._sclin, attn_maps=maps)
        return (lg, maps) if maps else lg

    @property
    def _graph(self):
        """The most recently used captured graph (None while nothing is captured)."""
        live = list(self._cache.entries.values())
        return live[-1].graph if live else None

    @torch.no_grad()
    def __call__(self, x, coords, genes: Sequence[torch.Tensor], clinical=None):
        """Logits (= the slide embeddings the probes consume) [len(task_ids), output_dim], on the device (a fresh
        tensor per call: replays write a static buffer that is copied out).  With an attention request: (logits, {site: map}),
        the maps fresh tensors as well."""
        eng = self.engine
        if not eng._caches_ready:
            eng._build_caches()
        x = x.reshape(-1, x.shape[-1])
        L, B = x.shape[0], self.onehots.shape[0]
        if isinstance(genes, dict):
            genes = [genes[k] for k in sorted(genes.keys())]
        if not (self.graphed and eng.replayable):      # (or: TITAN on the module's own torch blocks: nothing to capture)
            maps = eng.new_attention_maps(self.sites, B, L) if self.sites else None
            lg = eng.forward_slide(x, coords, list(genes), self.onehots, patch_size_lv0=self.patch_size_lv0, need_grad=False,
                                   clinical=clinical, attn_maps=maps)
            return (lg, maps) if maps else lg
        gflat = flatten_genes(genes)
        # long bags: the task passes as two concurrent groups on two HIP streams, as in the train step
        split = eng.PASS_GROUPS and pass_groups.eligible(eng, B, L, self.split_min_patches, self.split_passes)
        gB = [hi - lo for lo, hi in pass_groups.group_bounds(B)] if split else [B]
        for nb in gB[1:]:
            eng._workspace(nb, L)
        # (TITAN configuration: eager gridding + the one read-back -> token count; both lines may grow the workspace: bumps eng.generation)
        Lv = eng.stage_slide(x, coords, self.patch_size_lv0, B=gB[0])
        eng._workspace(gB[0], Lv)
        skey = int(gflat.numel())
        if self._static_key != skey:
            self._static_key = skey
            self._sgenes = torch.empty(skey, dtype=F32, device=self.dev)     # one flat static buffer
            self._sclin = torch.empty(1, eng.cfg.clinfeat_dim, dtype=F32, device=self.dev) if eng.cfg.clinical else None
            self._cache.clear()
        self._sgenes.copy_(gflat, non_blocking=True)
        if self._sclin is not None:
            self._sclin.copy_(clinical.reshape(1, -1), non_blocking=True)
        # the engine's generation is part of the key: a workspace that grew under another user of the engine (the trainer
        # shares the B = 3 storage), rebuilt weight caches (load_state_dict) or a stochastic toggle retire the captures
        key = (L, Lv, eng.generation, self.sites)           # (the maps are static outputs of the capture, like the logits)
        cache = self._cache
        cache.sync(eng.generation)
        run = (lambda: self._forward_groups(B, Lv)) if split else (lambda: self._forward_batched(B, Lv))
        ent = cache.get(key)
        if ent is None:
            if not cache.admit(key):
                return run()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=cache.pool_for(g), capture_error_mode="thread_local"):
                out = run()
            ent = SimpleNamespace(graph=g, out=out, generation=key[2])
            cache.put(key, ent)
        ent.graph.replay()
        self.graph_replays += 1
        if self.sites:
            lg, maps = ent.out
            return lg.clone(), {s: w.clone() for s, w in maps.items()}
        return ent.out.clone()


def attention_to_grid(weights, coords, tile: float = 256.0) -> np.ndarray:
    """One attention map over the patches of a slide (weights [L]: a row of an extractor map, or an injector map's column for one
    token) laid out on the slide's patch grid: cell (row, col) = config.coords_to_rowcol(coords, tile) -- the grid the positional
    embedding uses (slide_encoder.py:198-211) -- with NaN where there is no patch, and the mean where several patches share a cell.
    Returns a float64 array [max row + 1, max col + 1] (host only; plt.imshow draws it as the heatmap)."""
    w = weights.detach().double().cpu().numpy() if torch.is_tensor(weights) else np.asarray(weights, dtype=np.float64)
    c = coords.detach().cpu().numpy() if torch.is_tensor(coords) else np.asarray(coords)
    w, c = w.reshape(-1), c.reshape(-1, 2)
    if w.shape[0] != c.shape[0]:
        raise ValueError(f"{w.shape[0]} weights for {c.shape[0]} patch coordinates")
    if w.shape[0] == 0:
        return np.zeros((0, 0))
    r, col = coords_to_rowcol(c, float(tile))
    if int(min(r.min(), col.min())) < 0:
        raise ValueError("negative patch coordinates")
    shape = (int(r.max()) + 1, int(col.max()) + 1)
    tot, cnt = np.zeros(shape), np.zeros(shape)
    np.add.at(tot, (r, col), w)
    np.add.at(cnt, (r, col), 1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, tot / cnt, np.nan)


def get_features(extractor: EmbeddingExtractor, slides: Iterable[Dict]) -> Tuple[np.ndarray, List]:
    """Host-side collection as TM:262-327 does per split: returns (features [n, tasks, O], case ids).  `extractor`: an
    EmbeddingExtractor, or slide_encoder.BaselineFeatures for the plain slide encoder's features [n, 768] of the same slide dicts."""
    feats, ids = [], []
    for s in slides:
        feats.append(extractor(s["x"], s["coords"], s["genes"], s.get("clinical")).float().cpu().numpy())
        ids.append(s.get("case_id"))
    extractor.engine.check_inputs()       # the host has just synchronised on every slide's logits: raise for bad coords now
    return np.stack(feats) if feats else np.zeros((0,)), ids
