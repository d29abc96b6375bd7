"""The plain Prov-GigaPath slide encoder -- `LongNetViT.forward(x, coords, all_layer_embed=False)` of the reference
(models/prov_gigapath/gigapath/slide_encoder.py:213-290; SE below) -- on the HIP kernels: no adapters, no genes, no task tokens.
It is the "linear-probed SLFM" baseline of the ModalTune tables and the published API of Prov-GigaPath:

    from modaltune_amd import slide_encoder                      # instead of: from gigapath import slide_encoder
    model = slide_encoder.create_model("hf_hub:prov-gigapath/prov-gigapath", "gigapath_slide_enc12l768d", 1536).eval()
    outcomes = model(tile_embeds, coords)                        # list of [N, 768]

The patch embedding with its sin-cos epilogue, the cls row, the dilated plan and the layers' launch list (mt_longnet_layer_fwd, cut at
out_proj through its `steps` so that the fp32 stream is never rounded: _launch) are the adapter path's own code (Engine.stage_inputs /
_embed_patches / _attention_plan / _build_caches); what is new is the read-out, one mt_layernorm_pool_fwd launch per returned state
(include/modaltune_hip.h):

    single output (ENC:425-426, SE:279-285)   cls:  norm(encoder.layer_norm(x)[0])          pool: norm(mean_{1..L} encoder.layer_norm(x)[r])
    all_layer_embed (ENC:400-422)             cls:  norm(x_s[0])                            pool: norm(mean x_s[1:])     s = 0 .. depth

`norm` carries eps 1e-6 (SE:368-377), encoder.layer_norm the encoder's 1e-5.  Inference only: the reference draws Dropout / DropPath
in training mode, here a forward in training mode raises; every parameter is frozen (fine-tuning the backbone is refused where
freeze_vit=False is, config.ModelConfig.validate).
"""
from __future__ import annotations

import os
from collections import OrderedDict
from types import SimpleNamespace
from typing import Dict, Iterator, List, Optional, Tuple

import torch
import torch.nn as nn

from . import init, ops
from ._lib import rowmap
from .config import GEOMETRY_MSG, ModelConfig
from .engine import Engine, F32, H16
from .graph_cache import GraphCache
from .synth import param_specs

NORM_EPS = 1e-6             # `norm` of gigapath_slide_enc12l768d (SE:368-377: partial(nn.LayerNorm, eps=1e-6))
# Equal-length bags ride on the pass axis; a chunk holds at most this many token rows (twice the largest B * N the train step is
# measured at, far below the 2^31 elements of the kernels' 32-bit row arithmetic at 3072 columns) -- one bag of any length is its own chunk.
MAX_CHUNK_ROWS = 1 << 16


def _frozen_specs(cfg: ModelConfig, group_sizes=()):
    """The reference LongNetViT's tensors: the frozen entries of the adapter model's state dict (synth.param_specs)."""
    return [s for s in param_specs(cfg, list(group_sizes)) if not s[3]]


class BackboneEngine(Engine):
    """An Engine over the frozen LongNetViT tensors alone (no adapter, gene or head weights exist): weight caches, input staging,
    patch embedding and plans are the parent's; the adapter forward is not available."""
    PARAM_SPECS = staticmethod(_frozen_specs)
    DETERMINISTIC_REFUSAL = None

    def _cross_attn_prefixes(self) -> List[str]:
        return []

    def forward(self, *a, **k):
        raise NotImplementedError("this engine holds the plain slide encoder's tensors only: run it through slide_encoder.LongNetViT")


class LongNetViT(nn.Module):
    """Constructor keywords as the reference's LongNetViT.__init__ (SE:87-103); `device`, `init_seed`, `graphed`, `capture_after` and
    `graph_cache_size` belong to this port.  `engine`: run over an existing engine's frozen tensors (LongNetGeneAdapter.slide_encoder())
    instead of tensors of its own."""

    def __init__(self, in_chans=1536, embed_dim=256, depth=12, slide_ngrids=1000, tile_size=256, max_wsi_size=262144, norm_layer=None,
                 global_pool=False, dropout=0.25, drop_path_rate=0.1, return_feats=False, lora_adapter=False, lora_args=None, *,
                 device="cuda", init_seed: Optional[int] = None, graphed: bool = True, capture_after: int = 1, graph_cache_size: int = 8,
                 engine: Optional[Engine] = None, **kwargs):
        super().__init__()
        if int(embed_dim) != 768 or float(kwargs.get("mlp_ratio", 4)) != 4.0:
            raise NotImplementedError(f"embed_dim={embed_dim}, mlp_ratio={kwargs.get('mlp_ratio', 4)}: " + GEOMETRY_MSG)
        if lora_adapter:
            raise NotImplementedError("lora_adapter=True: the backbone is frozen here (fine-tuning it is refused, as freeze_vit=False is)")
        self.depth, self.embed_dim, self.drop_path_rate, self.return_feats = int(depth), int(embed_dim), drop_path_rate, bool(return_feats)
        self.slide_ngrids, self.global_pool = int(slide_ngrids), bool(global_pool)
        self.encoder_name = "LongNet_{}_layers_{}_dim".format(depth, embed_dim)      # (SE:122)
        if engine is None:
            cfg = ModelConfig(in_chans=int(in_chans), embed_dim=768, depth=self.depth, slide_ngrids=self.slide_ngrids, tile_size=int(tile_size),
                              max_wsi_size=int(max_wsi_size), global_pool=self.global_pool, dropout=float(dropout),
                              drop_path_rate=float(drop_path_rate), interaction_indexes=((0, self.depth - 1),), pretrained=False)
            engine = BackboneEngine(cfg, [], device, deterministic=False)
            state = init.init_state_dict(cfg, [], init_seed)
            engine.load_state_dict({k: state[k] for k, _, _, _ in engine.store.specs})
        elif type(engine)._attention_plan is not Engine._attention_plan or type(engine)._embed_patches is not Engine._embed_patches:
            raise NotImplementedError("the plain slide encoder runs over a LongNet backbone: this engine has another one")
        self.engine, self.cfg = engine, engine.cfg
        self._keys = [k for k, _, _, train in engine.store.specs if not train]
        self._params: "OrderedDict[str, nn.Parameter]" = OrderedDict(
            (k, nn.Parameter(engine.store.tensors[k], requires_grad=False)) for k in self._keys)
        self.graphed = bool(graphed)
        self._cache = GraphCache(graph_cache_size, capture_after)
        self._ws: Dict[int, dict] = {}      # passes -> {cap, flat buffers}
        self._gen = 0                       # bumped when a buffer captured graphs point to is replaced
        self.graph_replays = 0
        self.pretrained_report: Tuple[list, list] = ([], [])

    capture_after = property(lambda o: o._cache.capture_after, lambda o, v: setattr(o._cache, "capture_after", int(v)))
    graph_cache_size = property(lambda o: o._cache.size, lambda o, v: setattr(o._cache, "size", int(v)))

    # ---- parameter / state_dict surface under the reference's key names (pos_embed is a non-persistent buffer there: derived here)
    def named_parameters(self, prefix: str = "", recurse: bool = True, remove_duplicate: bool = True) -> Iterator[Tuple[str, nn.Parameter]]:
        for k, p in self._params.items():
            yield (prefix + ("." if prefix else "") + k, p)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = destination if destination is not None else OrderedDict()
        for k, p in self._params.items():
            out[prefix + k] = p if keep_vars else p.detach()
        return out

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        missing = [k for k in self._keys if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._params and k != "pos_embed"]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for {}: missing keys {}, unexpected keys {}".format(
                type(self).__name__, missing, unexpected))
        self.engine.load_state_dict({k: v for k, v in state_dict.items() if k in self._params}, strict=False)
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def requires_grad_(self, requires_grad: bool = True):
        if requires_grad:
            raise NotImplementedError("the plain slide encoder is inference-only: its parameters stay frozen (freeze_vit=False is refused)")
        return self

    def _apply(self, fn, recurse=True):
        """.to() / .cuda() / .float(): a no-op for the device and dtype the tensors already have, refused otherwise (as the adapter module)."""
        probe = fn(torch.empty(0, dtype=F32, device=self.engine.device))
        want, have = torch.device(probe.device), self.engine.device
        if want.type != have.type or probe.dtype != F32 or (want.index is not None and have.index is not None and want.index != have.index):
            raise RuntimeError(f"this model lives on {have} in fp32 masters (the `device=` argument of its constructor); it cannot be "
                               f"converted to {want} / {probe.dtype}")
        return self

    def load_slide_encoder(self, pretrained=False, weights_location: Optional[str] = None):
        """SE:292-322: `{weights_location}/slide_encoder.pth`, non-strict; a missing file leaves the random init and says so."""
        state = {k: p.detach() for k, p in self._params.items()}
        self.pretrained_report = init.load_slide_encoder(state, self._keys, bool(pretrained), weights_location)
        if pretrained and len(self.pretrained_report[0]) < len(self._keys):
            self.engine.load_state_dict(state, strict=False)

    # ---- workspace: ONE set of layer buffers (nothing is saved for a backward), two residual-stream buffers
    def _spec(self, B: int, Lx: int) -> Dict[str, tuple]:
        cfg, eng = self.cfg, self.engine
        D, Fd, nb, N = cfg.embed_dim, cfg.ffn_dim, len(eng.seg_lengths), Lx + 1
        M, Mp = B * N, B * Lx
        sp = {"x16": (H16, (Mp, cfg.in_chans)), "x0": (F32, (Mp, D)), "prow": (torch.int32, (Mp,)), "pcol": (torch.int32, (Mp,)),
              "h0": (F32, (M, D)), "h1": (F32, (M, D)), "hmid": (F32, (M, D)), "qkv": (H16, (M, 3 * D)), "obr": (H16, (nb, M, D)),
              "lsebr": (F32, (nb, M, 16)), "lsetot": (F32, (M, 16)), "a1": (H16, (M, Fd)), "t16": (H16, (M, Fd)), "u16": (H16, (M, D)),
              "br16": (H16, (M, D)), "outs": (F32, (cfg.depth + 1, B, D)),
              "pool": (torch.float64, (max(1, ops.layernorm_pool_partials_elems(B, max(1, Lx), D)),))}
        for st in ("st1", "stin", "st2", "stf"):
            sp[st] = (F32, (M, 2))
        return sp

    def _workspace(self, B: int, L: int) -> Dict[str, torch.Tensor]:
        """Views, at bag length L, of the flat buffers of B passes (sized for the largest bag seen, grown by >= 25 %)."""
        def numel(shape):
            n = 1
            for d in shape:
                n *= d
            return n
        store = self._ws.get(B)
        if store is None or L > store["cap"]:
            cap = L if store is None else max(L, store["cap"] + store["cap"] // 4)
            store = self._ws[B] = {"cap": cap, "views": {}, "flat": {k: torch.empty(numel(shape), dtype=dt, device=self.engine.device)
                                                                    for k, (dt, shape) in self._spec(B, cap).items()}}
            self._gen += 1                  # graphs captured on the old buffers are stale
        w = store["views"].get(L)
        if w is None:
            if len(store["views"]) > 64:
                store["views"].clear()
            w = {k: store["flat"][k][:numel(shape)].view(shape) for k, (dt, shape) in self._spec(B, L).items()}
            # the layer's buffer table (include/modaltune_hip.h: MtLongNetLayerBuffers; the backward's entries stay null), per input buffer
            for i in (0, 1):
                w[("cb", i)] = ops.struct_of(ops.MtLongNetLayerBuffers, hin=w[f"h{i}"], hmid=w["hmid"], qkv=w["qkv"], o_br=w["obr"],
                                             lse_br=w["lsebr"], lse_tot=w["lsetot"], a1=w["a1"], st1=w["st1"], stin=w["stin"], st2=w["st2"],
                                             stf=w["stf"], u16=w["u16"], br16=w["br16"], t16=w["t16"])
            store["views"][L] = w
        return w

    # ---- the launch list of one chunk of B equal-length bags (staged in ws): embedding, cls row, depth layers, read-outs
    def _readout(self, state: torch.Tensor, ws, k: int, B: int, N: int, pre: bool):
        t = self.engine.store.tensors
        r0, r1 = (1, N) if self.global_pool else (0, 1)
        ops.layernorm_pool_fwd(state, B, N, r0, r1, ws["outs"][k], pre=(t["encoder.layer_norm.weight"], t["encoder.layer_norm.bias"]) if pre else None,
                               post=(t["norm.weight"], t["norm.bias"]), post_eps=NORM_EPS, partials=ws["pool"], D=self.cfg.embed_dim)

    def _launch(self, ws, B: int, L: int, all_layers: bool):
        eng, cfg = self.engine, self.cfg
        N, D, Fd, depth = L + 1, cfg.embed_dim, cfg.ffn_dim, cfg.depth
        M = B * N
        t = eng.store.tensors
        Engine._embed_patches(eng, None, None, ws, True, B * L)                               # SE:227-232 for the B bags at once
        h = ws["h0"]
        ops.copy_rows(eng._cls_source().view(1, D), h, B, D, smap=rowmap(1, 0, 0), dmap=rowmap(1, N, 0))      # SE:235-240
        ops.copy_rows(ws["x0"], h, B * L, D, smap=rowmap(L, L, 0), dmap=rowmap(L, N, 1))
        plan = eng._attention_plan(N, B)
        # The fp32 stream is never rounded: the adapter path adds both branches of a layer through fp16 copies (out_proj's on the second
        # LayerNorm, mt_add_layernorm_fwd; an inner layer's fc2 on the next layer's first one, Engine._layer defer=True) -- two
        # roundings on rows that, like the cls row, consist of branch outputs almost entirely.  Here the outcome is all there is:
        # the layer's launch list is cut at out_proj (its `steps`), out_proj writes hmid = hin + branch with the fp32 residual
        # epilogue fc2 uses, a plain LayerNorm follows, and fc2 writes the stream itself; the layers alternate between the two stream
        # buffers.  Launch for launch the same count, and the last hidden state of all_layer_embed is bit for bit the state the
        # single output is read from.
        if all_layers:
            self._readout(h, ws, 0, B, N, pre=False)                                          # ENC:400-403: the embedded input
        for l in range(depth):
            p, cb, hin = f"encoder.layers.{l}.", ws[("cb", l % 2)], h
            h = ws[f"h{(l + 1) % 2}"]
            ops.longnet_layer_fwd(eng._layer_w[l], cb, plan, M, D, Fd, h, steps=ops.LNF_ATTENTION)
            ops.gemm_nt(ws["u16"], eng._frozen16[p + "out"].w, ws["hmid"], M, D, D, epilogue=ops.EPI_BIAS_RESID,
                        bias=t[p + "self_attn.out_proj.bias"], resid=hin, ldr=D)
            ops.layernorm_fwd(ws["hmid"], t[p + "final_layer_norm.weight"], t[p + "final_layer_norm.bias"], ws["u16"], ws["st2"], M, D)
            ops.longnet_layer_fwd(eng._layer_w[l], cb, plan, M, D, Fd, h, steps=ops.LNF_FFN)
            if all_layers:      # read out right behind the launch that wrote the state (ENC:420-422): nothing is kept for it
                self._readout(h, ws, l + 1, B, N, pre=False)
        if all_layers:
            return ws["outs"], (h.view(B, N, D).clone() if self.return_feats else None)
        self._readout(h, ws, 0, B, N, pre=True)                                               # ENC:425-426 + SE:279-285 in one launch
        feats = None
        if self.return_feats:                                                                 # x_list[-1] = encoder_out: encoder.layer_norm applied
            feats = torch.empty(B, N, D, dtype=F32, device=eng.device)
            ops.layernorm_fwd(h, t["encoder.layer_norm.weight"], t["encoder.layer_norm.bias"], feats, None, M, D)
        return ws["outs"][:1], feats

    def _run_chunk(self, x: torch.Tensor, coords, all_layers: bool):
        """x [B, L, C], coords [B, L, 2] -> (outcomes [K, B, D], feats [B, L + 1, D] or None), fresh tensors."""
        eng = self.engine
        B, L = int(x.shape[0]), int(x.shape[1])
        if eng.store.sync is not None:
            eng.store.sync()
        if not eng._caches_ready:
            eng._build_caches()
        ws = self._workspace(B, L)
        eng.stage_inputs(x.reshape(B * L, x.shape[-1]), coords.reshape(B * L, 2), ws)
        if not self.graphed:
            outs, feats = self._launch(ws, B, L, all_layers)
            return outs.clone(), feats
        cache, gen = self._cache, (eng.generation, self._gen)
        key = (B, L, bool(all_layers), self.global_pool, self.return_feats, gen)
        cache.sync(gen)
        ent = cache.get(key)
        if ent is None:
            if not cache.admit(key):
                outs, feats = self._launch(ws, B, L, all_layers)
                return outs.clone(), feats
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=cache.pool_for(g), capture_error_mode="thread_local"):
                out = self._launch(ws, B, L, all_layers)
            ent = SimpleNamespace(graph=g, out=out, generation=gen)
            cache.put(key, ent)
        ent.graph.replay()
        self.graph_replays += 1
        outs, feats = ent.out
        return outs.clone(), (feats.clone() if feats is not None else None)

    @torch.no_grad()
    def forward(self, x, coords, all_layer_embed: bool = False):
        """x [N, L, C] (or [L, C]) tile embeddings, coords [N, L, 2] (or [L, 2]) -> list of [N, 768] fp32 outcomes: one, or with
        all_layer_embed depth + 1 (the embedded input first).  return_feats: (outcomes, x_list[-1] [N, L + 1, 768])."""
        if self.training:
            raise RuntimeError("the plain slide encoder is inference-only: in training mode the reference draws Dropout / DropPath "
                               "(SE:128-135); call .eval() first")
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[-1] != self.cfg.in_chans:
            raise ValueError(f"x must be [N, L, {self.cfg.in_chans}] or [L, {self.cfg.in_chans}], got {tuple(x.shape)}")
        Nb, L = int(x.shape[0]), int(x.shape[1])
        if Nb < 1 or L < 1:
            raise ValueError(f"empty input: {Nb} bags of {L} tile embeddings")
        coords = coords if torch.is_tensor(coords) else torch.as_tensor(coords)
        coords = coords.reshape(Nb, L, 2)
        per = max(1, MAX_CHUNK_ROWS // (L + 1))
        outs, feats = [], []
        for lo in range(0, Nb, per):
            o, f = self._run_chunk(x[lo:lo + per], coords[lo:lo + per], bool(all_layer_embed))
            outs.append(o)
            feats.append(f)
        o = outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)
        outcomes = [o[k] for k in range(o.shape[0])]
        if self.return_feats:
            return outcomes, (feats[0] if len(feats) == 1 else torch.cat(feats, dim=0))
        return outcomes


ARCHS = {"gigapath_slide_enc12l768d": dict(embed_dim=768, depth=12, mlp_ratio=4),
         "gigapath_slide_enc24l1024d": dict(embed_dim=1024, depth=24, mlp_ratio=4),
         "gigapath_slide_enc12l1536d": dict(embed_dim=1536, depth=12, mlp_ratio=4)}


def gigapath_slide_enc12l768d(**kwargs) -> LongNetViT:
    """SE:368-377 (`norm` with eps 1e-6); `depth=` builds the same class at another depth."""
    kw = dict(ARCHS["gigapath_slide_enc12l768d"])
    kw.update(kwargs)
    return LongNetViT(**kw)


def create_model(pretrained: str, model_arch: str, in_chans: int, local_dir: str = os.path.join(os.path.expanduser("~"), ".cache/"),
                 **kwargs) -> LongNetViT:
    """SE:325-365: build `model_arch` and load `{local_dir}/slide_encoder.pth` (its "model" entry, non-strictly) if it exists; a
    missing file leaves the random init and says so.  (`pretrained` only names the source, as in the reference, whose hub download is
    commented out.)"""
    if model_arch not in ARCHS:
        raise RuntimeError(f"Unknown model ({model_arch})")
    kw = dict(ARCHS[model_arch])
    kw.update(kwargs)
    model = LongNetViT(in_chans=in_chans, **kw)      # (1024-d / 1536-d: NotImplementedError with the geometry message)
    model.load_slide_encoder(True, local_dir)
    return model


class BaselineFeatures:
    """The callable evaluate.get_features takes, for the linear-probe baseline: `extractor(x, coords, genes, clinical)` -> the plain
    slide encoder's outcome [768] of the slide (genes / clinical are ignored), so the same slide dicts give ModalTune and baseline
    features.  layer: which outcome (-1: the last; with all_layer_embed, an index into the depth + 1 states)."""

    def __init__(self, model: LongNetViT, all_layer_embed: bool = False, layer: int = -1):
        self.model, self.engine, self.all_layer_embed, self.layer = model, model.engine, bool(all_layer_embed), int(layer)

    def __call__(self, x, coords, genes=None, clinical=None) -> torch.Tensor:
        out = self.model(x.reshape(1, -1, x.shape[-1]), coords, all_layer_embed=self.all_layer_embed)
        out = out[0] if self.model.return_feats else out
        return out[self.layer][0]
