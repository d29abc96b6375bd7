"""CPU: the plain slide encoder's surface (modaltune_amd/slide_encoder.py) and the oracle restatement of its forward
(tests/slide_encoder_ref.py) against the reference's own outcomes (tests/golden/slide_encoder_L*.npz, make_golden_slide_encoder.py)."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import slide_encoder_ref as R
from modaltune_amd import slide_encoder as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_THREADS = 8          # (as tests/test_oracle_golden.py: MKL's fp64 rounding depends on the thread count)


@pytest.fixture(autouse=True)
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(ORACLE_THREADS)
    yield
    torch.set_num_threads(n)


def _maxrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.mark.parametrize("L", [37, 513, 1500])
def test_oracle_composition_equals_the_reference(golden_dir, L):
    """pos_embed_rows + encoder_layer + _ln, composed as LongNetViT.forward composes them, in fp64: every outcome of every mode and the
    head of the return_feats state, at the 1e-9 level of test_oracle_golden.py.  (L = 1500: two segments in the 1 024 branch; L = 37: N = 2.)"""
    g = np.load(os.path.join(golden_dir, f"slide_encoder_L{L}.npz"))
    depth = int(g["depth"])
    sd = {k: torch.from_numpy(v).double() for k, v in R.backbone_state(int(g["wseed"]), depth, int(g["ngrids"]), int(g["in_chans"])).items()}
    x, coords = (torch.from_numpy(a).double() for a in R.bags(L, g["iseeds"], int(g["ngrids"]), int(g["in_chans"])))
    assert x.shape[0] == (2 if L == 37 else 1)
    for gp in (0, 1):
        for al in (0, 1):
            outs, last = R.forward(sd, x, coords, depth, bool(gp), bool(al), ngrids=int(g["ngrids"]))
            ref = g[f"f64/gp{gp}_al{al}"]
            assert ref.shape == (depth + 1 if al else 1, x.shape[0], 768)
            assert _maxrel(torch.stack(outs).numpy(), ref) < 1e-9, (gp, al)
            assert _maxrel(last[:, :8].numpy(), g[f"f64/feats_al{al}"]) < 1e-9, (gp, al)
    # the fixtures can tell the two read-out paths apart (random LayerNorm affines): the last all-layer outcome is NOT the single output
    for gp in (0, 1):
        a, b = g[f"f64/gp{gp}_al1"][-1], g[f"f64/gp{gp}_al0"][0]
        assert np.linalg.norm(a - b) / np.linalg.norm(b) > 1e-2


def _small(**kw):
    return SE.gigapath_slide_enc12l768d(in_chans=1536, depth=3, slide_ngrids=128, device="cpu", init_seed=5, **kw)


def test_state_dict_is_the_reference_modules(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "slide_encoder_state_keys.json")))
    m = _small()
    sd = m.state_dict()
    assert sorted(k for k, _ in ref["keys"]) == sorted(sd)
    assert {k: list(v.shape) for k, v in sd.items()} == {k: sh for k, sh in ref["keys"]}
    assert "pos_embed" not in sd                                           # (a non-persistent buffer in the reference: derived here)
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(sd) and all(not p.requires_grad for p in m.parameters())
    # a reference checkpoint's "model" entry loads with strict=True, and so does this module's own state dict
    ck = {k: torch.from_numpy(v) for k, v in R.backbone_state(7).items()}
    res = m.load_state_dict(ck, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.state_dict()["norm.weight"], ck["norm.weight"])
    with pytest.raises(RuntimeError, match="missing keys"):
        m.load_state_dict({k: v for k, v in ck.items() if k != "norm.bias"}, strict=True)
    with pytest.raises(NotImplementedError):
        m.requires_grad_(True)


def test_other_architectures_and_training_mode_are_refused():
    for arch in ("gigapath_slide_enc24l1024d", "gigapath_slide_enc12l1536d"):
        with pytest.raises(NotImplementedError, match="Prov-GigaPath geometry"):
            SE.create_model("", arch, 1536, device="cpu")
    with pytest.raises(NotImplementedError, match="Prov-GigaPath geometry"):
        SE.LongNetViT(device="cpu")                                        # (the reference constructor's default embed_dim = 256)
    with pytest.raises(NotImplementedError, match="frozen"):
        SE.gigapath_slide_enc12l768d(depth=1, lora_adapter=True, device="cpu")
    with pytest.raises(RuntimeError, match="Unknown model"):
        SE.create_model("", "gigapath_slide_enc99", 1536, device="cpu")
    m = _small()
    assert m.training                                                      # (as a freshly built reference module)
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m(torch.zeros(1, 4, 1536), torch.zeros(1, 4, 2))
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m.eval().train()(torch.zeros(4, 1536), torch.zeros(4, 2), all_layer_embed=True)


def test_missing_weight_file_warns_and_keeps_the_random_init(tmp_path, capsys):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = SE.create_model("hf_hub:prov-gigapath/prov-gigapath", "gigapath_slide_enc12l768d", 1536, local_dir=str(tmp_path), depth=1,
                            slide_ngrids=16, device="cpu", init_seed=11)
    assert any("Pretrained weights not found" in str(x.message) and "slide_encoder.pth" in str(x.message) for x in w)
    assert "Randomly initialized the model" in capsys.readouterr().out
    assert len(a.pretrained_report[0]) == len(a.state_dict())
    b = SE.gigapath_slide_enc12l768d(in_chans=1536, depth=1, slide_ngrids=16, device="cpu", init_seed=11)
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())          # the seeded random init, untouched
    assert float(a.state_dict()["encoder.layers.0.ffn.fc1.weight"].std()) > 0
    # ... and a file that is there is loaded (its "model" entry, the reference's rule)
    ck = {k: torch.from_numpy(v) for k, v in R.backbone_state(13, depth=1, ngrids=16).items()}
    torch.save({"model": ck}, str(tmp_path / "slide_encoder.pth"))
    c = SE.create_model("x", "gigapath_slide_enc12l768d", 1536, local_dir=str(tmp_path), depth=1, slide_ngrids=16, device="cpu", init_seed=11)
    assert c.pretrained_report == ([], []) and all(torch.equal(v, ck[k]) for k, v in c.state_dict().items())


def test_launcher_is_in_the_header_the_exports_and_the_ctypes_table():
    import __graft_entry__ as ge
    ge.build()
    from modaltune_amd import _lib
    import modaltune_amd.torch_ops as tops
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "modaltune_hip.h")).read(), flags=re.S)
    for name in ("mt_layernorm_pool_fwd", "mt_layernorm_pool_partials_elems"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.mt_version() >= 360
    # (the two epsilons are plain arguments: the entry takes no options pointer -- tests/test_launch_opts_cpu.py lists the launchers that do)
    assert _lib.OP not in _lib.SIGNATURES["mt_layernorm_pool_fwd"]
    # host arithmetic of the workspace: none up to one workgroup's 64 rows, then one slot of D doubles per 64 rows and pass
    q = lib.mt_layernorm_pool_partials_elems
    assert [q(1, n, 768) for n in (1, 64, 65, 128, 129, 1500)] == [0, 0, 2 * 768, 2 * 768, 3 * 768, 24 * 768]
    assert q(3, 1500, 768) == 3 * 24 * 768 and q(1, 10, 1024) < 0 and q(0, 10, 768) < 0 and q(1, 0, 768) < 0
    # bad arguments answer before any HIP call (no GPU here): null pointers, an empty / reversed / overlong range, a short stride
    f = lib.mt_layernorm_pool_fwd
    ok = 1 << 12                                                                        # (a non-null, aligned stand-in pointer: never dereferenced)

    def call(x=ok, ldx=768, rows=4, r0=0, r1=1, pw=None, pb=None, pre_eps=0.0, post_eps=0.0, D=768):
        return f(x, ldx, 1, rows, r0, r1, pw, pb, pre_eps, None, None, post_eps, ok, None, 0, D, None)
    assert call(x=None) == -1
    for r0, r1 in ((0, 0), (2, 1), (0, 5), (-1, 2)):
        assert call(r0=r0, r1=r1) == -1
    assert call(ldx=764) == -1
    assert call(pw=ok) == -1                                                            # weight without bias
    assert call(rows=100, r1=100) == -1                                                 # two workgroups, no workspace
    assert call(pre_eps=-1.0) == -1 and call(post_eps=float("nan")) == -1
    assert call(ldx=1024, D=1024) == -3                                                 # another width
    assert "layernorm_pool_fwd" in tops.SCHEMAS
    y = torch.ops.modaltune_hip.layernorm_pool_fwd(torch.empty(3, 9, 768, device="meta"), 1, 9, None, None, 1e-5, None, None, 1e-6)
    assert tuple(y.shape) == (3, 768) and y.dtype == torch.float32
