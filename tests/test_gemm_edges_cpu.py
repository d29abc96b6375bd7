"""CPU tests of tests/gemm_edge_ref.py, the helper tests/test_gemm_edges_gpu.py measures the NT GEMM kernels with: a plain CPU product
(fp16 operands, float32 torch.matmul, fp32 epilogue) stays inside the derived per-element bound at every K and epilogue of the GPU
matrix, every planted fault leaves it at every K, and the canary check sees a single changed bit."""
import pytest
import torch

import gemm_edge_ref as R

N = 192
VARIANTS = {
    "bias-f16": dict(M=257, N=N, K=0),
    "bias-f16-8B-rows": dict(M=257, N=N, K=0, ldc_pad=4),
    "bias-f32": dict(M=257, N=N, K=0, out="f32", ldc_pad=4),
    "bias-amap": dict(M=258, N=N, K=0, maps="amap"),
    "nobias": dict(M=257, N=N, K=0, bias=False),
    "bias_resid-f32": dict(M=257, N=N, K=0, epi="bias_resid", out="f32", ldc_pad=4),
    "bias_resid-f16": dict(M=257, N=N, K=0, epi="bias_resid", out="f16", ldc_pad=4),
    "bias_resid-inplace": dict(M=257, N=N, K=0, epi="bias_resid", out="f32", ldc_pad=4, inplace=True),
    "inject": dict(M=258, N=N, K=0, epi="inject", out="f32", ldc_pad=4, maps="engine"),
    "posemb": dict(M=257, N=N, K=0, epi="posemb", out="f32", ldc_pad=4),
    "qkv_hm": dict(M=257, N=N, K=0, epi="qkv_hm", ldc_pad=0),
}


def _case(variant, K):
    return R.make_case(**dict(VARIANTS[variant], K=K))


def test_the_variants_cover_every_epilogue_of_the_gpu_matrix():
    keys = lambda kw: (kw.get("epi", "bias"), kw.get("out", "f16"), kw.get("maps"), kw.get("inplace", False), kw.get("bias", True))
    have = {keys(v) for v in VARIANTS.values()}
    for form in R.FORMS:
        for name, kw in R.matrix(form).items():
            assert keys(kw) in have, name
            assert kw["K"] in R.KS, name
    for kw in R.NATURAL.values():
        assert keys(kw) in have and kw["K"] in R.KS


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cpu_product_is_inside_the_bound(variant, K):
    c = _case(variant, K)
    ref, bound = R.reference(c)
    ratio, at = R.errors(R.cpu_product(c), ref, bound)
    print(f"{variant} K={K}: worst |got - ref| / bound = {ratio:.3f} at {at}")
    assert ratio <= 1.0, R.where(at, 128)
    assert float(bound.min()) > 0.0


@pytest.mark.parametrize("K", R.KS)
@pytest.mark.parametrize("fault", R.FAULTS)
@pytest.mark.parametrize("variant", ["bias-f16", "bias-f32", "inject"])
def test_planted_fault_exceeds_the_bound(variant, fault, K):
    c = _case(variant, K)
    ref, bound = R.reference(c)
    ratio, (m, n) = R.errors(R.cpu_product(c, fault), ref, bound)
    print(f"{variant} {fault} K={K}: worst ratio {ratio:.3g} at {(m, n)}")
    assert ratio > 1.0
    rs, cs = R.fault_region(c, fault)
    assert rs.start <= m < rs.stop and cs.start <= n < cs.stop, "the worst element is not one the fault moved"


def test_a_dropout_mask_enters_reference_and_bound():
    c = R.make_case(257, N, 64, epi="bias_resid", out="f32", ldc_pad=4, drop=(0.25, 0.5, 100))
    g = torch.Generator().manual_seed(3)
    mask = (torch.rand(257, N, generator=g) > 0.25).float() / 0.75
    mask[100:200] = 0.0
    ref, bound = R.reference(c, mask)
    acc = c.A_buf[:, :64].float() @ c.W.float().t() + c.bias
    got = c.resid_vals + mask * acc
    ratio, at = R.errors(got, ref, bound)
    assert ratio <= 1.0, at
    assert torch.equal(ref[100:200], c.resid_vals[100:200].double())
    assert R.errors(c.resid_vals + acc, ref, bound)[0] > 1.0      # (the unmasked product is far outside)


def test_head_major_layout_and_row_maps_round_trip():
    c = _case("qkv_hm", 64)
    ref, _ = R.reference(c)
    buf = c.c_init.double().clone()
    buf[:c.M * c.N] = R.head_major(c, ref)
    assert torch.equal(R.logical(c, buf), ref)
    assert float(buf[(3 * c.M + 5) * 48 + 11]) == float(ref[5, 3 * 48 + 11])      # [head][row][48]
    c = _case("inject", 64)
    assert c.crow.tolist()[:2] == [1, 2] and int(c.crow[c.L]) == c.L + 2 and c.rrow.tolist()[c.L - 1:c.L + 1] == [c.L - 1, 0]
    assert not bool(c.written[0].any()) and not bool(c.written[c.L + 1].any()) and bool(c.written[1, :c.N].all())
    assert not bool(c.written[:, c.N:].any()) and int(c.written.sum()) == c.M * c.N


def test_metric_counts_a_nan_as_a_miss_and_names_the_tile():
    c = _case("bias-f32", 64)
    ref, bound = R.reference(c)
    got = R.cpu_product(c)
    got[200, 70] = float("nan")
    ratio, at = R.errors(got, ref, bound)
    assert ratio == float("inf") and at == (200, 70)
    assert "row tile 1" in R.where(at, 128) and "inside the tile row 72, column 70" in R.where(at, 128)
    assert R.failure("x", dict(ratio=ratio, where=R.where(at, 128), canary=0)) is not None
    assert R.failure("x", dict(ratio=0.5, where="", canary=0)) is None
    assert R.failure("x", dict(ratio=0.5, where="", canary=1, canary_first=3)) is not None


@pytest.mark.parametrize("variant", ["bias-f16", "inject", "qkv_hm"])
def test_canary_check_sees_one_changed_bit_outside_the_written_elements(variant):
    c = _case(variant, 64)
    after = c.c_init.clone()
    if variant == "qkv_hm":
        after[:c.M * c.N] = 1.0
    else:
        after[c.crow, :c.N] = 1.0
    assert R.check_untouched(c.c_init, after, c.written) == (0, None)      # (NaN canaries compare by their bits)
    flat = after.view(-1)
    first = int((~c.written.view(-1)).nonzero()[0])
    it = torch.int16 if after.dtype == torch.float16 else torch.int32
    flat.view(it)[first] ^= 1                                               # another NaN: equal as a value to no one, one bit apart
    assert R.check_untouched(c.c_init, after, c.written) == (1, first)
