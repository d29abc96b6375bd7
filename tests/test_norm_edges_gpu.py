"""The LayerNorm kernels of csrc/norm.hip at their row, grid and dispatch edges, per element against float64 (tests/norm_edge_ref.py):
M = 1 .. 9 and 67 on every form (idle waves, the clamp of a last odd row), M around the 512-workgroup cap of the PARAM / DET forms and
of inject_resid_bwd, M around the 4096 / 8192 / 16384 caps of the grid-stride loops, five numerical regimes (six for fp16 GELU inputs),
every (D, dtypes, gelu) the dispatch accepts -- dw / db at 2304 and 3072, GELU off the packed kernels, fp16 dx accumulating, in place,
ymap, add_rows with a period of 5, a broadcast x --, the patch map on every operand with a pass boundary inside a workgroup's rows,
the add form under masks read from the device, and the live ranges.  Every case: worst |got - ref| / bound <= 1 for each output against
the derived bound (the statistics per row under their own), canaries around everything that is written bit-identical.  What the
launchers refuse answers MT_ERR_UNSUPPORTED and leaves the NaN-prefilled outputs as they were.

In process.  A HIP error or an unexpected status fails its test at once and nothing further is started here."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_edge_ref as R  # noqa: E402

_stopped = []         # why nothing further is started


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")


def _stop(msg):
    _stopped.append(msg)
    pytest.fail(msg)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from modaltune_amd import ops as _ops
    return _ops


def test_leading_dimensions_the_vector_accesses_cannot_take_are_refused_before_any_launch(ops):
    """lddy and lddx of mt_layernorm_bwd, at D = 512, which has no kernel: nothing is launched whatever the answer.  ldx of
    mt_layernorm_bwd and the three leading dimensions of mt_inject_resid_bwd (whose width check shares the answer, so a call that could
    tell would launch) are pinned in tests/test_norm_edges_cpu.py alone, in a process that sees no device."""
    _gpu()
    t = torch.zeros(8, 776, device="cuda")
    for ld in (770, 773):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.layernorm_bwd(t, t, t[0], t[:, :2], t, 4, 512, lddy=ld, ldx=772, lddx=772)
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            ops.layernorm_bwd(t, t, t[0], t[:, :2], t, 4, 512, lddy=772, ldx=772, lddx=ld)
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        ops.layernorm_bwd(t, t, t[0], t[:, :2], t, 4, 512, lddy=772, ldx=772, lddx=772)


@pytest.mark.parametrize("name", list(R.MATRIX))
def test_case(ops, name):
    _gpu()
    kw = R.MATRIX[name]
    dev = "cuda" if R.on_device(kw["M"]) else "cpu"      # above the grid caps inputs and float64 references live on the device
    try:
        c = R.case_of(kw, device=dev)
        r = R.run_gpu(ops, c)
    except RuntimeError as e:      # a HIP error or a status of the launcher: nothing further is started
        _stop(f"{name}: {e}")
    finally:
        if dev == "cuda" or kw["M"] > 1000:
            R.make_case.cache_clear()      # (the tensors of the large cases are not kept)
    print(R.line(name, r))
    bad = R.failure(name, r)
    assert bad is None, bad
    if c.drop and c.drop[1] > 0.0:      # a dropped pass: its branch rows were NaN; h = x there (asserted above), y and the statistics finite
        assert r["dead_rows"] > 0


@pytest.mark.parametrize("name", list(R.REFUSED))
def test_refused_combination_answers_unsupported_and_writes_nothing(ops, name):
    _gpu()
    c = R.case_of(R.REFUSED[name])
    t = R.device_buffers(c)
    before = {k: t[k].clone() for k in c.init}
    with pytest.raises(RuntimeError, match=r"\(-3\)"):
        R.launch(ops, c, t)
    torch.cuda.synchronize()
    for k in c.init:
        none = torch.zeros_like(c.written[k])
        assert R.check_untouched(before[k], t[k], none)[0] == 0, f"{name}: the {k} buffer changed"
