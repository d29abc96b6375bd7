"""mt_gemm_nt_f16 at the pipeline, tile and stride edges of its five kernel forms, per element against float64 (tests/gemm_edge_ref.py):
short K (nk = K / 64 = 1, 2, 3, 6, 12: the ping-pong pipeline's own code for one and two tiles and for the last two of any K, the
double buffer of the 128-row kernels), M around every tile height, every epilogue on every form it can run on, lda > K and ldc > N
with NaN canaries around everything that is written, the persistent kernel with 2 .. 12 tiles (workgroups without a tile, workgroups
that walk two), dropout masks read from the device, and four products of the shipped step that reach the ping-pong kernel by the
fill rule.  Every case: worst |got - ref| / bound <= 1 against the derived bound, canaries bit-identical.

The forced forms (MT_GEMM_FORCE is a per-process static) run in one fresh child each, one after another (tests/gemm_edge_worker.py);
the parent asserts per case.  A child that dies of a signal, times out or reports an error fails its tests at once and nothing
further is started here, in a child or in process."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_edge_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gemm_edge_worker.py")
CHILD_TIMEOUT = 240

_children = {}        # form -> the child's JSON
_stopped = []         # why nothing further is started


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")


def _stop(msg):
    _stopped.append(msg)
    pytest.fail(msg)


def _child(form, tmp_path_factory):
    if form in _children:
        return _children[form]
    _gpu()
    out = str(tmp_path_factory.mktemp("gemm_edges") / f"{form}.json")
    env = {k: v for k, v in os.environ.items() if k not in ("MT_GEMM_FORCE", "MT_GEMM_PS", "MT_GEMM_NOPP", "MT_GEMM_GC")}
    try:
        p = subprocess.run([sys.executable, WORKER, form, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _stop(f"the {form} child did not end within {CHILD_TIMEOUT} s")
    log = p.stdout.decode(errors="replace")[-3000:]
    if p.returncode < 0 or p.returncode > 128:
        _stop(f"the {form} child ended with status {p.returncode} (a signal):\n{log}")
    if not os.path.exists(out):
        _stop(f"the {form} child (status {p.returncode}) wrote no result:\n{log}")
    with open(out) as f:
        res = json.load(f)
    if p.returncode != 0 or res["error"] or "HIP error" in log or "illegal memory access" in log:
        _stop(f"the {form} child (status {p.returncode}) reports: {res['error']}\n{log}")
    _children[form] = res
    return res


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from modaltune_amd import ops as _ops
    return _ops


def _run(ops, kw, tile_h, device="cpu"):
    _gpu()
    try:
        return R.run_gpu(ops, R.make_case(**kw, device=device), tile_h)
    except RuntimeError as e:      # a HIP error or a status of the launcher: nothing further is started
        _stop(f"in process: {e}")


def _forced_cases():
    return [pytest.param(form, name, id=f"{form}:{name}") for form in R.FORCED for name in R.matrix(form)]


@pytest.mark.parametrize("form", R.FORCED)
def test_forced_form_ran_every_case_in_its_own_process(form, tmp_path_factory):
    res = _child(form, tmp_path_factory)
    assert res["form"] == form and res["force"] == form
    assert list(res["cases"]) == list(R.matrix(form))
    worst = max(res["cases"].items(), key=lambda kv: kv[1]["ratio"])
    print(f"{form}: {len(res['cases'])} cases, worst |got - ref| / bound = {worst[1]['ratio']:.3f} ({worst[0]}: {worst[1]['where']})")


@pytest.mark.parametrize("form,name", _forced_cases())
def test_forced_form_case(form, name, tmp_path_factory):
    r = _child(form, tmp_path_factory)["cases"][name]
    print(f"{form} {name}: ratio {r['ratio']:.3f}, canary {r['canary']}")
    bad = R.failure(f"{form} {name}", r)
    assert bad is None, bad


@pytest.mark.parametrize("name", list(R.matrix("k64")))
def test_128x64_form_case(ops, name):
    """N is no multiple of 128: the 128 x 64 tiles by the launcher's own rule, in process."""
    _gpu()
    assert os.environ.get("MT_GEMM_FORCE") is None
    kw = R.matrix("k64")[name]
    assert kw["N"] % 128 != 0
    r = _run(ops, kw, R.TILE_H["k64"])
    print(f"k64 {name}: ratio {r['ratio']:.3f}, canary {r['canary']}")
    bad = R.failure(f"k64 {name}", r)
    assert bad is None, bad


@pytest.mark.parametrize("name", list(R.NATURAL))
def test_natural_dispatch_to_the_pingpong_kernel(ops, name):
    """Products of the shipped step that land on the ping-pong kernel by the fill rule of launch_nt_bn (M >= 8192, N = 768, the 256-row
    tiles fill 80 % of their rounds; the persistent kernel declines K < 768, fp32 output and row maps): no force, in process, operands
    generated on the device."""
    _gpu()
    assert os.environ.get("MT_GEMM_FORCE") is None and os.environ.get("MT_GEMM_NOPP") is None
    kw = R.NATURAL[name]
    tiles = -(-kw["M"] // 256) * (kw["N"] // 256)
    assert kw["M"] >= 8192 and kw["N"] % 256 == 0 and 5 * tiles >= 4 * -(-tiles // 256) * 256, "the fill rule would not pick the ping-pong kernel"
    r = _run(ops, kw, R.TILE_H["natural"], device="cuda")
    R.make_case.cache_clear()      # (the device tensors of the large cases are not kept)
    print(f"natural {name}: ratio {r['ratio']:.3f}, canary {r['canary']}")
    bad = R.failure(f"natural {name}", r)
    assert bad is None, bad
