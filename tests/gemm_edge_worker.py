"""Worker of tests/test_gemm_edges_gpu.py: every case of one forced kernel form of mt_gemm_nt_f16 in one fresh process.

    python tests/gemm_edge_worker.py <pp_big | pp_small | k128 | ps> <output.json>

MT_GEMM_FORCE is read once per process into a static (csrc/gemm.hip, csrc/gemm_ps.hip), so the form is set here, before the library
loads.  Writes {"form", "force", "error", "cases": {name: result of gemm_edge_ref.run_gpu}}; a case that raises (a HIP error, a status
of the launcher) ends the run there: "error" names it, the exit status is 3 and the cases behind it are missing."""
import json
import os
import sys
import traceback


def main():
    form, out_path = sys.argv[1], sys.argv[2]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MT_GEMM_FORCE"] = form
    os.environ.pop("MT_GEMM_PS", None)
    os.environ.pop("MT_GEMM_NOPP", None)
    import torch

    import gemm_edge_ref as R
    from modaltune_amd import ops
    assert form in R.FORCED
    res = {"form": form, "force": os.environ["MT_GEMM_FORCE"], "error": None, "cases": {}}
    rc = 0
    for name, kw in R.matrix(form).items():
        try:
            res["cases"][name] = R.run_gpu(ops, R.make_case(**kw), R.TILE_H[form])
            torch.cuda.synchronize()
        except Exception:
            res["error"] = f"{name}: {traceback.format_exc()[-1500:]}"
            rc = 3
            break
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
