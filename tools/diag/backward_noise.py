"""How much run-to-run noise the fp32-atomic gradient sums carry, and that the deterministic mode removes it: the same train step
(update=False, fixture model_L1500_d3, Dropout / DropPath off) repeated N times from identical state; per mode: how many repeats differ
bitwise from the first in the flat gradient, and the largest relative difference |g_i - g_0|_max / |g_0|_max over the gradient tensors.
python tools/diag/backward_noise.py [N=20]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import torch  # noqa: E402
from test_model_gpu import _build  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
for mode in ("0", "1"):
    os.environ["MT_DETERMINISTIC"] = mode
    g, cfg, eng, ts, inp = _build(os.path.join(ROOT, "tests", "golden", "model_L1500_d3.npz"))
    x = torch.from_numpy(inp["x"]).cuda()
    genes = [torch.from_numpy(a).cuda() for a in inp["genes"]]
    text = torch.from_numpy(inp["text"]).cuda()
    first, differ, worst, worst_name = None, 0, 0.0, None
    for i in range(N + 1):
        ts.step(x, inp["coords"], genes, text, update=False)
        torch.cuda.synchronize()
        grads = {k: v.clone() for k, v in ts.unscaled_grads().items()}
        if first is None:
            first, flat0 = grads, eng.store.flat_grad.clone()
            continue
        differ += int(not torch.equal(eng.store.flat_grad, flat0))
        for k, v in grads.items():
            r = float((v - first[k]).abs().max() / (first[k].abs().max() + 1e-30))
            if r > worst:
                worst, worst_name = r, k
    print(f"deterministic={eng.deterministic}: {differ} of {N} repeated backward passes differ bitwise from the first; "
          f"largest relative difference in a gradient tensor {worst:.3e} ({worst_name})", flush=True)
