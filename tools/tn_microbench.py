"""gemm_tn (adapter weight gradients) at the step's shapes, for rocprofv3 --pmc runs.

--full-width: the two products of the full-width adapters (768 x 768: Injector q / out, 1536 x 768: Extractor k | v) at M = 30 003 and
12 291 rows, default and deterministic form, written into a row slice of a [2304, 768] destination as the engine does.  The tile these
launch is the library's choice or MT_GEMM_TN_TILE=64x64|128x64|128x128 (read once per process: one process per tile, alternate them)."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modaltune_amd import ops


def timed(fn, reps=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


g = torch.Generator(device="cuda").manual_seed(0)
if "--full-width" in sys.argv:
    tile = os.environ.get("MT_GEMM_TN_TILE", "default")
    for M in (30003, 12291):
        for N1, N2, row0 in [(768, 768, 0), (1536, 768, 768)]:
            A = (torch.randn(M, N1, device="cuda", generator=g) * 0.1).half()
            B = (torch.randn(M, N2, device="cuda", generator=g) * 0.1).half()
            C = torch.zeros(2304, 768, device="cuda")
            cs = torch.zeros(2304, device="cuda")
            dst, bdst = C[row0:row0 + N1], cs[row0:row0 + N1]
            det = torch.empty(ops.det_elems("gemm_tn_f16", M, N1, N2, 1), device="cuda")
            for what, ws in (("default", None), ("det", det)):
                ms = timed(lambda: ops.gemm_tn(A, B, dst, M, N1, N2, ldc=768, colsum=bdst, det=ws))
                print(f"gemm_tn tile={tile} {N1}x{N2} M={M} {what}: {ms*1e3:.1f} us  {2.0*M*N1*N2/ms/1e9:.0f} TFLOP/s", flush=True)
            del A, B, C, det
    sys.exit(0)
M = 30003
for N1, N2 in [(384, 768), (192, 768), (768, 192), (192, 192)]:
    A = (torch.randn(M, N1, device="cuda", generator=g) * 0.1).half()
    B = (torch.randn(M, N2, device="cuda", generator=g) * 0.1).half()
    C = torch.zeros(N1, N2, device="cuda")
    ms = timed(lambda: ops.gemm_tn(A, B, C, M, N1, N2))
    print(f"gemm_tn {N1}x{N2}: {ms*1e3:.1f} us  {2.0*M*N1*N2/ms/1e9:.0f} TFLOP/s")
