"""Branch mix + inner LayerNorm (forward, backward) and the backward's combine kernel at L = 10 000 (for rocprofv3 --pmc runs).
The in-place combine and --sweep (the mix kernels over a range of grids) need a library that has those entries; with an older
library they are left out."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from modaltune_amd import ops
from modaltune_amd.config import branch_table, segment_lengths
L = 10000; B, N = 3, L + 1; M = B * N
plan = ops.make_plan(branch_table(N, segment_lengths()), N, B)
g = torch.Generator(device="cuda").manual_seed(0)
qkv = (torch.randn(M * 2304, device="cuda", generator=g) * 0.8).half()
o_br = torch.zeros(5, M, 768, dtype=torch.float16, device="cuda"); lse_br = torch.zeros(5, M, 16, device="cuda")
ops.dilated_attn_fwd(qkv, plan, o_br, lse_br)
ln_w, ln_b = torch.ones(768, device="cuda"), torch.zeros(768, device="cuda")
y = torch.zeros(M, 768, dtype=torch.float16, device="cuda"); stats = torch.zeros(M, 2, device="cuda"); lse_tot = torch.zeros(M, 16, device="cuda")
dy = (torch.randn(M, 768, device="cuda", generator=g) * 0.1).half()
dmixed = torch.zeros(16, M, 48, dtype=torch.float16, device="cuda"); delta = torch.zeros(5, M, 16, device="cuda")
ws = torch.zeros(ops.dilated_attn_bwd_workspace_bytes(plan) // 2, dtype=torch.float16, device="cuda")
dqkv = torch.zeros(M, 2304, dtype=torch.float16, device="cuda")
def t(fn, n=10):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


fwd = t(lambda: ops.dilated_mix_ln_fwd(o_br, lse_br, plan, ln_w, ln_b, y, stats, lse_tot))
bwd = t(lambda: ops.dilated_mix_ln_bwd(dy, o_br, lse_br, lse_tot, plan, ln_w, stats, dmixed, delta))
comb = t(lambda: ops.dilated_attn_bwd_phases(qkv, dmixed, lse_tot, delta, plan, ws, dqkv, ops.ATTN_BWD_COMBINE))
print(f"mix_fwd {fwd:.4f} mix_bwd {bwd:.4f} combine {comb:.4f} ms  checksum {float(y.float().abs().sum()):.6e} {float(dmixed.float().abs().sum()):.6e} {float(delta.abs().sum()):.6e}")
if hasattr(ops, "dilated_attn_bwd_inplace_phases"):
    ops.dilated_attn_bwd_inplace_phases(qkv, dmixed, lse_tot, delta, plan, ws, dqkv, ops.ATTN_BWD_KV | ops.ATTN_BWD_Q)
    # (repeated in-place combines keep adding into dqkv until it overflows: the traffic and the time do not change, the values mean
    # nothing -- the checksum line above is printed before this on purpose, and nothing reads dqkv after it)
    print("combine_inplace " + " ".join(f"{t(lambda: ops.dilated_attn_bwd_inplace_phases(qkv, dmixed, lse_tot, delta, plan, ws, dqkv, ops.ATTN_BWD_COMBINE)):.4f}" for _ in range(3)) + " ms")
if "--sweep" in sys.argv and hasattr(ops, "dilated_mix_ln_fwd_grid"):
    for grid in (256, 512, 768, 1024, 1536, 2048, 4096):
        f = t(lambda: ops.dilated_mix_ln_fwd_grid(o_br, lse_br, plan, ln_w, ln_b, y, stats, lse_tot, grid))
        b = t(lambda: ops.dilated_mix_ln_bwd_grid(dy, o_br, lse_br, lse_tot, plan, ln_w, stats, dmixed, delta, grid))
        print(f"sweep grid {grid}: mix_fwd {f:.4f} mix_bwd {b:.4f} ms")
