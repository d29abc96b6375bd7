"""Which kernel, running on ANOTHER stream, corrupts the prompt self-attention (mt_token_mha_fwd) -- or any small victim kernel?
One backbone layer's launches (forward and backward, launch by launch: csrc/layer.hip's list) are the aggressors, one at a time, in
a loop on stream B; the victim loops on stream A and counts outputs that differ from its solo result.
    python tools/diag/victim_stress.py [L] [iters]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from modaltune_amd import ops, synth  # noqa: E402
from modaltune_amd._lib import rowmap  # noqa: E402
from modaltune_amd.config import DILATED_RATIOS, ModelConfig, branch_table  # noqa: E402
from modaltune_amd.engine import Engine  # noqa: E402

L = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
B, D, Fd = 2, 768, 3072
N = L + 1
M = B * N
cfg = ModelConfig(depth=1, interaction_indexes=((0, 0),))
sizes = synth.toy_group_sizes()
eng = Engine(cfg, sizes, "cuda")
eng.load_state_dict(synth.synth_state_dict(cfg, sizes, seed=31))
eng._build_caches()
ws = eng._workspace(B, L)
plan = ops.make_plan(branch_table(N, eng.seg_lengths, DILATED_RATIOS), N, B)
eng._ctx = dict(B=B, L=L, N=N, M=M, Mp=B * L, ws=ws, plan=plan, patch_map=rowmap(L, N, 1))
eng._drop_now = False
tape = eng.tape
tape.grad_enabled = True
tape.reset()
g = torch.Generator(device="cuda").manual_seed(1)
ws["hin0"].copy_(torch.randn(M, D, generator=g, device="cuda"))
eng._layer(0, ws["hout0"], None, defer=False)
ws["dh"].copy_(torch.randn(M, D, generator=g, device="cuda") * 64)
eng._ctx["dh16_valid"] = False
bwd = tape.back[-1]
bwd()
torch.cuda.synchronize()
lw, cb = eng._layer_w[0], ws[("_cb", 0)]
# one aggressor per launch of the layer: the single-step calls of the composite launchers, named by ops.LAYER_STEPS' keys
AGG = {}
for entry, call in (("longnet_layer_fwd", lambda steps: ops.longnet_layer_fwd(lw, cb, plan, M, D, Fd, ws["hout0"], steps=steps)),
                    ("longnet_layer_bwd", lambda steps: ops.longnet_layer_bwd(lw, cb, plan, M, D, Fd, False, False, steps=steps))):
    for bit, key in ops.layer_steps(entry, M, D, Fd, False):
        AGG[f"{entry[-3:]}.{bit.bit_length() - 1} {key}"] = lambda call=call, bit=bit: call(bit)
AGG["copy(hbm)"] = lambda: ws["dt16"].copy_(ws["t16"])

# victim: the prompt self-attention at the step's geometry (one pass, 65 tokens, 12 heads x 16)
T, E, H = 65, 192, 12
q, k, v = (torch.randn(1, T, E, generator=g, device="cuda") for _ in range(3))
out, probs = torch.empty(1, T, E, device="cuda"), torch.empty(1 * H * T * T, device="cuda")
ops.token_mha_fwd(q, k, v, out, probs, 1, T, E, H)
torch.cuda.synchronize()
ref_out, ref_probs = out.clone(), probs.clone()
sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
bad = torch.zeros(2, dtype=torch.int64, device="cuda")


def trial(name, agg, iters):
    bad.zero_()
    torch.cuda.synchronize()
    stop_after = iters
    with torch.cuda.stream(sb):
        for _ in range(max(1, iters // 20)):
            agg()
    with torch.cuda.stream(sa):
        for i in range(stop_after):
            ops.token_mha_fwd(q, k, v, out, probs, 1, T, E, H)
            bad[0] += (out != ref_out).any()
            bad[1] += (probs != ref_probs).any()
            if i % 20 == 0:
                with torch.cuda.stream(sb):
                    agg()
    torch.cuda.synchronize()
    print(f"{name:28s}: victim wrong out {int(bad[0])} / probs {int(bad[1])} of {iters}", flush=True)


trial("(alone)", lambda: None, ITERS)
for name, agg in AGG.items():
    trial(name, agg, ITERS)
