"""CPU: MtLaunchOpts (include/modaltune_hip.h) -- every launcher that takes the options pointer checks it before anything else: a set
field it honours passes on to the argument checks (all data pointers null here: MT_ERR_BAD_ARG), a set field it does not honour is
MT_ERR_UNSUPPORTED, never ignored.  In a child process, like the null probe of tests/test_abi.py: no GPU is touched."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAD_ARG, UNSUPPORTED = -1, -3
# launcher -> the option fields it honours (the header comment of each entry)
HONOURS = {
    "mt_layernorm_fwd": {"eps", "live"},
    "mt_add_layernorm_fwd": {"eps"},
    "mt_layernorm_bwd": {"live", "partials"},
    "mt_gemm_nt_f16": {"live"},
    "mt_gemm_tn_f16": {"partials"},
    "mt_colsum_f16": {"partials"},
    "mt_inject_resid_bwd": {"partials"},
    "mt_inject_attn_bwd_hd": {"partials"},
    "mt_extract_attn_bwd_hd": {"partials"},
    "mt_dilated_attn_fwd": {"live"},
    "mt_dilated_mix_ln_fwd": {"live", "grid_wgs"},
    "mt_dilated_mix_ln_bwd": {"live", "grid_wgs"},
    "mt_dilated_attn_bwd_inplace": {"live"},
}

_PROBE = r'''
import ctypes as C
import sys
sys.path.insert(0, %r)
from modaltune_amd import _lib
lib = _lib.load()
OP = C.POINTER(_lib.MtLaunchOpts)
keep = (C.c_int * 2)(0, 1), (C.c_float * 4)()          # host memory: nothing reads through it, the pointers only have to be set
FIELDS = {"eps": dict(eps=1e-6), "live": dict(live=C.addressof(keep[0]), live_rows=5),
          "partials": dict(partials=C.addressof(keep[1]), partials_elems=4), "grid_wgs": dict(grid_wgs=7)}


def call(name, **fields):
    sig = _lib.SIGNATURES[name]
    assert sig[-2] is OP, name
    o = _lib.MtLaunchOpts(**fields)
    args = [C.byref(o) if t is OP else 0 if t in (_lib.I, _lib.L) else 0.0 if t in (_lib.F, _lib.D) else None for t in sig]
    return getattr(lib, name)(*args)


for name in [n for n, sig in _lib.SIGNATURES.items() if OP in sig]:
    print("zeroed", name, call(name), flush=True)
    for f, kw in FIELDS.items():
        print("field", name, f, call(name, **kw), flush=True)
    print("negeps", name, call(name, eps=-1.0), flush=True)
print("both mt_layernorm_bwd", call("mt_layernorm_bwd", **FIELDS["live"], **FIELDS["partials"]), flush=True)
print("naneps mt_layernorm_fwd", call("mt_layernorm_fwd", eps=float("nan")), flush=True)
'''


def test_launchers_check_their_options_before_anything_else():
    import __graft_entry__ as ge
    ge.build()
    p = subprocess.run([sys.executable, "-c", _PROBE % ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-400:] + p.stderr[-400:]
    rows = [ln.split() for ln in p.stdout.splitlines()]
    zeroed = {r[1]: int(r[2]) for r in rows if r[0] == "zeroed"}
    assert set(zeroed) == set(HONOURS)                    # exactly the thirteen take the pointer
    assert all(rc == BAD_ARG for rc in zeroed.values()), zeroed          # a zeroed struct: the null arguments are what is wrong
    field = {(r[1], r[2]): int(r[3]) for r in rows if r[0] == "field"}
    assert len(field) == 4 * len(HONOURS)
    for (name, f), rc in field.items():
        assert rc == (BAD_ARG if f in HONOURS[name] else UNSUPPORTED), (name, f, rc)
    # a negative epsilon: a bad argument where epsilon is honoured, an option too many elsewhere
    negeps = {r[1]: int(r[2]) for r in rows if r[0] == "negeps"}
    for name, rc in negeps.items():
        assert rc == (BAD_ARG if "eps" in HONOURS[name] else UNSUPPORTED), (name, rc)
    assert ["both", "mt_layernorm_bwd", str(UNSUPPORTED)] in rows          # each honoured, not together
    assert ["naneps", "mt_layernorm_fwd", str(BAD_ARG)] in rows
