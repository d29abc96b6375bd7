"""Bits of every launcher of csrc/norm.hip, for a change that must leave them as they were: seeded cases through ONE library in a
fresh process (MODALTUNE_HIP_LIB selects it), a SHA-256 per (case, output) of the raw bytes of the whole buffer -- padding, canary rows
and partial workspaces included -- written to a JSON file; and the comparison of such files.

    MODALTUNE_HIP_LIB=<parent's library> python tools/norm_bits.py run parent_a.json
    MODALTUNE_HIP_LIB=<parent's library> python tools/norm_bits.py run parent_b.json
    python tools/norm_bits.py run tree.json
    python tools/norm_bits.py compare parent_a.json parent_b.json tree.json

Every output is pre-filled with a fixed pattern (NaN by tests/norm_edge_ref.py, 0.8125 here), so an element that one library writes
and the other leaves alone differs.  Cases: every name of tests/norm_edge_ref.py: MATRIX through that helper's case builder and
launcher; mt_layernorm_pool_fwd at n = 1, 2, 63, 64, 65, 129, 1023 x B = 1, 3 x pre x post with its partial workspace; the elementwise
launchers and the two packers at one small shape each.

Unordered outputs -- fp32 atomics of more than one workgroup onto one address: dw / db of the non-deterministic PARAM form and dgamma
of the non-deterministic injector form above four rows -- are hashed and marked, and `compare` leaves them out.  Any further output on
which the first two files (the same library twice) disagree is named and left out; on everything else the last file must agree with
the first.  Exit status 1 if it does not."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 0.8125
LAUNCHER = {"fwd": "mt_layernorm_fwd", "add": "mt_add_layernorm_fwd", "bwd": "mt_layernorm_bwd", "inj": "mt_inject_resid_bwd"}


def sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def run(path):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import norm_edge_ref as R
    from modaltune_amd import _lib, ops
    dev = "cuda"
    out = {}      # launcher -> case -> output -> {"sha": ..., "unordered": bool}

    def put(launcher, case, tensors, unordered=()):
        torch.cuda.synchronize()
        out.setdefault(launcher, {})[case] = {k: {"sha": sha(v), "unordered": k in unordered} for k, v in tensors.items()}

    for name, kw in R.MATRIX.items():
        c = R.case_of(kw, device=dev if R.on_device(kw["M"]) else "cpu")
        t = R.device_buffers(c, dev)
        spec = None
        if c.drop:
            t["_rng"] = torch.tensor([123, 456, 7, 0], dtype=torch.int32, device=dev)
            spec = ops.dropout_spec(t["_rng"], 40, c.drop[0], 41, c.drop[1], c.drop[2])
        R.launch(ops, c, t, spec)
        res = {k: t[k] for k in c.init}
        if c.det:
            res["partials"] = t["_keep"][-1]
        many = c.M > 4      # more than one workgroup of four rows
        unordered = () if c.det or not many else ("dw", "db") if c.param else ("dgamma",) if c.kind == "inj" else ()
        put(LAUNCHER[c.kind], name, res, unordered)

    g = torch.Generator(device=dev).manual_seed(1234)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    fill = lambda *s, dtype=torch.float32: torch.full(s, PATTERN, dtype=dtype, device=dev)
    D = 768
    pre, post = (1 + 0.1 * rn(D), 0.1 * rn(D)), (1 + 0.1 * rn(D), 0.1 * rn(D))
    for n in (1, 2, 63, 64, 65, 129, 1023):
        for B in (1, 3):
            rpp, r0 = n + 3, 2
            x = rn(B * rpp, D + 4)
            for use_pre in (False, True):
                for use_post in (False, True):
                    elems = ops.layernorm_pool_partials_elems(B, n, D)
                    part = fill(elems + 8, dtype=torch.float64) if elems else None
                    o = fill(B + 1, D)
                    ops.layernorm_pool_fwd(x, B, rpp, r0, r0 + n, o, pre=pre if use_pre else None, post=post if use_post else None,
                                           partials=part, ldx=D + 4)
                    res = {"out": o}
                    if part is not None:
                        res["partials"] = part
                    put("mt_layernorm_pool_fwd", f"n{n}-B{B}-pre{int(use_pre)}-post{int(use_post)}", res)

    # the elementwise launchers: 5 x 768 (the casts three elements more: their scalar tail)
    M, n = 5, 5 * D
    rng = torch.tensor([123, 456, 7, 0], dtype=torch.int32, device=dev)
    spec = ops.dropout_spec(rng, 40, 0.25, 41, 0.5, 2)
    x, y = rn(n + 3), rn(n + 3)
    o = fill(n + 8, dtype=torch.float16); ops.cast_f32_to_f16(x, o, n + 3); put("mt_cast_f32_to_f16", "plain", {"y": o})
    o = fill(n + 8, dtype=torch.float16); ops.cast_f32_to_f16(x, o, n, drop=spec, D=D); put("mt_cast_f32_to_f16", "drop", {"y": o})
    o = fill(n + 8); ops.cast_f16_to_f32(x.half(), o, n + 3); put("mt_cast_f16_to_f32", "plain", {"y": o})
    r2 = rng.clone(); ops.rng_advance(r2); put("mt_rng_advance", "step", {"rng": r2})
    table = torch.full((6, 2), 77, dtype=torch.int32, device=dev)
    ops.droppath_live([41, 42, 43, 44, 45], [0.5, 0.9, 0.1, 0.0, 0.99], 7, rng, table); put("mt_droppath_live", "5sites-B7", {"table": table})
    xp = rn(9, D + 4)      # (rows 1, 2, 4, 5, 7 under the map of two rows per segment of three, behind a leading one)
    o = fill(M + 1, D); ops.dropout_f32(xp, o, M, D, spec, ldx=D + 4, xmap=_lib.rowmap(2, 3, 1)); put("mt_dropout_f32", "5x768-map", {"y": o})
    o = rn(M + 1, D); ops.droppath_rows(o, M, D, spec); put("mt_droppath_rows_f32", "5x768", {"x": o})
    for act in (1, 2, 3):
        o = fill(n + 8); ops.act_fwd(x, o, act, n); put("mt_act_fwd", f"act{act}", {"y": o})
        o = fill(n + 8); ops.act_bwd(x, y, o, act, n); put("mt_act_bwd", f"act{act}", {"dx": o})
    o = fill(n + 8); ops.axpy(x, y, 0.37, o, n); put("mt_axpy", "5x768", {"y": o})
    o = fill(n + 8); ops.axpy_bcast(x, y, 0.37, o, D, n); put("mt_axpy_bcast", "5x768", {"y": o})
    o = rn(D + 8); ops.fold_rows(x, M, D, o); put("mt_fold_rows", "5x768", {"out": o})
    for acc in (False, True):
        o = rn(3 * (M // 2 + 1) + 1, D + 4)
        ops.copy_rows(xp, o, M, D, lds=D + 4, ldd=D + 4, dmap=_lib.rowmap(2, 3, 1), accumulate=acc)
        put("mt_copy_rows_f32", f"5x768-map-acc{int(acc)}", {"dst": o})
    # the packers: a 33 x 65 weight
    Rw, Cw = 33, 65
    w = rn(Rw, Cw)
    for tr in (False, True):
        o = fill(Rw * Cw + 8, dtype=torch.float16); ops.pack_weight(w, o, Rw, Cw, transpose=tr); put("mt_pack_weight_f16", f"33x65-t{int(tr)}", {"dst": o})
    d0, d1 = fill(Rw + 3, Cw + 7, dtype=torch.float16), fill(Cw + 1, Rw + 5, dtype=torch.float16)
    items = torch.tensor([[w.data_ptr(), d0.data_ptr(), d1.data_ptr(), Rw, Cw, 2, Cw + 7, Rw + 5]], dtype=torch.int64, device=dev)
    ops.pack_weights(items, 1); put("mt_pack_weights_f16", "33x65-both", {"dst": d0, "dst_t": d1})

    with open(path, "w") as f:
        json.dump({"build": _lib.build_info(), "results": out}, f, indent=0, sort_keys=True)
    print("wrote", path, "cases", sum(len(v) for v in out.values()), "library", _lib.LIB_PATH)


def compare(a_path, b_path, c_path):
    a, b, c = (json.load(open(p))["results"] for p in (a_path, b_path, c_path))
    assert a.keys() == b.keys() == c.keys(), "the files hold different launchers"
    total = bad = 0
    for launcher in sorted(a):
        assert a[launcher].keys() == b[launcher].keys() == c[launcher].keys(), f"{launcher}: the files hold different cases"
        compared = diff = skipped = 0
        names = set()
        for case in sorted(a[launcher]):
            for k, ra in a[launcher][case].items():
                rb, rc = b[launcher][case][k], c[launcher][case][k]
                if ra["unordered"]:
                    skipped += 1
                    continue
                if ra["sha"] != rb["sha"]:
                    print(f"  LEFT OUT {launcher} {case} {k}: the same library gives other bits in its second run")
                    skipped += 1
                    continue
                compared += 1
                names.add(k)
                if ra["sha"] != rc["sha"]:
                    diff += 1
                    print(f"  DIFFERENT {launcher} {case} {k}")
        print(f"{launcher:32s} cases {len(a[launcher]):4d}  outputs compared {compared:5d}  different {diff}  left out {skipped:3d}  outputs: {' '.join(sorted(names))}")
        total += compared
        bad += diff
    print(f"outputs compared: {total}  different: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
