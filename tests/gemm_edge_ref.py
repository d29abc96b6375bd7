"""Helper (not a test module): mt_gemm_nt_f16 per element, in float64, at the kernels' pipeline, tile and stride edges.

The entry point has five kernel forms (csrc/gemm.hip, csrc/gemm_ps.hip): 128 x 64 and 128 x 128 tiles (double-buffered LDS), the
ping-pong kernel with 256- and 128-row tiles (software pipeline with separate code for nk = K / 64 = 1, 2 and the last two tiles of any
K) and the persistent 192 x 256 kernel.  Everything here works FROM EXACTLY THE TENSORS THE KERNELS READ and restates the epilogues of
include/modaltune_hip.h:

    BIAS        C = acc + bias                                  BIAS_RESID  C = resid + drop(acc + bias)
    INJECT      C = (1 + g[n]) resid + g[n] (acc + bias)        POSEMB      C = acc + bias + [table[pos_col] | table[pos_row]]
    QKV_HM      C = acc + bias, stored head-major [N / 48][M][48]

* make_case(...): the inputs of one call, built once from a seeded generator: fp16 A in a buffer with lda = K + 8 (and, with a row map,
  one unread row in front of every pass), fp16 W, fp32 bias / resid / gamma / position table, int32 pos_row / pos_col, and a C buffer
  with ldc > N and rows behind M.  Everything the kernel must not read is NaN (padding columns of A and resid, unmapped rows), the
  whole C buffer is NaN before the call.
* reference(c, mask): the epilogue in float64 and, per element, the bound

      bound = gamma_K S + u_out |ref|        gamma_K = 2 (K + 8) 2^-24        u_out = 2^-11 (fp16 output) | 2^-24 (fp32)

  S is the same epilogue on absolute values: |A| |W|^T + |bias| (+ |resid|, |1 + g| |resid| and |g| (...) for INJECT, + |pe|).  The
  products of two fp16 numbers are exact in fp32, so the error of a correct kernel is the rounding of K - 1 fp32 additions and of the
  handful of fp32 operations of the epilogue -- at most (K + 8) 2^-24 S to first order with round-to-nearest additions, whatever their
  order -- plus one rounding to the output type.  THE FACTOR 2 IS AN ASSUMPTION: the rounding mode of the MFMA accumulator has not been
  measured here; a truncating accumulator loses up to 2^-23 per addition.  The bound is derived, not tuned: the measured worst ratios
   are a record, nothing here was adjusted to them.  A kernel that exceeds it uniformly by a factor below 2 or so
  would point at the assumption; an excess structured by tile or k-position is a defect.  Seen on the MI355X: nothing above 1 -- fp32
  outputs below 0.02 of the bound on every form, fp16 outputs up to 0.97 at K = 64, which is the output rounding itself (half an fp16
  ulp is u_out |ref|) -- so gamma_K stands as derived.
* errors(got, ref, bound): the metric -- the worst |got - ref| / bound and its (row, column); a NaN where a value belongs is inf.
  where(...) names the tile and the position inside it for the message of a failing assertion.
* check_untouched(before, after, written): canaries -- every element outside `written` must keep its bits.
* cpu_product(c, fault): the plain CPU product (fp16 operands, float32 torch.matmul, fp32 epilogue) and the planted FAULTS, for
  tests/test_gemm_edges_cpu.py, which holds the first inside the bound and every fault outside it at every K of the GPU matrix.
* matrix(form) / NATURAL: the cases of tests/test_gemm_edges_gpu.py; run_gpu(ops, c): one call on the device, measured.
"""
import functools
import zlib

import torch

EPI = {"bias": 0, "bias_resid": 1, "inject": 2, "posemb": 3, "qkv_hm": 4}
DT = {"f16": torch.float16, "f32": torch.float32}
U_OUT = {"f16": 2.0 ** -11, "f32": 2.0 ** -24}
FORMS = ("k64", "k128", "pp_big", "pp_small", "ps")      # k64: no force (N is no multiple of 128); the others: MT_GEMM_FORCE
FORCED = ("pp_big", "pp_small", "k128", "ps")
TILE_H = {"k64": 128, "k128": 128, "pp_big": 256, "pp_small": 128, "ps": 192, "natural": 256}
KS = (64, 128, 192, 384, 768, 832, 1536)                # every K of the GPU matrix
NPASS = 2                                               # task passes of the cases with row maps


def gamma(K):
    return 2.0 * (K + 8) * 2.0 ** -24


class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(M, N, K, epi="bias", out="f16", ldc_pad=8, maps=None, inplace=False, bias=True, drop=None, device="cpu"):
    """maps: None | "engine" (C through the patch map of a [B, L + 1, N] token buffer -- the cls rows are skipped --, one slide's
    residual broadcast to the B passes: Engine._injector) | "amap" (A and C through the patch map, a residual per row).
    inplace: resid is C (BIAS_RESID accumulating in place).  drop: (p, path_p, rows_per_pass) or None.  ldc_pad = 0: ldc == N (what the
    persistent kernel requires)."""
    c = Case()
    c.M, c.N, c.K, c.epi, c.out, c.maps, c.inplace, c.drop, c.device = M, N, K, epi, out, maps, inplace, drop, device
    key = repr((M, N, K, epi, out, ldc_pad, maps, inplace, bias, drop))
    gen = torch.Generator(device=device).manual_seed(zlib.crc32(key.encode()))
    rn = lambda *s: torch.randn(*s, generator=gen, device=device)
    nan = float("nan")
    c.lda, c.ldc = K + 8, N + ldc_pad
    assert c.lda % 8 == 0 and c.ldc % 4 == 0 and (out == "f32" or epi in ("bias", "bias_resid", "qkv_hm"))
    rows = torch.arange(M, device=device)
    if maps:
        assert M % NPASS == 0
        c.L = L = M // NPASS
        patch = (rows // L) * (L + 1) + 1 + rows % L          # rowmap(L, L + 1, 1)
        phys = NPASS * (L + 1)
    else:
        c.L, patch, phys = M, rows, M
    c.arow = patch if maps == "amap" else rows
    c.crow = patch if maps else rows
    c.A_buf = torch.full((phys if maps == "amap" else M, c.lda), nan, dtype=torch.float16, device=device)
    c.A_buf[c.arow, :K] = rn(M, K).half()
    c.W = (rn(N, K) * 0.05).half()
    c.bias = rn(N) if bias else None
    c.resid = c.gamma = c.tab = c.pos_row = c.pos_col = None
    c.ldr, c.rrow = 0, rows
    if epi in ("bias_resid", "inject"):
        if inplace:
            assert epi == "bias_resid" and out == "f32"
            c.ldr, c.rrow = c.ldc, c.crow
            c.resid_vals = rn(M, N)
        else:
            c.ldr = N + 4
            c.rrow = rows % c.L if maps == "engine" else rows
            nr = c.L if maps == "engine" else M
            c.resid = torch.full((nr, c.ldr), nan, device=device)
            c.resid[:, :N] = rn(nr, N)
            c.resid_vals = c.resid[c.rrow, :N]
    if epi == "inject":
        c.gamma = rn(N) * 0.1
    if epi == "posemb":
        from modaltune_amd.config import sincos_1d_table
        c.tab = torch.from_numpy(sincos_1d_table(64, N // 2)).float().to(device)
        c.pos_row = torch.randint(0, 64, (M,), generator=gen, device=device, dtype=torch.int32)
        c.pos_col = torch.randint(0, 64, (M,), generator=gen, device=device, dtype=torch.int32)
    # the C buffer: NaN everywhere; two rows behind the last one (QKV_HM: 64 elements behind the slabs)
    if epi == "qkv_hm":
        assert N % 48 == 0 and not maps
        c.c_init = torch.full((M * N + 64,), nan, dtype=DT[out], device=device)
        c.written = torch.zeros(M * N + 64, dtype=torch.bool, device=device)
        c.written[:M * N] = True
    else:
        c.c_init = torch.full((phys + 2, c.ldc), nan, dtype=DT[out], device=device)
        c.written = torch.zeros(phys + 2, c.ldc, dtype=torch.bool, device=device)
        c.written[c.crow, :N] = True
        if inplace:
            c.c_init[c.crow, :N] = c.resid_vals
    return c


def _terms(c):
    """acc, |A| |W|^T in float64 from the tensors of the case (cached on it)."""
    if not hasattr(c, "_acc"):
        A, W = c.A_buf[c.arow, :c.K].double(), c.W.double()
        c._acc, c._aacc = A @ W.t(), A.abs() @ W.abs().t()
    return c._acc, c._aacc


def epilogue(c, acc, mask=None, absolute=False, bias=None):
    """The epilogue of the case on `acc` [M, N] in acc's dtype (float64: the reference; float32: the CPU product), logical layout.
    absolute: the same on absolute values (acc is |A| |W|^T then) -- the S of the bound."""
    f = (lambda t: t.to(acc.dtype).abs()) if absolute else (lambda t: t.to(acc.dtype))
    bias = c.bias if bias is None else bias
    v = acc + f(bias) if bias is not None else acc
    if c.epi == "bias_resid":
        if mask is not None:      # (a dropped element is SELECTED to 0: csrc/common.h, drop_apply4)
            v = torch.where(mask != 0, v * mask.to(acc.dtype), torch.zeros_like(v))
        v = v + f(c.resid_vals)
    elif c.epi == "inject":
        g = c.gamma.to(acc.dtype)
        v = f(1 + g) * f(c.resid_vals) + f(g) * v
    elif c.epi == "posemb":
        v = v + f(torch.cat([c.tab[c.pos_col.long()], c.tab[c.pos_row.long()]], 1))
    return v


def reference(c, mask=None):
    """(ref, bound), float64 [M, N] in the logical layout.  mask [M, N] (BIAS_RESID with dropout): the factor of every element as
    ops.dropout_f32 reads it from the device."""
    acc, aacc = _terms(c)
    ref = epilogue(c, acc, mask)
    S = epilogue(c, aacc, mask, absolute=True)
    return ref, gamma(c.K) * S + U_OUT[c.out] * ref.abs()


def plain_bound(A, W, ref, out_dtype, *extra):
    """The bound for a product outside make_case (the shape tests of tests/test_kernels_gpu.py): A [M, K], W [N, K] as the kernel reads
    them, ref float64 [M, N], extra: the addends of the epilogue ([N] or [M, N]: bias, resid)."""
    S = A.double().abs() @ W.double().abs().t()
    for e in extra:
        S = S + e.double().abs()
    return gamma(A.shape[1]) * S + U_OUT["f16" if out_dtype == torch.float16 else "f32"] * ref.abs()


def logical(c, buf):
    """The [M, N] result out of a C buffer of the case (row map, ldc, the head-major permutation of QKV_HM undone)."""
    if c.epi == "qkv_hm":
        return buf[:c.M * c.N].view(c.N // 48, c.M, 48).permute(1, 0, 2).reshape(c.M, c.N)
    return buf[c.crow, :c.N]


def head_major(c, t):
    """[M, N] logical -> the flat head-major image [N / 48][M][48] MT_EPI_QKV_HM stores."""
    return t.view(c.M, c.N // 48, 48).permute(1, 0, 2).reshape(-1)


# ------------------------------------------------------------------------------------------------ the metric
def errors(got, ref, bound):
    """-> (worst |got - ref| / bound, (row, column)).  A NaN (or inf) where a value belongs counts as inf."""
    r = (got.to(ref.device).double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), (i // ref.shape[1], i % ref.shape[1])


def where(at, tile_h):
    """The tile of an element and its k-independent position inside it, for messages."""
    m, n = at
    return f"row {m}, column {n}: row tile {m // tile_h} (rows of {tile_h}), column tile {n // 256}; inside the tile row {m % tile_h}, column {n % 256}"


def check_untouched(before, after, written):
    """Every element outside `written` (bool, the buffer's shape) must be bit-identical in `before` and `after` (same shape and dtype).
    -> (number of changed elements, flat index of the first or None)."""
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[before.element_size()]
    bad = ((before.view(it) != after.view(it)) & ~written.to(before.device)).reshape(-1)
    n = int(bad.sum())
    return n, (int(bad.nonzero()[0]) if n else None)


# ------------------------------------------------------------------------------------------------ CPU product and planted faults
FAULTS = ("drop_k_step", "k_tile_twice", "rows_swapped", "quad_shifted", "neighbour_bias", "stale_last_row")


def fault_region(c, fault):
    """Rows and columns (slices of the logical result) a planted fault may move."""
    last = c.M - 1
    return {"drop_k_step": (slice(16, 32), slice(8, 12)), "k_tile_twice": (slice(16, 32), slice(8, 12)),
            "rows_swapped": (slice(3, 21), slice(0, c.N)), "quad_shifted": (slice(16, 32), slice(8, 16)),
            "neighbour_bias": (slice(0, c.M), slice(9, 10)), "stale_last_row": (slice(last, last + 1), slice(0, c.N))}[fault]


def cpu_product(c, fault=None):
    """fp16 operands, float32 torch.matmul, the epilogue in fp32, rounded to the output type: [M, N] logical.  fault: one of FAULTS --
    what a kernel with that defect would leave."""
    A, W = c.A_buf[c.arow, :c.K].float(), c.W.float()
    acc = A @ W.t()
    bias = c.bias
    if fault == "drop_k_step":          # one 32-wide k-step lost for one 16 x 4 accumulator patch (the last step of the last K-tile)
        acc[16:32, 8:12] -= A[16:32, c.K - 32:] @ W[8:12, c.K - 32:].t()
    if fault == "k_tile_twice":         # one 64-deep K-tile added twice for that patch (a buffer read again before it was refilled)
        acc[16:32, 8:12] += A[16:32, :64] @ W[8:12, :64].t()
    if fault == "neighbour_bias":       # column 9 takes the bias of column 10
        bias = c.bias.clone()
        bias[9] = c.bias[10]
    v = epilogue(c, acc, bias=bias).to(DT[c.out])
    if fault == "rows_swapped":
        v[[3, 20]] = v[[20, 3]]
    if fault == "quad_shifted":         # the column quad 8 .. 11 of 16 rows lands 4 columns to the right, over 12 .. 15 (its own place is
        v[16:32, 12:16] = v[16:32, 8:12].clone()      # left right here: the NaN fill it would keep is not what the bound has to catch)
    if fault == "stale_last_row":       # the last row of the ragged tile holds the same row of the tile before
        v[c.M - 1] = v[c.M - 1 - 128]
    return v


# ------------------------------------------------------------------------------------------------ the cases of the GPU matrix
def _name(kw):
    s = f"{kw.get('epi', 'bias')}-{kw.get('out', 'f16')}-M{kw['M']}-N{kw['N']}-K{kw['K']}"
    for k, v in kw.items():
        if k not in ("M", "N", "K", "epi", "out"):
            s += f"-{k}={'x'.join(map(str, v)) if isinstance(v, tuple) else v}"
    return s


@functools.lru_cache(maxsize=None)
def matrix(form):
    """{case name: make_case keyword arguments} of one kernel form, in order."""
    cs = []
    if form == "ps":      # needs M >= 256, K >= 768, N % 256 == 0, fp16 output, BIAS or QKV_HM with a bias, ldc == N: 2 .. 12 tiles of 192 x 256
        for M in (256, 383, 384, 385, 577):
            for N in (256, 768):
                for K in (768, 832, 1536):
                    cs.append(dict(M=M, N=N, K=K, ldc_pad=0))
        cs.append(dict(M=385, N=2304, K=768, epi="qkv_hm", ldc_pad=0))
        cs.append(dict(M=385, N=768, K=768, ldc_pad=0, bias=False))      # (the dX form: zero instead of the bias as the first C operand)
        return {_name(k): k for k in cs}
    Ms = {"k64": (1, 127, 128, 129, 257), "k128": (1, 127, 128, 129, 257), "pp_big": (1, 255, 256, 257, 513), "pp_small": (127, 129, 385)}[form]
    Ns = {"k64": (64, 192), "k128": (128, 384), "pp_big": (256, 768), "pp_small": (256, 768)}[form]
    Ks = (64, 128, 192, 384) if form in ("k64", "k128") else (64, 128, 192, 384, 768)
    for M in Ms:
        for N in Ns:
            for K in Ks:
                cs.append(dict(M=M, N=N, K=K))      # BIAS, fp16, ldc = N + 8: the 16-byte store path of the shipped calls
    # the epilogues at one ragged M (inject: M + 1 = 2 passes of L rows)
    Me = 385 if form == "pp_small" else 257
    Ne = Ns[1]
    for K in (64, 192):
        cs += [dict(M=Me, N=Ne, K=K, ldc_pad=4),      # fp16 rows that are only 8-byte aligned: the generic epilogue
               dict(M=Me, N=Ne, K=K, out="f32", ldc_pad=4),
               dict(M=Me + 1, N=Ne, K=K, maps="amap"),
               dict(M=Me, N=Ne, K=K, epi="bias_resid", out="f32", ldc_pad=4),
               dict(M=Me, N=Ne, K=K, epi="bias_resid", out="f16", ldc_pad=4),
               dict(M=Me, N=Ne, K=K, epi="bias_resid", out="f32", ldc_pad=4, inplace=True),
               dict(M=Me + 1, N=Ne, K=K, epi="inject", out="f32", ldc_pad=4, maps="engine"),
               dict(M=Me, N=Ne, K=K, epi="posemb", out="f32", ldc_pad=4),
               dict(M=Me, N=960 if form == "k64" else 2304, K=K, epi="qkv_hm", ldc_pad=0)]
    cs.append(dict(M=Me, N=Ne, K=1536, epi="posemb", out="f32", ldc_pad=4))
    # element dropout + DropPath: passes shorter than a tile, passes a 128-row tile straddles, passes of a 256-row tile's height
    for rpp in (100, 130, 256):
        cs.append(dict(M=Me, N=Ne, K=64, epi="bias_resid", out="f32", ldc_pad=4, drop=(0.25, 0.5, rpp)))
    return {_name(k): k for k in cs}


# Natural dispatch: products of the shipped step that the fill rule of launch_nt_bn sends to the ping-pong kernel (M >= 8192, N = 768,
# 256-row tiles filling 80 % of their rounds) and that have no unit test of their own; operands generated on the device.
NATURAL = {
    "adapter-dx-K192": dict(M=17500, N=768, K=192, ldc_pad=8),
    "adapter-dx-K384": dict(M=20002, N=768, K=384, ldc_pad=8),
    "patch-embed-posemb": dict(M=20000, N=768, K=1536, epi="posemb", out="f32", ldc_pad=4),
    "injector-cmap-K192": dict(M=20000, N=768, K=192, epi="inject", out="f32", ldc_pad=4, maps="engine"),
}


def run_gpu(ops, c, tile_h, dev="cuda"):
    """One mt_gemm_nt_f16 call of the case on the device -> {"ratio", "at", "where", "canary", "nan"} (+ for a dropout case "dropped",
    "dropped_exact", "mixed_passes")."""
    from modaltune_amd._lib import rowmap
    d = lambda t: None if t is None else t.to(dev)
    buf = c.c_init.to(dev).clone()
    before = buf.clone()
    pm = rowmap(c.L, c.L + 1, 1)
    kw = dict(lda=c.lda, ldc=c.ldc, epilogue=EPI[c.epi], bias=d(c.bias), amap=pm if c.maps == "amap" else None, cmap=pm if c.maps else None)
    if c.epi in ("bias_resid", "inject"):
        kw.update(resid=buf if c.inplace else d(c.resid), ldr=c.ldr)
        if c.inplace and c.maps:
            kw["rmap"] = pm
        elif c.maps == "engine":
            kw["rmap"] = rowmap(c.L, 0, 0)
    if c.epi == "inject":
        kw["colscale"] = d(c.gamma)
    if c.epi == "posemb":
        kw.update(pos_table=d(c.tab), pos_row=d(c.pos_row), pos_col=d(c.pos_col))
    res, mask = {}, None
    keep = []      # (tensors the launch reads stay referenced until it has run)
    if c.drop:
        p, pp, rpp = c.drop
        rng = torch.tensor([123, 456, 7, 0], dtype=torch.int32, device=dev)
        ones = torch.ones(c.M, c.N, device=dev)
        for path_site in range(41, 57):      # the first DropPath site that drops one pass and keeps another (the mask is read from the device)
            spec = ops.dropout_spec(rng, 40, p, path_site, pp, rpp)
            mk = torch.zeros(c.M, c.N, device=dev)
            ops.dropout_f32(ones, mk, c.M, c.N, spec)
            torch.cuda.synchronize()
            alive = [bool((mk[a:a + rpp] != 0).any()) for a in range(0, c.M, rpp)]
            if any(alive) and not all(alive):
                break
        res["mixed_passes"] = any(alive) and not all(alive)
        mask = mk.to(c.device)
        kw["drop"] = spec
        keep += [rng, spec]
    ops.gemm_nt(d(c.A_buf), d(c.W), buf, c.M, c.N, c.K, **kw)
    torch.cuda.synchronize()
    ref, bound = reference(c, mask)
    got = logical(c, buf).to(c.device)
    ratio, at = errors(got, ref, bound)
    changed, first = check_untouched(before, buf, c.written)
    res.update(ratio=ratio, at=list(at), where=where(at, tile_h), canary=changed, canary_first=first, nan=int(torch.isnan(got).sum()))
    if c.drop:
        dead = mask == 0
        res["dropped"] = int(dead.sum())
        res["dropped_exact"] = bool(torch.equal(got[dead].view(torch.int32), c.resid_vals[dead].view(torch.int32)))
    return res


def failure(name, r):
    """None, or what is wrong with the result of one case."""
    bad = []
    if not r["ratio"] <= 1.0:
        bad.append(f"worst |got - ref| / bound = {r['ratio']:.3g} > 1 at {r['where']}")
    if r["canary"]:
        bad.append(f"{r['canary']} elements outside the written ones changed (first: flat index {r['canary_first']})")
    if "dropped" in r and not (r["dropped"] > 0 and r["dropped_exact"] and r["mixed_passes"]):
        bad.append(f"dropout: {r['dropped']} dropped elements, equal to resid bit for bit: {r['dropped_exact']}, "
                   f"a dropped and a kept pass: {r['mixed_passes']}")
    return f"{name}: " + "; ".join(bad) if bad else None
