"""Registers, spills and LDS of EVERY kernel (spill_table.py lists the spilling and the hot ones), from the code-object metadata of the
library's sources compiled to ISA with the build's own flags -- and the comparison of two such tables, for a change that must leave
existing kernels as they were:

    python tools/diag/kernel_regs.py > new.txt                      (in each tree)
    python tools/diag/kernel_regs.py --diff old.txt new.txt         -> profiles/

A kernel that gained a trailing defaulted `bool` template parameter (`template <..., bool DET = false>`) is matched with its old symbol:
the `false` instantiation IS the old kernel -- also when the new forms bring trailing kernel parameters along (`DropArgs drop` of the
prompt self-attention's DROP forms), which the `false` instantiation never reads -- and when the kernel was no template before
(`adamw_groups_kernel<EMA>`: its qualified name is compared, the template argument list renumbers the parameter list's substitutions)."""
import os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIELDS = ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "lds_bytes", "scratch_bytes")


def table():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    tmp = tempfile.mkdtemp()

    def isa(src):
        out = os.path.join(tmp, src.replace(".hip", ".s"))
        flags = [f for f in ge._flags_for(src) if f != "-fPIC"]
        subprocess.run([ge.HIPCC] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(ge.CSRC, src)], check=True, stderr=subprocess.DEVNULL)
        return out
    with ThreadPoolExecutor(max_workers=4) as ex:
        paths = list(ex.map(isa, [s for s in ge.SOURCES if s != "layer.hip"]))
    print("# file kernel " + " ".join(FIELDS))
    for f in sorted(paths):
        for chunk in open(f).read().split("- .agpr_count:")[1:]:
            num = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, chunk).group(1))
            print(os.path.basename(f)[:-2], re.search(r"\.name:\s+(\S+)", chunk).group(1), num("vgpr_count"), int(re.match(r"\s*(\d+)", chunk).group(1)),
                  num("sgpr_count"), num("vgpr_spill_count"), num("sgpr_spill_count"), num("group_segment_fixed_size"), num("private_segment_fixed_size"))


def load(path):
    return {(l.split()[0], l.split()[1]): l.split()[2:] for l in open(path) if l.strip() and not l.startswith("#")}


def nested_name(sym):
    """`_ZN<len><id>...` of a mangled symbol up to the end of its last length-prefixed identifier (None: not a nested name)."""
    if not sym.startswith("_ZN"):
        return None
    i = 3
    while True:
        m = re.match(r"\d+", sym[i:])
        if not m:
            return sym[:i] if i > 3 else None
        i += len(m.group(0)) + int(m.group(0))


def diff(old_path, new_path):
    old, new = load(old_path), load(new_path)

    def twin(key):
        if key in new:
            return key
        f, n = key
        for c in new:         # `Lb0E` appended to the template argument list (a non-template kernel also gains `I...E` and its return type `v`)
            if c[0] == f and (c[1].replace("Lb0EE", "E", 1) == n or c[1].replace("ILb0EEEv", "E", 1) == n):
                return c
        for c in new:         # ... and with it trailing kernel parameters that only the `true` form reads (their mangled types follow the old list)
            if c[0] == f and "Lb0EE" in c[1] and c[1].replace("Lb0EE", "E", 1).startswith(n):
                return c
        q = nested_name(n)    # ... and a kernel that was NO template before: its new template argument list renumbers the substitutions
        if q is not None and n[len(q)] == "E":      # (S0_ -> S1_) of the parameter list, so only the qualified name is compared
            for c in new:
                if c[0] == f and c[1].startswith(q + "ILb0EEEv"):
                    return c
        return None
    pairs = {k: twin(k) for k in old}
    gone = [k for k, t in pairs.items() if t is None]
    changed = [(k, old[k], new[t]) for k, t in pairs.items() if t is not None and old[k] != new[t]]
    renamed = sum(1 for k, t in pairs.items() if t is not None and t != k)
    added = sorted(set(new) - set(pairs.values()))
    print(f"kernels before: {len(old)}; after: {len(new)}; same symbol: {len(old) - renamed - len(gone)}; matched as the `false` instantiation of "
          f"a new trailing bool template parameter: {renamed}; missing: {len(gone)}; new: {len(added)}")
    print(f"existing kernels whose figures ({', '.join(FIELDS)}) changed: {len(changed)}")
    for k, a, b in changed:
        print("  CHANGED", k[0], k[1], a, "->", b)
    for k in gone:
        print("  MISSING", k[0], k[1])
    print("\nnew kernels:  file kernel " + " ".join(FIELDS))
    for k in added:
        print(" ", k[0], k[1], " ".join(new[k]))
    return 1 if (changed or gone) else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    table()
