"""Compare the gfx950 machine code of two builds, kernel by kernel, without disassembling anything.

    python tests/tools/kernel_code_diff.py BEFORE_DIR AFTER_DIR        (no GPU needed)

Each directory holds the objects (*.o) that `__graft_entry__.build()` leaves beside the sources (csrc/), one built from the parent
commit (e.g. in a `git worktree`), one from this tree, both with `__graft_entry__.HIP_FLAGS`.  Per unit: the device code object is
taken out of the object's .hip_fatbin section (llvm-objcopy) and unbundled (clang-offload-bundler), its function symbols are read with
llvm-readelf, and the bytes [st_value, st_value + st_size) of every function are hashed out of .text.  Printed per unit: kernels and
.text bytes before -> after, the symbols that are new, and the surviving symbols whose bytes differ.  Exit status 1 if any unit has a
new symbol or a surviving symbol with different bytes.

Symbols are matched by mangled name.  A kernel whose template parameter list changed is matched by its template arguments with the
removed positions struck out: RENAMED below is that map (empty unless the pull request at hand removes template parameters).
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

# kernel name -> {position of a template argument the BEFORE build had and the AFTER build has not: the value the AFTER build fixes it
# to, as a function of the BEFORE argument list}.  A BEFORE kernel with another value there has no successor and counts as removed.
# An entry describes ONE pull request and goes away once that is merged: applied to a BEFORE build that already has the short list it
# would strike out live arguments.  How the removal of DBG, RDW and WVEC from the time-Winograd kernel was written:
#   cconv_tw_kernel<PH, CIK, LEFT, DBG, RDW, WVEC, STATS, NCT> -> <PH, CIK, LEFT, STATS, NCT>   with DBG = 0, RDW = 2, WVEC = (PH == 0)
#   "cconv_tw_kernel": {3: lambda a: 0, 4: lambda a: 2, 5: lambda a: int(a[0] == 0)}
RENAMED = {}
_TMPL = re.compile(r"^(_ZN12_GLOBAL__N_1\d+(%s))I((?:L[ib]\d+E)+)E(.*)$" % "|".join(RENAMED)) if RENAMED else None


def match_key(sym: str, before: bool) -> str:
    """The name two builds share: the mangled name, or for RENAMED kernels `name<args>` without the removed arguments."""
    m = _TMPL.match(sym) if _TMPL else None
    if not m:
        return sym
    args = [int(a) for a in re.findall(r"L[ib](\d+)E", m.group(3))]
    if before:
        fixed = RENAMED[m.group(2)]
        if any(args[i] != f(args) for i, f in fixed.items()):
            return sym
        args = [a for i, a in enumerate(args) if i not in fixed]
    return "%s<%s>%s" % (m.group(2), ", ".join(map(str, args)), m.group(4))


def run(*cmd) -> str:
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def functions(obj: str, tmp: str):
    """(.text size, {symbol: sha256 of its bytes}) of the gfx950 code object inside a host object; None without device code."""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, "copy.o")],
                   capture_output=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET, "--output=" + co)
    text = None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "-SW", co).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text = (int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16))
    if text is None:
        return 0, {}
    ndx, addr, off, size = text
    blob = open(co, "rb").read()
    out = {}
    for line in run(os.path.join(LLVM, "llvm-readelf"), "-sW", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] == str(ndx):
            v, n = int(f[1], 16), int(f[2])
            assert addr <= v and v + n <= addr + size, f[7]
            out[f[7]] = hashlib.sha256(blob[off + v - addr: off + v - addr + n]).hexdigest()
    return size, out


def main(before_dir: str, after_dir: str) -> int:
    units = sorted({f for d in (before_dir, after_dir) for f in os.listdir(d) if f.endswith(".o")})
    bad = 0
    tot = [0, 0, 0, 0]
    print("| unit | kernels | .text bytes | new | differ |\n|---|---|---|---|---|")
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            sides = []
            for d, is_before in ((before_dir, True), (after_dir, False)):
                p = os.path.join(d, u)
                r = functions(p, tmp) if os.path.exists(p) else None
                keyed = {} if r is None else {match_key(s, is_before): h for s, h in r[1].items()}
                assert r is None or len(keyed) == len(r[1]), "two kernels of one build share a name"
                sides.append((0 if r is None else r[0], keyed))
            (tb, fb), (ta, fa) = sides
            if not fb and not fa:
                continue
            new = sorted(set(fa) - set(fb))
            differ = sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
            bad += len(new) + len(differ)
            for i, v in enumerate((len(fb), len(fa), tb, ta)):
                tot[i] += v
            print(f"| `{u[:-2]}.hip` | {len(fb)} -> {len(fa)} | {tb} -> {ta} | {len(new)} | {len(differ)} |")
            for k in new:
                print(f"    new:    {k}")
            for k in differ:
                print(f"    differ: {k}")
    print(f"| all | {tot[0]} -> {tot[1]} | {tot[2]} -> {tot[3]} | | |")
    print("RESULT:", "identical code for every surviving kernel, no new kernel" if not bad else f"{bad} new or different kernels")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
