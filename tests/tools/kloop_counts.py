"""Instruction counts of the MFMA-carrying basic blocks (the K loops) of every kernel in two gfx950 assembly listings, side by side.

    hipcc <__graft_entry__.HIP_FLAGS> --offload-device-only -S csrc/cgemm_tw2.hip -o after.s      (the same on the parent: before.s)
    python tests/tools/kloop_counts.py before.s after.s [-v]                                        (no GPU needed)

tests/tools/kernel_code_diff.py says WHETHER a kernel's bytes changed; this says what changed in its loops.  Per kernel and basic block
that holds an MFMA: MFMA, other VALU, ds_read, ds_write, global loads, barriers, scratch loads and stores.  A block of BEFORE counts as
kept when AFTER has a block with the same counts (blocks are matched as multisets: labels and block order change with any edit).
Printed per kernel: blocks before -> after, whether every BEFORE block is kept, the BEFORE blocks without a match and (-v) the blocks
only AFTER has.  Exit status 1 if any kernel lost a block."""
import re
import sys
from collections import Counter

KEYS = (("mfma", "v_mfma"), ("scratch_st", "scratch_store"), ("scratch_ld", "scratch_load"), ("ds_read", "ds_read"), ("ds_write", "ds_write"),
        ("barrier", "s_barrier"), ("load", "global_load"))


def blocks(path):
    """{kernel: Counter of the count tuples of its MFMA-carrying basic blocks}"""
    cur, bb, out = None, None, {}
    for line in open(path):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur, bb = m.group(1), "entry"
            continue
        m = re.match(r"^\.LBB(\d+_\d+):", line)
        if m:
            bb = m.group(1)
            continue
        t = line.split()
        if cur is None or not t or t[0][0] in ".;":
            continue
        d = out.setdefault(cur, {}).setdefault(bb, Counter())
        for key, prefix in KEYS:
            if t[0].startswith(prefix):
                d[key] += 1
        if t[0].startswith("v_") and not t[0].startswith("v_mfma"):
            d["valu"] += 1
    return {k: Counter(tuple(sorted(d.items())) for d in v.values() if d["mfma"]) for k, v in out.items()}


def main(before, after, verbose):
    a, b = blocks(before), blocks(after)
    lost = 0
    for k in a:
        if k not in b or not a[k]:
            continue
        miss = a[k] - b[k]
        lost += sum(miss.values())
        print(f"{k}: MFMA blocks {sum(a[k].values())} -> {sum(b[k].values())}, every block of BEFORE kept: {not miss}")
        for x, n in miss.items():
            print(f"    only BEFORE x{n}: {dict(x)}")
        if verbose or miss:
            for x, n in (b[k] - a[k]).items():
                print(f"    only AFTER  x{n}: {dict(x)}")
    return 1 if lost else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "-v"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], "-v" in sys.argv))
