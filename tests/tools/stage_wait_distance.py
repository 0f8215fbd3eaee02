"""How long the K loops of the time-Winograd kernels let a staging load fly: per loop of a gfx950 assembly listing, the number of MFMAs
between the issue of each staging load and the first wait that retires it.

    hipcc <__graft_entry__.HIP_FLAGS> --offload-device-only -S csrc/cgemm_tw2.hip -o tw2.s
    python tests/tools/stage_wait_distance.py tw2.s [more.s ...] [--kernel SUBSTRING]           (no GPU needed)

A wave's vector-memory loads return in order: `s_waitcnt vmcnt(N)` holds the wave until at most N of them are outstanding, so it
retires a load as soon as N is smaller than the number of loads issued from that load on, whatever the wait was placed for.  A wait
for weights that were fetched after a staging load therefore also waits for the staging load, and a wait right behind the staging
loads costs a global round trip in the MFMA slot that issued them.

Per kernel whose name holds SUBSTRING (default: cconv_tw2_kernel and cconv_tw_kernel) and per innermost loop that holds an MFMA (a
backward branch to a label; the loop's blocks are walked in layout order, twice: two consecutive iterations), loads are counted in
issue order.  A load whose destination registers are read by an MFMA before anything else redefines them is a WEIGHT load (it comes
from the weight base); every other load is a STAGING load.  For each staging load of the first iteration: the MFMAs between its issue
and the first `s_waitcnt vmcnt(N)` with N smaller than the number of loads issued from it on ('>= n': not retired within the two
iterations).  Only loads, vmcnt waits and MFMAs are interpreted; of any other instruction just the first operand is read, as the
register it redefines.

Printed per loop: its header label, MFMAs per iteration, loads per iteration (weight + staging), the distances in issue order and,
if there are any, the number of vmcnt waits (of any N) between a staging load and the next MFMA.
As a module: loops(path) -> {kernel: [Loop]} in listing order."""
import re
import sys
from collections import namedtuple

Loop = namedtuple("Loop", "label mfma weight_loads staging_loads distances open slot_waits")
DEFAULT_KERNELS = ("cconv_tw2_kernel", "cconv_tw_kernel")
_LOAD = ("global_load", "buffer_load", "flat_load", "scratch_load")
_REG = re.compile(r"\b([va])(?:(\d+)|\[(\d+):(\d+)\])")


def _regs(operand):
    """The vector / accumulator registers an operand names, as a set of (file, index)."""
    out = set()
    for f, one, lo, hi in _REG.findall(operand):
        if one:
            out.add((f, int(one)))
        else:
            out.update((f, k) for k in range(int(lo), int(hi) + 1))
    return out


def _kernels(path):
    """{kernel: [(label or None, mnemonic, [operands])]} -- the instructions of every kernel in listing order, labels as entries."""
    cur, out = None, {}
    for line in open(path):
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            cur.append((m.group(1), None, None))
            continue
        code = line.split(";")[0].strip()
        if not code or code[0] == ".":
            if code.startswith(".end_amdhsa_kernel") or code.startswith(".Lfunc_end"):
                cur = None
            continue
        t = code.split(None, 1)
        cur.append((None, t[0], [x.strip() for x in t[1].split(",")] if len(t) > 1 else []))
    return out


def _loop_spans(ins):
    """(first, last) instruction index of every innermost loop: a branch to a label at or above it."""
    pos = {lab: k for k, (lab, _, _) in enumerate(ins) if lab}
    spans = []
    for k, (lab, op, args) in enumerate(ins):
        if op and op.startswith(("s_branch", "s_cbranch")) and args and pos.get(args[0], k + 1) <= k:
            spans.append((pos[args[0]], k))
    return [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]


def _vmcnt(op, args):
    if op != "s_waitcnt":
        return None
    m = re.search(r"vmcnt\((\d+)\)", " ".join(args))
    return int(m.group(1)) if m else None


def _walk(label, body):
    stream = body + body                                        # two consecutive iterations
    n = len(body)
    is_load = [bool(op) and op.startswith(_LOAD) for _, op, _ in stream]
    weight = {}
    for k in range(n):
        if not is_load[k]:
            continue
        live, fed = _regs(stream[k][2][0]), False
        for _, op, args in stream[k + 1:]:
            if not op or not args:
                continue
            if op.startswith("v_mfma") and any(live & _regs(a) for a in args[1:3]):
                fed = True
                break
            live -= _regs(args[0])
            if not live:
                break
        weight[k] = fed
    dist, still_open, slot_waits = [], [], 0
    for k in range(n):
        if not is_load[k] or weight[k]:
            continue
        issued, mfma, retired = 0, 0, False
        for _, op, args in stream[k + 1:]:                      # vmcnt waits of any N in what is left of the load's MFMA slot
            if op and op.startswith("v_mfma"):
                break
            if op and _vmcnt(op, args) is not None:
                slot_waits += 1
        for j in range(k, len(stream)):
            _, op, args = stream[j]
            if not op:
                continue
            if is_load[j]:
                issued += 1
            elif op.startswith("v_mfma"):
                mfma += 1
            else:
                w = _vmcnt(op, args)
                if w is not None and w < issued:
                    retired = True
                    break
        dist.append(mfma)
        still_open.append(not retired)
    return Loop(label, sum(1 for _, op, _ in body if op and op.startswith("v_mfma")), sum(1 for k in weight if weight[k]),
                sum(1 for k in weight if not weight[k]), tuple(dist), tuple(still_open), slot_waits)


def loops(path, kernels=DEFAULT_KERNELS):
    out = {}
    for name, ins in _kernels(path).items():
        if not any(s in name for s in kernels):
            continue
        found = []
        for a, b in sorted(_loop_spans(ins)):
            body = ins[a:b + 1]
            if any(op and op.startswith("v_mfma") for _, op, _ in body):
                found.append(_walk(ins[a][0], body))
        out[name] = found
    return out


def main(argv):
    kernels = DEFAULT_KERNELS
    if "--kernel" in argv:
        k = argv.index("--kernel")
        kernels = (argv[k + 1],)
        argv = argv[:k] + argv[k + 2:]
    if not argv:
        sys.exit(__doc__)
    for path in argv:
        print(f"[{path}]")
        for name, found in loops(path, kernels).items():
            print(f"{name}: {len(found)} MFMA loops")
            for lp in found:
                d = " ".join((">= " if o else "") + str(x) for x, o in zip(lp.distances, lp.open))
                print(f"    {lp.label:<12} {lp.mfma:3d} MFMAs  loads {lp.weight_loads} weight + {lp.staging_loads} staging   "
                      f"MFMAs from issue to the retiring wait: {d or '-'}" + (f"   ({lp.slot_waits} vmcnt waits between a staging "
                      "load and the next MFMA)" if lp.slot_waits else ""))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
