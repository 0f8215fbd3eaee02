"""CPU test of what the K loops of the time-Winograd kernels spend between their MFMAs (csrc/cgemm_tw.hip, csrc/cgemm_tw2.hip compiled
to gfx950 listings with the build's flags; skipped without hipcc), against the counts of the build before the K-loop address work
("K loops: addresses and transforms out of the MFMAs' way"): profiles/tw_kloop_alu/kloop_parent.json, written by

    python tests/test_tw_kloop_alu_host.py PARENT_cgemm_tw.s PARENT_cgemm_tw2.s > profiles/tw_kloop_alu/kloop_parent.json

from the parent's listings.  No count is typed in here.

A K-LOOP COPY is a loop that holds an MFMA: a backward branch to a label, and where the compiler lays the blocks of one loop out
with several backward branches (the unpaired kernels: branches back to the blocks of the waves with two, one and no second staging
item) their spans, which overlap, count as ONE copy.  Its counts are those of all instructions between the first label and the last
backward branch, the blocks of the masked staging path included (instructions move between neighbouring blocks with every edit,
the loop's sum is what the listing holds for it).  Per instantiation the copies come in listing
order, which is the order of the source's `run(...)` calls.  Kept fixed, loop copy by loop copy:

  (a) MFMA, `ds_write`, global-load and barrier counts equal the parent's;
  (b) no more `ds_read` and no more vector-ALU instructions (`v_*` other than MFMA) than the parent's copy;
  (c) the copies of the forms that were changed have FEWER vector-ALU instructions: every copy of cconv_tw_kernel but the unpaired
      odd-row kernel's (operand reads on per-lane LDS bases + compile-time offsets, staging loads on a scalar base + 32-bit lane
      offset) and every copy of cconv_tw2_kernel (staging loads; waves 0 .. 2 and the edge waves also their operand reads).  The
      unpaired odd-row kernel cconv_tw_kernel<1, ., ., ., 1> keeps its forms (csrc/cgemm_tw.hip, KBASE) and is held to (a) and (b);
  (d) in those forms whose transform runs one MFMA ahead -- the changed cconv_tw_kernel copies, and the copies of waves 0 .. 2 of a
      full tile in cconv_tw2_kernel (16 MFMA slots x 2 k-steps = 32 MFMAs) -- no `s_nop` stands between a transform (`v_fma_f32` /
      `v_fmac_f32`) and the MFMA that reads its result, and such a loop holds fewer `s_nop` than the parent's;
  (e) the paired cconv_tw_kernel loops open with a k-step that carries no staging: from the loop's label to its ninth (odd rows:
      seventh) MFMA every vector-ALU instruction is a transform (`v_fma_f32` / `v_fmac_f32`) -- no integer instruction at all;
  (f) two waves per SIMD (at most 256 VGPRs) and 0 bytes of scratch in every instantiation of both files.

tests/test_tw_stage_wait_host.py keeps the staging-load distances of the same listings."""
import importlib.util
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dccrn-vae_amd", "csrc")
PARENT = os.path.join(ROOT, "profiles", "tw_kloop_alu", "kloop_parent.json")
KEYS = (("mfma", "v_mfma"), ("ds_read", "ds_read"), ("ds_write", "ds_write"), ("barrier", "s_barrier"), ("load", "global_load"),
        ("nop", "s_nop"))


def _swd():
    spec = importlib.util.spec_from_file_location("stage_wait_distance", os.path.join(ROOT, "tests", "tools", "stage_wait_distance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def short(kernel):
    """cconv_tw_kernel<0,8,1,0,2> from the mangled name."""
    m = re.search(r"\d+(cconv_tw2?_kernel)I((?:L[ib]\d+E)+)E", kernel)
    return m.group(1) + "<" + ",".join(re.findall(r"L[ib](\d+)E", m.group(2))) + ">" if m else None


def _nops_before_product(body):
    """Number of MFMAs of the loop that stand behind `transform, s_nop` with the transform writing the MFMA's B operand."""
    ins = [(op, args) for lab, op, args in body if op]
    hits = 0
    for k, (op, args) in enumerate(ins):
        if not op.startswith("v_mfma"):
            continue
        j = k - 1
        while j >= 0 and ins[j][0] == "s_nop":
            j -= 1
        if j < k - 1 and j >= 0 and ins[j][0].startswith(("v_fma_f32", "v_fmac_f32")) and ins[j][1][0] == args[2]:
            hits += 1
    return hits


def _spans(ins):
    """(first, last) instruction index of every loop copy that holds an MFMA: the backward branches' spans, overlapping ones merged."""
    pos = {lab: k for k, (lab, _, _) in enumerate(ins) if lab}
    spans = sorted((pos[args[0]], k) for k, (lab, op, args) in enumerate(ins)
                   if op and op.startswith(("s_branch", "s_cbranch")) and args and pos.get(args[0], k + 1) <= k)
    spans = [(a, b) for a, b in spans if any(op and op.startswith("v_mfma") for _, op, _ in ins[a:b + 1])]
    merged = []
    for a, b in spans:
        if merged and a <= merged[-1][1]:
            merged[-1] = (merged[-1][0], max(merged[-1][1], b))
        else:
            merged.append((a, b))
    return merged


def loop_counts(path):
    """{short kernel name: [counts per K-loop copy, in listing order]}"""
    tool = _swd()
    out = {}
    for name, ins in tool._kernels(path).items():
        key = short(name)
        if key is None:
            continue
        found = []
        for a, b in _spans(ins):
            body = ins[a:b + 1]
            c = {k: 0 for k, _ in KEYS}
            c["valu"] = 0
            for _, op, _ in body:
                if not op:
                    continue
                for k, prefix in KEYS:
                    if op.startswith(prefix):
                        c[k] += 1
                if op.startswith("v_") and not op.startswith("v_mfma"):
                    c["valu"] += 1
            c["nop_before_product"] = _nops_before_product(body)
            found.append(c)
        out[key] = found
    return out


def resources(path):
    """{short kernel name: (VGPRs, scratch bytes)} from the listing's metadata."""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(path).read(), re.S):
        key = short(m.group(1))
        if key:
            out[key] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1)),
                        int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)))
    return out


if __name__ == "__main__":
    res = {}
    for p in sys.argv[1:]:
        res.update(loop_counts(p))
    print(json.dumps(res, indent=1, sort_keys=True))
    sys.exit(0)

import pytest  # noqa: E402

sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not os.path.exists(G.HIPCC):
        pytest.skip("no hipcc here")
    d = tmp_path_factory.mktemp("tw_kloop_listings")
    procs = {}
    for name in ("cgemm_tw2", "cgemm_tw"):
        out = str(d / (name + ".s"))
        cmd = [G.HIPCC] + G.HIP_FLAGS + ["--offload-device-only", "-S", os.path.join(CSRC, name + ".hip"), "-o", out]
        procs[name] = (out, subprocess.Popen(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    res = {}
    for name, (out, pr) in procs.items():
        log = pr.communicate()[0]
        assert pr.returncode == 0, log[-2000:]
        res[name] = out
    return res


@pytest.fixture(scope="module")
def both(listings):
    this = {}
    for path in listings.values():
        this.update(loop_counts(path))
    with open(PARENT) as f:
        parent = json.load(f)
    return parent, this


def _kept(kernel):
    """The unpaired odd-row kernel: cconv_tw_kernel<PH = 1, CIK, LEFT, STATS, NCT = 1>."""
    return bool(re.match(r"cconv_tw_kernel<1,\d+,\d,\d,1>$", kernel))


def _ahead(kernel, c):
    """The loop copies whose transform runs one MFMA ahead."""
    return (kernel.startswith("cconv_tw_kernel") and not _kept(kernel)) or (kernel.startswith("cconv_tw2_kernel") and c["mfma"] == 32)


def test_every_loop_copy_is_there(both):
    parent, this = both
    assert sorted(parent) == sorted(this) and len(parent) == 24
    for k in parent:
        assert len(parent[k]) == len(this[k]) and parent[k], (k, len(parent[k]), len(this[k]))


def test_work_per_loop_copy_is_the_parents(both):
    parent, this = both
    for k in sorted(parent):
        for n, (p, t) in enumerate(zip(parent[k], this[k])):
            print(k, n, "parent", p, "this", t)
            for key in ("mfma", "ds_write", "load", "barrier"):
                assert t[key] == p[key], (k, n, key, p, t)
            assert t["ds_read"] <= p["ds_read"], (k, n, p, t)
            assert t["valu"] <= p["valu"], (k, n, p, t)


def test_changed_forms_issue_fewer_vector_alu_instructions(both):
    parent, this = both
    kept = 0
    for k in sorted(parent):
        for n, (p, t) in enumerate(zip(parent[k], this[k])):
            if _kept(k):
                assert t["valu"] <= p["valu"], (k, n, p, t)                  # (its forms are the parent's: (a) and (b) above)
                kept += 1
            else:
                assert t["valu"] < p["valu"], (k, n, p, t)
    assert kept == 4


def test_no_nop_between_a_transform_and_its_product(both):
    parent, this = both
    seen = 0
    for k in sorted(parent):
        for n, (p, t) in enumerate(zip(parent[k], this[k])):
            if not _ahead(k, t):
                continue
            seen += 1
            assert p["nop_before_product"] > 0, (k, n, p)          # (the parent had them: the check sees what it is meant to see)
            assert t["nop_before_product"] == 0, (k, n, t)
            assert t["nop"] < p["nop"], (k, n, p, t)
    for k in this:                                                  # (waves 0 .. 2 of a full tile: one copy, with two co tiles two)
        if k.startswith("cconv_tw2_kernel"):
            assert sum(1 for c in this[k] if c["mfma"] == 32) == int(k[-2]), (k, [c["mfma"] for c in this[k]])
    assert seen == 4 + 4 + 2 * 4 + 4 + 2 * 4        # tw: even rows unpaired, paired, odd rows paired (early, late); tw2: NCT 1, 2 (early, late)


def test_a_k_step_without_staging_has_no_integer_valu(listings):
    tool = _swd()
    seen = 0
    for name, ins in tool._kernels(listings["cgemm_tw"]).items():
        m = re.match(r"cconv_tw_kernel<(\d),\d+,\d,\d,2>$", short(name) or "")
        if not m:
            continue
        ntw = 9 if m.group(1) == "0" else 7
        spans = [(a, b) for a, b in sorted(tool._loop_spans(ins)) if any(op and op.startswith("v_mfma") for _, op, _ in ins[a:b + 1])]
        assert spans, name
        heads = []                                                  # (a span that begins inside another one is no loop head)
        for a, b in spans:
            if not heads or a > heads[-1][1]:
                heads.append((a, b))
        assert len(heads) == (1 if m.group(1) == "0" else 2), (name, heads)    # even rows: one copy; odd rows: early and late staging
        for a, b in heads:
            mfma, valu = 0, []
            for _, op, _ in ins[a:b + 1]:
                if not op:
                    continue
                if op.startswith("v_mfma"):
                    mfma += 1
                    if mfma == ntw:
                        break
                elif op.startswith("v_"):
                    valu.append(op)
            print(short(name), ins[a][0], valu)
            assert mfma == ntw and len(valu) >= ntw - 1, (name, mfma, valu)
            assert all(op.startswith(("v_fma_f32", "v_fmac_f32")) for op in valu), (name, valu)
            seen += 1
    assert seen >= 8


def test_resources(listings):
    seen = 0
    for path in listings.values():
        for k, (vgpr, scratch) in resources(path).items():
            assert vgpr <= 256 and scratch == 0, (k, vgpr, scratch)
            seen += 1
    assert seen == 24
