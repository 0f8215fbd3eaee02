"""CPU test of how long the K loops of the time-Winograd kernels let a staging load fly (tests/tools/stage_wait_distance.py on the gfx950
listings of csrc/cgemm_tw2.hip and csrc/cgemm_tw.hip, compiled with the build's flags; skipped without hipcc).

A wave's loads return in order, so the first `s_waitcnt vmcnt(N)` with N below the number of loads issued since retires a staging
load, whatever it was placed for.  The tap-left conv form once waited for its staging loads in the MFMA slot that issued them (the
window was loaded as an aligned vector plus the column in front; the compiler merged the two, re-assembled the loop-carried registers
right behind the loads and waited there), and the roles with empty MFMA slots waited for ALL loads behind every weight load whose dead
components had been handed out again.  Kept fixed here, per instantiation and per MFMA-carrying loop:

  (a) no staging load is retired before the next MFMA after it, and no cconv_tw2_kernel loop has a vmcnt wait of any N between a
      staging load and the next MFMA;
  (b) loop copy by loop copy, the distances of a tap-left cconv_tw2_kernel equal those of the tap-right one with the same STATS, NCT;
  (c) every distance is at least 8 MFMAs -- a floor, not a target: the full-tile loops of the conv form have 14 - 15.  Loops that were
      below 8 before the tap-left fix keep the value measured then as their floor (BELOW_8: the in-order rule against the weight ring,
      not the defect above).

The kernels keep 0 bytes of scratch, at most 256 VGPRs and two waves per SIMD (the listing's own metadata)."""
import importlib.util
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "i-dccrn-vae_amd", "csrc")
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

FLOOR = 8
# min distance per loop, in listing order, where the build before the tap-left fix had less than FLOOR (measured with the tool on that
# build's listings; the same for both STATS).  cconv_tw2_kernel<RIGHT, *, 1>: the two edge-workgroup loops (odd waves 2, even waves 5:
# item 1 is loaded at slot 13, and the wait for the next k-step's second weight group retires it).  cconv_tw2_kernel<RIGHT, *, 2> had 2
# (wave 7) and 3 (odd edge waves) from the dead-weight-register waits; both are 14 and 11 now and need no entry.  cconv_tw_kernel<1, ...>
# (odd-row phase): two 16-byte weight loads per k-step and a ring of two k-steps retire a staging load after 6 - 7 MFMAs.
BELOW_8 = {
    ("tw2", 1): {2: 2, 3: 5},
    ("tw", 1, 1): {0: 7, 1: 6, 2: 6},
    ("tw", 1, 2): {0: 7, 1: 7},
}


def _tool():
    spec = importlib.util.spec_from_file_location("stage_wait_distance", os.path.join(ROOT, "tests", "tools", "stage_wait_distance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    if not os.path.exists(G.HIPCC):
        pytest.skip("no hipcc here")
    d = tmp_path_factory.mktemp("tw_listings")
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
    tool = _tool()
    return {name: (path, tool.loops(path)) for name, path in res.items()}


def _tw2_args(kernel):
    m = re.search(r"cconv_tw2_kernelILb(\d)ELb(\d)ELi(\d)E", kernel)
    return (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else None       # LEFT, STATS, NCT


def _tw_args(kernel):
    m = re.search(r"cconv_tw_kernelILi(\d)ELi\d+ELb(\d)ELb(\d)ELi(\d)E", kernel)
    return tuple(int(x) for x in m.groups()) if m else None                          # PH, LEFT, STATS, NCT


def test_every_instantiation_and_loop_copy_is_seen(listings):
    tw2 = {_tw2_args(k): v for k, v in listings["cgemm_tw2"][1].items() if _tw2_args(k)}
    assert sorted(tw2) == [(left, stats, nct) for left in (0, 1) for stats in (0, 1) for nct in (1, 2)]
    for (left, stats, nct), found in tw2.items():
        # full and edge tiles x waves 0 .. 2 and wave 3 (x early and late staging with two co tiles)
        assert len(found) == 4 * nct, (left, stats, nct, len(found))
        assert all(lp.staging_loads in (4, 8) and lp.weight_loads == 8 for lp in found), found
    tw = {_tw_args(k): v for k, v in listings["cgemm_tw"][1].items() if _tw_args(k)}
    assert len(tw) == 16 and all(found and all(lp.staging_loads >= 4 for lp in found) for found in tw.values())


def test_no_staging_load_is_waited_for_in_its_slot(listings):
    for name in ("cgemm_tw2", "cgemm_tw"):
        for kernel, found in listings[name][1].items():
            for lp in found:
                print(kernel, lp)
                assert min(lp.distances) >= 1, (kernel, lp)
                assert not any(lp.open), (kernel, lp)             # (every staging load is retired within two iterations)
                if name == "cgemm_tw2":
                    assert lp.slot_waits == 0, (kernel, lp)


def test_tap_left_equals_tap_right(listings):
    tw2 = {_tw2_args(k): v for k, v in listings["cgemm_tw2"][1].items() if _tw2_args(k)}
    for stats in (0, 1):
        for nct in (1, 2):
            left, right = tw2[(1, stats, nct)], tw2[(0, stats, nct)]
            assert [(lp.mfma, lp.distances) for lp in left] == [(lp.mfma, lp.distances) for lp in right], (stats, nct, left, right)


def test_distance_floor(listings):
    for kernel, found in listings["cgemm_tw2"][1].items():
        if not found:
            continue                                              # (the pack kernel)
        _, _, nct = _tw2_args(kernel)
        for k, lp in enumerate(found):
            floor = BELOW_8.get(("tw2", nct), {}).get(k, FLOOR)
            assert min(lp.distances) >= floor, (kernel, k, lp, floor)
    for kernel, found in listings["cgemm_tw"][1].items():
        if not found:
            continue
        ph, _, _, nct = _tw_args(kernel)
        for k, lp in enumerate(found):
            floor = BELOW_8.get(("tw", ph, nct), {}).get(k, FLOOR)
            assert min(lp.distances) >= floor, (kernel, k, lp, floor)


def test_resources(listings):
    """0 bytes of scratch, at most 256 VGPRs (two waves per SIMD of 512) in every instantiation of the conv form."""
    text = open(listings["cgemm_tw2"][0]).read()
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S*cconv_tw2_kernel\S*)(.*?)\.end_amdhsa_kernel", text, re.S):
        if "pack_" in m.group(1):
            continue
        body = m.group(2)
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        assert scratch == 0 and vgpr <= 256, (m.group(1), scratch, vgpr)
        seen += 1
    assert seen == 8
