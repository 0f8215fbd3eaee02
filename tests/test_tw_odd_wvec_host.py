"""CPU test of the weight loads of the odd-row phase of the time-Winograd transposed conv (tests/tools/stage_wait_distance.py on the
gfx950 listing of csrc/cgemm_tw.hip, compiled with the build's flags; skipped without hipcc).

The odd-row phase (cconv_tw_kernel<1, ...>) takes its weights as two 16-byte loads per k-step from [64 lanes][4 tiles] groups, as the
even-row phase does.  Its seven tiles per wave leave the eighth component of the second load without a reader; the kernel reads that
register in front of the group's first MFMA so that it stays the load's until the load has landed (otherwise the register is handed
out again and a wait for ALL loads sits right behind the load's issue: DESIGN.md 3.1e, *Weights*).  Kept fixed here, for the eight
odd-row instantiations and per MFMA-carrying loop:

  (a) at least three MFMAs per weight load (full loops 28 / 8, the unpaired kernels' shorter loop copies 20 / 6 and 13 / 4; one load
      per MFMA with 4-byte loads);
  (b) every staging load is retired within two iterations, and never less than 7 MFMAs after its issue (with the dead register handed
      out again: 0 - 1);
  (c) the paired kernels keep the distances of this build, PAIRED_FLOOR per loop copy in listing order (early, late staging).

All sixteen cconv_tw_kernel instantiations keep 0 bytes of scratch, at most 256 VGPRs and two waves per SIMD (the listing's own
metadata: 512 threads per workgroup and one workgroup per CU, or 256 threads and two)."""
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

MIN_MFMA_PER_WEIGHT_LOAD = 3
MIN_DISTANCE = 7
PAIRED_FLOOR = (7, 7)            # early copy, late copy (staging loads in front of the k-step's weight loads)


def _tool():
    spec = importlib.util.spec_from_file_location("stage_wait_distance", os.path.join(ROOT, "tests", "tools", "stage_wait_distance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(G.HIPCC):
        pytest.skip("no hipcc here")
    out = str(tmp_path_factory.mktemp("tw_odd_wvec") / "cgemm_tw.s")
    cmd = [G.HIPCC] + G.HIP_FLAGS + ["--offload-device-only", "-S", os.path.join(CSRC, "cgemm_tw.hip"), "-o", out]
    pr = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert pr.returncode == 0, pr.stdout[-2000:]
    return out, _tool().loops(out, ("cconv_tw_kernel",))


def _args(kernel):
    m = re.search(r"cconv_tw_kernelILi(\d)ELi\d+ELb(\d)ELb(\d)ELi(\d)E", kernel)
    return tuple(int(x) for x in m.groups()) if m else None                          # PH, LEFT, STATS, NCT


def _odd(listing):
    found = {_args(k): v for k, v in listing[1].items() if _args(k) and _args(k)[0] == 1}
    assert sorted(found) == [(1, left, stats, nct) for left in (0, 1) for stats in (0, 1) for nct in (1, 2)]
    return found


def test_three_mfmas_per_weight_load(listing):
    for args, found in _odd(listing).items():
        assert len(found) == (3 if args[3] == 1 else 2), (args, found)               # unpaired: three loop copies; paired: early, late
        for lp in found:
            print(args, lp)
            assert lp.mfma >= 13 and lp.weight_loads >= 1, (args, lp)
            assert lp.mfma >= MIN_MFMA_PER_WEIGHT_LOAD * lp.weight_loads, (args, lp)
        assert (found[0].mfma, found[0].weight_loads) == (28, 8), (args, found[0])   # the full loop: 2 k-steps x 2 copies of the ring


def test_staging_loads_fly_at_least_seven_mfmas(listing):
    for args, found in _odd(listing).items():
        for k, lp in enumerate(found):
            assert lp.staging_loads >= 4, (args, lp)
            assert not any(lp.open), (args, lp)                                      # retired within two iterations
            assert min(lp.distances) >= MIN_DISTANCE, (args, lp)
            if args[3] == 2:
                assert min(lp.distances) >= PAIRED_FLOOR[k], (args, k, lp)


def test_resources_of_all_sixteen(listing):
    text = open(listing[0]).read()
    seen = 0
    for m in re.finditer(r"\.amdhsa_kernel (\S*cconv_tw_kernel\S*)(.*?)\.end_amdhsa_kernel", text, re.S):
        name, body = m.group(1), m.group(2)
        if "pack_" in name:
            continue
        nct = _args(name)[3]
        scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1))
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1))
        assert scratch == 0 and vgpr <= 256, (name, scratch, vgpr)
        # the kernel's entry in the metadata note: registers per lane (vector + accumulator) and the workgroup size
        meta = re.search(r"\.max_flat_workgroup_size: (\d+)\n\s+\.name:\s+" + re.escape(name) + r"\n(.*?)\.vgpr_count:\s+(\d+)", text, re.S)
        assert meta, name
        wg, count = int(meta.group(1)), int(meta.group(3))
        assert int(re.search(r"\.private_segment_fixed_size: (\d+)", meta.group(2)).group(1)) == 0, name
        assert wg == 256 * nct, (name, wg)
        # a SIMD holds 512 registers per lane, handed out in blocks of 8: two waves of this kernel, not one and not three; a workgroup
        # puts nct waves on each SIMD (4 nct waves on four SIMDs), so 2 / nct workgroups share a CU
        alloc = (count + 7) // 8 * 8
        assert 512 // alloc == 2, (name, count)
        seen += 1
    assert seen == 16
