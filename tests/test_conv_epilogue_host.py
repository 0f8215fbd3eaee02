"""CPU: the exact-fp32 conv kernel families share ONE epilogue (csrc/conv_epilogue.hpp).

A plain text test over csrc/, so that a further kernel family includes the header instead of growing a copy: the folded batch-norm
expression and the five moment sums of an output point (yr, yi) stand in conv_epilogue.hpp and nowhere else, and every fp32 conv unit
includes the header.  (cgemm_body.hpp / cgemm_bf16.hip keep their own epilogue: another register layout, eight channels per thread.)
"""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "i-dccrn-vae_amd", "csrc")
HEADER = "conv_epilogue.hpp"
UNITS = ["cgemm_gauss.hip", "cgemm_wino.hip", "cgemm_tw.hip", "cgemm_tw2.hip"]

FOLD = re.compile(r"e0\[0\] \* re \+ e0\[1\] \* im")
# st[0] += yr; st[1] += yi; st[2] += yr * yr; st[3] += yi * yi; st[4] += yr * yi   (any array name; yr / yi plain or indexed)
_R, _I = r"(yr(?:\[\w+\])?)", r"(yi(?:\[\w+\])?)"
MOMENTS = re.compile(r"(\w+)\[0\] \+= %s; \1\[1\] \+= %s; \1\[2\] \+= \2 \* \2; \1\[3\] \+= \3 \* \3; \1\[4\] \+= \2 \* \3;" % (_R, _I))


def _sources():
    """file name -> its text with every run of white space as one blank (the copies were written on one line and on five)"""
    files = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))
    return {os.path.basename(f): " ".join(open(f).read().split()) for f in files}


def test_the_patterns_find_the_copies_the_kernels_used_to_carry():
    one_line = "st[0] += yr; st[1] += yi; st[2] += yr * yr; st[3] += yi * yi; st[4] += yr * yi;"
    indexed = " ".join("""st[0] += yr[q];
                    st[1] += yi[q];
                    st[2] += yr[q] * yr[q];
                    st[3] += yi[q] * yi[q];
                    st[4] += yr[q] * yi[q];""".split())
    assert MOMENTS.search(one_line) and MOMENTS.search(indexed)
    assert FOLD.search("r_ = e0[0] * re + e0[1] * im + e4;")


def test_fold_and_moment_sums_stand_in_the_epilogue_header_only():
    src = _sources()
    assert len(src) > 40 and HEADER in src
    assert [f for f, t in sorted(src.items()) if FOLD.search(t)] == [HEADER]
    assert [f for f, t in sorted(src.items()) if MOMENTS.search(t)] == [HEADER]
    assert len(FOLD.findall(src[HEADER])) == 1 and len(MOMENTS.findall(src[HEADER])) == 1


def test_every_fp32_conv_unit_includes_the_header_and_calls_it():
    src = _sources()
    for u in UNITS:
        assert '#include "%s"' % HEADER in src[u], u
        for helper in ("epi_row(", "epi_point(", "epi_stats_add("):
            assert helper in src[u], (u, helper)
