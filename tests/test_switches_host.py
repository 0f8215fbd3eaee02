"""CPU: the environment switches and the conv dispatch tables.

(a) every IDV_* variable the library (`getenv` in csrc/) or the package (`os.environ`) reads is a row of the table in DESIGN.md
    section 6.1, and every row of that table is read by one of them;
(b) the configuration ids and `*_supported` answers of the fp32 conv ladder, pinned at the DCCRN-CL layer shapes and three narrow
    ones.  The values were recorded from the build BEFORE the unreachable tile forms were removed from csrc/: a changed value means
    a layer moved to another kernel.
"""
import ctypes
import glob
import os
import re

from conftest import ROOT

PKG = os.path.join(ROOT, "i-dccrn-vae_amd")


def _names_read():
    names = set()
    for f in glob.glob(os.path.join(PKG, "csrc", "*.hip")) + glob.glob(os.path.join(PKG, "csrc", "*.hpp")):
        names |= set(re.findall(r'getenv\(\s*"(IDV_[A-Z0-9_]+)"', open(f).read()))
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py"):
                names |= set(re.findall(r'os\.environ(?:\.get\(|\[)\s*"(IDV_[A-Z0-9_]+)"', open(os.path.join(d, f)).read()))
    return names


def _names_documented():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("## 6.1 Switches (environment)"):]
    lines = sec.splitlines()
    first = lines.index("| variable | default | meaning |")          # the section's first table of variables (bench.py's own follow)
    names = set()
    for row in lines[first + 2:]:                    # (header and rule)
        if not row.startswith("|"):
            break
        names |= set(re.findall(r"`(IDV_[A-Z0-9_]+)`", row.split("|")[1]))
    return names


def test_every_switch_read_is_documented_and_every_documented_switch_is_read():
    read, documented = _names_read(), _names_documented()
    assert len(read) > 30 and len(documented) > 30
    assert read - documented == set(), "read but missing from the DESIGN.md 6.1 table"
    assert documented - read == set(), "in the DESIGN.md 6.1 table but read nowhere"


# (name, transposed, C0, C1, Cout, Fin,
#  idv_cconv_gauss_config, idv_cconv_wino_config, idv_cconv_config,
#  supported: gauss, wino, tw, tw2, bf16 (x1_div = 1), wgrad_gauss)
PINNED = [
    ('enc1', 0, 32, 0, 64, 129, 3022122, 222, 221524, 1, 1, 1, 0, 1, 0),
    ('enc2', 0, 64, 0, 128, 65, 3022122, 412, 221334, 1, 1, 1, 1, 1, 1),
    ('enc3', 0, 128, 0, 128, 33, 3022122, 412, 221334, 1, 1, 1, 1, 1, 1),
    ('enc4', 0, 128, 0, 256, 17, 3022122, 412, 221334, 1, 1, 1, 1, 1, 1),
    ('enc5', 0, 256, 0, 256, 9, 3022122, 412, 221524, 1, 1, 1, 1, 1, 1),
    ('dec0', 1, 256, 256, 256, 5, 3141121, 418, 1221514, 1, 1, 1, 1, 1, 1),
    ('dec1', 1, 256, 256, 128, 9, 3141121, 418, 1221324, 1, 1, 1, 1, 1, 1),
    ('dec2', 1, 128, 128, 128, 17, 3141121, 418, 1221324, 1, 1, 1, 1, 1, 1),
    ('dec3', 1, 128, 128, 64, 33, 3122121, 228, 1221324, 1, 1, 1, 1, 1, 1),
    ('dec4', 1, 64, 64, 32, 65, 3114112, 144, 1221514, 1, 0, 1, 1, 1, 1),
    ('conv8to16', 0, 8, 0, 16, 17, 3014122, 222, 221334, 1, 0, 0, 0, 0, 0),
    ('conv1to32', 0, 1, 0, 32, 257, 3014122, 222, 221332, 0, 0, 0, 0, 0, 0),
    ('tconv32to1', 1, 16, 16, 1, 129, 3114112, 144, 1000001, 0, 0, 0, 0, 0, 0),
]


def test_conv_configs_and_supported_answers_are_those_of_the_parent_build(amd):
    lib = amd._lib.lib()
    I = ctypes.c_int
    for name, tr, c0, c1, co, fin, g_cfg, w_cfg, c_cfg, g_ok, w_ok, tw_ok, tw2_ok, bf_ok, wg_ok in PINNED:
        cin = c0 + c1
        cs, cl = (cin, co) if tr else (co, cin)
        got = (lib.idv_cconv_gauss_config(I(tr), I(cin), I(co), I(fin)), lib.idv_cconv_wino_config(I(tr), I(cin), I(co)),
               lib.idv_cconv_config(I(tr), I(cin), I(co), I(fin)),
               lib.idv_cconv_gauss_supported(I(c0), I(c1), I(co)), lib.idv_cconv_wino_supported(I(tr), I(c0), I(c1), I(co), I(fin)),
               lib.idv_cconv_tw_supported(I(c0), I(c1), I(co), I(fin)), lib.idv_cconv_tw2_supported(I(cin), I(co), I(fin)),
               lib.idv_cconv_bf16_supported(I(tr), I(c0), I(c1), I(1), I(co)), lib.idv_cconv_wgrad_gauss_supported(I(cs), I(cl)))
        assert got == (g_cfg, w_cfg, c_cfg, g_ok, w_ok, tw_ok, tw2_ok, bf_ok, wg_ok), name
