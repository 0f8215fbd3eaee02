"""Writes the P808_MOS fixtures of tests/golden/:

    python tests/golden/make_p808_golden.py --reference /path/to/reference

  p808_weights.npz    the 16 initializer tensors of DNSMOS/DNSMOS/model_v8.onnx under the names of dnsmos.P808_SHAPES (about 225 KB)
  p808_expected.npz   for the signals of SIGNALS (tests/dnsmos_ref.signal; 3 segments in all): the float64 definition's
      (tests/p808_ref.py) value per segment (<kind>.raw64) and per clip (<kind>.clip64), and the per-segment values of the float32
      torch-CPU evaluation of the same definition (<kind>.raw32: the float64 feature rounded to float32, then the float32 network),
      the yardstick of the device test.

Needs a checkout of the reference; it is run once, by hand, where one exists.  Only tensors are written: no graph and no byte of the
.onnx container.  The file is read with the library's own reader (dnsmos.read_onnx), which needs no onnx package and no GPU.
"""
import argparse
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dnsmos_ref as R  # noqa: E402
import p808_ref as P  # noqa: E402

SIGNALS = (("tone", 144160), ("speechlike", 176000))        # 1 + 2 segments
MODEL = os.path.join("DNSMOS", "DNSMOS", "model_v8.onnx")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (the folder that holds DNSMOS/)")
    a = ap.parse_args()
    dnsmos = importlib.import_module("i-dccrn-vae_amd.dnsmos")
    ops_, inits = dnsmos.read_onnx(os.path.join(a.reference, MODEL))
    if tuple(ops_) != dnsmos.P808_OP_SEQUENCE:
        raise SystemExit(f"{MODEL}: not the expected graph")
    t = {}
    for k, (name, shape) in dnsmos.P808_ONNX_NAMES.items():
        if inits[name].dtype != np.float32 or inits[name].shape != shape:
            raise SystemExit(f"{MODEL}: {name} is {inits[name].dtype} {inits[name].shape}")
        t[k] = inits[name]
    np.savez(os.path.join(HERE, "p808_weights.npz"), **t)
    expected = {}
    for kind, n in SIGNALS:
        x = R.signal(kind, n)
        clip64, raw64 = P.score_clip(x, t)
        _, raw32 = P.score_clip(x, t, raw_fn=P.network_float32)
        expected[f"{kind}.raw64"] = raw64
        expected[f"{kind}.raw32"] = raw32
        expected[f"{kind}.clip64"] = np.float64(clip64)
        print(kind, raw64, np.abs(raw32 - raw64).max())
    np.savez(os.path.join(HERE, "p808_expected.npz"), **expected)


if __name__ == "__main__":
    main()
