"""CPU tests of the adversarial decoder fine-tune (csrc/dis.hip): the additive C-ABI entries and every refusal
before any GPU work (loads the library, needs no GPU), and the float64 restatement tests/adv_ref.py pinned to the reference's own
float64 run stored in tests/golden/op_dis_mini.npz and grad_adv_mini.npz."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import adv_ref  # noqa: E402
from oracle import idccrn_oracle as O  # noqa: E402

LIB = importlib.import_module("i-dccrn-vae_amd._lib")
ENTRIES = ("idv_rlstm1_fwd", "idv_rlstm1_bwd", "idv_lsgan", "idv_lsgan_bwd", "idv_rlstm1_save_doubles",
           "idv_rlstm1_fwd_scratch_doubles", "idv_rlstm1_bwd_scratch_doubles")


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ENTRIES:
        assert name in declared and name in protos and hasattr(lib, name), name
    assert protos["idv_rlstm1_fwd"] == ("int", ["ptr"] + ["int"] * 6 + ["ptr"] * 12)
    assert protos["idv_rlstm1_bwd"] == ("int", ["ptr"] + ["int"] * 6 + ["ptr"] * 11)
    assert protos["idv_lsgan"] == ("int", ["ptr", "ptr", "long long", "ptr", "ptr"])
    assert protos["idv_lsgan_bwd"] == ("int", ["ptr", "ptr", "long long", "ptr", "ptr", "ptr", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9      # additive entries


def test_work_sizes():
    lib = LIB.lib()
    assert lib.idv_rlstm1_save_doubles(3, 8) == 12 * 3 * 8
    assert lib.idv_rlstm1_fwd_scratch_doubles(320, 28) == (4 + 4 * 3) * 28            # K = 320: chunks of 128, 128, 64 planes
    assert lib.idv_rlstm1_fwd_scratch_doubles(2560, 41088) == (4 + 4 * 20) * 41088
    assert lib.idv_rlstm1_bwd_scratch_doubles(320, 3, 28) == 4 * 28 + 20 * 3 + 1 * 4 * 320
    assert lib.idv_rlstm1_bwd_scratch_doubles(2560, 64, 41088) == 4 * 41088 + 20 * 64 + 41 * 4 * 2560
    for bad in ((0, 8), (65536, 8), (3, 0), (3, (1 << 20) + 1)):
        assert lib.idv_rlstm1_save_doubles(*bad) == -1, bad
    assert lib.idv_rlstm1_fwd_scratch_doubles(0, 28) == -1 and lib.idv_rlstm1_bwd_scratch_doubles(320, 0, 28) == -1


def _runner(fn, good):
    order = list(good)

    def run(**kw):
        a = dict(good, **kw)
        return fn(*[a[k] for k in order], None)
    return run


def test_every_lstm_refusal_comes_before_any_gpu_work():
    """Dummy pointers are never looked at: each call returns IDV_EINVAL (-1), not a launch failure."""
    lib = LIB.lib()
    geom = dict(C=32, F=5, B=3, T=8, Tp=9, Jp=28)
    fwd = _runner(lib.idv_rlstm1_fwd, dict(x=64, **geom, wih0=16, whh0=16, bih0=16, bhh0=16, wih1=16, whh1=16, bih1=16, bhh1=16,
                                           save=64, scratch=64, y=16))
    bwd = _runner(lib.idv_rlstm1_bwd, dict(x=64, **geom, dy=16, wih0=16, whh0=16, wih1=16, whh1=16, save=64, scratch=64, dx=64,
                                           dwih0=16, dsmall=16))
    bad_geom = [dict(C=0), dict(C=-1), dict(F=0), dict(C=32768, F=2), dict(B=0), dict(B=-2), dict(B=65536, Jp=65536 * 9),
                dict(T=0), dict(T=-1), dict(T=(1 << 20) + 1, Tp=(1 << 20) + 2, Jp=4 * ((1 << 20) + 2)), dict(Tp=8), dict(Jp=24),
                dict(Jp=27), dict(Jp=30), dict(Jp=0x7fffffff - 3)]
    for run, ptrs, mis in ((fwd, ("x", "wih0", "whh0", "bih0", "bhh0", "wih1", "whh1", "bih1", "bhh1", "scratch", "y"),
                            [dict(x=68), dict(x=72), dict(save=68), dict(scratch=12), dict(y=18), dict(wih0=17), dict(bhh1=6)]),
                           (bwd, ("x", "dy", "wih0", "whh0", "wih1", "whh1", "save", "scratch", "dsmall"),
                            [dict(x=72), dict(dx=72), dict(save=68), dict(scratch=12), dict(dy=18), dict(dwih0=17), dict(dsmall=6)])):
        for name in ptrs:
            assert run(**{name: None}) == -1, name
        for kw in bad_geom + mis:
            assert run(**kw) == -1, kw


def test_every_lsgan_refusal_comes_before_any_gpu_work():
    lib = LIB.lib()
    fwd = _runner(lib.idv_lsgan, dict(a=16, b=16, n=24, out=16))
    bwd = _runner(lib.idv_lsgan_bwd, dict(a=16, b=16, n=24, gout=16, da=16, db=16))
    for kw in (dict(a=None), dict(out=None), dict(n=0), dict(n=-1), dict(n=(1 << 28) + 1), dict(a=18), dict(b=6), dict(out=5)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(gout=None), dict(n=0), dict(n=(1 << 28) + 1), dict(da=None, db=None), dict(a=None), dict(b=None),
               dict(a=18), dict(b=6), dict(gout=5), dict(da=7), dict(db=9)):
        assert bwd(**kw) == -1, kw


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def test_state_dict_list_has_the_reference_98_entries(golden):
    d = golden("op_dis_mini")
    keys, shapes = [str(k) for k in d["sd_keys"]], [str(s) for s in d["sd_shapes"]]
    assert len(keys) == len(shapes) == 98
    lstm = dict(zip(keys, shapes))
    assert [lstm["lstms.0." + n] for n in adv_ref.NAMES] == ["4,320", "4,1", "4", "4", "4,1", "4,1", "4", "4"]
    assert sum(k.startswith("encoders.") for k in keys) == 90 and all(int(f) == 1 for f in d["init_flag"])


def test_adv_ref_lstm_matches_the_reference_float64_run(golden):
    d = golden("op_dis_mini")
    shapes = {str(k): tuple(int(n) for n in str(s).split(",") if n) for k, s in zip(d["sd_keys"], d["sd_shapes"])}
    sd = O.synth_state_dict(shapes, int(d["seed"]))
    w = {n: sd["lstms.0." + n].double().numpy() for n in adv_ref.NAMES}
    y, tape = adv_ref.lstm1_forward(d["lstm_in64"], w)
    assert _rel(y.transpose(1, 0, 2), d["lstm_y64"]) < 1e-6
    n = y.size
    dx, g = adv_ref.lstm1_backward(0.5 * 2.0 * (y - 1.0) / n, tape)                  # d/dy of 0.5 * mean((y - 1)^2)
    assert _rel(dx, d["lstm_gin64"]) < 1e-6
    for name in adv_ref.NAMES:
        assert _rel(g[name], d["lstm_g64:" + name]) < 1e-6, name
    loss, _ = adv_ref.generator_dis_loss(y)
    assert abs(0.5 * loss - float(d["loss64"])) < 1e-6 * float(d["loss64"])


def test_adv_ref_lsgan_matches_the_reference_float64_run(golden):
    d = golden("grad_adv_mini")
    want = d["loss064"]                                                               # gen, si_snr, dis_gen, dist of iteration 0
    dist, da, db = adv_ref.distinguisher_loss(d["dis_true64"], d["dis_est64"])
    gen, dg = adv_ref.generator_dis_loss(d["dis_gen64"])
    assert abs(dist - want[3]) < 1e-6 * abs(want[3]) and abs(gen - want[2]) < 1e-6 * abs(want[2])
    assert abs(0.5 * gen + want[1] - want[0]) < 1e-6 * abs(want[0])
    # the gradients against central differences of the restated losses
    h = 1e-6
    for grad, fn, arg in ((da, lambda v: adv_ref.distinguisher_loss(v, d["dis_est64"])[0], d["dis_true64"]),
                          (db, lambda v: adv_ref.distinguisher_loss(d["dis_true64"], v)[0], d["dis_est64"]),
                          (dg, lambda v: adv_ref.generator_dis_loss(v)[0], d["dis_gen64"])):
        for idx in ((0, 0, 0), (1, 5, 0), (3, 16, 0)):
            e = np.zeros_like(arg)
            e[idx] = h
            num = (fn(arg + e) - fn(arg - e)) / (2 * h)
            assert abs(num - grad[idx]) < 1e-6 * max(abs(grad[idx]), 1e-3), (idx, num, grad[idx])
