"""CPU: host-side logic - the C-ABI library loads and exports every symbol include/idccrn_hip.h declares
(no compute calls), the config tables and state_dict keys, the planar view algebra, the ini reader."""
import ctypes
import importlib
import os

import pytest
import torch

from conftest import ROOT

NFFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]


def test_library_exports_every_declared_symbol(amd):
    L = amd._lib
    names = L.declared_symbols()
    assert len(names) >= 24 and "idv_cconv2d_fwd" in names and "idv_clstm_fwd" in names
    lib = L.lib()                                    # raises if the .so is missing or a symbol is absent
    for n in names:
        assert hasattr(lib, n), n
    assert lib.idv_abi_version() == 9          # 2: backward entry points; 3: split-image hand-over inside idv_clstm_fwd; 4: IDV_ECOOP status; 5: idv_cconv_gauss_config takes Cin, idv_lstm_stack2_f32 / idv_clstm_fwd2; 6: idv_bucket_*; 7: idv_cconv_wino_*; 8: idv_cconv_tw_* / idv_ctconv2d_tw_fwd; 9: idv_cconv_tw2_* / idv_cconv2d_tw_fwd
    assert lib.idv_cconv_cck(ctypes.c_int(1)) == 2 and lib.idv_cconv_cck(ctypes.c_int(32)) == 4
    assert lib.idv_cconv_config(ctypes.c_int(1), ctypes.c_int(64), ctypes.c_int(1), ctypes.c_int(129)) == 1000001          # the one-output-channel vector-ALU kernel
    lib.idv_clstm_work_floats.restype = ctypes.c_longlong
    assert lib.idv_clstm_work_floats(ctypes.c_int(128), ctypes.c_int(2), ctypes.c_int(641), ctypes.c_int(1284)) == 24 * 641 * 2 * 128 + 4 * 2 * 128 + 8 * 128 * 1284          # scratch = 4*H*Jp here (>= the cooperative exchange buffer)


def test_lstm_scratch_covers_the_cooperative_exchange_buffers(amd):
    """The scratch region inside idv_clstm_fwd's work buffer also hosts the exchange buffer + arrive counters of the
    cooperative recurrences, whose size does not shrink with T or Jp (a short input used to overflow it)."""
    lib = amd._lib.lib()
    I, LL = ctypes.c_int, ctypes.c_longlong
    for fn in (lib.idv_clstm_work_floats, lib.idv_clstm_train_work_floats, lib.idv_lstm_pers_work_bytes, lib.idv_lstm_coop_f32_work_bytes,
               lib.idv_lstm_stack2_f32_work_bytes, lib.idv_lstm_bptt_work_floats, lib.idv_lstm_bptt_coop_work_bytes,
               lib.idv_lstm_bptt_stack2_work_bytes):
        fn.restype = LL
    # H = 128 at the batches where the kernel changes (240 cooperative workgroups, the figure without a device): 7 / 8 and
    # 15 / 16 sequence tiles, one frame, a Jp far below the exchange buffers' size
    edges = ((128, 112, 1, 228), (128, 113, 1, 228), (128, 240, 1, 484), (128, 241, 1, 484))
    for H, B, T, Jp in ((128, 1, 3, 8), (128, 64, 17, 64 * 18), (384, 3, 5, 20), (768, 32, 2, 96), (768, 20, 7, 160),
                        (384, 64, 641, 64 * 642)) + edges:
        need = 0
        if lib.idv_lstm_pers_supported(I(H), I(B)):
            need = max(need, lib.idv_lstm_pers_work_bytes(I(H), I(B)))
        if lib.idv_lstm_coop_f32_supported(I(H), I(B)):
            need = max(need, lib.idv_lstm_coop_f32_work_bytes(I(H), I(B)))
        if lib.idv_lstm_stack2_f32_supported(I(H), I(B)):
            need = max(need, lib.idv_lstm_stack2_f32_work_bytes(I(H), I(B)))
        assert need > 0 or (H, B) == (128, 241)                 # no cooperative form at 16 tiles
        TBH = T * B * H
        scratch_eval = lib.idv_clstm_work_floats(I(H), I(B), I(T), I(Jp)) - (24 * TBH + 4 * B * H + 4 * H * Jp)
        scratch_train = lib.idv_clstm_train_work_floats(I(H), I(B), I(T), I(Jp)) - (48 * TBH + 4 * B * H + 4 * H * Jp)
        assert 4 * scratch_eval >= need and 4 * scratch_train >= need, (H, B, T, Jp, scratch_eval, scratch_train, need)
        assert scratch_eval >= 4 * H * Jp and scratch_train >= 4 * H * Jp
        # the BPTT scratch hosts the per-step kernels' buffers and, where supported, the cooperative form's
        per_step = 4 * B * H + 2 * 4 * ((B + 15) // 16) * 4 * H * 16
        assert lib.idv_lstm_bptt_work_floats(I(H), I(B)) >= per_step
        if lib.idv_lstm_bptt_coop_supported(I(H), I(B)):
            assert 4 * lib.idv_lstm_bptt_work_floats(I(H), I(B)) >= lib.idv_lstm_bptt_coop_work_bytes(I(H), I(B)) > 0
        if lib.idv_lstm_bptt_stack2_supported(I(H), I(B)):
            assert lib.idv_lstm_bptt_stack2_work_bytes(I(H), I(B)) > 0
    assert lib.idv_coop_max_workgroups() == 240                 # no device here
    want = {112: (1, 1), 113: (0, 1), 240: (0, 1), 241: (0, 0)}
    for H, B, _, _ in edges:
        fwd = (lib.idv_lstm_stack2_f32_supported(I(H), I(B)), lib.idv_lstm_coop_f32_supported(I(H), I(B)))
        bwd = (lib.idv_lstm_bptt_stack2_supported(I(H), I(B)), lib.idv_lstm_bptt_coop_supported(I(H), I(B)))
        assert fwd == want[B] and bwd == want[B], (B, fwd, bwd)
    for B in (1, 17, 112, 113, 230, 240):                       # wherever the coop form is supported
        assert lib.idv_lstm_bptt_coop_supported(I(128), I(B))
        assert 4 * lib.idv_lstm_bptt_work_floats(I(128), I(B)) >= lib.idv_lstm_bptt_coop_work_bytes(I(128), I(B))


def test_missing_library_fails_loudly(amd, monkeypatch):
    L = amd._lib
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", os.path.join(ROOT, "no_such_lib.so"))
    with pytest.raises(L.IdvError, match="no CPU fallback"):
        L.lib()


def test_cpu_tensors_are_rejected(amd):
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    cn = importlib.import_module("i-dccrn-vae_amd.model.causal_netconfig")
    m = pm.DCCRN_(NFFT, HOP, cn.get_net_params(), True, "cpu", WIN, SKIP, "mask", False, None, None)
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(1, 6400))


def test_net_tables():
    cn = importlib.import_module("i-dccrn-vae_amd.model.causal_netconfig").get_net_params()
    nc = importlib.import_module("i-dccrn-vae_amd.model.net_config").get_net_params()
    assert cn["encoder_channels"] == [1, 32, 64, 128, 128, 256, 256]
    assert cn["decoder_channels"] == [256, 256, 128, 128, 64, 32, 1]
    assert cn["lstm_dim"] == [1280, 128] and cn["dense"] == [128, 1280] and cn["lstm_layer_num"] == 2
    assert cn["encoder_paddings"] == [(2, 1)] * 6 and nc["encoder_paddings"] == [(2, 0)] * 6
    assert {k: v for k, v in cn.items() if k != "encoder_paddings"} == {k: v for k, v in nc.items() if k != "encoder_paddings"}
    assert cn["encoder_chw"][0] == (32, 129, 1600) and cn["decoder_chw"][-1] == (1, 257, 1601)


def test_state_dict_keys_and_param_counts():
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    np_ = importlib.import_module("i-dccrn-vae_amd.model.causal_netconfig").get_net_params()
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cpu", WIN, SKIP, "mask", False, None, None)
    keys = set(m.state_dict())
    for k in ("std_DCCRN.encoders.0.conv.conv_re.weight", "std_DCCRN.encoders.5.bn.gamma_ri", "std_DCCRN.encoders.2.bn.Vri",
              "std_DCCRN.encoders.1.prelu.weight", "std_DCCRN.lstms.0.lstm_re.weight_ih_l0", "std_DCCRN.lstms.0.lstm_im.bias_hh_l1",
              "std_DCCRN.dense.linear_read.weight", "std_DCCRN.dense.linear_imag.bias",
              "std_DCCRN.decoders.0.transconv.tconv_re.weight", "std_DCCRN.decoders.5.bn.running_mean_imag",
              "std_DCCRN.linear.conv_im.bias"):
        assert k in keys, k
    assert len(keys) == 204
    count = lambda mod: sum(p.numel() for p in mod.parameters())
    assert count(m) == 9546199                                                       # SURVEY.md section 8(c) probe
    assert m.state_dict()["std_DCCRN.decoders.0.transconv.tconv_re.weight"].shape == (512, 256, 5, 2)
    enc = pm.pvae_dccrn_encoder_skip_prepare(np_, True, "cpu", 128, NFFT, HOP, WIN, 5)
    dec = pm.pvae_dccrn_decoder_skip_prepare(np_, True, "cpu", 5, 128, NFFT, HOP, WIN, "real_imag", SKIP)
    ns = pm.nsvae_pvae_dccrn_encoder_twophase(np_, True, "cpu", 128, NFFT, HOP, WIN, 2, 2)
    assert (count(enc), count(dec), count(ns)) == (10318886, 5332909, 24880166)
    assert enc.lstms[0].hidden_size == 384 and ns.lstms[0].hidden_size == 768
    assert "dense.linear_read.weight" in enc.state_dict()                           # the unused dense of the reference
    old = importlib.import_module("i-dccrn-vae_amd.model.module").DCCRN_(NFFT, HOP, importlib.import_module(
        "i-dccrn-vae_amd.model.net_config").get_net_params(), "cpu", WIN)
    assert "DCCRN.encoders.0.conv.conv_re.weight" in old.state_dict()


def test_planar_views_roundtrip(amd):
    P = amd.ops.Planar
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 4, 5, 7, 2, generator=g)
    pl = P.from_tensor5(x, Tp=9)
    assert pl.Jp % 4 == 0 and pl.Jp >= 3 * 9
    assert torch.equal(pl.tensor5(), x)
    planes = pl.planes()
    assert planes.shape == (2, 4, 5, 3, 9)
    assert float(planes[..., 0].abs().max()) == 0 and float(planes[..., 8:].abs().max()) == 0     # guard columns
    assert torch.equal(planes[0, 1, 2, 1, 1:8], x[1, 1, 2, :, 0])
    lat = P.from_tensor5(torch.randn(2, 6, 1, 5, 2, generator=g))
    assert lat.channel_slice(2, 4).shape == (2, 5, 2, 2)
    assert torch.equal(lat.channel_slice(2, 4), lat.tensor5()[:, 2:4, 0].permute(0, 2, 1, 3))


def test_synth_weights_are_deterministic():
    synth = importlib.import_module("i-dccrn-vae_amd.utils.synth")
    a = synth.synth_tensor("encoders.0.conv.conv_re.weight", (4, 1, 5, 2), 7)
    b = synth.synth_tensor("encoders.0.conv.conv_re.weight", (4, 1, 5, 2), 7)
    c = synth.synth_tensor("encoders.0.conv.conv_re.weight", (4, 1, 5, 2), 8)
    assert torch.equal(a, b) and not torch.equal(a, c) and a.dtype == torch.float32
    v = synth.synth_tensor("bn.Vrr", (1, 8, 1, 1), 1)
    assert float(v.min()) >= 0.5


def test_ini_surface(tmp_path):
    rc = importlib.import_module("i-dccrn-vae_amd.utils.read_config")
    ini = tmp_path / "cfg.ini"
    ini.write_text("[User]\nsaved_root = /tmp/x\nmodel_name = supervised_dccrn\n[Network]\nz_dim = 128\n"
                   "[STFT]\nwinlen = 400\nnfft = 512\nhopfrac = 100\nfs = 16000\nmingain = -80\n"
                   "[Training]\noptimization = adam\nlr = 3e-4\nepochs = 1000\nearly_stop_patience = 20\nsave_frequency = 10\n"
                   "[DataFrame]\ndataset_name = d\nsuffix = wav\nnum_workers = 1\nbatch_size = 48\nshuffle = True\nsequence_len = 481\n")
    cfg = rc.myconf()
    cfg.read(str(ini))
    assert cfg.getint("STFT", "winlen") == 400 and cfg.getint("STFT", "hopfrac") == 100 and cfg.getint("STFT", "nfft") == 512
    assert cfg.getfloat("Training", "lr") == 3e-4 and cfg.getint("DataFrame", "sequence_len") == 481
    assert "saved_root" in cfg["User"] and "Saved_Root" not in cfg["User"]            # key case is preserved


def test_kl_annealing_schedule():
    pl = importlib.import_module("i-dccrn-vae_amd.model.pretrain_pvaes_loss")
    w = pl.KL_annealing(20).frange_cycle_linear(0.0, 1.0, 1, 1)
    assert w.shape == (20,) and float(w[0]) == 0.0 and abs(float(w[10]) - 0.5) < 1e-6 and float(w[19]) <= 1.0


def test_no_packed_fp32_in_device_code(tmp_path, amd):
    """The SHIPPED library must not contain packed-fp32 VALU instructions (v_pk_*_f32): they produced wrong results while
    an MFMA-saturating kernel of another HIP stream shared the SIMD.  build() passes -fno-slp-vectorize
    (hashed into the build stamp); this disassembles every gfx950 code object of the built libidccrn_hip.so -- all
    translation units, not a sample of the sources."""
    import glob
    import re
    import shutil
    import subprocess
    import __graft_entry__ as ge
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    assert "-fno-slp-vectorize" in ge.HIP_FLAGS
    lib = tmp_path / "lib.so"
    shutil.copy(amd._lib.LIB_PATH, lib)
    subprocess.check_call([objdump, "--offloading", str(lib)], cwd=tmp_path, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    cos = glob.glob(str(tmp_path / "lib.so.*gfx950*"))
    host_only = {"coop.hip"}          # state + launch path of the cooperative kernels: host code, so no code object of its own
    units = [p for p in glob.glob(os.path.join(ge.CSRC, "*.hip")) if os.path.basename(p) not in host_only]
    assert len(units) >= 30 and len(cos) >= len(units), "one code object per .hip unit with device code expected"
    n_kernels = 0
    for co in cos:
        isa = subprocess.run([objdump, "-d", co], capture_output=True, text=True, check=True).stdout
        n_kernels += isa.count("s_endpgm")
        hit = re.search(r"v_pk_[a-z0-9]+_f32", isa)
        assert not hit, (os.path.basename(co), hit.group(0))
    assert n_kernels > 100


def test_stock_cpu_baseline_module_matches_the_oracle():
    """oracle/stock_cpu.py (what bench.py times as `cpu_baseline`: the reference's op sequence on stock nn.Conv2d /
    nn.LSTM / torch.stft) computes the same DCCRN-CL forward as the pinned oracle, eval and train mode."""
    from oracle import idccrn_oracle as O
    from oracle import stock_cpu
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    np_ = O.net_params(True, 4)
    m = pm.DCCRN_(NFFT, HOP, np_, True, "cpu", WIN, SKIP, "mask", False, None, None)
    sd = O.synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 3)
    net = stock_cpu.StockDCCRN(np_, NFFT, HOP, WIN).load_reference_state(sd)
    x = torch.randn(2, 1600, generator=torch.Generator().manual_seed(0)) * 0.1
    with torch.no_grad():
        for train in (False, True):
            est, pred = net(x, train=train)
            want, wpred, _ = O.dccrn_forward(x, sd, np_, True, NFFT, HOP, WIN, SKIP, "mask", train, O.BNState())
            assert est.shape == want.shape
            assert float((est - want).norm() / want.norm()) < 1e-4
            assert float((pred - wpred).norm() / wpred.norm()) < 1e-4


def test_library_is_newer_than_its_sources(amd):
    """The in-tree libidccrn_hip.so travels to the GPU box as built here: a source edited after the last build() would be
    tested there against stale device code."""
    import glob
    lib = amd._lib.LIB_PATH
    srcs = glob.glob(os.path.join(ROOT, "i-dccrn-vae_amd", "csrc", "*.hip")) + \
        glob.glob(os.path.join(ROOT, "i-dccrn-vae_amd", "csrc", "*.hpp")) + [amd._lib.HEADER_PATH]
    stale = [os.path.basename(f) for f in srcs if os.path.getmtime(f) > os.path.getmtime(lib)]
    assert not stale, f"rebuild (python __graft_entry__.py): {stale} changed after libidccrn_hip.so was linked"


CKPT = os.path.join(ROOT, "tests", "golden", "ckpt",
                    "2025-01-01-00h00_DCCRN_causal=True_skipuse=012345_reconw=001_recontype=mask_resynthesis=False_datanorm=False")


def test_run_folder_parsing_follows_the_reference():
    """Hyper-parameters live in the run-folder name (supervised_dccrn/test.py:362-393, train_nsvae.py:94-120,
    train_second_phase_decoder.py:732-775)."""
    ck = importlib.import_module("i-dccrn-vae_amd.utils.checkpoint")
    hp = ck.parse_run_folder(CKPT)
    assert hp["causal"] is True and hp["skipuse"] == [0, 1, 2, 3, 4, 5] and hp["recon_type"] == "mask"
    assert hp["resynthesis"] is False and hp["datanorm"] is False and hp["reconw"] == "001"
    hp = ck.parse_run_folder("/x/2024-05-01-10h00_CVAE_causal=True_zdim=128_numsamples=5_klw=1.000_miw=0_skipc=False_"
                             "skipuse=[0, 1, 2, 3]_spadd=True_recon=real_imag_reconweight=[1.0, 1.0, 0.0]_prior=ri_inde/")
    assert hp["zdim"] == 128 and hp["num_samples"] == 5 and hp["skipc"] == "False" and hp["skipuse"] == [0, 1, 2, 3]
    assert hp["spadd"] is True and hp["recon_type"] == "real_imag" and hp["klw"] == 1.0
    hp = ck.parse_run_folder("2024_NSVAE_causal=True_zdim=128_alpha=1.00_wresi=0.0_wkl=1_wdismiu=0_numsamples=2_nsvae=original_"
                             "latentnum=2_match=both")
    assert hp["latent_num"] == 2 and hp["nsvae"] == "original" and hp["alpha"] == 1.0 and hp["match"] == "both"
    hp = ck.parse_run_folder("2024_P2_causal=True_zdim=128_latentnum=2_decodeupdate=True_skipc=True_skipuse=012345_reconw=001_"
                             "numsamples=2_loadde=True_recontype=mask_resyn=False")
    assert hp["decodeupdate"] is True and hp["loadde"] is True and hp["resynthesis"] is False and hp["skipuse"] == [0, 1, 2, 3, 4, 5]
    assert ck.parse_run_folder("2024_DCCRN_recontype=real")["causal"] is False          # absent keys: the reference's defaults
    assert ck.parse_run_folder("2024_DCCRN_recontype=real")["recon_type"] == "real_imag"


def test_reference_written_checkpoint_loads_and_round_trips(tmp_path):
    """tests/golden/ckpt/* was written by the REFERENCE's DCCRN_ + Adam + ReduceLROnPlateau
    (tests/golden/make_golden.py extras): same keys, same shapes -> loads strictly into this package's module."""
    from oracle import idccrn_oracle as O
    ck = importlib.import_module("i-dccrn-vae_amd.utils.checkpoint")
    pm = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
    hp = ck.parse_run_folder(CKPT)
    m = pm.DCCRN_(NFFT, HOP, O.net_params(True, 2, 16), hp["causal"], "cpu", WIN, hp["skipuse"], hp["recon_type"],
                  hp["resynthesis"], None, None)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=0.001)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, 'min', factor=0.5, patience=3)
    info = ck.load_checkpoint(os.path.join(CKPT, "DCCRN_checkpoint.pt"), {"model": m}, {"model": opt}, {"model": sch})
    assert info["epoch"] == 3 and info["cpt_patience"] == 1 and len(info["loss_log"]["train_loss"]) == 4
    assert float(opt.state_dict()["state"][0]["step"]) == 1.0 and sch.state_dict()["num_bad_epochs"] == 0
    bn = m.std_DCCRN.encoders[0].bn
    assert bn.init_flag is True                       # not part of the state_dict: the reference's behaviour is kept
    ck.set_bn_init_flag(m, False)
    assert bn.init_flag is False
    ref = torch.load(os.path.join(CKPT, "DCCRN_curr_best_epoch.pt"), weights_only=False)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ref[k]), k
    p1 = ck.save_checkpoint(str(tmp_path), "DCCRN", 4, 0.5, 0, {"model": m}, {"model": opt}, {"model": sch}, {"train_loss": [1.0]})
    p2 = ck.save_best_epoch(m, str(tmp_path), "DCCRN")
    assert os.path.basename(p1) == "DCCRN_checkpoint.pt" and os.path.basename(p2) == "DCCRN_curr_best_epoch.pt"
    again = torch.load(p1, weights_only=False)
    assert set(again) == {"epoch", "best_val_loss", "cpt_patience", "loss_log", "model_state_dict", "model_optim_dict",
                          "model_scheduler_dict"}
    assert os.path.basename(ck.save_best_epoch(m, str(tmp_path), "NSVAE", "noisy_encoder")) == "NSVAE_noisy_encoder_best_epoch.pt"


def test_bench_self_launch_starts_ranks_as_a_child_and_relays_rank0(monkeypatch, capsys):
    """`python bench.py --gpus N` without WORLD_SIZE: the process becomes the launcher -- `python -m torch.distributed.run
    --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py <same flags>` as a CHILD process (no exec, no torch import in
    the parent), rank 0's JSON line relayed on stdout, everything else on stderr, the child's exit code returned."""
    import importlib
    import io
    import sys as _sys
    bench = importlib.import_module("bench")
    seen = {}

    class FakeProc:
        pid = 0

        def __init__(self, cmd, env=None, stdout=None, text=None, start_new_session=False):
            seen["cmd"], seen["env"], seen["session"] = cmd, env, start_new_session
            self.stdout = io.StringIO('rank noise\n{"metric": "m", "value": 1.5, "n_gpus": 4, "rccl_ranks": 4}\ntrailing\n')

        def wait(self, timeout=None):
            return 0

        def poll(self):
            return 0                               # already exited: the launcher's clean-up has nothing to end
    import subprocess
    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--workload", "nsvae_train"])
    had_torch = "torch" in _sys.modules
    rc = bench.self_launch(4)
    out = capsys.readouterr()
    assert rc == 0
    assert out.out.strip() == '{"metric": "m", "value": 1.5, "n_gpus": 4, "rccl_ranks": 4}'          # ONE line on stdout
    assert "rank noise" in out.err and "trailing" in out.err
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--workload", "nsvae_train"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert seen["session"] is True                                      # own process group: ended as a whole on a signal / deadline
    assert ("torch" in _sys.modules) == had_torch                       # the launcher itself imports no torch


def test_bench_dump_outputs_fits_the_budget_and_samples_the_same_elements(tmp_path):
    """`bench.py --dump-outputs DIR`: every output of the last step as DIR/<name>.npy in float32 (float64 stays float64),
    complex as (real, imag) pairs, a train step's parameter list flattened; all files together under the budget, an output
    over its share replaced by a seeded sample that is the same in every run."""
    import numpy as np
    bench = importlib.import_module("bench")
    g = torch.Generator().manual_seed(3)
    outs = {"loss": torch.tensor(0.25), "est": torch.randn(8, 6400, generator=g),
            "est_stft": torch.randn(8, 257, 65, 2, generator=g), "d": torch.randn(5, generator=g, dtype=torch.float64),
            "params": [torch.randn(40, 3, generator=g), torch.randn(7, generator=g).bfloat16()]}
    outs["est_stft"] = torch.view_as_complex(outs["est_stft"])
    budget = 500_000                  # est (205 kB) fits its share, est_stft (1.07 MB) does not
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), bench.host_arrays(outs), budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["d.npy", "est.npy", "est_stft.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= budget
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert a["d"].dtype == np.float64 and all(v.dtype == np.float32 for k, v in a.items() if k != "d")
    assert float(a["loss"]) == 0.25 and a["params"].shape == (127,)
    np.testing.assert_array_equal(a["est"], outs["est"].numpy())                                # small enough: whole
    stft = torch.view_as_real(outs["est_stft"]).numpy().reshape(-1)
    assert 0 < a["est_stft"].size < stft.size and np.isin(a["est_stft"], stft).all()           # too large: a sample
    for f in files:
        np.testing.assert_array_equal(a[f[:-4]], np.load(tmp_path / "b" / f))


def test_call_sites_match_header_prototypes(amd):
    """Static ABI check (no GPU): every ``call("idv_x", ...)`` / ``lib().idv_x(...)`` / ``_ll_fn("idv_x")(...)`` site of the package,
    bench.py and the tests passes as many arguments as include/idccrn_hip.h declares, with wrappers (p / i / ll / f / d) of the
    declared kind.  ``_lib.lib()`` turns the same prototypes into ctypes signatures, so a ``long long`` or ``double`` argument can
    not be truncated by a forgotten wrapper (VERDICT r3 housekeeping)."""
    import ast
    import glob
    L = amd._lib
    protos = L.prototypes()
    assert len(protos) == len(L.declared_symbols())
    lib = L.lib()
    assert lib.idv_bucket_adam.argtypes[8] is ctypes.c_double and lib.idv_clstm_work_floats.restype is ctypes.c_longlong
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def kind(node):
        if isinstance(node, ast.Call):
            f = node.func
            name = f.id if isinstance(f, ast.Name) else (f.attr if isinstance(f, ast.Attribute) else None)
            return {"p": "ptr", "ptr": "ptr", "_P": "ptr", "stream_ptr": "ptr", "i": "int", "ll": "long long", "f": "float",
                    "d": "double"}.get(name)
        if isinstance(node, ast.IfExp):
            a, b = kind(node.body), kind(node.orelse)
            return a if a == b else (a or b)
        return None

    files = (glob.glob(os.path.join(root, "i-dccrn-vae_amd", "**", "*.py"), recursive=True) + [os.path.join(root, "bench.py")]
             + glob.glob(os.path.join(root, "tests", "*.py")) + glob.glob(os.path.join(root, "tests", "tools", "*.py")))
    bad, seen = [], 0
    for path in files:
        for node in ast.walk(ast.parse(open(path).read())):
            if not isinstance(node, ast.Call):
                continue
            name, args, via_call = None, node.args, False
            fn = node.func
            if isinstance(fn, (ast.Name, ast.Attribute)) and (fn.id if isinstance(fn, ast.Name) else fn.attr) == "call":
                if args and isinstance(args[0], ast.Constant) and isinstance(args[0].value, str):
                    name, args, via_call = args[0].value, args[1:], True
            elif isinstance(fn, ast.Attribute) and fn.attr.startswith("idv_"):
                name = fn.attr
            elif isinstance(fn, ast.Call) and isinstance(fn.func, (ast.Name, ast.Attribute)):
                inner = fn.func.id if isinstance(fn.func, ast.Name) else fn.func.attr
                if inner == "_ll_fn" and fn.args and isinstance(fn.args[0], ast.Constant):
                    name = fn.args[0].value
            if name is None or any(isinstance(a, ast.Starred) for a in args):
                continue
            if name not in protos:
                if via_call:
                    bad.append((path, node.lineno, name, "not declared in the header"))
                continue
            params = protos[name][1]
            seen += 1
            if len(args) != len(params):
                bad.append((path, node.lineno, name, f"{len(args)} arguments, header declares {len(params)}"))
                continue
            for k, (a, t) in enumerate(zip(args, params)):
                kd = kind(a)
                # call() passes wrapped scalars by value (int widens to long long, float to double); a direct call needs the exact type
                ok = kd is None or kd == t or (via_call and ((kd == "int" and t == "long long") or (kd == "float" and t == "double")))
                if not ok:
                    bad.append((path, node.lineno, name, f"argument {k}: {kd} for a {t} parameter"))
    assert seen > 140 and not bad, "\n".join(map(str, bad))
