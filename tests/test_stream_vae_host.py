"""Host side of streaming.StreamingVAE (no GPU): every construction guard raises before any GPU call, and the three new C
entries are declared, exported and answer their host-only queries."""
import importlib

import pytest
import torch

from oracle import idccrn_oracle as O

S = importlib.import_module("i-dccrn-vae_amd.streaming")
PM = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")
StreamingVAE = S.StreamingVAE

N_FFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]


def _enc(causal=True, zdim=16, ns=2, latent_num=2, n_fft=N_FFT):
    return PM.nsvae_pvae_dccrn_encoder_twophase(O.net_params(causal, 4), causal, "cpu", zdim, n_fft, HOP, WIN, ns, latent_num)


def _enc1(zdim=16, ns=2):
    return PM.pvae_dccrn_encoder_skip_prepare(O.net_params(True, 4), True, "cpu", zdim, N_FFT, HOP, WIN, ns)


def _dec(causal=True, zdim=16, ns=2, recon="mask", skip=SKIP, n_fft=N_FFT, base=4):
    return PM.nsvae_pvae_dccrn_decoder_twophase(O.net_params(causal, base), causal, "cpu", ns, zdim, n_fft, HOP, WIN, recon, True, skip,
                                                False)


def _dec_zero(zdim=16, ns=2):
    return PM.pvae_dccrn_decoder_skip_prepare(O.net_params(True, 4), True, "cpu", ns, zdim, N_FFT, HOP, WIN, "real_imag", SKIP)


def _dccrn():
    return PM.DCCRN_(N_FFT, HOP, O.net_params(True, 4), True, "cpu", WIN, SKIP, "mask", False, None, None)


def test_entries_declared_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_stream_clstm_wide_supported", "idv_stream_clstm_wide_hstep_floats", "idv_stream_clstm_wide", "idv_stream_eps",
                 "idv_stream_repeat"):
        assert name in declared and name in protos and hasattr(lib, name), name
    assert protos["idv_stream_clstm_wide"] == protos["idv_stream_clstm"]
    assert LIB.declared_abi_version() == int(lib.idv_abi_version())


def test_wide_lstm_sizes():
    sup = LIB.lib().idv_stream_clstm_wide_supported
    for H in (16, 48, 96, 128, 384, 768):
        assert sup(H) == 1, H
    for H in (0, -16, 8, 24, 100, 769, 784, 1536):
        assert sup(H) == 0, H
    work = LIB.lib().idv_stream_clstm_wide_hstep_floats
    assert work(768, 2, 3) == 8 * 3 * 2 * 768 and work(100, 2, 3) < 0 and work(96, 0, 3) < 0 and work(96, 1, 0) < 0


@pytest.mark.parametrize("case", ["encoder_type", "decoder_type", "pad_zero_decoder", "non_causal_encoder", "non_causal_decoder",
                                  "zdim", "num_samples", "n_fft", "noise_latent_num_1", "noise_skip_prepare", "latent", "batch_zero",
                                  "batch_bool", "batch_float", "conv", "seed_negative", "seed_float", "seed_bool", "eps", "recon",
                                  "chain"])
def test_guards_raise_value_error_before_gpu_work(case):
    kw = dict(batch=2)
    enc, dec = _enc(), _dec()
    match = None
    if case == "encoder_type":
        enc, match = _dccrn(), "noisy_encoder"
    elif case == "decoder_type":
        dec, match = _dccrn(), "decoder"
    elif case == "pad_zero_decoder":
        dec, match = _dec_zero(), "pad='zero'"
    elif case == "non_causal_encoder":
        enc, match = _enc(causal=False), "causal"
    elif case == "non_causal_decoder":
        dec, match = _dec(causal=False), "causal"
    elif case == "zdim":
        dec, match = _dec(zdim=32), "zdim"
    elif case == "num_samples":
        dec, match = _dec(ns=3), "num_samples"
    elif case == "n_fft":
        dec, match = _dec(n_fft=400), "n_fft"
    elif case == "noise_latent_num_1":
        enc, match = _enc(latent_num=1), "latent_num"
        kw["latent"] = "noise"
    elif case == "noise_skip_prepare":
        enc, match = _enc1(), "latent_num"
        kw["latent"] = "noise"
    elif case == "latent":
        kw["latent"], match = "music", "latent"
    elif case == "batch_zero":
        kw["batch"], match = 0, "batch"
    elif case == "batch_bool":
        kw["batch"], match = True, "batch"
    elif case == "batch_float":
        kw["batch"], match = 2.0, "batch"
    elif case == "conv":
        kw["conv"], match = "auto", "conv"
    elif case == "seed_negative":
        kw["seed"], match = -1, "seed"
    elif case == "seed_float":
        kw["seed"], match = 1.5, "seed"
    elif case == "seed_bool":
        kw["seed"], match = True, "seed"
    elif case == "eps":
        kw["eps"], match = (torch.zeros(1), torch.zeros(1)), "eps"
    elif case == "recon":
        dec, match = _dec(recon="polar"), "recon_type"
    elif case == "chain":
        dec, match = _dec(base=8), "decoder"
    with pytest.raises(ValueError, match=match):
        StreamingVAE(enc, dec, **kw)
    if case not in ("conv",):
        with pytest.raises(ValueError, match=match):
            S.check_vae(enc, dec, kw["batch"], kw.get("latent", "speech"), kw.get("seed", 0), kw.get("eps"))


@pytest.mark.parametrize("latent_num", [1, 2])
def test_cpu_parameters_raise_the_streamers_runtime_error(latent_num):
    with pytest.raises(RuntimeError, match="GPU"):
        StreamingVAE(_enc(latent_num=latent_num), _dec(), batch=2)
    with pytest.raises(RuntimeError, match="GPU"):
        StreamingVAE(_enc1(), _dec(), batch=1, eps=lambda t0, k: None)
    with pytest.raises(RuntimeError, match="GPU"):
        S.check_vae(_enc(), _dec(recon="real_imag"), 3, "noise", 2 ** 40, None)
