"""Host side of streaming.StreamingVAETwoLatents (no GPU): the two new C entries are declared and exported, every construction
guard raises ValueError before any GPU call, and CPU parameters raise the streamers' RuntimeError."""
import importlib

import pytest
import torch

from oracle import idccrn_oracle as O

S = importlib.import_module("i-dccrn-vae_amd.streaming")
PM = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")
INF = importlib.import_module("i-dccrn-vae_amd.inference")
Two = S.StreamingVAETwoLatents

N_FFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]


def _enc(causal=True, zdim=16, ns=2, latent_num=2):
    return PM.nsvae_pvae_dccrn_encoder_twophase(O.net_params(causal, 4), causal, "cpu", zdim, N_FFT, HOP, WIN, ns, latent_num)


def _enc1(zdim=16, ns=2):
    return PM.pvae_dccrn_encoder_skip_prepare(O.net_params(True, 4), True, "cpu", zdim, N_FFT, HOP, WIN, ns)


def _dec(causal=True, zdim=16, ns=2, recon="mask", skip=SKIP, n_fft=N_FFT, hop=HOP, win=WIN, base=4, use_sc=True, resynthesis=False):
    return PM.nsvae_pvae_dccrn_decoder_twophase(O.net_params(causal, base), causal, "cpu", ns, zdim, n_fft, hop, win, recon, use_sc,
                                                skip, resynthesis)


def _dec_zero(zdim=16, ns=2, recon="real_imag"):
    return PM.pvae_dccrn_decoder_skip_prepare(O.net_params(True, 4), True, "cpu", ns, zdim, N_FFT, HOP, WIN, recon, SKIP)


def _dccrn():
    return PM.DCCRN_(N_FFT, HOP, O.net_params(True, 4), True, "cpu", WIN, SKIP, "mask", False, None, None)


def test_entries_declared_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_stream_eps_pair", "idv_stream_estimate"):
        assert name in declared and name in protos and hasattr(lib, name), name
    # idv_stream_eps with a second pair of outputs
    ret, params = protos["idv_stream_eps"]
    assert protos["idv_stream_eps_pair"] == (ret, params[:-1] + ["ptr", "ptr"] + params[-1:])
    assert protos["idv_stream_estimate"] == ("int", ["ptr"] * 3 + ["int"] * 9 + ["ptr", "ptr"])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version())
    assert S.ESTIMATES == ("clean_direct",) + tuple(sorted(INF.OUTTYPES, key=INF.OUTTYPES.get))


CASES = ["encoder_type", "latent_num_1", "encoder_skip_prepare", "non_causal_encoder", "non_causal_speech", "non_causal_noise",
         "n_fft_speech", "hop_noise", "win_noise", "zdim_speech", "zdim_noise", "num_samples_noise", "recon_differs", "recon_unknown",
         "skip_set_differs", "use_sc_differs", "resynthesis_speech", "resynthesis_noise", "phase2_skip_prepare_speech",
         "phase2_skip_prepare_noise", "skip_prepare_mask_recon", "outtype", "outtype_none", "phase_0", "phase_3", "phase_bool",
         "phase_str", "noise_none_mask", "speech_type", "noise_type", "chain_noise", "batch_zero", "batch_bool", "conv",
         "seed_negative", "seed_bool", "eps"]


@pytest.mark.parametrize("case", CASES)
def test_guards_raise_value_error_before_gpu_work(case):
    kw = dict(batch=2)
    enc, ds, dn = _enc(), _dec(), _dec()
    match = None
    if case == "encoder_type":
        enc, match = _dccrn(), "noisy_encoder"
    elif case == "latent_num_1":
        enc, match = _enc(latent_num=1), "latent_num"
    elif case == "encoder_skip_prepare":
        enc, match = _enc1(), "latent_num"
    elif case == "non_causal_encoder":
        enc, match = _enc(causal=False), "causal"
    elif case == "non_causal_speech":
        ds, match = _dec(causal=False), "causal encoder and speech_decoder"
    elif case == "non_causal_noise":
        dn, match = _dec(causal=False), "causal encoder and noise_decoder"
    elif case == "n_fft_speech":
        ds, match = _dec(n_fft=400), "speech_decoder differ in n_fft"
    elif case == "hop_noise":
        dn, match = _dec(hop=128), "noise_decoder differ in n_fft / hop / win"
    elif case == "win_noise":
        dn, match = _dec(win=512), "noise_decoder differ in n_fft / hop / win"
    elif case == "zdim_speech":
        ds, match = _dec(zdim=32), "speech_decoder differ in zdim"
    elif case == "zdim_noise":
        dn, match = _dec(zdim=32), "noise_decoder differ in zdim"
    elif case == "num_samples_noise":
        dn, match = _dec(ns=3), "num_samples"
    elif case == "recon_differs":
        dn, match = _dec(recon="real_imag"), "differ in recon_type"
    elif case == "recon_unknown":
        ds, dn, match = _dec(recon="polar"), _dec(recon="polar"), "unknown recon_type"
    elif case == "skip_set_differs":
        dn, match = _dec(skip=[0, 1, 2]), "skip set"
    elif case == "use_sc_differs":
        dn, match = _dec(use_sc=False), "skip set"
    elif case == "resynthesis_speech":
        ds, match = _dec(resynthesis=True), "speech_decoder has resynthesis=True"
    elif case == "resynthesis_noise":
        dn, match = _dec(resynthesis=True), "noise_decoder has resynthesis=True"
    elif case == "phase2_skip_prepare_speech":
        ds, dn, match = _dec_zero(), _dec_zero(), "phase=2 .* speech_decoder"
    elif case == "phase2_skip_prepare_noise":
        ds, dn, match = _dec(recon="real_imag"), _dec_zero(), "phase=2 .* noise_decoder"
    elif case == "skip_prepare_mask_recon":
        ds, dn, match = _dec_zero(recon="mask"), _dec_zero(recon="mask"), "real_imag"
        kw["phase"] = 1
    elif case == "outtype":
        kw["outtype"], match = "wiener", "outtype"
    elif case == "outtype_none":
        kw["outtype"], match = None, "outtype"
    elif case == "phase_0":
        kw["phase"], match = 0, "phase"
    elif case == "phase_3":
        kw["phase"], match = 3, "phase"
    elif case == "phase_bool":
        kw["phase"], match = True, "phase"
    elif case == "phase_str":
        kw["phase"], match = "2", "phase"
    elif case == "noise_none_mask":
        dn, match = None, "needs a noise_decoder"
    elif case == "speech_type":
        ds, match = _dccrn(), "as speech_decoder"
    elif case == "noise_type":
        dn, match = _dccrn(), "as noise_decoder"
    elif case == "chain_noise":
        dn, match = _dec(base=8), "noise_decoder"
    elif case == "batch_zero":
        kw["batch"], match = 0, "batch"
    elif case == "batch_bool":
        kw["batch"], match = True, "batch"
    elif case == "conv":
        kw["conv"], match = "auto", "conv"
    elif case == "seed_negative":
        kw["seed"], match = -1, "seed"
    elif case == "seed_bool":
        kw["seed"], match = True, "seed"
    elif case == "eps":
        kw["eps"], match = tuple(torch.zeros(1) for _ in range(4)), "eps"
    with pytest.raises(ValueError, match=match):
        Two(enc, ds, dn, **kw)
    if case != "conv":
        with pytest.raises(ValueError, match=match):
            S.check_vae_two_latents(enc, ds, dn, kw["batch"], kw.get("outtype", "phase_mask"), kw.get("phase", 2), kw.get("seed", 0),
                                    kw.get("eps"))


@pytest.mark.parametrize("outtype", S.ESTIMATES)
@pytest.mark.parametrize("phase", [1, 2])
def test_cpu_parameters_raise_the_streamers_runtime_error(outtype, phase):
    """Every accepted configuration passes all ValueError guards and stops at the CPU parameters."""
    with pytest.raises(RuntimeError, match="GPU"):
        Two(_enc(), _dec(), _dec(), batch=2, outtype=outtype, phase=phase)
    if phase == 1:
        with pytest.raises(RuntimeError, match="GPU"):
            Two(_enc(), _dec_zero(), _dec_zero(), batch=1, outtype=outtype, phase=1, eps=lambda t0, k: None)
    if outtype == "clean_direct":      # the noise decoder is not run: None, or anything else, is accepted; resynthesis does not matter
        for dn in (None, _dec(zdim=32)):
            with pytest.raises(RuntimeError, match="GPU"):
                Two(_enc(), _dec(resynthesis=True), dn, batch=3, outtype=outtype, phase=phase)
    with pytest.raises(RuntimeError, match="GPU"):
        S.check_vae_two_latents(_enc(), _dec(recon="real_imag"), _dec(recon="real_imag"), 3, outtype, phase, 2 ** 40, None)
