"""Host side of streaming.StreamingVAETwoLatentsSessions and of the per-slot seeds of both VAE sessions classes (no GPU): the new
draws entry is declared, prototyped and exported, every construction guard raises ValueError before any device check, a slot's
seed can be set between its signals only, and the one host buffer of a call holds the tables, the zero list and the seeds."""
import importlib

import pytest
import torch

from oracle import idccrn_oracle as O

S = importlib.import_module("i-dccrn-vae_amd.streaming")
PM = importlib.import_module("i-dccrn-vae_amd.model.pvae_module")
LIB = importlib.import_module("i-dccrn-vae_amd._lib")

N_FFT, HOP, WIN = 512, 100, 400
SKIP = [0, 1, 2, 3, 4, 5]
F = {name: j for j, name in enumerate(S.ROW_FIELDS)}


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


def test_entry_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    name = "idv_stream_eps_pair_rows"
    assert name in declared and name in protos and hasattr(lib, name)
    assert protos[name] == ("int", ["ptr", "ptr", "int", "int", "int", "int", "ptr", "ptr", "ptr", "ptr", "ptr"])
    # idv_stream_eps_rows with the seed array in the seed's place and a second pair of outputs; the siblings stay as they were
    rows = protos["idv_stream_eps_rows"][1]
    assert protos[name][1] == ["ptr"] + rows[1:-1] + ["ptr", "ptr"] + rows[-1:]
    assert protos["idv_stream_eps_pair"] == ("int", ["long long", "long long"] + ["int"] * 4 + ["ptr"] * 5)
    assert protos["idv_stream_eps"] == ("int", ["long long", "long long"] + ["int"] * 4 + ["ptr"] * 3)
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9


CASES = ["encoder_type", "latent_num_1", "encoder_skip_prepare", "non_causal_encoder", "non_causal_speech", "non_causal_noise",
         "n_fft_speech", "hop_noise", "win_noise", "zdim_speech", "zdim_noise", "num_samples_noise", "recon_differs", "recon_unknown",
         "skip_set_differs", "use_sc_differs", "resynthesis_speech", "resynthesis_noise", "phase2_skip_prepare_speech",
         "phase2_skip_prepare_noise", "skip_prepare_mask_recon", "outtype", "outtype_none", "phase_0", "phase_3", "phase_bool",
         "phase_str", "noise_none_mask", "speech_type", "noise_type", "chain_noise", "slots_zero", "slots_bool", "slots_float", "conv",
         "seed_negative", "seed_bool", "seed_float"]


@pytest.mark.parametrize("case", CASES)
def test_construction_guards_raise_value_error_before_any_device_check(case):
    """Every check_vae_two_latents guard through the new class with slots as the batch, plus the engine check; the models are on
    the CPU, so a guard that came late would meet the RuntimeError of the device check first."""
    kw = dict(slots=2)
    enc, ds, dn = _enc(), _dec(), _dec()
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
    elif case == "slots_zero":
        kw["slots"], match = 0, "batch"
    elif case == "slots_bool":
        kw["slots"], match = True, "batch"
    elif case == "slots_float":
        kw["slots"], match = 2.0, "batch"
    elif case == "conv":
        kw["conv"], match = "auto", "conv"
    elif case == "seed_negative":
        kw["seed"], match = -1, "seed"
    elif case == "seed_bool":
        kw["seed"], match = True, "seed"
    elif case == "seed_float":
        kw["seed"], match = 1.5, "seed"
    with pytest.raises(ValueError, match=match):
        S.StreamingVAETwoLatentsSessions(enc, ds, dn, **kw)


def test_no_callable_eps_and_cpu_models_raise_the_runtime_error():
    with pytest.raises(TypeError):
        S.StreamingVAETwoLatentsSessions(_enc(), _dec(), _dec(), slots=2, eps=lambda t0, k: None)
    for outtype in S.ESTIMATES:
        for phase in (1, 2):
            with pytest.raises(RuntimeError, match="GPU"):
                S.StreamingVAETwoLatentsSessions(_enc(), _dec(), _dec(), slots=2, outtype=outtype, phase=phase)
    with pytest.raises(RuntimeError, match="GPU"):      # clean_direct does not run the noise decoder: None is accepted
        S.StreamingVAETwoLatentsSessions(_enc(), _dec(), None, slots=2, outtype="clean_direct")


def _bare(cls, slots=3):
    """The host side of a sessions streamer alone, as tests/test_stream_vae_sessions_host.py builds it: only ``_seed`` is set
    before ``_init_slots()``."""
    st = object.__new__(cls)
    st.B, st.ns, st.Bn, st.device, st._seed = slots, 2, 2 * slots, torch.device("cpu"), 0
    st.n_fft, st.hop, st.win, st.cap = N_FFT, HOP, WIN, 8
    st._init_slots()
    return st


@pytest.mark.parametrize("cls", ["StreamingVAESessions", "StreamingVAETwoLatentsSessions"])
def test_per_slot_seeds_on_a_bare_object(cls):
    st = _bare(getattr(S, cls))
    assert st.seed == 0 and st.seeds == [0, 0, 0]
    st.seed = 7
    assert st.seeds == [7, 7, 7]
    st.set_seed([2], 2 ** 40 + 3)
    assert st.seed == 7 and st.seeds == [7, 7, 2 ** 40 + 3]
    st.sessions.push([0, 300, 0], [])
    assert st.positions == [0, 300, 0]
    # a slot in mid-signal: the call names it and changes nothing, not even the idle slot named with it
    with pytest.raises(ValueError, match="slot 1"):
        st.set_seed([0, 1], 9)
    with pytest.raises(ValueError, match="slot 1"):
        st.set_seed((1,), 9)
    assert st.seeds == [7, 7, 2 ** 40 + 3]
    st.set_seed([0], 5)                         # its neighbour at position 0 can be set meanwhile
    st.set_seed({2, 0}, 5)
    assert st.seeds == [5, 7, 5] and st.seed == 7
    for bad in (-1, 1.5, True, 2 ** 63, "3", None):
        with pytest.raises(ValueError, match="seed"):
            st.set_seed([0], bad)
    for bad in ([3], [-1], [True], [1.0], torch.tensor([0]), "0", 0):
        with pytest.raises(ValueError, match="slot"):
            st.set_seed(bad, 1)
    assert st.seeds == [5, 7, 5]
    st.set_seed([], 11)
    assert st.seeds == [5, 7, 5]
    # seed = keeps its rule, and clears the overrides only when it goes through
    with pytest.raises(ValueError, match="between signals"):
        st.seed = 8
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            st.seed = bad
    assert st.seed == 7 and st.seeds == [5, 7, 5]
    # a slot's own seed survives the end of its signal and drop
    st.set_seed([2], 6)
    st.sessions.push([0, 0, 300], [])
    st.sessions.push([0, 0, 100], [2])
    assert st.positions == [0, 300, 0] and st.seeds == [5, 7, 6]
    st.sessions.drop([1])
    st.set_seed([1], 4)
    assert st.seeds == [5, 4, 6]
    st.seed = 8
    assert st.seed == 8 and st.seeds == [8, 8, 8]


def test_call_buffer_is_tables_zero_list_seeds_and_nothing_else():
    ns, B = 3, 4
    sp = S.SessionPlan(B, N_FFT, HOP, WIN, cap=4)
    sp.push([700, 0, 300, 250], [])
    call = sp.push([250, 0, 100, 50], [2])        # slot 0: 2 frames, slot 1 idle, slot 2 ends at 400 samples, slot 3: 1 frame
    assert len(call.groups) >= 2 and any(g.flush for g in call.groups) and call.zero == [2]
    seeds = [0, 5, 2 ** 40 + 3, 2 ** 63 - 1]
    flat = S.vae_session_tables(call, ns, seeds)
    per = (B + B * ns) * S.NF
    assert len(flat) == per * len(call.groups) + len(call.zero) + B
    for gi, g in enumerate(call.groups):
        slot_t = torch.tensor(flat[gi * per:gi * per + B * S.NF]).view(B, S.NF)
        dec_t = torch.tensor(flat[gi * per + B * S.NF:(gi + 1) * per]).view(B * ns, S.NF)
        assert slot_t.tolist() == g.rows
        assert torch.equal(dec_t, slot_t.repeat_interleave(ns, dim=0))
    rest = flat[per * len(call.groups):]
    assert rest == call.zero + seeds
    assert S.vae_session_tables(call, ns) == flat[:-B]                   # without seeds: what it returned before
    # the whole buffer is int64 material
    assert torch.tensor(flat, dtype=torch.int64).tolist() == flat
    # a call without groups still carries nothing but the zero list and the seeds
    empty = S.SessionCall([], [0] * B, [])
    assert S.vae_session_tables(empty, ns, seeds) == seeds
