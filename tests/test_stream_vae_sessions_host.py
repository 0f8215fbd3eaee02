"""Host side of streaming.StreamingVAESessions (no GPU): the three _rows entries are declared, prototyped and exported, every
construction guard and every push guard raises before any GPU call, the seed cannot change in mid-signal, and the decoder-side
table of a launch group is the slots' table with every row repeated num_samples times."""
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


def test_entries_declared_prototyped_and_exported():
    declared, protos, lib = LIB.declared_symbols(), LIB.prototypes(), LIB.lib()
    for name in ("idv_stream_clstm_wide_rows", "idv_stream_eps_rows", "idv_stream_repeat_rows"):
        assert name in declared and name in protos and hasattr(lib, name), name
    # the lock-step prototype with k_launch in k's place and the table in front of the stream (eps: in t0's and k's place)
    wide = protos["idv_stream_clstm_wide"][1]
    assert protos["idv_stream_clstm_wide_rows"] == ("int", wide[:-1] + ["ptr", "ptr"])
    assert protos["idv_stream_clstm_wide_rows"] == protos["idv_stream_clstm_rows"]
    assert protos["idv_stream_eps_rows"] == ("int", ["long long", "ptr", "int", "int", "int", "int", "ptr", "ptr", "ptr"])
    rep = protos["idv_stream_repeat"][1]
    assert protos["idv_stream_repeat_rows"] == ("int", rep[:9] + ["ptr"] + rep[9:])
    assert LIB.declared_abi_version() == int(lib.idv_abi_version()) == 9
    with open(LIB.HEADER_PATH) as f:
        assert "Lock-step only" not in f.read()


@pytest.mark.parametrize("case", ["encoder_type", "decoder_type", "pad_zero_decoder", "non_causal_encoder", "non_causal_decoder",
                                  "zdim", "num_samples", "n_fft", "noise_latent_num_1", "noise_skip_prepare", "latent", "slots_zero",
                                  "slots_bool", "slots_float", "conv", "seed_negative", "seed_float", "seed_bool", "recon", "chain"])
def test_construction_guards_raise_value_error_before_gpu_work(case):
    """Every check_vae guard, through the new class, with slots as batch (the models are on the CPU: a guard that came late
    would meet the RuntimeError of the device check or a GPU call first)."""
    kw = dict(slots=2)
    enc, dec = _enc(), _dec()
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
    elif case == "seed_float":
        kw["seed"], match = 1.5, "seed"
    elif case == "seed_bool":
        kw["seed"], match = True, "seed"
    elif case == "recon":
        dec, match = _dec(recon="polar"), "recon_type"
    elif case == "chain":
        dec, match = _dec(base=8), "decoder"
    with pytest.raises(ValueError, match=match):
        S.StreamingVAESessions(enc, dec, **kw)


def test_no_callable_eps_and_cpu_models_raise_the_runtime_error():
    with pytest.raises(TypeError):
        S.StreamingVAESessions(_enc(), _dec(), slots=2, eps=lambda t0, k: None)
    with pytest.raises(RuntimeError, match="GPU"):
        S.StreamingVAESessions(_enc(), _dec(), slots=2)


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it lives on the GPU (there is none here)."""
    is_cuda = property(lambda self: True)


def _bare(slots=3):
    """The host side of a StreamingVAESessions alone: what push's guards and the seed setter read.  It owns no buffer, so a
    guard that let a call through would fail on the first attribute of the GPU side."""
    st = object.__new__(S.StreamingVAESessions)
    st.B, st.ns, st.Bn, st.device, st._seed = slots, 2, 2 * slots, torch.device("cpu"), 0
    st.n_fft, st.hop, st.win, st.cap = N_FFT, HOP, WIN, 8
    st._init_slots()
    return st


def test_push_guards_raise_before_gpu_work_and_bookkeeping():
    st = _bare()
    x = torch.zeros(3, 10).as_subclass(_OnGpu)
    st.sessions.push([100, 250, 0], [])
    before = (st.positions, st.sessions.snapshot())
    with pytest.raises(ValueError, match="tensor"):
        st.push([[0.0] * 10] * 3)
    with pytest.raises(ValueError, match="expected 3 streams"):
        st.push(torch.zeros(2, 10).as_subclass(_OnGpu))
    with pytest.raises(RuntimeError, match="GPU"):
        st.push(torch.zeros(3, 10))
    with pytest.raises(ValueError, match="GPU tensor"):
        st.push(x, counts=torch.tensor([1, 2, 3]).as_subclass(_OnGpu))
    with pytest.raises(ValueError, match="2 counts for 3 slots"):
        st.push(x, counts=[1, 2])
    for bad in ([1, 2, 11], [1, -1, 3]):
        with pytest.raises(ValueError, match="0 .. 10"):
            st.push(x, counts=bad)
    with pytest.raises(ValueError, match="integers"):
        st.push(x, counts=[1, 2.0, 3])
    with pytest.raises(ValueError, match="0 .. 2"):
        st.push(x, end=[3])
    with pytest.raises(ValueError, match="collection"):
        st.push(x, end=torch.tensor([1]))
    for counts, end in (([10, 0, 0], [0]), ([0, 6, 0], [1]), ([0, 0, 7], [2, 1])):      # 110 / 256 / 7 samples in total
        with pytest.raises(ValueError, match="n_fft/2"):
            st.push(x, counts=counts, end=end)
    with pytest.raises(ValueError, match="0 .. 2"):
        st.drop([-1])
    assert (st.positions, st.sessions.snapshot()) == before


def test_seed_setter_raises_in_mid_signal():
    st = _bare()
    st.seed = 7
    assert st.seed == 7
    st.sessions.push([0, 300, 0], [])
    assert st.positions == [0, 300, 0]
    with pytest.raises(ValueError, match="between signals"):
        st.seed = 8
    assert st.seed == 7
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="seed"):
            st.seed = bad
    st.sessions.drop([1])
    st.seed = 8
    assert st.seed == 8


def test_decoder_table_repeats_every_slot_row():
    ns = 3
    sp = S.SessionPlan(4, N_FFT, HOP, WIN, cap=4)
    sp.push([700, 0, 300, 250], [])
    call = sp.push([250, 0, 100, 50], [2])        # slot 0: 2 frames, slot 1 idle, slot 2 ends at 400 samples, slot 3: 1 frame
    ks = [[r[F["k"]] for r in g.rows] for g in call.groups]
    assert ks[0] == [2, 0, 1, 1] and any(g.flush for g in call.groups) and call.zero == [2]
    assert call.groups[-1].rows[2][F["L_end"]] == 400 and call.groups[-1].rows[1][F["k"]] == 0
    flat = S.vae_session_tables(call, ns)
    per = (4 + 4 * ns) * S.NF
    assert len(flat) == per * len(call.groups) + 1 and flat[-1:] == [2]
    for gi, g in enumerate(call.groups):
        slot_t = torch.tensor(flat[gi * per:gi * per + 4 * S.NF]).view(4, S.NF)
        dec_t = torch.tensor(flat[gi * per + 4 * S.NF:(gi + 1) * per]).view(4 * ns, S.NF)
        assert slot_t.tolist() == g.rows
        assert torch.equal(dec_t, slot_t.repeat_interleave(ns, dim=0))
        assert S.decoder_rows(g.rows, ns) == dec_t.tolist()
        for b in range(4):
            for s in range(ns):
                assert dec_t[b * ns + s].tolist() == g.rows[b]
        # the decoder side's overlap-add at batch B * ns passes the same host check as the slots' table
        host = dec_t.contiguous()
        assert LIB.lib().idv_stream_rows_check(LIB._P(host.data_ptr()), 4 * ns, N_FFT, 0 if g.flush else 250, N_FFT, WIN, HOP,
                                               N_FFT + WIN, g.k, g.k + 1, max(call.m), g.span) == 0
