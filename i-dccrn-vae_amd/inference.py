"""Enhancement inference as the reference's evaluation scripts run it, batched on the GPU.

  * supervised (supervised_dccrn/test.py:123-137): ``model(noisy, train=False)[0]``;
  * I-DCCRN-VAE (i_dccrn_vae/nsvae_dccrn/test_se_cvaefinetune.py:251-311): noisy encoder (eval) -> fine-tuned decoder with
    the noisy skips (``pad='sig'``) on ``num_samples`` (10 in test_se_cvaefinetune.sh) latent draws -> mean over the sampled
    waveforms.  The reference feeds one utterance at a time (``tmp_x[None]``); here a batch of utterances goes through at
    once (utterances are independent in eval mode: folded batch norm);
  * the two-latent evaluation (test_se_cvaefinetune.py:261-305, ``latent_to_use == 2``): speech AND noise decoders on their
    latents, then one of the ``outtype`` estimators -- ``clean_direct`` (mean of the sampled speech waveforms),
    ``real_imag_mask`` (:85-101), ``complex_mask`` (:104-116), ``phase_mask`` (:119-135) -- as one HIP kernel
    (``idv_outtype_estimate``) + the ISTFT (``torch.istft`` with the analysis window, :288 etc.);
  * the metrics of ``EvalMetrics.eval`` (utils/eval_metrics.py:67-122) that are closed-form signal pipelines, on the device:
    ``compute_sisdr`` (:49-64), ``compute_rmse`` (:33-41) and ``compute_stoi`` / ``compute_estoi`` (the ``pystoi`` call of :92-95
    and :119; csrc/stoi.hip, DESIGN 3.8 -- the package's definition restated, parity with the package itself pinned only where it
    is installed); :func:`score_list` scores a list of recordings of any lengths in padded batches.  PESQ (an ITU program) and
    DNSMOS (an ONNX model) are third-party CPU metrics and stay out of scope;
  * beside them ``compute_sdr``, the BSS-eval SDR with a 512-tap distortion filter (``mir_eval.separation.bss_eval_sources`` for one
    source; csrc/sdr.hip): the waveform metric that does not count a delay or the early reflections of a reverberant
    mixture as error when the estimate is scored against the dry recording; ``score_list`` knows it as "sdr";
  * and ``compute_bss``, the same decomposition with the noise as second source (csrc/bss.hip): SDR, SIR (the other
    source leaking through) and SAR (distortion the system made itself); ``score_list(..., interferers=...)`` knows them as "sir"
    and "sar";
  * the resampling the evaluation scripts do with librosa in front of these (test_se_cvaefinetune.py:236-239, the 48 kHz
    VoiceBank-DEMAND references): :func:`resample` / :func:`resample_list`, a rational polyphase resampler with
    ``scipy.signal.resample_poly``'s definition (csrc/resample.hip; librosa's own soxr filter is another one and is
    not pinned).  ``enhance_list`` and ``score_list`` take 16 kHz signals as before: the calls compose;
  * the silence trimming in front of the scoring (i_dccrn_vae/pretrained_vaes/test_prevae.py:154-155, ``librosa.effects.trim(x,
    top_db=30)``) and of the loaders' segment index: :func:`trim` / :func:`trim_list` (csrc/trim.hip; librosa 0.10's
    definition restated, parity with the package itself unpinned).

Utterances of different lengths (causal models, the ones every shipped recipe builds): every entry point takes ``lengths``
(a python sequence or a CPU integer tensor, one sample count per row of the zero- or anything-padded ``[B, Lmax]`` batch).  Row
b of the result then holds the ``hop * (lengths[b] // hop)`` samples the model gives for that utterance alone, followed by zeros up
to ``hop * (Tmax - 1)``, ``Tmax = 1 + max(lengths) // hop``.  In a causal network frame t depends on frames <= t only, so only the
STFT framing (each row mirrored at its own end), the ISTFT overlap-add (each row over its own frames and their envelope) and
``compute_sisdr`` read the lengths.  :func:`enhance_list` takes a list of signals of any lengths, groups them into such batches
(:func:`plan_ragged_batches`) and returns the enhanced signals in the caller's order.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import torch

from . import ops
from ._lib import call, p, i, ll, stream_ptr


def mean_over_samples(recon: torch.Tensor, num_samples: int) -> torch.Tensor:
    """[B*ns, L] -> [B, L]: ``torch.mean(recon_sig_clean, dim=0)`` per utterance (test_se_cvaefinetune.py:309-311)."""
    ops.check_dev_f32(recon, "recon")
    Bn, L = recon.shape
    if Bn % num_samples:
        raise ValueError("batch is not a multiple of num_samples")
    recon = recon.float().contiguous()
    out = torch.empty(Bn // num_samples, L, dtype=torch.float32, device=recon.device)
    call("idv_mean_over_samples", p(recon), i(num_samples), i(Bn // num_samples), i(L), p(out), stream_ptr())
    return out


@torch.no_grad()
def enhance_supervised(model, noisy: torch.Tensor, check: bool = True, lengths=None) -> torch.Tensor:
    """DCCRN / DCCRN-CL: [B, L] -> enhanced [B, hop*(T-1)].  ``check`` (all three entry points): synchronise and raise
    ``ops.CoopTimeout`` here, at the operation that owns it, if a cooperative LSTM recurrence of this forward timed out
    (its outputs would be NaN); ``check=False`` keeps the call asynchronous (call ``ops.coop_check()`` yourself).
    ``lengths`` (all three entry points): per-row sample counts of a padded batch, see the module docstring."""
    if lengths is None:
        return _checked(model(noisy, train=False)[0], check)
    return _checked(model(noisy, train=False, lengths=lengths)[0], check)


def _checked(out: torch.Tensor, check: bool) -> torch.Tensor:
    if check:
        ops.coop_check()
    return out


@torch.no_grad()
def enhance_vae(noisy_encoder, decoder, noisy: torch.Tensor, eps=None, latent: str = "speech", check: bool = True,
                lengths=None) -> torch.Tensor:
    """I-DCCRN-VAE (phase 2, latent_to_use 1): [B, L] -> mean of the num_samples decoded waveforms, [B, hop*(T-1)].
    ``eps``: optional injected Gaussian draws (see the encoder's forward)."""
    r = _encode(noisy_encoder, noisy, eps, lengths)
    z = r[0] if latent == "speech" else r[4]
    if z is None:
        raise ValueError("this encoder has no noise latent (latent_num == 1)")
    skiper, C, F, stft_x = r[8], r[9], r[10], r[11]
    recon, _ = decoder(stft_x, z, skiper, C, F, train=False, pad="sig")
    return _checked(mean_over_samples(recon, noisy_encoder.num_samples), check)


def _encode(noisy_encoder, noisy, eps, lengths):
    if lengths is None:
        return noisy_encoder(noisy, train=False, eps=eps)
    return noisy_encoder(noisy, train=False, eps=eps, lengths=lengths)


OUTTYPES = {"real_imag_mask": 0, "complex_mask": 1, "phase_mask": 2}


def outtype_estimate(predict_noise: torch.Tensor, predict_speech: torch.Tensor, stft_noisy: torch.Tensor, outtype: str,
                     num_samples: int):
    """The mask estimators of test_se_cvaefinetune.py:85-135 for a batch: predict_* complex [B*ns, F, T] (the decoders'
    second output), stft_noisy [B, F, T, 2] (any strides) -> (planar spectrum for ops.istft, complex [B, F, T])."""
    if outtype not in OUTTYPES:
        raise ValueError(f"outtype {outtype!r}: expected one of {sorted(OUTTYPES)} (or 'clean_direct')")
    for t, n in ((predict_noise, "predict_noise"), (predict_speech, "predict_speech")):
        if not (t.is_cuda and t.dtype == torch.complex64):
            raise RuntimeError(f"{n} must be a complex64 tensor on the GPU (there is no CPU fallback)")
    ops.check_dev_f32(stft_noisy, "stft_noisy", predict_speech.device)
    Bn, F, T = predict_speech.shape
    if Bn % num_samples or predict_noise.shape != predict_speech.shape:
        raise ValueError("predict_speech / predict_noise must both be [B * num_samples, F, T]")
    B = Bn // num_samples
    if tuple(stft_noisy.shape) != (B, F, T, 2):
        raise ValueError(f"stft_noisy {tuple(stft_noisy.shape)}: expected {(B, F, T, 2)}")
    sp = torch.view_as_real(predict_speech.contiguous())
    no = torch.view_as_real(predict_noise.contiguous())
    out = ops.Planar.empty(1, F, B, T, T + 1, sp.device)
    oc = torch.empty(B, F, T, 2, dtype=torch.float32, device=sp.device)
    sb, sf, st_, sr = stft_noisy.stride()
    call("idv_outtype_estimate", p(sp), p(no), p(stft_noisy), ll(sb), ll(sf), ll(st_), ll(sr), i(OUTTYPES[outtype]), i(num_samples),
         i(B), i(F), i(T), i(out.Tp), i(out.Jp), out.ptr(), p(oc), stream_ptr())
    return out, torch.view_as_complex(oc)


@torch.no_grad()
def enhance_vae_two_latents(noisy_encoder, speech_decoder, noise_decoder, noisy: torch.Tensor, outtype: str = "clean_direct",
                            phase: int = 2, eps=None, check: bool = True, lengths=None) -> torch.Tensor:
    """latent_to_use == 2 (test_se_cvaefinetune.py:261-305): the noisy encoder's speech latent through the speech decoder and
    its noise latent through the noise decoder (phase 1: the pre-trained decoders, zero skips, :263-264; phase 2: the
    fine-tuned decoders with the noisy skips, ``pad='sig'``, :295-296), then the ``outtype`` estimator -> enhanced [B, L]."""
    r = _encode(noisy_encoder, noisy, eps, lengths)
    if r[4] is None:
        raise ValueError("this encoder has no noise latent (latent_num == 1)")
    z_s, z_n, skiper, C, F, stft_x = r[0], r[4], r[8], r[9], r[10], r[11]
    kw = {"pad": "sig"} if phase == 2 else {}
    rec_s, pred_s = speech_decoder(stft_x, z_s, skiper, C, F, train=False, **kw)
    ns = noisy_encoder.num_samples
    if outtype == "clean_direct":
        return _checked(mean_over_samples(rec_s, ns), check)
    _, pred_n = noise_decoder(stft_x, z_n, skiper, C, F, train=False, **kw)
    spec, _ = outtype_estimate(pred_n, pred_s, stft_x, outtype, ns)
    from .model.pvae_module import dft_plan
    st = noisy_encoder.stft
    return _checked(ops.istft(spec, dft_plan(st.n_fft, st.win_length, st.hop_length, spec.T, spec.buf.device),
                              lengths=getattr(getattr(stft_x, "_idv", None), "lengths", None)), check)


def compute_sisdr(x_est: torch.Tensor, x_ref: torch.Tensor, lengths=None) -> torch.Tensor:
    """SI-SDR in dB per utterance (utils/eval_metrics.py:49-64); inputs [L] or [B, L] on the GPU -> tensor [B] (or scalar).
    ``lengths``: row b is scored over its first lengths[b] samples only (the two inputs may then differ in padded width)."""
    ops.check_dev_f32(x_est, "x_est")
    ops.check_dev_f32(x_ref, "x_ref", x_est.device)
    single = x_est.dim() == 1
    e = x_est.reshape(1, -1) if single else x_est
    r = x_ref.reshape(1, -1) if single else x_ref
    if lengths is not None:
        if e.shape[0] != r.shape[0]:
            raise ValueError(f"estimate {tuple(e.shape)} and reference {tuple(r.shape)} differ in batch size")
        lens = ops.Lengths(ops.check_lengths(lengths, e.shape[0], min(e.shape[1], r.shape[1]), None), e.device)
        e, r = e.float().contiguous(), r.float().contiguous()
        B = e.shape[0]
        work = torch.empty(3 * B, dtype=torch.float64, device=e.device)
        out = torch.empty(B, dtype=torch.float32, device=e.device)
        call("idv_sisdr_ragged", p(r), i(r.stride(0)), p(e), i(e.stride(0)), p(lens.dev), i(B), p(work), p(out), stream_ptr())
        return out[0] if single else out
    if e.shape != r.shape:
        raise ValueError(f"estimate {tuple(e.shape)} and reference {tuple(r.shape)} differ")
    e, r = e.float().contiguous(), r.float().contiguous()
    B, L = e.shape
    work = torch.empty(3 * B, dtype=torch.float64, device=e.device)
    out = torch.empty(B, dtype=torch.float32, device=e.device)
    call("idv_sisdr", p(r), i(r.stride(0)), p(e), i(e.stride(0)), i(B), i(L), p(work), p(out), stream_ptr())
    return out[0] if single else out


def _score_args(x_est, x_ref, lengths):
    """The guards the per-utterance metrics share (all on the host, before any GPU work) -> (est rows, ref rows, Lengths or None,
    samples per row, single).  The value guards come first and the device check last, so each can be met with CPU tensors."""
    if not isinstance(x_est, torch.Tensor) or not isinstance(x_ref, torch.Tensor):
        raise ValueError("x_est and x_ref must be tensors")
    single = x_est.dim() == 1
    e = x_est.reshape(1, -1) if single else x_est
    r = x_ref.reshape(1, -1) if single else x_ref
    if e.dim() != 2 or r.dim() != 2:
        raise ValueError(f"estimate {tuple(x_est.shape)} / reference {tuple(x_ref.shape)}: [L] or [B, L] expected")
    if e.shape[0] != r.shape[0]:
        raise ValueError(f"estimate {tuple(e.shape)} and reference {tuple(r.shape)} differ in batch size")
    if lengths is None:
        if e.shape != r.shape:
            raise ValueError(f"estimate {tuple(e.shape)} and reference {tuple(r.shape)} differ")
        if e.shape[1] < 1:
            raise ValueError("empty signals")
        host, n = None, e.shape[1]
    else:
        host = ops.check_lengths(lengths, e.shape[0], min(e.shape[1], r.shape[1]), None)
        n = max(host)
    ops.check_dev_f32(x_est, "x_est")
    ops.check_dev_f32(x_ref, "x_ref", x_est.device)
    lens = None if host is None else ops.Lengths(host, e.device)
    return e.float().contiguous(), r.float().contiguous(), lens, n, single


def compute_stoi(x_est: torch.Tensor, x_ref: torch.Tensor, fs: int = 16000, extended: bool = False, lengths=None, counts: bool = False):
    """STOI (Taal et al. 2011) or, with ``extended``, ESTOI (Jensen & Taal 2016) per utterance on the device: inputs [L] or [B, L] on
    the GPU -> float32 tensor [B] (or a scalar).  The definition is the ``pystoi`` package's (10 kHz, 256-sample frames at hop 128,
    40 dB silent-frame removal on the reference, 15 third-octave bands, 30-frame segments; exactly 1e-5 when fewer than 30 frames
    remain); parity with the package itself is pinned only where it is installed.

    The argument order is :func:`compute_sisdr`'s and ``EvalMetrics.eval``'s, ESTIMATE FIRST; the package's own call is
    ``stoi(clean, processed, fs, extended)``.  ``fs``: 16000 (resampled on the device) or 10000.  ``lengths``: row b is scored
    over its first lengths[b] samples only; nothing behind them is read and a row's value does not depend on the rest of the batch.
    ``counts=True`` also returns the int32 tensor [B, 3] (or [3]) of (frames, frames kept, segments)."""
    if isinstance(fs, bool) or fs not in (10000, 16000):
        raise ValueError(f"fs = {fs!r}: STOI is defined here for 10000 and 16000 Hz input")
    e, r, lens, n, single = _score_args(x_est, x_ref, lengths)
    B = e.shape[0]
    nbytes = int(ops._ll_fn("idv_stoi_work_bytes")(i(B), i(n), i(fs)))
    if nbytes < 0:
        raise ValueError(f"compute_stoi: a batch of {B} rows of {n} samples is not supported")
    work = torch.empty(nbytes, dtype=torch.uint8, device=e.device)
    out = torch.empty(B, dtype=torch.float32, device=e.device)
    cnt = torch.empty(B, 3, dtype=torch.int32, device=e.device)
    call("idv_stoi", p(r), ll(r.stride(0)), p(e), ll(e.stride(0)), p(None if lens is None else lens.dev), i(B), i(n), i(fs),
         i(1 if extended else 0), p(work), ll(nbytes), p(out), p(cnt), stream_ptr())
    if single:
        out, cnt = out[0], cnt[0]
    return (out, cnt) if counts else out


def compute_estoi(x_est: torch.Tensor, x_ref: torch.Tensor, fs: int = 16000, lengths=None, counts: bool = False):
    """:func:`compute_stoi` with ``extended=True`` (what ``EvalMetrics.eval(..., metric='all')`` reports)."""
    return compute_stoi(x_est, x_ref, fs=fs, extended=True, lengths=lengths, counts=counts)


def compute_rmse(x_est: torch.Tensor, x_ref: torch.Tensor, lengths=None) -> torch.Tensor:
    """The scaled RMSE of utils/eval_metrics.py:33-41 per utterance on the device: alpha = <est, ref> / <est, est>,
    sqrt(mean((alpha est - ref)^2)); inputs and ``lengths`` as :func:`compute_sisdr`."""
    e, r, lens, n, single = _score_args(x_est, x_ref, lengths)
    B = e.shape[0]
    if lens is None:
        lens = ops.Lengths([n] * B, e.device)
    work = torch.empty(3 * B, dtype=torch.float64, device=e.device)
    out = torch.empty(B, dtype=torch.float32, device=e.device)
    call("idv_rmse_ragged", p(r), ll(r.stride(0)), p(e), ll(e.stride(0)), p(lens.dev), i(B), p(work), p(out), stream_ptr())
    return out[0] if single else out


def compute_sdr(x_est: torch.Tensor, x_ref: torch.Tensor, filt_len: int = 512, lengths=None, details: bool = False):
    """BSS-eval SDR in dB per utterance on the device (Vincent et al. 2006; what ``mir_eval.separation.bss_eval_sources`` reports for
    one source with ``flen = filt_len``): inputs [L] or [B, L] on the GPU, ESTIMATE FIRST as in :func:`compute_sisdr` -> float32 tensor
    [B] (or a scalar).  The estimate is split into the part a ``filt_len``-tap filter of the reference explains and the rest:
    ``r[k] = sum s[n] s[n + k]``, ``d[k] = sum s[n] est[n + k]``, ``G c = d`` with ``G[i][j] = r[|i - j|]``, ``p = c * s`` over its
    ``L + filt_len - 1`` samples, ``SDR = 10 log10(sum p^2 / sum (est - p)^2)``, every sum in double (csrc/sdr.hip, DESIGN 3.18;
    tests/sdr_ref.py is the float64 definition; parity with the package itself is pinned only where it is installed).  A delay, a gain
    or early reflections of up to ``filt_len`` samples (32 ms at 16 kHz) therefore do not count as distortion, which they do for SI-SDR.

    ``filt_len``: a multiple of 16 in 16 .. 512.  ``lengths``: row b is scored over its first lengths[b] samples only (a row shorter
    than ``filt_len`` is valid); nothing behind them is read and a row's value does not depend on the rest of the batch.  Special rows:
    NaN for a silent reference, -inf for a silent estimate, +inf for a zero residual, and NaN where the Levinson solve meets a
    non-positive prediction error -- a numerically singular ``G``, e.g. a pure tone without a noise floor, for which the package
    returns an arbitrary finite number.  ``details=True`` also returns a dict of float64 device tensors: ``"filter"`` [B, filt_len]
    (the ``c`` above, the estimated short channel), ``"target_energy"`` and ``"error_energy"`` [B] (without the leading axis for [L]
    input); a float32 dB value hides everything below 4e-6 of it."""
    if isinstance(filt_len, bool) or not isinstance(filt_len, int) or filt_len < 16 or filt_len > 512 or filt_len % 16:
        raise ValueError(f"filt_len = {filt_len!r}: a multiple of 16 in 16 .. 512 expected")
    e, r, lens, n, single = _score_args(x_est, x_ref, lengths)
    B = e.shape[0]
    nbytes = int(ops._ll_fn("idv_sdr_work_bytes")(i(B), i(n), i(filt_len)))
    if nbytes < 0:
        raise ValueError(f"compute_sdr: a batch of {B} rows of {n} samples is not supported")
    work = torch.empty(nbytes, dtype=torch.uint8, device=e.device)
    out = torch.empty(B, dtype=torch.float32, device=e.device)
    det = torch.empty(B, 2, dtype=torch.float64, device=e.device) if details else None
    filt = torch.empty(B, filt_len, dtype=torch.float64, device=e.device) if details else None
    call("idv_sdr", p(r), ll(r.stride(0)), p(e), ll(e.stride(0)), p(None if lens is None else lens.dev), i(B), i(n), i(filt_len),
         p(work), ll(nbytes), p(out), p(det), p(filt), stream_ptr())
    if not details:
        return out[0] if single else out
    info = {"filter": filt, "target_energy": det[:, 0], "error_energy": det[:, 1]}
    if single:
        return out[0], {k: v[0] for k, v in info.items()}
    return out, info


def _score_args3(x_est, x_ref, x_interf, lengths):
    """:func:`_score_args` for an estimate and two references -> (est rows, ref rows, interferer rows, Lengths or None, samples per row,
    single); with ``lengths`` the three inputs may differ in padded width and the lengths are held against the narrowest."""
    if not all(isinstance(x, torch.Tensor) for x in (x_est, x_ref, x_interf)):
        raise ValueError("x_est, x_ref and x_interf must be tensors")
    single = x_est.dim() == 1
    e, r, v = (x.reshape(1, -1) if single else x for x in (x_est, x_ref, x_interf))
    if e.dim() != 2 or r.dim() != 2 or v.dim() != 2:
        raise ValueError(f"estimate {tuple(x_est.shape)} / reference {tuple(x_ref.shape)} / interferer {tuple(x_interf.shape)}: "
                         "[L] or [B, L] expected")
    if e.shape[0] != r.shape[0] or e.shape[0] != v.shape[0]:
        raise ValueError(f"estimate {tuple(e.shape)}, reference {tuple(r.shape)} and interferer {tuple(v.shape)} differ in batch size")
    if lengths is None:
        if e.shape != r.shape or e.shape != v.shape:
            raise ValueError(f"estimate {tuple(e.shape)}, reference {tuple(r.shape)} and interferer {tuple(v.shape)} differ")
        if e.shape[1] < 1:
            raise ValueError("empty signals")
        host, n = None, e.shape[1]
    else:
        host = ops.check_lengths(lengths, e.shape[0], min(e.shape[1], r.shape[1], v.shape[1]), None)
        n = max(host)
    ops.check_dev_f32(x_est, "x_est")
    ops.check_dev_f32(x_ref, "x_ref", x_est.device)
    ops.check_dev_f32(x_interf, "x_interf", x_est.device)
    lens = None if host is None else ops.Lengths(host, e.device)
    return e.float().contiguous(), r.float().contiguous(), v.float().contiguous(), lens, n, single


def compute_bss(x_est: torch.Tensor, x_ref: torch.Tensor, x_interf: torch.Tensor, filt_len: int = 512, lengths=None,
                details: bool = False):
    """BSS-eval SDR, SIR and SAR in dB per utterance on the device, with the noise as the second source (Vincent et al. 2006; what
    ``mir_eval.separation.bss_eval_sources(np.stack([ref, interf]), ..., compute_permutation=False)`` reports for source 0 with
    ``flen = filt_len``): inputs [L] or [B, L] on the GPU, ESTIMATE FIRST as in :func:`compute_sdr`, then the reference of the target
    and the reference of the interferer -> ``(sdr, sir, sar)``, float32 tensors [B] (or scalars).  With ``s = x_ref``, ``v = x_interf``,
    ``y = x_est``: ``p1 = c * s`` is the part of ``y`` a ``filt_len``-tap filter of ``s`` alone explains (:func:`compute_sdr`'s), ``pall =
    C_s * s + C_v * v`` the part filters of both explain jointly (a ``2 filt_len``-square system of four Toeplitz blocks), and

        SDR = 10 log10(sum p1^2 / sum (y - p1)^2)         the value of :func:`compute_sdr`, bit for bit
        SIR = 10 log10(sum p1^2 / sum (pall - p1)^2)      how much of the error is the other source leaking through
        SAR = 10 log10(sum pall^2 / sum (y - pall)^2)     how much is distortion the system made itself

    every sum in double (csrc/bss.hip; tests/bss_ref.py is the float64 definition; parity with the package itself is
    pinned only where it is installed).  To score a NOISE estimate call it with the roles swapped: ``compute_bss(noise_est, noise,
    clean)``.

    ``filt_len``: a multiple of 16 in 16 .. 512.  ``lengths``: row b is scored over its first lengths[b] samples only; nothing behind
    them is read and a row's values do not depend on the rest of the batch.  Each ratio is -inf for a zero numerator, otherwise +inf
    for a zero denominator.  Special rows: three NaN for a silent reference; the SDR of :func:`compute_sdr` and NaN for SIR and SAR
    for a silent interferer, for a row of ``filt_len`` samples or fewer (the joint system is singular whatever the signals) and where
    the block Levinson solve meets an error matrix that is not positive definite -- a numerically singular system, e.g. an interferer
    that is a multiple of the reference.  Rows shorter than about ``2 filt_len`` samples are OVERFITTED: the joint filters explain
    nearly everything and SAR says nothing (293 dB at ``L = filt_len + 1 = 17``).  ``details=True`` also returns a dict of float64
    device tensors: ``"filters"`` [B, 2, filt_len] (``C_s``, ``C_v``), ``"target_energy"`` (sum p1^2), ``"error_energy"`` (sum (y -
    p1)^2), ``"interf_energy"`` (sum (pall - p1)^2), ``"projection_energy"`` (sum pall^2) and ``"artif_energy"`` (sum (y - pall)^2)
    [B] (without the leading axis for [L] input), NaN where the value they stand under is NaN by the special rows."""
    if isinstance(filt_len, bool) or not isinstance(filt_len, int) or filt_len < 16 or filt_len > 512 or filt_len % 16:
        raise ValueError(f"filt_len = {filt_len!r}: a multiple of 16 in 16 .. 512 expected")
    e, r, v, lens, n, single = _score_args3(x_est, x_ref, x_interf, lengths)
    B = e.shape[0]
    nbytes = int(ops._ll_fn("idv_bss_work_bytes")(i(B), i(n), i(filt_len)))
    if nbytes < 0:
        raise ValueError(f"compute_bss: a batch of {B} rows of {n} samples is not supported")
    work = torch.empty(nbytes, dtype=torch.uint8, device=e.device)
    out = torch.empty(B, 3, dtype=torch.float32, device=e.device)
    det = torch.empty(B, 5, dtype=torch.float64, device=e.device) if details else None
    filt = torch.empty(B, 2, filt_len, dtype=torch.float64, device=e.device) if details else None
    call("idv_bss", p(r), ll(r.stride(0)), p(v), ll(v.stride(0)), p(e), ll(e.stride(0)), p(None if lens is None else lens.dev), i(B),
         i(n), i(filt_len), p(work), ll(nbytes), p(out), p(det), p(filt), stream_ptr())
    vals = tuple(out[0, k] if single else out[:, k] for k in range(3))
    if not details:
        return vals
    info = {"filters": filt}
    for k, name in enumerate(("target_energy", "error_energy", "interf_energy", "projection_energy", "artif_energy")):
        info[name] = det[:, k]
    if single:
        info = {k: t[0] for k, t in info.items()}
    return vals + (info,)


# metric name of score_list -> f(padded estimates, padded references, fs, lengths)
METRICS = {"sisdr": lambda e, r, fs, lengths: compute_sisdr(e, r, lengths=lengths),
           "sdr": lambda e, r, fs, lengths: compute_sdr(e, r, lengths=lengths),
           "rmse": lambda e, r, fs, lengths: compute_rmse(e, r, lengths=lengths),
           "stoi": lambda e, r, fs, lengths: compute_stoi(e, r, fs=fs, lengths=lengths),
           "estoi": lambda e, r, fs, lengths: compute_estoi(e, r, fs=fs, lengths=lengths)}


# the names score_list takes with interferers= only
BSS_METRICS = ("sir", "sar")


def score_list(estimates: Sequence[torch.Tensor], references: Sequence[torch.Tensor], metrics: Sequence[str] = ("sisdr", "estoi"),
               fs: int = 16000, max_batch: int = 64, interferers: Optional[Sequence[torch.Tensor]] = None) -> dict:
    """Score a folder of recordings at batch throughput.  ``estimates`` / ``references``: lists of 1-D float32 GPU tensors of any
    lengths; pair k is scored over the first ``min(len(estimates[k]), len(references[k]))`` samples of both, as ``EvalMetrics.eval``
    aligns them.  ``metrics``: names out of "sisdr", "sdr" (:func:`compute_sdr` with its 512-tap filter), "rmse", "stoi", "estoi".  The pairs are sorted by length, padded into batches
    of at most ``max_batch`` and scored with ``lengths=``; every value equals the per-utterance call's.  Returns
    ``{metric: CPU float32 tensor [N]}`` in the caller's order, with one copy to the host per metric at the end.

    ``interferers``: a third list, the reference of the other source of every pair (the noise of a ``(noisy, clean, noise)`` triple when
    speech is scored).  With it ``metrics`` also takes "sir" and "sar" (:func:`compute_bss` with its 512-tap filters; one call per
    batch serves both and "sdr"), and triple k is scored over the first samples all three of its signals have.  "sir" or "sar"
    without ``interferers`` raises ``ValueError``."""
    metrics = list(metrics)
    for m in metrics:
        if m in BSS_METRICS:
            if interferers is None:
                raise ValueError(f"metric {m!r} needs interferers=: the references of the other source")
        elif m not in METRICS:
            raise ValueError(f"metric {m!r}: expected one of {sorted(METRICS)}")
    if isinstance(fs, bool) or fs not in (10000, 16000):
        raise ValueError(f"fs = {fs!r}: STOI is defined here for 10000 and 16000 Hz input")
    if len(estimates) != len(references):
        raise ValueError(f"{len(estimates)} estimates for {len(references)} references")
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
        raise ValueError("score_list: max_batch must be a positive integer")
    if interferers is not None and len(interferers) != len(estimates):
        raise ValueError(f"{len(interferers)} interferers for {len(estimates)} estimates")
    named = (("estimates", estimates), ("references", references)) + ((("interferers", interferers),) if interferers is not None else ())
    for name, seq in named:
        for k, sgn in enumerate(seq):
            if not isinstance(sgn, torch.Tensor) or sgn.dim() != 1 or sgn.shape[0] < 1:
                raise ValueError(f"{name}[{k}] must be a non-empty 1-D tensor")
            ops.check_dev_f32(sgn, f"{name}[{k}]")
    N = len(estimates)
    lens = [min(int(a.shape[0]), int(b.shape[0])) for a, b in zip(estimates, references)]
    if interferers is not None:
        lens = [min(n, int(c.shape[0])) for n, c in zip(lens, interferers)]
    joint = any(m in BSS_METRICS for m in metrics)                          # then compute_bss gives "sdr" as well
    order = sorted(range(N), key=lambda k: (-lens[k], k))
    parts = {m: [] for m in metrics}
    for b0 in range(0, N, max_batch):
        batch = order[b0:b0 + max_batch]
        blens = [lens[k] for k in batch]
        dev = estimates[batch[0]].device
        pe = torch.zeros(len(batch), blens[0], dtype=torch.float32, device=dev)
        pr = torch.zeros(len(batch), blens[0], dtype=torch.float32, device=dev)
        for row, k in enumerate(batch):
            pe[row, :lens[k]] = estimates[k][:lens[k]]
            pr[row, :lens[k]] = references[k][:lens[k]]
        if joint:
            pv = torch.zeros(len(batch), blens[0], dtype=torch.float32, device=dev)
            for row, k in enumerate(batch):
                pv[row, :lens[k]] = interferers[k][:lens[k]]
            three = dict(zip(("sdr",) + BSS_METRICS, compute_bss(pe, pr, pv, lengths=blens)))
        for m in metrics:
            parts[m].append(three[m] if joint and m in three else METRICS[m](pe, pr, fs, blens))
    inv = torch.empty(N, dtype=torch.long)
    inv[torch.tensor(order, dtype=torch.long)] = torch.arange(N)
    out = {}
    for m in metrics:
        vals = torch.cat(parts[m]).cpu() if parts[m] else torch.empty(0, dtype=torch.float32)
        out[m] = vals[inv]
    return out


def resample(x: torch.Tensor, fs_in: int, fs_out: int = 16000, lengths=None):
    """Rational polyphase resampling on the device: x [B, L] (or [L]) at ``fs_in`` Hz -> ``(y [B, ceil(L * up / down)], out_lengths)``
    at ``fs_out`` Hz, up / down = fs_out / fs_in reduced.  The definition is ``scipy.signal.resample_poly(x, up, down)`` with its
    default filter (kaiser(5.0)-windowed sinc of 20 * max(up, down) + 1 taps; fp32 samples and taps, a double accumulator; DESIGN
    3.9) -- NOT ``librosa.resample``, whose default is soxr: parity with librosa itself is unpinned.  ``lengths`` (a python
    sequence or a CPU integer tensor): row b holds lengths[b] samples; nothing behind them is read, its result does not depend on the
    rest of the batch, and its ``out_lengths[b] = ceil(lengths[b] * up / down)`` samples are followed by zeros.  ``out_lengths`` is a
    list of ints.  ``fs_in == fs_out`` returns ``x`` itself.  Raises on the host, before any GPU work, for non-positive rates,
    max(up, down) > 640 after reduction and rows longer than 2^27 samples."""
    up, down = ops.resample_ratio(fs_in, fs_out)
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("resample: x must be a tensor [L] or [B, L]")
    single = x.dim() == 1
    xr = x.reshape(1, -1) if single else x
    B, L = xr.shape
    if L < 1 or L > ops.RESAMPLE_MAX_LEN:
        raise ValueError(f"resample: rows of {L} samples; 1 .. 2^27 are supported")
    host = [L] * B if lengths is None else ops.check_lengths(lengths, B, L, None)
    out_lens = [ops.resample_len(v, up, down) for v in host]
    ops.check_dev_f32(x, "x")
    if up == down:
        return x, out_lens
    lens = None if lengths is None else (lengths if isinstance(lengths, ops.Lengths) else ops.Lengths(host, x.device))
    y = ops.resample(xr, up, down, lens)
    return (y[0] if single else y), out_lens


def resample_list(signals: Sequence[torch.Tensor], fs_in, fs_out: int = 16000, max_batch: int = 64) -> List[torch.Tensor]:
    """Resample recordings of any lengths (and rates) at batch throughput.  ``signals``: 1-D float32 GPU tensors; ``fs_in``: an int
    or one int per signal.  The signals of one rate are sorted by length and padded into batches of at most ``max_batch``, the way
    :func:`score_list` batches; every result equals the per-signal :func:`resample` call bit for bit and comes back in the caller's
    order.  A signal already at ``fs_out`` is returned as it is (the same tensor)."""
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
        raise ValueError("resample_list: max_batch must be a positive integer")
    N = len(signals)
    rates = list(fs_in) if isinstance(fs_in, (list, tuple)) else [fs_in] * N
    if len(rates) != N:
        raise ValueError(f"{len(rates)} sampling rates for {N} signals")
    ratios = {fs: ops.resample_ratio(fs, fs_out) for fs in dict.fromkeys(rates)}
    for k, sgn in enumerate(signals):
        if not isinstance(sgn, torch.Tensor) or sgn.dim() != 1 or sgn.shape[0] < 1:
            raise ValueError(f"signals[{k}] must be a non-empty 1-D tensor")
        if sgn.shape[0] > ops.RESAMPLE_MAX_LEN:
            raise ValueError(f"signals[{k}]: {sgn.shape[0]} samples; at most 2^27 are supported")
    for k, sgn in enumerate(signals):
        ops.check_dev_f32(sgn, f"signals[{k}]")
    out: List[Optional[torch.Tensor]] = [None] * N
    for fs, (up, down) in ratios.items():
        idx = [k for k in range(N) if rates[k] == fs]
        if up == down:
            for k in idx:
                out[k] = signals[k]
            continue
        idx.sort(key=lambda k: (-int(signals[k].shape[0]), k))
        for b0 in range(0, len(idx), max_batch):
            batch = idx[b0:b0 + max_batch]
            blens = [int(signals[k].shape[0]) for k in batch]
            padded = torch.zeros(len(batch), blens[0], dtype=torch.float32, device=signals[batch[0]].device)
            for row, k in enumerate(batch):
                padded[row, :blens[row]] = signals[k]
            y = ops.resample(padded, up, down, ops.Lengths(blens, padded.device))
            for row, k in enumerate(batch):
                out[k] = y[row, :ops.resample_len(blens[row], up, down)].clone()
    return out


def trim(x: torch.Tensor, top_db: float = 30.0, lengths=None, frame_length: int = 2048, hop_length: int = 512, power: bool = False):
    """Cut the leading and trailing silence of every row on the device: x [B, L] (or [L]) -> ``(y, out_lengths, bounds)``.  The
    definition is ``librosa.effects.trim(x, top_db=top_db, frame_length=frame_length, hop_length=hop_length)`` of librosa 0.10 with
    ``ref=np.max`` restated (csrc/trim.hip; parity with the package itself is unpinned): the mean square of every centred,
    zero-padded frame in double, frames more than ``top_db`` dB below the loudest are silent, ``start = t0 * hop_length`` and ``end =
    min(n, (t1 + 1) * hop_length)`` from the first / last non-silent frame.  ``bounds`` is the list of ``(start, end)``,
    ``out_lengths`` the list of ``end - start`` and ``y [B, max(out_lengths)]`` (or ``[out_lengths[0]]``) holds ``x[b, start:end]``
    followed by zeros; ``[B, 0]`` if every row is trimmed to nothing.  A row of zeros comes back untrimmed.  ``lengths`` (a python
    sequence or a CPU integer tensor): row b holds lengths[b] samples; nothing behind them is read and its result does not depend on
    the rest of the batch.  ``power=True`` also returns the float64 frame powers ``[B, 1 + L // hop_length]`` (zeros behind a row's
    own ``1 + lengths[b] // hop_length``).  The bounds come to the host with one synchronisation.  Raises on the host, before any GPU
    work, for a bad ``top_db``, frame sizes other than ``hop_length % 4 == 0``, ``frame_length % (2 * hop_length) == 0`` and
    ``frame_length <= 64 * hop_length``, and rows longer than 2^27 samples."""
    top_db = ops.check_trim_args(top_db, frame_length, hop_length)
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("trim: x must be a tensor [L] or [B, L]")
    single = x.dim() == 1
    xr = x.reshape(1, -1) if single else x
    B, L = xr.shape
    if L < 1 or L > ops.TRIM_MAX_LEN:
        raise ValueError(f"trim: rows of {L} samples; 1 .. 2^27 are supported")
    if B < 1 or B > 65535:
        raise ValueError(f"trim: a batch of {B} rows; 1 .. 65535 are supported")
    host = None if lengths is None else ops.check_lengths(lengths, B, L, None)
    ops.check_dev_f32(x, "x")
    lens = None if host is None else (lengths if isinstance(lengths, ops.Lengths) else ops.Lengths(host, x.device))
    xr = ops._ragged_rows(xr)
    got = ops.trim_bounds(xr, top_db, frame_length, hop_length, lens, power)
    bounds_dev, P = got if power else (got, None)
    bounds = [(int(s), int(e)) for s, e in bounds_dev.tolist()]
    out_lens = [e - s for s, e in bounds]
    y = ops.trim_gather(xr, bounds_dev, max(out_lens))
    if single:
        y, P = y[0], (None if P is None else P[0])
    return (y, out_lens, bounds, P) if power else (y, out_lens, bounds)


def _trim_batches(lengths: Sequence[int], max_batch: int) -> List[List[int]]:
    """The batches of :func:`trim_list` (host only): indices sorted by length (descending, ties by index) in groups of ``max_batch``."""
    order = sorted(range(len(lengths)), key=lambda k: (-lengths[k], k))
    return [order[b0:b0 + max_batch] for b0 in range(0, len(order), max_batch)]


def _trim_pad(signals: Sequence[torch.Tensor], device) -> torch.Tensor:
    """The signals (1-D float32, host or device) as rows of one zero-padded device batch [B, len(signals[0])], the first one the
    longest.  The row pitch is a multiple of 4 samples, so every row starts on a 16-byte boundary."""
    n0 = int(signals[0].shape[0])
    padded = torch.zeros(len(signals), (n0 + 3) // 4 * 4, dtype=torch.float32, device=device)[:, :n0]
    for row, sgn in enumerate(signals):
        padded[row, :sgn.shape[0]].copy_(sgn, non_blocking=True)
    return padded


def _trim_list_run(signals, top_db, max_batch, frame_length, hop_length, gather: bool, who: str):
    """The guards and the batches :func:`trim_list` and :func:`trim_bounds_list` share -> [(indices, device bounds, gathered rows or
    None)], every launch queued and nothing fetched yet."""
    top_db = ops.check_trim_args(top_db, frame_length, hop_length)
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
        raise ValueError(f"{who}: max_batch must be a positive integer")
    for k, sgn in enumerate(signals):
        if not isinstance(sgn, torch.Tensor) or sgn.dim() != 1 or sgn.shape[0] < 1:
            raise ValueError(f"signals[{k}] must be a non-empty 1-D tensor")
        if sgn.shape[0] > ops.TRIM_MAX_LEN:
            raise ValueError(f"signals[{k}]: {sgn.shape[0]} samples; at most 2^27 are supported")
    for k, sgn in enumerate(signals):
        ops.check_dev_f32(sgn, f"signals[{k}]")
    pending = []
    for batch in _trim_batches([int(s.shape[0]) for s in signals], max_batch):
        blens = [int(signals[k].shape[0]) for k in batch]
        padded = _trim_pad([signals[k] for k in batch], signals[batch[0]].device)
        bdev = ops.trim_bounds(padded, top_db, frame_length, hop_length, ops.Lengths(blens, padded.device))
        # as wide as the longest input: the bounds need not come to the host in between
        pending.append((batch, bdev, ops.trim_gather(padded, bdev, blens[0]) if gather else None))
    return pending


def trim_list(signals: Sequence[torch.Tensor], top_db: float = 30.0, max_batch: int = 64, frame_length: int = 2048,
              hop_length: int = 512):
    """Trim recordings of any lengths at batch throughput.  ``signals``: 1-D float32 GPU tensors.  They are sorted by length and padded
    into batches of at most ``max_batch``, the way :func:`resample_list` batches -> ``(trimmed signals, bounds)`` in the caller's
    order, ``bounds`` a list of ``(start, end)``.  Every result equals the per-signal :func:`trim` call bit for bit."""
    out: List[Optional[torch.Tensor]] = [None] * len(signals)
    bounds: List[Optional[tuple]] = [None] * len(signals)
    for batch, bdev, y in _trim_list_run(signals, top_db, max_batch, frame_length, hop_length, True, "trim_list"):
        for row, (k, (s, e)) in enumerate(zip(batch, bdev.tolist())):
            bounds[k] = (int(s), int(e))
            out[k] = y[row, :e - s].clone()
    return out, bounds


def trim_bounds_list(signals: Sequence[torch.Tensor], top_db: float = 30.0, max_batch: int = 64, frame_length: int = 2048,
                     hop_length: int = 512) -> List[tuple]:
    """The ``bounds`` of :func:`trim_list` alone, with its batches and without the gather: what an index of segments needs."""
    bounds: List[Optional[tuple]] = [None] * len(signals)
    for batch, bdev, _ in _trim_list_run(signals, top_db, max_batch, frame_length, hop_length, False, "trim_bounds_list"):
        for k, (s, e) in zip(batch, bdev.tolist()):
            bounds[k] = (int(s), int(e))
    return bounds


def plan_ragged_batches(lengths: Sequence[int], hop: int, max_batch: int = 64, max_columns: int = 64 * 642,
                        max_waste: float = 0.1) -> List[List[int]]:
    """Group utterances of ``lengths`` samples into batches for the ``lengths=`` entry points (host only, no device use) ->
    list of batches, each a list of indices into ``lengths``; every index appears exactly once.

    Utterance b has T_b = 1 + lengths[b] // hop frames; a batch of B utterances is laid out as B * (Tmax + 1) columns, Tmax its
    longest.  Indices are sorted by length (descending, ties by index) and a batch is filled greedily; it is closed when adding
    the next utterance would exceed ``max_batch`` utterances, make B * (Tmax + 1) > ``max_columns`` (default: 64 utterances x 642
    columns, the headline launch shape) or push the padding share 1 - sum_b T_b / (B * Tmax) above ``max_waste``.  A single
    utterance longer than ``max_columns - 1`` frames gets a batch of its own."""
    if hop <= 0 or max_batch < 1 or max_columns < 2 or not 0 <= max_waste < 1:
        raise ValueError("plan_ragged_batches: need hop > 0, max_batch >= 1, max_columns >= 2, 0 <= max_waste < 1")
    lengths = [int(v) for v in lengths]
    if any(v < 0 for v in lengths):
        raise ValueError("plan_ragged_batches: negative length")
    order = sorted(range(len(lengths)), key=lambda k: (-lengths[k], k))
    batches: List[List[int]] = []
    cur: List[int] = []
    frames = tmax = 0
    for k in order:
        t = 1 + lengths[k] // hop
        if cur:                       # descending order: Tmax stays the first utterance's
            n = len(cur) + 1
            if n > max_batch or n * (tmax + 1) > max_columns or 1 - (frames + t) / (n * tmax) > max_waste:
                batches.append(cur)
                cur = []
        if not cur:
            frames, tmax = 0, t
        cur.append(k)
        frames += t
    if cur:
        batches.append(cur)
    return batches


@torch.no_grad()
def enhance_list(enhance: Callable, signals: Sequence[torch.Tensor], hop: int, check: bool = True, **plan_kw) -> List[torch.Tensor]:
    """Enhance utterances of any lengths at batch throughput.  ``signals``: 1-D float32 GPU tensors; ``enhance``: a callable
    ``enhance(padded [B, Lmax], lengths=[...], check=False) -> [B, hop*(Tmax-1)]`` -- ``functools.partial(enhance_supervised,
    model)``, ``functools.partial(enhance_vae, encoder, decoder)``, ... ; ``hop``: the model's hop length; ``plan_kw``: the
    knobs of :func:`plan_ragged_batches`.  Returns the enhanced signals in the caller's order, signal k exactly
    ``hop * (len(signals[k]) // hop)`` samples long.  One ``ops.coop_check()`` per batch when ``check``."""
    for k, sgn in enumerate(signals):
        if not isinstance(sgn, torch.Tensor) or sgn.dim() != 1:
            raise ValueError(f"signals[{k}] must be a 1-D tensor")
        ops.check_dev_f32(sgn, f"signals[{k}]")
    lens = [int(sgn.shape[0]) for sgn in signals]
    out: List[Optional[torch.Tensor]] = [None] * len(signals)
    for batch in plan_ragged_batches(lens, hop, **plan_kw):
        blens = [lens[k] for k in batch]
        padded = torch.zeros(len(batch), max(blens), dtype=torch.float32, device=signals[batch[0]].device)
        for row, k in enumerate(batch):
            padded[row, :lens[k]] = signals[k]
        y = _checked(enhance(padded, lengths=blens, check=False), check)
        for row, k in enumerate(batch):
            out[k] = y[row, :hop * (lens[k] // hop)].clone()
    return out


def compute_dnsmos(x: torch.Tensor, model, lengths=None, fs: int = 16000, p808=None) -> dict:
    """DNSMOS P.835 of a padded batch x [B, L] (or one recording [L]) without a clean reference: ``model`` is a
    :class:`dnsmos.DNSMOS`; -> ``{"OVRL_raw", "SIG_raw", "BAK_raw", "OVRL", "SIG", "BAK"}`` float64 device tensors [B] (scalars for
    [L]) and ``"num_hops"`` (int64, host), as :meth:`dnsmos.DNSMOS.score`.  The definition is the reference's
    ``DNSMOS/dnsmos_local.py`` restated (tests/dnsmos_ref.py): parity with onnxruntime itself is unpinned, ``fs !=
    16000`` goes through :func:`resample` (not ``librosa.resample``: unpinned).  ``p808`` (a :class:`dnsmos.P808`): also the
    script's ``"P808_MOS"`` column, float64 [B], over the same segments (tests/p808_ref.py; parity with librosa / onnxruntime
    unpinned); without it the result is that of the call without the argument."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("compute_dnsmos: x must be a tensor [L] or [B, L]")
    single = x.dim() == 1
    out = model.score(x.reshape(1, -1) if single else x, lengths, fs, p808=p808)
    return {k: v[0] for k, v in out.items()} if single else out


def dnsmos_list(signals: Sequence[torch.Tensor], model, fs: int = 16000, max_batch: int = 64, p808=None) -> dict:
    """DNSMOS P.835 of a folder of recordings of any lengths at batch throughput.  ``signals``: 1-D float32 GPU tensors.  They are
    sorted by length and padded into batches of at most ``max_batch``, the way :func:`score_list` batches; every value equals the
    per-recording :func:`compute_dnsmos` call's bit for bit.  Returns ``{name: CPU tensor [N]}`` in the caller's order (float64, and
    ``"num_hops"`` int64), with one copy to the host per batch at the end.  ``p808`` (a :class:`dnsmos.P808`): also ``"P808_MOS"``."""
    if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
        raise ValueError("dnsmos_list: max_batch must be a positive integer")
    for k, sgn in enumerate(signals):
        if not isinstance(sgn, torch.Tensor) or sgn.dim() != 1 or sgn.shape[0] < 1:
            raise ValueError(f"signals[{k}] must be a non-empty 1-D tensor")
        ops.check_dev_f32(sgn, f"signals[{k}]")
    N = len(signals)
    lens = [int(s.shape[0]) for s in signals]
    order = sorted(range(N), key=lambda k: (-lens[k], k))
    parts = []
    for b0 in range(0, N, max_batch):
        batch = order[b0:b0 + max_batch]
        blens = [lens[k] for k in batch]
        padded = _trim_pad([signals[k] for k in batch], signals[batch[0]].device)
        parts.append(model.score(padded, blens, fs, p808=p808))
    inv = torch.empty(N, dtype=torch.long)
    inv[torch.tensor(order, dtype=torch.long)] = torch.arange(N)
    out = {}
    for name in ("OVRL_raw", "SIG_raw", "BAK_raw", "OVRL", "SIG", "BAK", "num_hops") + (("P808_MOS",) if p808 is not None else ()):
        dt = torch.int64 if name == "num_hops" else torch.float64
        vals = torch.cat([part[name].cpu() for part in parts]) if parts else torch.empty(0, dtype=dt)
        out[name] = vals[inv]
    return out
