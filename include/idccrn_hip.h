/* libidccrn_hip.so -- C ABI of the MI355X (gfx950) I-DCCRN-VAE enhancement hot path.
 *
 * The reference (iris1997jiatong/I-DCCRN-VAE) is pure PyTorch and has no FFI of its own; each entry
 * point below replaces the stock torch operator(s) behind one reference function (file:line cited
 * per entry, paths relative to the reference root).  Conventions:
 *   - every pointer is a DEVICE pointer (hipMalloc / torch.cuda memory) unless it says "host";
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it, never allocate device memory,
 *     never synchronise and are re-entrant across streams.  The ONLY process state the library keeps belongs to the
 *     cooperative recurrences (idv_lstm_rec_pers / _pers_f32 / _coop_f32 / idv_lstm_stack2_f32, idv_lstm_bptt_coop / _stack2): per device, the
 *     CU count, an event that orders cooperative launches of different streams, and a 256-byte host-mapped status word
 *     (see idv_coop_last_status);
 *   - return value: 0 ok, -1 invalid argument, -2 launch failure, -3 (IDV_ECOOP) an EARLIER cooperative recurrence ran into
 *     its spin bound (its outputs are NaN-poisoned) and that has not been acknowledged yet (idv_coop_last_status); nothing throws;
 *   - activations use the planar-J layout  act[ri][C][F][Jp]  (fp32):
 *       column j = b*Tp + tp, Tp = T+1, tp = t+1, tp==0 and tp>t_valid are zero guard columns,
 *       Jp >= B*Tp is the row stride; buffers need IDV_SLACK floats of slack in front and behind.
 *     A reference tensor x[B,C,F,T,2] is act.view(2,C,F,B,Tp)[..., 1:].permute(3,1,2,4,0).
 */
#ifndef IDCCRN_HIP_H
#define IDCCRN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define IDV_ABI_VERSION 9
#define IDV_SLACK_FLOATS 256

int idv_abi_version(void);

/* Sticky status of the cooperative recurrences on the current device: -3 if one of them has run into its spin bound (a sibling
 * workgroup never became resident, e.g. on a CU-masked or shared GPU; its outputs were poisoned with NaN) since the status was
 * last cleared, else 0.  clear != 0 acknowledges and resets it.  The status is sticky like a device error: until it is
 * acknowledged EVERY cooperative entry of the device returns -3 without launching, so no unrelated caller can consume it.  The
 * operation that owns the time-out is the one whose stream was synchronised last: check after the synchronise (the Python
 * side does: ops.coop_check()).  The word is written by the device: synchronise the stream first for a definite answer. */
int idv_coop_last_status(int clear);
/* Workgroups a cooperative launch may use on the current device: multiProcessorCount minus 1/16 head room (240 on MI355X). */
int idv_coop_max_workgroups(void);

/* ---- weight preparation (device -> device, run once per parameter update) ------------------ */

/* K-chunk (in planar channels) the contraction kernel uses for `cin_used` complex input channels;
 * wfrag for a complex conv holds  roundup(2*Cout,128)/32 * roundup(2*cin_used, cck)*5 * 64 floats. */
int idv_cconv_cck(int cin_used);
/* Which cgemm_kernel instantiation idv_cconv2d_fwd launches for a layer shape: the template arguments
 * <MODE, WM, WN, MT_W, FO_T, JC_W, CCK> written as decimal digits (e.g. 1221324), -1 if unsupported; 1000001 = the
 * transposed conv with ONE output channel (last decoder block), which runs on the vector-ALU kernel of ctconv_c1_f32.hip.
 * Lets bench.py / profiles name the kernel a measured launch belongs to. */
int idv_cconv_config(int transposed, int cin_used, int Cout, int Fin);

/* ComplexBatchNormal statistics -> affine: model/complex_progress.py:168-209 (cbn).
 * moments: [5][C] = mean_r, mean_i, Vrr, Vri, Vii (Vrr/Vii already carry +1e-5, as the reference's
 * running buffers do).  fold[C][6] = Zrr,Zri,Zir,Zii, sr, si with  y = Z*x + s. */
int idv_cbn_fold(const float* moments, const float* gamma_rr, const float* gamma_ri, const float* gamma_ii,
                 const float* beta_r, const float* beta_i, int C, float* fold, void* stream);

/* Pack ComplexConv2d / causal_complex_conv2d weights (complex_progress.py:8-36; w_*: [Cout,Cin,5,2])
 * or (Causal)ComplexConvTranspose2d weights (:222-279; w_*: [Cin,Cout,5,2], transposed=1) into the
 * MFMA fragment order of the block matrix [[Wr,-Wi],[Wi,Wr]]; biases become (b_re-b_im, b_re+b_im)
 * (:16-18,:32-34).  fold (or NULL) is applied on the output side (eval-mode BN folded into the conv). */
int idv_pack_cconv(const float* w_re, const float* w_im, const float* b_re, const float* b_im, const float* fold,
                   int Cout, int Cin_total, int Cin_used, int transposed, float* wfrag, float* bias_out, void* stream);

/* Pack a row-major real matrix w[M][K] (+ bias[M] or NULL) for idv_pw_gemm;
 * wfrag holds roundup(M,128)/32 * roundup(K,8)/2 * 64 floats, bias_out roundup(M,128). */
int idv_pack_pw(const float* w, const float* bias, int M, int K, float* wfrag, float* bias_out, void* stream);

/* nn.LSTM input weights of ComplexLSTM (complex_progress.py:45-48): rows of the packed matrix are
 * [lstm_re gates | lstm_im gates], gate columns re-ordered for the recurrent kernel, bias = b_ih + b_hh.
 * w_ih_*: [4H][K].  Same sizes as idv_pack_pw with M = 8H. */
int idv_pack_lstm_ih(const float* w_ih_re, const float* b_ih_re, const float* b_hh_re, const float* w_ih_im,
                     const float* b_ih_im, const float* b_hh_im, int H, int K, float* wfrag, float* bias_out,
                     void* stream);
/* Recurrent weights w_hh_*: [4H][H] -> fragment order of the recurrent kernels: 2*4H*H floats of fp32 fragments
 * followed by the same number of bytes of split-bf16 (hi, lo) fragments; whh_frag holds 4*4H*H floats. */
int idv_pack_lstm_hh(const float* w_hh_re, const float* w_hh_im, int H, float* whh_frag, void* stream);

/* Windowed DFT / inverse-DFT matrices of torch.stft / torch.istft as used by STFT.forward /
 * ISTFT.forward (model/pvae_module.py:21-27, :38-42): hann(win) centred in n_fft, onesided.
 * w_fwd: [2F][win] row-major, w_inv: [win][2F] row-major, F = n_fft/2+1; env_inv: [n_fft + hop*(T-1)]
 * = 1 / overlap-added squared window (0 where the envelope is 0). */
int idv_make_dft(int n_fft, int win, int hop, int T, float* w_fwd, float* w_inv, float* env_inv, void* stream);

/* ---- forward operators ---------------------------------------------------------------------- */

/* ComplexConv2d.forward / causal_complex_conv2d.forward (complex_progress.py:16-22, :32-36) and
 * (causal_)ComplexConvTranspose2d.forward (:244-250, :275-279), kernel (5,2), stride (2,1), freq
 * padding 2; fused with torch.cat([p, skip], 1) of standard_DCCRN.forward (pvae_module.py:195;
 * x1 = skip, x1_div = num_samples for the repeated skips of pvae_module.py:2563-2567), with the
 * folded eval BatchNorm and PReLU (pvae_module.py:64-68, :88-93) when prelu_slope != NULL, and with
 * the train-mode moment sums (complex_progress.py:132-143) when stats != NULL (stats: [Cout][5]
 * doubles, zeroed by the caller: sum r, i, r*r, i*i, r*i over kept positions).  stats_work (or NULL) / stats_rep:
 * [stats_rep][Cout][5] zeroed doubles, stats_rep a power of two >= 2: the epilogue's atomic adds are spread over that many
 * replicas (chosen by workgroup) and folded into stats afterwards -- at 32 / 64 channels and ~10^4 workgroups the same-address
 * atomics otherwise cost more than the contraction (first encoder blocks, B = 32: 4.1 ms against 1.65).
 * tshift: -1 causal conv (taps x[t-1], x[t]) / any transposed conv of the model (taps x[t], x[t-1]); 0 non-causal conv
 * (taps x[t], x[t+1]); a transposed conv with tshift 0 reads (x[t+1], x[t]) -- with conjugate-transposed weights the
 * adjoint (data gradient) of the causal conv, as the non-causal conv is of the transposed conv (tests:
 * test_conv_adjoint_identity).  t_valid_out: frames kept. */
int idv_cconv2d_fwd(const float* x0, int C0, const float* x1, int C1, int Jp1, int x1_div, const float* wfrag,
                    const float* bias, const float* prelu_slope, float* out, double* stats, double* stats_work, int stats_rep,
                    int transposed, int tshift, int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out, void* stream);

/* idv_cconv2d_fwd with THREE real products per complex product (Gauss: t1 = Wr (xr + xi), t2 = (Wi - Wr) xr,
 * t3 = (Wr + Wi) xi; re = t1 - t3, im = t1 + t2 -- cgemm_gauss.hip), exact fp32 MFMA: the same reference lines
 * (model/complex_progress.py:16-22, :32-36, :244-250, :275-279), 25 % fewer multiplications than the reference's four real
 * convolutions.  idv_cconv_gauss_supported(C0, C1, Cout): >= 2 complex input channels, > 1 output channel, and with a second
 * source C0 even; callers use idv_cconv2d_fwd otherwise (the one-channel ends of the network).  idv_pack_cconv_gauss: weight
 * layouts as idv_pack_cconv; wfrag: idv_cconv_gauss_wfrag_floats(Cout, Cin_used) floats; epi: idv_cconv_gauss_epi_rows(Cout)
 * x 8 floats per output channel (Zrr, Zri, Zir, Zii, (Z b + s)_r, (Z b + s)_i, 0, 0) with b = (b_re - b_im, b_re + b_im) --
 * eval-mode ComplexBatchNormal (fold, complex_progress.py:161-209) is a real 2x2 map, so it cannot be folded into the three
 * weight planes and is applied by the epilogue when has_fold != 0 (then PReLU, pvae_module.py:58,82).  conj != 0 packs the
 * adjoint (data-gradient) operator: W_i negated, the caller passes the swapped channel roles as for idv_pack_cconv_adjoint.
 * addend (or NULL): planar [2][Cout][Fout][addend_Jp] holding B / addend_div utterances, added to the contraction
 * before bias / BN / PReLU: output utterance b takes addend utterance b / addend_div.  The convolution is linear in its input
 * channels, so for the repeated skips of pvae_module.py:2563-2567 the skip half is computed ONCE per utterance (a call with
 * x0 = skip, the skip rows of the weight, no bias) and added to each of its num_samples latent halves.
 * idv_cconv_gauss_config: the kernel instantiation as digits 3 MODE WM WN FO_T JC_W OCC (profiles; Cin = C0 + C1). */
int idv_cconv_gauss_supported(int C0, int C1, int Cout);
long long idv_cconv_gauss_wfrag_floats(int Cout, int cin_used);
int idv_cconv_gauss_epi_rows(int Cout);
int idv_cconv_gauss_config(int transposed, int Cin, int Cout, int Fin);
int idv_pack_cconv_gauss(const float* w_re, const float* w_im, const float* b_re, const float* b_im, const float* fold, int Cout,
                         int Cin_total, int Cin_used, int transposed, int conj, float* wfrag, float* epi, void* stream);
int idv_cconv2d_gauss_fwd(const float* x0, int C0, const float* x1, int C1, int Jp1, int x1_div, const float* wfrag,
                          const float* epi, int has_fold, const float* prelu_slope, float* out, double* stats, double* stats_work,
                          int stats_rep, int transposed, int tshift, int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out,
                          const float* addend, int addend_div, int addend_Jp, void* stream);

/* Split-precision variant of idv_cconv2d_fwd (same reference lines): operands split into two bf16 (x = hi + lo),
 * w*x ~= w_hi*x_hi + w_hi*x_lo + w_lo*x_hi accumulated in fp32 on the bf16 MFMA (relative error ~2^-16 per
 * product; waveform parity vs the fp32 path ~1e-5, north_star tolerance 1e-3).  Needs C0 % 8 == 0, C1 % 8 == 0,
 * x1_div == 1, Cout >= 32, 16-byte aligned rows (idv_cconv_bf16_supported); callers fall back to
 * idv_cconv2d_fwd otherwise.  wfrag_bf16: idv_pack_cconv_bf16 (idv_cconv_bf16_wfrag_bytes bytes);
 * bias: the fp32 bias vector produced by idv_pack_cconv. */
long long idv_cconv_bf16_wfrag_bytes(int Cout, int cin_used);
int idv_cconv_bf16_supported(int transposed, int C0, int C1, int x1_div, int Cout);
int idv_cconv_bf16_config(int transposed, int Cout, int Fin);   /* <MODE, WM, WN, FO_T, JC_W, MT_W> as digits, for profiles */
int idv_pack_cconv_bf16(const float* w_re, const float* w_im, const float* fold, int Cout, int Cin_total, int Cin_used,
                        int transposed, void* wfrag, void* stream);
int idv_cconv2d_bf16x3_fwd(const float* x0, int C0, const float* x1, int C1, int Jp1, int x1_div, const void* wfrag_bf16,
                           const float* bias, const float* prelu_slope, float* out, double* stats, double* stats_work,
                           int stats_rep, int transposed, int tshift, int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out,
                           void* stream);   /* stats_work / stats_rep: as idv_cconv2d_fwd */

/* Split image: the inter-layer activation format of the bf16x3 path (eval mode).  bf16 elements,
 *   image[hi|lo][octet o][F][Jp][8],  element e of octet o = planar channel cc = 8*o + e = 2*ci + ri,
 * hi = value truncated to bf16, lo = round-to-nearest bf16 of the remainder (hi + lo reproduces the fp32 value to
 * ~2^-17, exactly the operand split idv_cconv2d_bf16x3_fwd applies while staging, so both entries give identical
 * results).  The lo plane starts lo_off elements (idv_cconv2d_img_fwd sources: 16-byte slots) after the hi plane;
 * callers keep >= 256 readable and writable bytes before each plane (every producer zeroes the 16-byte slot
 * 128 bytes before each plane; consumers read it for out-of-range frequency rows) and 4 KiB after them.
 * idv_cconv2d_img_fwd: same contraction, folded BN and PReLU epilogue as idv_cconv2d_bf16x3_fwd (reference
 * model/complex_progress.py:16-22, :244-250; pvae_module.py:64-68, :88-93) with image sources, writing planar fp32
 * (out_planar), an image (out_img) or both. */
int idv_cconv2d_fwd_img(const float* x0, int C0, const float* x1, int C1, int Jp1, const float* wfrag, const float* bias,
                        const float* prelu_slope, float* out_planar, void* out_img, long long out_lo_off_elems,
                        int transposed, int tshift, int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out,
                        void* stream);   /* exact-fp32 idv_cconv2d_fwd (eval, x1_div 1) writing planar and/or image */
/* training forward from split images (bf16x3 training mode): planar fp32 y + the per-channel moments, as idv_cconv2d_fwd with
 * `stats`; sources as idv_cconv2d_img_fwd with src_is_image = 1 */
int idv_cconv2d_img_train_fwd(const void* x0_img, long long lo_off0, int C0, const void* x1_img, long long lo_off1, int C1,
                              const void* wfrag_bf16, const float* bias, float* out_planar, double* stats, double* stats_work,
                              int stats_rep, int transposed, int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out, void* stream);
int idv_cconv_img_config(int src_is_image, int transposed, int Cin, int Cout, int Fin);   /* template digits <MODE, WM, WN,
                        FO_T, JC_W, MT_W, IMGIN, AD> of the cgemm_bf16_kernel idv_cconv2d_img_fwd launches (profiles) */
int idv_planar_to_image(const float* x, int C, int F, int J, int Jp, void* img, long long lo_off_elems, void* stream);
/* the same with every utterance repeated rep times in a row (skip.repeat_interleave(num_samples, 0) of the two-phase decoder,
 * pvae_module.py:2563-2567, fused into the conversion): x has B utterances (pitch Jp_in), the image B * rep (pitch Jp) */
int idv_planar_to_image_repeat(const float* x, int C, int F, int B, int Tp, int Jp_in, int rep, void* img, long long lo_off_elems,
                               int Jp, void* stream);
int idv_image_to_planar(const void* img, long long lo_off_elems, int C, int F, int J, int Jp, float* x, void* stream);
int idv_cconv2d_img_fwd(int src_is_image /* 0: x0/x1 are planar fp32 (row stride Jp) */, const void* x0_img, long long lo_off0_slots, int C0, const void* x1_img, long long lo_off1_slots,
                        int C1, const void* wfrag_bf16, const float* bias, const float* prelu_slope, float* out_planar,
                        void* out_img, long long out_lo_off_elems, int transposed, int tshift,
                        int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out, void* stream);

/* Last decoder block (Cout = 1): transposed conv re-associated so that the five frequency taps sit in the MFMA
 * M dimension (10 rows instead of 2), taps combined in the epilogue; split-bf16 arithmetic, eval mode only
 * (folded BN + PReLU; train-mode statistics use idv_cconv2d_fwd).  Same reference lines as idv_cconv2d_fwd.
 * Needs C0 % 8 == 0, C1 % 8 == 0, no repeated skips.  bias: bias_out of idv_pack_cconv (2 values used). */
long long idv_ctconv_c1_wfrag_bytes(int cin_used);
int idv_pack_ctconv_c1_bf16(const float* w_re, const float* w_im, const float* fold, int Cin_total, int Cin_used,
                            void* wfrag, void* stream);
int idv_ctconv_c1_bf16x3_fwd(const float* x0, int C0, const float* x1, int C1, int Jp1, const void* wfrag,
                             const float* bias, const float* prelu_slope, float* out, int Fin, int B, int Tp, int Jp,
                             int t_valid_out, void* stream);
int idv_ctconv_c1_img_fwd(const void* x0_img, long long lo_off0_slots, int C0, const void* x1_img, long long lo_off1_slots,
                          int C1, const void* wfrag, const float* bias, const float* prelu_slope, float* out, int Fin, int B,
                          int Tp, int Jp, int t_valid_out, void* stream);   /* same block, split-image sources */

/* out[m][j] = bias[m] + sum_k w[m][k] x[k][j] over K planes of stride Jp: ComplexDense.forward
 * (complex_progress.py:83-89, one call per real/imag linear), the LSTM input projections, and the
 * DFT / inverse DFT.  swap=1 writes out[((tp-1)*B + b)*ldo + m] instead of planar rows.
 * Refused (-1) before any GPU work: K odd, Tp <= 1, t_valid < 1, Jp < B*Tp, and swap != 0 with ldo < M (rows of the
 * row-major store would overlap). */
int idv_pw_gemm(const float* x, int K, const float* wfrag, const float* bias, const float* prelu_slope, float* out,
                int M, int B, int Tp, int Jp, int t_valid, int swap, int ldo, void* stream);
/* Which kernel form idv_pw_gemm launches for (M, swap, Jp, x), decided on the host by the function the launch itself
 * calls: the decimal digits <WM><WN><swap><vec> -- WM x WN waves per workgroup (22: 2 x 2 waves, 128-column tiles; 41:
 * 4 x 1 waves, 64-column tiles, taken where ((M+31)/32) % 8 == 0), the store (0 planar, 1 row-major) and the staging
 * (1: float4, needs Jp % 4 == 0 and x 16-byte aligned; 0: scalar).  E.g. 2201, 4110.  x is only looked at as an
 * address.  -1 for M <= 0 or Jp <= 0. */
int idv_pw_gemm_form(int M, int swap, int Jp, const float* x);

/* Train-mode ComplexBatchNormal (complex_progress.py:131-160): sums -> moments[5][C] (mean_r, mean_i,
 * Vrr+eps, Vri, Vii+eps), running buffers updated in place (first call copies, later 0.9/0.1 blend),
 * fold[C][6] for idv_cbn_apply_prelu. count = B*F*T > 0.  momentum weighs the OLD running value (old*momentum + new*(1 -
 * momentum)).  moments may be NULL; the five running pointers are given together or running_mean_r is NULL (then no running
 * buffer is touched), one without the others is -1. */
int idv_cbn_finalize(const double* stats, double count, const float* gamma_rr, const float* gamma_ri,
                     const float* gamma_ii, const float* beta_r, const float* beta_i, int C, int first_call,
                     float momentum, float* running_mean_r, float* running_mean_i, float* Vrr, float* Vri,
                     float* Vii, float* moments, float* fold, void* stream);
/* Moment sums of a planar activation (stand-alone ComplexBatchNormal.forward, complex_progress.py:131-143);
 * stats [C][5] doubles, zeroed by the caller (the sums are ADDED to what stats holds); same layout as the conv epilogue's: sum r, i,
 * r*r, i*i, r*i over the kept columns 1 <= tp <= t_valid.  Geometry: t_valid >= 1, Tp >= t_valid + 1, Jp >= B*Tp, else -1. */
int idv_cbn_stats(const float* act, int C, int F, int B, int Tp, int Jp, int t_valid, double* stats, void* stream);
/* y = PReLU(Z*x + s) in place on the kept columns of a planar activation (u >= 0 is the positive branch; prelu_slope NULL: no
 * activation); guard columns, pitch columns [B*Tp, Jp) and everything else are neither read nor written, so zero guard columns
 * stay zero.  Geometry: t_valid >= 1, Tp >= t_valid + 1, Jp >= B*Tp, else -1 and nothing is written. */
int idv_cbn_apply_prelu(float* act, const float* fold, const float* prelu_slope, int C, int F, int B, int Tp, int Jp,
                        int t_valid, void* stream);

/* STFT.forward (pvae_module.py:21-27): x[B][L] -> frames[win][Jp] (reflect-padded, centred frames, guard columns tp == 0
 * and tp > T zeroed); the DFT itself is idv_pw_gemm with the idv_make_dft matrix.  L > n_fft/2, T == 1 + L/hop, Tp >= T+1,
 * Jp >= B*Tp. */
int idv_stft_frames(const float* x, int B, int L, int n_fft, int win, int hop, int T, float* frames, int Tp, int Jp,
                    void* stream);
/* ISTFT.forward (pvae_module.py:38-42) tail: overlap-add of windowed inverse-DFT frames
 * frames[win][Jp] / envelope, trimmed to y[B][hop*(T-1)].  T >= 2, Tp >= T+1, Jp >= B*Tp. */
int idv_istft_ola(const float* frames, const float* env_inv, int B, int n_fft, int win, int hop, int T, int Tp,
                  int Jp, float* y, void* stream);

/* Mask branch of DCCRN_.forward (pvae_module.py:224-234) / decoder_twophase (:2594-2608):
 * predict = |X| tanh|M| exp(j(angle X + angle M)).  mask, X: planar [2][F][Jp] (X utterance b/x_div);
 * writes planar `pred` (guard columns tp == 0 and tp > T zeroed) and the interleaved complex64 API tensor pred_c[B][F][T][2]
 * (may be NULL).  x_div >= 1, Tp >= T+1, Jp >= B*Tp, JpX >= ceil(B/x_div)*Tp. */
int idv_mask_apply(const float* mask, const float* X, int x_div, int JpX, float* pred, float* pred_c, int F, int B,
                   int T, int Tp, int Jp, void* stream);
/* Optional data normalisation of DCCRN_.forward (pvae_module.py:217-221 / :235-238; data_mean, data_std: [F][2] from
 * dataset/mean_*_spksplit.txt): out = (X - mean) / (std + 1e-6) with the imaginary part of bins 0 and F-1 zeroed, and the
 * inverse std * P + mean written planar (out) and interleaved [B][F][T][2] (out_c).  Eval path.  These two, their gradients and
 * idv_outtype_estimate write the valid columns of their planar output and zero its guard columns tp == 0 and tp > T; the
 * pitch columns [B*Tp, Jp) are not touched.  Tp >= T+1, Jp >= B*Tp. */
int idv_datanorm(const float* X, const float* mean, const float* stdv, int F, int B, int T, int Tp, int Jp, float* out, void* stream);
int idv_datadenorm(const float* P, const float* mean, const float* stdv, int F, int B, int T, int Tp, int Jp, float* out,
                   float* out_c, void* stream);
/* gradients of the two (training with the reference's --data_norm): dX = dout / (std + 1e-6) with no gradient for the imaginary
 * parts of the first and last bin; dP = std * (dout + dout_c), either gradient may be NULL. */
int idv_datanorm_bwd(const float* dout, const float* stdv, int F, int B, int T, int Tp, int Jp, float* dX, void* stream);
int idv_datadenorm_bwd(const float* dout, const float* dout_c, const float* stdv, int F, int B, int T, int Tp, int Jp, float* dP,
                       void* stream);
/* Two-latent enhancement estimators of the evaluation script (i_dccrn_vae/nsvae_dccrn/test_se_cvaefinetune.py:
 * real_and_imag_mask :85-101, complex_mask :104-116, phase_sensitive_mask :119-135, applied at :283-305): S / N = mean over the
 * ns sampled speech / noise spectra of an utterance, X = its noisy spectrum.  mode 0: per-part Wiener-like masks
 * (Sr^2 / (Sr^2 + Nr^2 + 1e-10)) Xr, same for the imaginary part; 1: S / (S + N + 1e-10) * X; 2: |S| / (|S| + |N| + 1e-10) *
 * cos(angle S - angle X) * |X| * exp(j angle S).  speech_c / noise_c: interleaved complex [B*ns][F][T][2] (the decoders'
 * `predict`); X: [B][F][T][2] with element strides (sb, sf, st, sr); out: planar [2][F][Jp] (feeds the ISTFT), out_c or NULL:
 * interleaved complex [B][F][T][2]. */
int idv_outtype_estimate(const float* speech_c, const float* noise_c, const float* X, long long sb, long long sf, long long st,
                         long long sr, int mode, int ns, int B, int F, int T, int Tp, int Jp, float* out, float* out_c,
                         void* stream);
/* planar [2][F][Jp] -> interleaved [B][F][T][2] (recon_type 'real_imag', pvae_module.py:245-253).  Tp >= T+1, Jp >= B*Tp. */
int idv_planar_to_complex(const float* act, float* out_c, int F, int B, int T, int Tp, int Jp, void* stream);

/* ComplexLSTM.forward (complex_progress.py:50-74): four 2-layer LSTM passes, real = rr - ii,
 * imag = ir + ri.  x: planar [2][K][Jp]; out: planar [2][H][Jp].  flags bit 0: split-bf16 recurrence (H = 128).  wihN / bihN: idv_pack_lstm_ih of layer
 * N, whhN: idv_pack_lstm_hh of layer N.  work: idv_clstm_work_floats(H, B, T, Jp) floats. */
long long idv_clstm_work_floats(int H, int B, int T, int Jp);   /* 24*T*B*H + 4*B*H + scratch(H, B, Jp) + 4*H*Jp */
/* Persistent cooperative recurrence of one layer for H = 384 / 768 (the VAE encoders' 3*zdim / 6*zdim, reference
 * model/pvae_module.py:1819, :2160-2163), split-bf16 arithmetic: H/16 co-resident workgroups per weight set keep their
 * W_hh slice in registers for all T steps and exchange h_t through global memory (write-through stores, one arrive
 * counter per group of workgroups, no cache-wide fences; bounded spins; on a time-out the outputs are NaN).  idv_clstm_fwd
 * uses it when flags bit 0 is set and idv_lstm_pers_supported; flags bit 3 forces the per-step kernel.  g / g_run_z /
 * g_run_s / ldg address the gate pre-activations as G0 / G1 below, whh_frag: idv_pack_lstm_hh, work:
 * idv_lstm_pers_work_bytes(H, B) bytes, 16-byte aligned.  Outputs (at least one): hout [4 runs][T*B][H] fp32; kimg, the
 * K-major split image of h (slot ((run * H/8 + octet) * Jp + b*Tp + t + 1), lo plane kimg_lo_slots 16-byte slots behind
 * the hi plane) that idv_lstm_proj1_bf16x3 consumes. */
int idv_lstm_pers_supported(int H, int B);
long long idv_lstm_pers_work_bytes(int H, int B);
int idv_lstm_rec_pers(const float* g, long long g_run_z, long long g_run_s, int ldg, const float* whh_frag, float* hout, int H,
                      int B, int T, void* work, void* kimg, long long kimg_lo_slots, int Tp, int Jp, float* gsave, float* csave,
                      void* stream);   /* gsave (== g) / csave: training forward, layouts of idv_clstm_fwd flags bit 2; or NULL */
/* Layer-1 input projection (nn.LSTM weight_ih_l1 of lstm_re / lstm_im, complex_progress.py:50-74) in split-bf16 from that
 * image: G1[run = 2z + s][(t, b)][4H].  wfrag_bf16: idv_pack_lstm_ih_bf16(w_ih_l1 re, im, H, K = H); bias: bih1 of
 * idv_pack_lstm_ih.  Needs 4H % 256 == 0 and H % 64 == 0. */
int idv_lstm_proj1_bf16x3(const void* himg, long long lo_off_slots, const void* wfrag_bf16, const float* bias, float* G1, int H,
                          int B, int T, int Tp, int Jp, void* stream);
/* The H = 128 recurrence (DCCRN-CL bottleneck) in exact fp32 on FOUR CUs per (run, 16-sequence tile) with the same hand-off
 * (lstm_coop_f32.hip): idv_clstm_fwd uses it in fp32 mode when idv_lstm_coop_f32_supported (H == 128, 16 * ceil(B/16) <= 240
 * workgroups; IDV_LSTM_COOP_F32=0 or flags bit 3 keep the one-CU register-resident kernel).  hout required; gsave (== g) /
 * csave as above; work: idv_lstm_coop_f32_work_bytes(H, B) bytes, 16-byte aligned. */
int idv_lstm_coop_f32_supported(int H, int B);
long long idv_lstm_coop_f32_work_bytes(int H, int B);
int idv_lstm_rec_coop_f32(const float* g, long long g_run_z, long long g_run_s, int ldg, const float* whh_frag, float* hout, int H,
                          int B, int T, void* work, float* gsave, float* csave, void* stream);
/* The same persistent cooperative recurrence in EXACT fp32 (lstm_pers_f32.hip; reference model/complex_progress.py:50-74 at the
 * hidden sizes of model/pvae_module.py:1819, :2160-2163): W_hh slices as fp32 in registers, v_mfma_f32_16x16x4_f32, h exchanged
 * as fp32 16-byte sc1 granules.  idv_clstm_fwd uses it in fp32 mode for H = 384 / 768 when idv_lstm_pers_f32_supported
 * (IDV_LSTM_PERS_F32=0 or flags bit 3 keep the per-step kernel).  Arguments as idv_lstm_rec_coop_f32. */
int idv_lstm_pers_f32_supported(int H, int B);
long long idv_lstm_pers_f32_work_bytes(int H, int B);
int idv_lstm_rec_pers_f32(const float* g, long long g_run_z, long long g_run_s, int ldg, const float* whh_frag, float* hout, int H,
                          int B, int T, void* work, float* gsave, float* csave, void* stream);
/* diagnostic (not part of the drop-in boundary): while a device buffer of 256 x 8 counters is registered, idv_lstm_rec_pers runs
 * an instrumented twin in which every workgroup accumulates core-clock cycles per phase (spin, -, barrier, loads + MFMA,
 * reduce + cell, drain + barrier, -, XCC id); NULL restores the production kernel.  tests/tools/lstm_phase_probe.py */
void idv_lstm_pers_set_profile(unsigned long long* prof_cycles);
/* flags bit 2 (training forward; with bit 0 only where idv_lstm_pers_supported, else EINVAL: exact-fp32 recurrence): the activated gates (i, f, g, o) and the cell states are kept
 * for idv_lstm_bptt.  work then holds idv_clstm_train_work_floats floats, laid out (TBH = T*B*H)
 *   [G0 16 TBH | G1 16 TBH | h0 4 TBH | h1 4 TBH | c0 4 TBH | c1 4 TBH | scratch]
 * G0: [z][T*B][8H] (z = real / imag input; columns [weight set s][4H]), G1: [run = 2z+s][T*B][4H], h/c: [run][T*B][H];
 * gate columns are ordered colp = ((u/16)*4 + gate)*16 + u%16. */
long long idv_clstm_train_work_floats(int H, int B, int T, int Jp);   /* 48*T*B*H + 4*B*H + scratch(H, B, Jp) + 4*H*Jp */
/* wih1_bf16 (may be NULL): idv_pack_lstm_ih_bf16 of layer 1; with it, flags bit 0 and the persistent recurrence, layer 0
 * hands h0 to the layer-1 projection as a split image (idv_lstm_proj1_bf16x3) instead of fp32 rows. */
int idv_clstm_fwd(const float* x, int K, const float* wih0, const float* bih0, const float* whh0, const float* wih1,
                  const float* bih1, const float* whh1, int H, int B, int T, int Tp, int Jp, float* work, float* out,
                  int flags, const void* wih1_bf16, void* stream);

/* Both layers of the H = 128 complex LSTM (reference ComplexLSTM.forward, model/complex_progress.py:50-74: nn.LSTM(num_layers = 2))
 * in ONE cooperative launch, exact fp32 (lstm_stack2_f32.hip): layer 1 runs one step behind layer 0 on its own four
 * CUs per (run, 16-sequence tile) and computes W_ih h0[t+1] in the hand-off latency of its own step t, so the hoisted layer-1
 * projection GEMM and the second recurrence launch disappear.  wih1_hh: idv_pack_lstm_hh applied to weight_ih_l1 (re, im) --
 * [4H][H] like W_hh; bias1: bih of idv_pack_lstm_ih for layer 1 ([2 sets][4H], gate-column order); h0, hout: [4 runs][T*B][H];
 * work: idv_lstm_stack2_f32_work_bytes bytes, 16-byte aligned; gsave1 ([run][T*B][4H]) / csave0 / csave1 ([4 runs][T*B][H]):
 * training forward (all three; layer 0's activated gates replace g in place -- the buffers idv_lstm_bptt reads) or all NULL.
 * Supported: H == 128 and 32 * ceil(B/16) <= idv_coop_max_workgroups() (IDV_LSTM_STACK2=0 turns it off).
 * idv_clstm_fwd2 = idv_clstm_fwd + wih1_hh (may be NULL): takes this path in fp32 mode (evaluation and flags bit 2) where
 * supported, idv_clstm_fwd's otherwise. */
int idv_lstm_stack2_f32_supported(int H, int B);
long long idv_lstm_stack2_f32_work_bytes(int H, int B);
int idv_lstm_stack2_f32(const float* g, long long g_run_z, long long g_run_s, int ldg, const float* whh0, const float* wih1_hh,
                        const float* whh1, const float* bias1, float* h0, float* hout, int H, int B, int T, void* work,
                        float* gsave1, float* csave0, float* csave1, void* stream);
int idv_clstm_fwd2(const float* x, int K, const float* wih0, const float* bih0, const float* whh0, const float* wih1,
                   const float* bih1, const float* whh1, const float* wih1_hh, int H, int B, int T, int Tp, int Jp, float* work,
                   float* out, int flags, const void* wih1_bf16, void* stream);

/* The layer-0 input projection INSIDE that cooperative launch (lstm_stack2_f32.hip, lstm_proj_split.hpp): producer workgroups
 * on the CUs the recurrence leaves empty compute G = W_ih0 x + b in time chunks of 16 steps, after an opening phase in which
 * every workgroup of the launch computes the first c0 chunks; G, the saved buffers and the output have the bits of idv_pw_gemm +
 * idv_lstm_stack2_f32.  idv_lstm_stack2_f32_proj_split: 1 where this form is taken (there is room for producers and T is longer
 * than the opening phase; IDV_LSTM_PROJ_OVERLAP=0 turns it off), *c0 / *P (may be NULL): the opening chunks and the producer
 * count; force_c0: -1 automatic, tests: the opening phase, clamped to the chunk count.  x, wih0, bih0: as idv_clstm_fwd;
 * g: [2 parts][T*B][8H]; work: idv_lstm_stack2_f32_proj_work_bytes(H, B, Tmax >= T) bytes; the rest as idv_lstm_stack2_f32.
 * idv_clstm_fwd2 takes this form where the split says 1 unless flags bit 4 (value 16) keeps the projection hoisted;
 * idv_clstm_fwd3 = idv_clstm_fwd2 + proj_c0 (= force_c0). */
int idv_lstm_stack2_f32_proj_split(int H, int B, int T, int K, int force_c0, int* c0, int* P);
long long idv_lstm_stack2_f32_proj_work_bytes(int H, int B, int Tmax);
int idv_lstm_stack2_f32_proj(const float* x, int K, int Tp, int Jp, const float* wih0, const float* bih0, float* g,
                             const float* whh0, const float* wih1_hh, const float* whh1, const float* bias1, float* h0,
                             float* hout, int H, int B, int T, void* work, float* gsave1, float* csave0, float* csave1,
                             int force_c0, void* stream);
int idv_clstm_fwd3(const float* x, int K, const float* wih0, const float* bih0, const float* whh0, const float* wih1,
                   const float* bih1, const float* whh1, const float* wih1_hh, int H, int B, int T, int Tp, int Jp, float* work,
                   float* out, int flags, const void* wih1_bf16, int proj_c0, void* stream);

/* Split-precision (bf16x3) form of the layer-0 input projection inside idv_clstm_fwd (nn.LSTM weight_ih_l0 of
 * lstm_re / lstm_im applied to the real / imaginary input, complex_progress.py:50-74): ximg = K-major split image of
 * the 2*K input planes (idv_planar_to_kimage: octet o = planes 8o..8o+7, layout as "split image" with F = 1),
 * wfrag from idv_pack_lstm_ih_bf16 (idv_lstm_ih_bf16_bytes), bias = bih0 of idv_pack_lstm_ih, G = the first
 * 16*T*B*H floats of idv_clstm_fwd's work buffer; then call idv_clstm_fwd with flags bit 1 set.  Needs
 * 8H % 256 == 0 and K % 64 == 0 (idv_lstm_proj_bf16_supported). */
long long idv_lstm_ih_bf16_bytes(int H, int K);
int idv_lstm_proj_bf16_supported(int H, int K);
int idv_pack_lstm_ih_bf16(const float* w_ih_re, const float* w_ih_im, int H, int K, void* wfrag, void* stream);
int idv_planar_to_kimage(const float* x, int nvalid, int nplanes, int J, int Jp, void* img, long long lo_off_elems, void* stream);
/* bf16x3 form of idv_pw_gemm (swap = 0): out[m][Jp] = sum_k W[m][k] x[k][j] + bias[m], guard columns zero -- the
 * windowed DFT / inverse DFT of STFT.forward / ISTFT.forward (pvae_module.py:21-27, :38-42) and the two linears of
 * ComplexDense (complex_progress.py:83-89).  ximg: K-major split image with K rounded up to 64 planes
 * (idv_planar_to_kimage with nplanes = that, or idv_stft_frames_kimage = idv_stft_frames writing the image directly);
 * wfrag: idv_pack_pw_bf16 of the row-major [M][K] matrix (idv_pw_bf16_wfrag_bytes).  t_valid < 1 is refused (-1). */
/* Column tile (64 or 128) the bf16x3 point-wise entries launch with for M rows per launch and B*Tp columns, by the function
 * the launches themselves call (idv_lstm_proj_bf16x3: M = 8H; idv_lstm_proj1_bf16x3: M = 4H per launch).  -1 for M <= 0,
 * B <= 0 or Tp <= 1. */
int idv_pw_bf16_coltile(int M, int B, int Tp);
/* the same contraction with the row-major transposed store out[(t*B + b)*ldo + m] over the valid (t, b): dh = W^T dG in the
 * form idv_lstm_bptt reads (bf16x3 training mode) */
int idv_pw_bf16x3_rows(const void* ximg, long long lo_off_slots, int K, const void* wfrag_bf16, const float* bias, float* out_rows,
                       int M, int ldo, int B, int T, int Tp, int Jp, void* stream);
long long idv_pw_bf16_wfrag_bytes(int M, int K);
int idv_pack_pw_bf16(const float* w, int M, int K, void* wfrag, void* stream);
int idv_pw_bf16x3(const void* ximg, long long lo_off_slots, int K, const void* wfrag_bf16, const float* bias, float* out, int M,
                  int B, int Tp, int Jp, int t_valid, void* stream);
/* idv_stft_frames straight into the K-major split image idv_pw_bf16x3 reads: slot (octet o, column j) holds samples 8o .. 8o+7
 * of frame j (zeros from sample win on), roundup(win, 64)/8 octets; the slots of the guard columns tp == 0 and tp > T are zeros. */
int idv_stft_frames_kimage(const float* x, int B, int L, int n_fft, int win, int hop, int T, void* img, long long lo_off_elems,
                           int Tp, int Jp, void* stream);
int idv_lstm_proj_bf16x3(const void* ximg, long long lo_off_slots, int K, const void* wfrag_bf16, const float* bias, float* G,
                         int H, int B, int T, int Tp, int Jp, void* stream);

/* reparameterization (pvae_module.py:1832-1886) with the two randn draws supplied by the caller.
 * lat: planar LSTM output [2][Hl][Jp]; miu/log_sigma/delta are channel offsets off_miu/off_ls/off_dl
 * (zdim channels each).  eps_r/eps_i: [B][ns][T][zdim].  z: planar [2][zdim][Jpz], columns (b*ns+s)*Tp+tp; its guard columns
 * tp == 0 and every tp > T (Tp may exceed T + 1) are written as +0.0, columns at or beyond B*ns*Tp are left alone.
 * IDV_EINVAL: a channel group past Hl, Jpz < B*ns*Tp. */
int idv_reparam(const float* lat, int Hl, int off_miu, int off_ls, int off_dl, int zdim, const float* eps_r,
                const float* eps_i, int ns, int B, int T, int Tp, int Jp, float* z, int Jpz, void* stream);

/* ---- losses ---------------------------------------------------------------------------------- */

/* si_snr (model/sisnr_loss.py:7-19): three dot products per utterance; out[0] = -mean_b(snr).
 * src_div: source row = b / src_div (repeat over num_samples).  work: 3*B doubles (zeroed here); afterwards
 * work[3b .. 3b+2] = (<s,s>, <e,s>, <e,e>) of utterance b.  IDV_EINVAL (idv_sisnr, idv_sisdr, idv_sisnr_bwd): B > 65535
 * (one grid row per utterance), a row pitch src_ld / ref_ld / est_ld shorter than L. */
int idv_sisnr(const float* source, int src_ld, int src_div, const float* est, int est_ld, int B, int L, double* work,
              float* out, void* stream);
/* Enhancement inference.  idv_sisdr: compute_sisdr of utils/eval_metrics.py:49-64 on the device, one value per
 * utterance (out[B]); work: 3*B doubles.  idv_mean_over_samples: the mean over the num_samples sampled waveforms of one
 * utterance, i_dccrn_vae/nsvae_dccrn/test_se_cvaefinetune.py:309-311 (x: [B*ns][L] -> out [B][L]). */
int idv_sisdr(const float* ref, int ref_ld, const float* est, int est_ld, int B, int L, double* work, float* out, void* stream);
int idv_mean_over_samples(const float* x, int ns, int B, int L, float* out, void* stream);
/* multiple_recon_loss terms (model/nsvae_loss.py:775-797): out[0] = loss_cpx, out[1] = loss_mag
 * (the original magnitude uses the real part twice, nsvae_loss.py:783).  pred_c: interleaved
 * [B][F][T][2]; ori: element (b,f,t,ri) at ori[(b/ori_div)*sb + f*sf + t*st + ri*sr]. */
int idv_recon_loss(const float* pred_c, const float* ori, long long sb, long long sf, long long st, long long sr,
                   int ori_div, int B, int F, int T, double* work, float* out, void* stream);
/* Closed-form complex-Gaussian KL, mean over (b,t): cal_kl_arbi_prior
 * (model/pretrain_pvaes_loss.py:225-281, eps 1e-9) / cal_kl (model/nsvae_loss.py:275-328, eps 1e-10).
 * q1, q2: planar latents [2][Hn][Jpn] with channel offsets on_miu / on_ls / on_dl; q2 == NULL is the
 * standard prior (0, 0, 0).  work: 3 doubles.  out[0] = mean KL.
 * IDV_EINVAL (idv_ckl, idv_ckl_bwd, and with one offset per latent idv_miu_dist, idv_miu_dist_bwd): a channel offset outside
 * [0, Hn - zdim], Tp < T + 1, Jpn < B*Tp; for q2 only where q2 is given. */
int idv_ckl(const float* q1, int H1, int Jp1, int o1_miu, int o1_ls, int o1_dl, const float* q2, int H2, int Jp2,
            int o2_miu, int o2_ls, int o2_dl, int zdim, float eps, int B, int T, int Tp, double* work, float* out,
            void* stream);
/* One term of residual_loss (model/nsvae_loss.py:363-446: torch.mean((connct - connct2).pow(2)) per skip connection): the mean
 * over [B, C, F, T, 2] of (a[:, ca0:ca0+C] - b[:, cb0:cb0+C])^2 for two planar activations with Ca / Cb channels.  The reference
 * computes and RETURNS the term but never adds it to the loss it back-propagates (:460-466), so there is no gradient entry.
 * work: 3 doubles.  IDV_EINVAL: 2*C*F > 65535 (one grid row per (part, channel, bin)). */
int idv_msd(const float* a, int Ca, int ca0, int JpA, const float* b, int Cb, int cb0, int JpB, int C, int F, int B, int Tp,
            int t_valid, double* work, float* out, void* stream);
/* Minibatch mutual-information estimate of the CVAE / NVAE ELBO (complex_standard_vae_loss.mutual_information,
 * model/pretrain_pvaes_loss.py:129-159 on cal_gaussian_prob :64-127; the "- mi_weight * mi" term of cal_loss :334-343):
 * mean over (i, s, t) of log q(z[i,s,t] | x_i) - (logsumexp_j log q(z[i,s,t] | x_j) - log B).
 * lat: planar posterior [2][H][Jp] with (miu, log_sigma, delta) at channel offsets (column b*Tp + t + 1); z: the planar samples
 * [2][zdim][Jpz] of idv_reparam (column (b*ns + s)*Tp + t + 1).  work: idv_mi_work_floats floats, kept for idv_mi_bwd (it holds
 * d MI / d log q afterwards); acc: 1 double.  idv_mi_bwd: dz (same shape as z, written) and dlat (same shape as lat, += on the
 * three channel groups), each scaled by gout[0]; either may be NULL. */
long long idv_mi_work_floats(int B, int ns, int T, int zdim);
int idv_mi_fwd(const float* lat, int H, int Jp, int o_miu, int o_ls, int o_dl, const float* z, int Jpz, int zdim, int ns, int B,
               int T, int Tp, float eps, float* work, double* acc, float* out, void* stream);
int idv_mi_bwd(const float* lat, int H, int Jp, int o_miu, int o_ls, int o_dl, const float* z, int Jpz, int zdim, int ns, int B,
               int T, int Tp, float eps, const float* work, const float* gout, float* dlat, float* dz, void* stream);
/* miu_dis_loss term (model/nsvae_loss.py:349-360): sqrt(sum_{h,ri} mean_{b,t} (miu1 - miu2)^2).  work: 3*2*zdim doubles;
 * afterwards work[3*(2h + ri)] = sum_{b,t} (miu1 - miu2)^2 of channel h, part ri.  Refusals as for idv_ckl. */
int idv_miu_dist(const float* q1, int H1, int Jp1, int off1, const float* q2, int H2, int Jp2, int off2, int zdim,
                 int B, int T, int Tp, double* work, float* out, void* stream);

/* ==== backward (gradient) entry points =========================================================================
 * The reference has no backward code of its own: torch.autograd differentiates the stock operators behind
 * `loss.backward()` in its train steps (supervised_dccrn/train.py:239-243, i_dccrn_vae/pretrained_vaes/train.py:296-301,
 * i_dccrn_vae/nsvae_dccrn/train_nsvae.py:557-561, train_second_phase_decoder.py:420-433).  Each entry below is the
 * gradient of the forward entry it names, for the same reference lines.  Planar gradients keep the layout invariant
 * (guard columns zero).  Data gradients of the conv blocks reuse idv_cconv2d_fwd with the adjoint weights. */

/* Adjoint weights for the DATA gradient of ComplexConv2d / ComplexConvTranspose2d (complex_progress.py:16-22, :244-250):
 * the parameter tensor read with the other layout (conv [Cout][Cin] as transposed-conv [Cin' = Cout][Cout' = Cin] and vice
 * versa), imaginary part negated, zero bias.  `transposed` / Cout / Cin_* describe the adjoint operator, which is then run by
 * idv_cconv2d_fwd: transposed = 1, tshift = 0 for the causal conv's gradient; transposed = 0, tshift = 0 and
 * t_valid_out = T for the causal transposed conv's. */
int idv_pack_cconv_adjoint(const float* w_re, const float* w_im, int Cout, int Cin_total, int Cin_used, int transposed,
                           float* wfrag, float* bias_out, void* stream);
/* the same operator as split-bf16 fragments for idv_cconv2d_bf16x3_fwd (training in bf16x3 mode; idv_cconv_bf16_wfrag_bytes) */
int idv_pack_cconv_bf16_adjoint(const float* w_re, const float* w_im, int Cout, int Cin_total, int Cin_used, int transposed,
                                void* wfrag, void* stream);

/* WEIGHT gradient of idv_cconv2d_fwd for one source of the channel concat (x: planar [2][Cx][Fin][Jp_x] = channels
 * ci_off .. ci_off+Cx of the weight tensor; dy: planar [2][Cout][Fout][Jp_dy], the gradient at the conv output, i.e. after
 * idv_cbn_bwd_apply in a train-mode block).  Writes dw_re / dw_im entries [*, ci_off:ci_off+Cx] (conv [Cout][Cin_total][5][2])
 * or [ci_off:ci_off+Cx, *] (transposed [Cin_total][Cout][5][2]).  Split-K over the B*Tp columns with deterministic
 * two-stage summation; work: idv_cconv_wgrad_work_floats(Cs, Cl, B, Tp) floats with (Cs, Cl) = (Cout, Cx) for a conv and
 * (Cx, Cout) for a transposed conv.  tshift as in idv_cconv2d_fwd.  Every weight-gradient entry below returns IDV_EINVAL,
 * and launches nothing, when work_floats is less than its sizer returns for the same arguments. */
long long idv_cconv_wgrad_work_floats(int Cs, int Cl, int B, int Tp);
int idv_cconv2d_bwd_weight(const float* x, int Cx, int ci_off, const float* dy, int Cout, int Cin_total, int transposed,
                           int tshift, int Fin, int B, int Tp, int Jp_x, int Jp_dy, float* work, long long work_floats,
                           float* dw_re, float* dw_im, void* stream);
/* the same contraction in split-bf16 arithmetic (both operands split on the fly, three v_mfma_f32_32x32x16_bf16 per product
 * block, fp32 accumulate): the weight gradient of the bf16x3 training mode; work: idv_cconv_wgrad_bf16_work_floats */
long long idv_cconv_wgrad_bf16_work_floats(int Cs, int Cl, int B, int Tp);
int idv_cconv2d_bwd_weight_bf16x3(const float* x, int Cx, int ci_off, const float* dy, int Cout, int Cin_total, int transposed,
                                  int tshift, int Fin, int B, int Tp, int Jp_x, int Jp_dy, float* work, long long work_floats,
                                  float* dw_re, float* dw_im, void* stream);
/* idv_cconv2d_bwd_weight with THREE real contractions per complex channel pair (Gauss / Karatsuba: P1 = p u, P2 = q v,
 * P3 = (p - q)(u + v); dWr = P1 + P2, dWi = +-(P1 - P2 - P3) with (p, q) / (u, v) the real / imaginary planes of the two operands): the same
 * weight gradient (reference: torch.autograd of nn.Conv2d / nn.ConvTranspose2d, model/complex_progress.py:8-36, :222-279) with 25 %
 * fewer multiplications; arguments as idv_cconv2d_bwd_weight.  idv_cconv_wgrad_gauss_supported(Cs, Cl): Cs >= 128 and Cl >= 32
 * complex channels (Cs / Cl = the S / L side: conv (Cout, Cx), transposed conv (Cx, Cout); a narrower S side would leave the
 * kernel's 128-plane tile half empty); work: idv_cconv_wgrad_gauss_work_floats. */
int idv_cconv_wgrad_gauss_supported(int Cs, int Cl);
long long idv_cconv_wgrad_gauss_work_floats(int Cx, int Cout, int transposed, int Fin, int B, int Tp, int Jp_x, int Jp_dy);
int idv_cconv2d_bwd_weight_gauss(const float* x, int Cx, int ci_off, const float* dy, int Cout, int Cin_total, int transposed,
                                 int tshift, int Fin, int B, int Tp, int Jp_x, int Jp_dy, float* work, long long work_floats,
                                 float* dw_re, float* dw_im, void* stream);
/* bias gradients (b_re enters real as +, imag as +; b_im real as -, imag as +; complex_progress.py:16-18) from
 * idv_cbn_stats(dy): db_re = sum dy_r + sum dy_i, db_im = sum dy_i - sum dy_r. */
int idv_cconv2d_bwd_bias(const double* stats_dy, int Cout, float* db_re, float* db_im, void* stream);

/* Weight gradient of idv_pw_gemm (ComplexDense complex_progress.py:83-89; nn.LSTM weight_ih / weight_hh :45-48):
 * dw[rowmap(m)][k] (+)= sum_j dout[m][j] * x[k][j + shift]; dout / x planar rows of stride Jp_d / Jp_x; shift = -1 pairs
 * every column with its left neighbour (h_{t-1} of the recurrent weights; the guard column supplies h_{-1} = 0).
 * rowmap 1: rows arrive in the recurrent kernels' gate order (colp) and are written in torch's (gate*H + unit), M a
 * multiple of 4H.  work: idv_pw_wgrad_work_floats(M, K, J). */
long long idv_pw_wgrad_work_floats(int M, int K, int J);
int idv_pw_bwd_weight(const float* dout, int M, int Jp_d, const float* x, int K, int Jp_x, int J, int shift, float* work,
                      long long work_floats, float* dw, int ldw, int rowmap, int H, int accumulate, void* stream);
/* the same contraction in split-bf16 arithmetic (bf16x3 training mode: LSTM projection, dense and DFT weight gradients) */
int idv_pw_bwd_weight_bf16x3(const float* dout, int M, int Jp_d, const float* x, int K, int Jp_x, int J, int shift, float* work,
                             long long work_floats, float* dw, int ldw, int rowmap, int H, int accumulate, void* stream);
int idv_planar_rowsum(const float* x, int M, int Jp, int J, int accumulate, float* out, void* stream);   /* bias gradients */

/* Train-mode ComplexBatchNormal + PReLU (complex_progress.py:131-209, pvae_module.py:64-68, :88-93).
 * idv_cbn_apply_prelu_to: out-of-place idv_cbn_apply_prelu (training keeps the conv output y for the backward pass).
 * Backward, three steps: idv_cbn_bwd_reduce (per-channel sums [C][8] doubles of du = dz*PReLU'(u), du (x) y and the PReLU
 * slope term; data-parallel training all-reduces these), idv_cbn_bwd_finalize (moments = the [5][C] output of
 * idv_cbn_finalize, count = B*F*T of the whole batch; -> coef[C][12], d gamma_rr/ri/ii, d beta_r/i, dslope[1], each times
 * param_grad_scale: 1 normally, 1/world when the sums were all-reduced, because the ranks then all hold the gradient of
 * the SUM of their losses and the gradient all-reduce averages), idv_cbn_bwd_apply (dy = Z^T du + A (y - mu) + c).
 * idv_cbn_bwd_reduce overwrites sums (slot 7 of a channel is 0); the gradient takes u > 0 as the positive PReLU branch (torch's
 * convention: u == 0 gets the slope) while the forward takes u >= 0 -- the value at u == 0 is 0 either way.  dslope may be NULL
 * (nothing is written there); coef[c][11] is 0.
 * Geometry of the four planar entries (idv_cbn_apply_prelu_to, idv_cbn_bwd_reduce, idv_cbn_bwd_apply and their _img twins):
 * t_valid >= 1, Tp >= t_valid + 1, Jp >= B*Tp, else -1 and nothing is written.  out / dy get every column of [0, B*Tp) of their
 * 2*C*F rows: the result on the kept columns 1 <= tp <= t_valid, +0.0 on the guard columns; pitch columns [B*Tp, Jp) are not
 * written.  Guard and pitch columns of the inputs are not read. */
int idv_cbn_apply_prelu_to(const float* y, const float* fold, const float* prelu_slope, int C, int F, int B, int Tp, int Jp,
                           int t_valid, float* out, void* stream);
int idv_cbn_bwd_reduce(const float* dz, const float* y, const float* fold, const float* prelu_slope, int C, int F, int B,
                       int Tp, int Jp, int t_valid, double* sums, void* stream);
int idv_cbn_bwd_finalize(const double* sums, double count, const float* moments, const float* gamma_rr, const float* gamma_ri,
                         const float* gamma_ii, int C, float* coef, float* dgamma_rr, float* dgamma_ri, float* dgamma_ii,
                         float* dbeta_r, float* dbeta_i, float* dslope, float param_grad_scale, void* stream);
int idv_cbn_bwd_apply(const float* dz, const float* y, const float* fold, const float* coef, const float* prelu_slope, int C,
                      int F, int B, int Tp, int Jp, int t_valid, float* dy, void* stream);
/* the out-of-place normalise + PReLU and the batch-norm backward apply, each also writing the split image of its result (bf16x3
 * training mode: the conv kernels read images; C % 4 == 0, lo_off_elems % 8 == 0, img 16-byte aligned and the planar entries'
 * geometry, else -1; image layout and edge slots as idv_planar_to_image: every slot of [0, C/4 * F * Jp) is written, zeros in the
 * guard and pitch columns, plus the zero slot in front of each plane and the 8 behind it) */
int idv_cbn_apply_prelu_to_img(const float* y, const float* fold, const float* prelu_slope, int C, int F, int B, int Tp, int Jp,
                               int t_valid, float* out, void* img, long long lo_off_elems, void* stream);
int idv_cbn_bwd_apply_img(const float* dz, const float* y, const float* fold, const float* coef, const float* prelu_slope, int C,
                          int F, int B, int Tp, int Jp, int t_valid, float* dy, void* img, long long lo_off_elems, void* stream);

/* idv_mask_apply backward (pvae_module.py:224-234): gradient w.r.t. the mask from the gradients of the planar prediction
 * and / or of the interleaved complex64 tensor (either may be NULL); dX (optional, x_div == 1 only): gradient w.r.t. the
 * input spectrum, needed when the waveform itself requires grad.  Guard columns of dmask and dX zeroed; the geometry checks of
 * idv_mask_apply. */
int idv_mask_apply_bwd(const float* mask, const float* X, int x_div, int JpX, const float* dpred, const float* dpred_c, int F,
                       int B, int T, int Tp, int Jp, float* dmask, float* dX, void* stream);
/* Adjoint of repeating every utterance of a planar activation n times in a row (the skip connections of the fine-tuned
 * decoder, pvae_module.py:2563-2567): dx[row][b*Tp+tp] = sum_s drep[row][(b*n+s)*Tp+tp], rows = 2*C*F planar rows. */
int idv_repeat_batch_bwd(const float* drep, int n, int rows, int B, int Tp, int Jp_rep, int Jp, float* dx, void* stream);
/* interleaved [B][F][T][2] -> planar [2][F][Jp] (adjoint of idv_planar_to_complex; also packs a caller's complex tensor);
 * guard columns zeroed.  Tp >= T+1, Jp >= B*Tp. */
int idv_complex_to_planar(const float* in_c, float* act, int F, int B, int T, int Tp, int Jp, void* stream);
/* idv_istft_ola backward (pvae_module.py:38-42): dy[B][hop*(T-1)] -> dframes[win][Jp]; the inverse-DFT adjoint is idv_pw_gemm
 * with the transposed matrix. */
int idv_istft_ola_bwd(const float* dy, const float* env_inv, int B, int n_fft, int win, int hop, int T, int Tp, int Jp,
                      float* dframes, void* stream);
/* idv_stft_frames backward (pvae_module.py:21-27, reflect padding included): dframes[win][Jp] -> dx[B][L]. */
int idv_stft_frames_bwd(const float* dframes, int B, int L, int n_fft, int win, int hop, int T, int Tp, int Jp, float* dx,
                        void* stream);
/* idv_reparam backward (pvae_module.py:1832-1886): dz planar [2][zdim][Jpz] -> += on the (miu, log_sigma, delta) channels of
 * dlat planar [2][Hl][Jp] (caller zeroes it). */
int idv_reparam_bwd(const float* lat, int Hl, int off_miu, int off_ls, int off_dl, int zdim, const float* eps_r,
                    const float* eps_i, int ns, int B, int T, int Tp, int Jp, const float* dz, int Jpz, float* dlat, void* stream);

/* Loss gradients.  grad_out / g_*: device scalars (the incoming gradient of the loss value).
 * idv_sisnr_bwd: work = the 3*B doubles idv_sisnr left behind; dest[B][L] = d loss / d estimate (sisnr_loss.py:7-19).
 * idv_recon_loss_bwd: d(loss_cpx, loss_mag) / d pred_c (nsvae_loss.py:775-797).
 * idv_ckl_bwd: d KL / d q1, += into dq1 (same layout as q1) (nsvae_loss.py:275-328, pretrain_pvaes_loss.py:225-281).
 * idv_miu_dist_bwd: loss_value = the forward result; += into dq1 and / or dq2 (nsvae_loss.py:349-360). */
int idv_sisnr_bwd(const float* source, int src_ld, int src_div, const float* est, int est_ld, int B, int L, const double* work,
                  const float* grad_out, float* dest, void* stream);
int idv_recon_loss_bwd(const float* pred_c, const float* ori, long long sb, long long sf, long long st, long long sr,
                       int ori_div, int B, int F, int T, const float* g_cpx, const float* g_mag, float* dpred_c, void* stream);
int idv_ckl_bwd(const float* q1, int H1, int Jp1, int o1_miu, int o1_ls, int o1_dl, const float* q2, int H2, int Jp2,
                int o2_miu, int o2_ls, int o2_dl, int zdim, float eps, int B, int T, int Tp, const float* grad_out, float* dq1,
                void* stream);
int idv_miu_dist_bwd(const float* q1, int H1, int Jp1, int off1, const float* q2, int H2, int Jp2, int off2, int zdim, int B,
                     int T, int Tp, const float* grad_out, const float* loss_value, float* dq1, float* dq2, void* stream);

/* ComplexLSTM backward (complex_progress.py:50-74), building blocks driven by the host mirror (ops.clstm_bwd):
 * idv_lstm_uncombine: planar output gradient -> per-run dh[4][T*B][H] (real = run0 - run3, imag = run2 + run1);
 * idv_pack_lstm_hh_bwd: W_hh [4H][H] x 2 -> fragments for the (16 x 4H) x (4H x H) step contraction, 2*4H*H floats;
 * idv_lstm_bptt: back-propagation through time of one layer, one launch per step; `gates` (activated i,f,g,o from the
 *   training forward, addressing as G0 / G1 above) is overwritten with the pre-activation gate gradients;
 *   work: idv_lstm_bptt_work_floats(H, B);
 * idv_rows_to_planar: src[(t*B + b)*ld + c0 + u] -> planar dst[u][b*Tp + t + 1] (guard columns zeroed);
 * idv_lstm_bias_grad: db[gate*H + unit] (+)= sum_j dGp[colp][j] for 4H planar rows. */
int idv_lstm_uncombine(const float* dout, int H, int B, int T, int Tp, int Jp, float* dh, void* stream);
int idv_pack_lstm_hh_bwd(const float* w_hh_re, const float* w_hh_im, int H, float* whhT, void* stream);
long long idv_lstm_bptt_work_floats(int H, int B);
int idv_lstm_bptt(float* gates, long long g_run_z, long long g_run_s, int ldg, const float* cstates, const float* dhout,
                  const float* whhT, int H, int B, int T, float* work, void* stream);
/* the same as ONE cooperative launch per layer for H = 128 (four workgroups per (run, 16-sequence tile), W_hh^T and the running
 * dc in registers, dA_t exchanged with the fence-free hand-off of idv_lstm_rec_pers); idv_lstm_bptt dispatches to it when
 * idv_lstm_bptt_coop_supported (IDV_LSTM_BPTT_COOP=0 keeps the per-step launches).  work: idv_lstm_bptt_coop_work_bytes. */
int idv_lstm_bptt_coop_supported(int H, int B);
/* BPTT of BOTH H = 128 layers in one cooperative launch (lstm_bptt_stack2_f32.hip; the backward twin of idv_lstm_stack2_f32):
 * layer 0 runs one step behind layer 1 and contracts dh0[t] = dA1[t] W_ih1 inside its recurrence, so the dh0 buffer and its
 * GEMM disappear.  g1: [run][T*B][4H] activated gates of layer 1 -> gate gradients; g0 (+ g0_run_z, g0_run_s, ldg0): layer 0's,
 * addressed as in idv_lstm_bptt; c1, c0: cell states [4][T*B][H]; dhout1: gradient arriving at layer 1's output; whhT1, wihT1,
 * whhT0: idv_pack_lstm_hh_bwd of weight_hh_l1, weight_ih_l1 ([4H][H] as well), weight_hh_l0; work:
 * idv_lstm_bptt_stack2_work_bytes bytes, 16-byte aligned.  Supported: H == 128, 32 * ceil(B/16) <= idv_coop_max_workgroups()
 * (IDV_LSTM_BPTT_STACK2=0 turns it off). */
int idv_lstm_bptt_stack2_supported(int H, int B);
long long idv_lstm_bptt_stack2_work_bytes(int H, int B);
int idv_lstm_bptt_stack2(float* g1, float* g0, long long g0_run_z, long long g0_run_s, int ldg0, const float* c1, const float* c0,
                         const float* dhout1, const float* whhT1, const float* wihT1, const float* whhT0, int H, int B, int T,
                         void* work, void* stream);
long long idv_lstm_bptt_coop_work_bytes(int H, int B);
int idv_lstm_bptt_coop(float* gates, long long g_run_z, long long g_run_s, int ldg, const float* cstates, const float* dhout,
                       const float* whhT, int H, int B, int T, void* work, void* stream);
int idv_rows_to_planar(const float* src, long long ld, int c0, int ncol, int B, int T, int Tp, int Jp, float* dst, void* stream);
int idv_lstm_bias_grad(const float* dGp, int H, int Jp, int J, int accumulate, float* db, void* stream);

/* ---- data-parallel train step: gradient bucket and optimiser as multi-tensor kernels (bucket.hip) --------------------------
 * The reference trains on one device with stock torch (`loss.backward(); optimizer.step()` with
 * torch.optim.Adam(lr, weight_decay=0.001): supervised_dccrn/train.py:109, 239-243; i_dccrn_vae/nsvae_dccrn/train_nsvae.py:200,
 * 557-561; i_dccrn_vae/nsvae_dccrn/train_second_phase_decoder.py:420-433; i_dccrn_vae/pretrained_vaes/train.py:296-301).
 * Bucket layout: a flat fp32 buffer in which tensor i occupies [off_i, off_i + numel_i), every off_i a multiple of 4 floats,
 * the gaps zero padding; table[n][3] (int64, device memory, sorted by off) = {device pointer of the tensor's first element
 * (0: absent), off_i, numel_i}; total = the padded length (multiple of 4); flat is 16-byte aligned.
 *   idv_bucket_gather : flat <- tensors (absent tensors and padding as zeros): the operand of the RCCL all-reduce;
 *   idv_bucket_scatter: tensors <- scale * flat (scale 1 after ReduceOp.AVG, 1 / world after a SUM);
 *   idv_bucket_adam   : one torch.optim.Adam step (no amsgrad / maximize) over all tensors of the table: parameters through
 *     ptable, gradients EITHER through gtable (same offsets) OR straight from a bucket gflat (e.g. the all-reduced one, so the
 *     scatter pass disappears), multiplied by grad_scale; exp_avg / exp_avg_sq in the bucket layout;
 *     bias_correction1 = 1 - beta1^t, bias_correction2_sqrt = sqrt(1 - beta2^t) for the step count t of this step; the betas are
 *     doubles because torch forms 1 - beta in double before rounding (1 - 0.999f in float is 1.3e-5 off).  A table row with a
 *     NULL parameter pointer is skipped (a parameter that received no gradient keeps its value and moments, as in torch). */
int idv_bucket_gather(const long long* table, int n, long long total, float* flat, void* stream);
int idv_bucket_scatter(const long long* table, int n, long long total, const float* flat, float scale, void* stream);
int idv_bucket_adam(const long long* ptable, const long long* gtable, const float* gflat, float* exp_avg, float* exp_avg_sq,
                    int n, long long total, float lr, double beta1, double beta2, float eps, float weight_decay,
                    float bias_correction1, float bias_correction2_sqrt, float grad_scale, void* stream);

/* ---- global gradient norm, clipping and the non-finite guard on the bucket (bucket.hip; optim.Adam(max_norm, skip_nonfinite),
 * optim.clip_grad_norm_; additive entries: IDV_ABI_VERSION is unchanged).  Tables, layout and the refusals of the
 * entries above.
 *   idv_bucket_sqnorm: partials[first + k] = the sum, over the elements of flat range [4096 k, 4096 (k + 1)) that belong to a
 *     present parameter (non-NULL ptable row) with a gradient, of x^2 with x = the FLOAT product g * grad_scale (the first operation
 *     of the Adam kernel) widened to double: every square is exact, every addition is in double and in a fixed order (per thread
 *     in increasing flat index, a fixed butterfly across the wave, the four wave sums in wave order), no atomics, so two runs
 *     return the same bits.  Gradients through gtable or gflat as in idv_bucket_adam.  Padding and absent rows are never
 *     added, whatever they hold.  idv_bucket_sqnorm_partials(total) = ceil(total / 4096) = the partials one table takes (-1 for a
 *     total that idv_bucket_sqnorm refuses); the caller lays the partials of several tables one after another with `first`.
 *   idv_bucket_clip_finalize: one workgroup adds partials[0 .. count) in a fixed order and writes the 32-byte device record
 *     (8-byte aligned, zeroed by the caller before its first use; byte offsets IDV_CLIP_*): sumsq (double), norm = sqrt(sumsq)
 *     (double), coef (float) = min(1, max_norm / (norm + 1e-6)) formed in double and rounded once (torch's clip_grad_norm_ rule; 1
 *     for max_norm <= 0: "norm only"), finite (int) = isfinite(sumsq) -- a float squares to at most 1.2e77, so the sum is
 *     non-finite exactly when a gradient is -- and skipped (int64), which is incremented when guard != 0 and finite == 0.
 *   idv_bucket_adam_clipped: idv_bucket_adam with g = (g * grad_scale) * coef + weight_decay * p, coef read from the record.
 *     guard != 0: a step with finite == 0 returns before any store (parameters and both moments keep their bits), and the bias
 *     corrections are formed on the device from t = t_host - skipped and the double betas (t_host >= 1: the step count the host
 *     would have without refused steps), so a refused step does not advance them; bias_correction1 / bias_correction2_sqrt are
 *     then only checked.  guard == 0: the host's bias corrections are used as in idv_bucket_adam.
 *   idv_bucket_scale: tensors of the table *= coef of the record, in place (nothing is written when coef == 1).
 * IDV_EINVAL (before any GPU work): a NULL or misaligned buffer (partials, record: 8 bytes; gflat, the moments: 16), n <= 0,
 * total <= 0 or total & 3, first < 0, count <= 0, a NaN max_norm, both or neither of gtable / gflat, a NULL record. */
#define IDV_CLIP_RECORD_BYTES 32
#define IDV_CLIP_SUMSQ 0
#define IDV_CLIP_NORM 8
#define IDV_CLIP_COEF 16
#define IDV_CLIP_FINITE 20
#define IDV_CLIP_SKIPPED 24
int idv_bucket_sqnorm_partials(long long total);
int idv_bucket_sqnorm(const long long* ptable, const long long* gtable, const float* gflat, int n, long long total, float grad_scale,
                      double* partials, long long first, void* stream);
int idv_bucket_clip_finalize(const double* partials, int count, double max_norm, int guard, void* record, void* stream);
int idv_bucket_adam_clipped(const long long* ptable, const long long* gtable, const float* gflat, float* exp_avg, float* exp_avg_sq,
                            int n, long long total, float lr, double beta1, double beta2, float eps, float weight_decay,
                            float bias_correction1, float bias_correction2_sqrt, float grad_scale, const void* record, int guard,
                            long long t_host, void* stream);
int idv_bucket_scale(const long long* table, int n, long long total, const void* record, void* stream);

/* ---- complex conv / transposed conv with Winograd-transformed frequency taps (cgemm_wino.hip) -------------------------------
 * The encoder / decoder blocks' contractions (model/complex_progress.py:8-36, :222-279) with 7 instead of 10 real products per
 * input channel and pair of rows (F(2,3) on the even, F(2,2) on the odd frequency taps) on top of the three-product complex form
 * of idv_cconv2d_gauss_fwd; same result up to the rounding of the transforms.  idv_pack_cconv_wino: weights as
 * idv_pack_cconv_gauss (transposed / conj conventions), wfrag of idv_cconv_wino_wfrag_floats floats; the epilogue table (epi,
 * has_fold) is idv_pack_cconv_gauss's.  idv_cconv2d_wino_fwd: arguments as idv_cconv2d_gauss_fwd with x1_div = 1 and both
 * sources at pitch Jp (Jp % 4 == 0, 16-byte aligned).  IDV_WINO=0 turns it off (IDV_WINO_CONV=0: the conv form only). */
int idv_cconv_wino_supported(int transposed, int C0, int C1, int Cout, int Fin);
long long idv_cconv_wino_wfrag_floats(int transposed, int Cout, int cin_used);
int idv_cconv_wino_config(int transposed, int Cin, int Cout);
int idv_pack_cconv_wino(const float* w_re, const float* w_im, int Cout, int Cin_total, int Cin_used, int transposed, int conj,
                        float* wfrag, void* stream);
int idv_cconv2d_wino_fwd(const float* x0, int C0, const float* x1, int C1, const float* wfrag, const float* epi, int has_fold,
                         const float* prelu_slope, float* out, double* stats, double* stats_work, int stats_rep, int transposed,
                         int tshift, int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out, const float* addend,
                         int addend_div, int addend_Jp, void* stream);

/* ---- transposed conv with Winograd-transformed frequency AND time taps (cgemm_tw.hip) ----------------------------------------
 * The decoder block's contraction (model/complex_progress.py:222-279) as idv_cconv2d_wino_fwd(transposed = 1), with the two time
 * taps in F(2,2) form over pairs of output columns: 3 instead of 4 real products per column pair and channel pair, i.e. 3/4 x 7/10
 * x 3/4 = 0.39 of the reference's real products.  Same result up to the rounding of the transforms.  idv_pack_cconv_tw re-orders
 * the fragments of idv_pack_cconv_wino(transposed = 1) (wino_frag) into idv_cconv_tw_wfrag_floats floats; epi / has_fold from
 * idv_pack_cconv_gauss; statistics and addend as idv_cconv2d_wino_fwd.  Sources at pitch Jp (Jp % 4 == 0, 16-byte aligned),
 * C0 % 8 == 0 with a second source.  IDV_TW=0 (Python side) keeps idv_cconv2d_wino_fwd. */
int idv_cconv_tw_supported(int C0, int C1, int Cout, int Fin);
long long idv_cconv_tw_wfrag_floats(int Cout, int cin_used);
int idv_pack_cconv_tw(const float* wino_frag, int Cout, int cin_used, float* tw_frag, void* stream);
int idv_ctconv2d_tw_fwd(const float* x0, int C0, const float* x1, int C1, const float* wfrag, const float* epi, int has_fold,
                        const float* prelu_slope, float* out, double* stats, double* stats_work, int stats_rep, int tshift,
                        int Cout, int Fin, int B, int Tp, int Jp, int t_valid_out, const float* addend, int addend_div,
                        int addend_Jp, void* stream);

/* ---- conv with Winograd-transformed frequency AND time taps (cgemm_tw2.hip) ---------------------------------------------------
 * The encoder block's contraction (model/complex_progress.py:8-36) as idv_cconv2d_wino_fwd(transposed = 0) with the two time taps
 * in F(2,2) form (0.39 of the reference's real products); one source, no addend.  idv_pack_cconv_tw2 re-orders the fragments of
 * idv_pack_cconv_wino(transposed = 0) into idv_cconv_tw2_wfrag_floats floats; epi / has_fold from idv_pack_cconv_gauss;
 * statistics as idv_cconv2d_wino_fwd.  Source at pitch Jp (Jp % 4 == 0, 16-byte aligned). */
int idv_cconv_tw2_supported(int Cin, int Cout, int Fin);
long long idv_cconv_tw2_wfrag_floats(int Cout, int cin_used);
int idv_pack_cconv_tw2(const float* wino_frag, int Cout, int cin_used, float* tw_frag, void* stream);
int idv_cconv2d_tw_fwd(const float* x0, int Cin, const float* wfrag, const float* epi, int has_fold, const float* prelu_slope,
                       float* out, double* stats, double* stats_work, int stats_rep, int tshift, int Cout, int Fin, int B, int Tp,
                       int Jp, int t_valid_out, void* stream);

/* ---- streaming enhancement (stream_conv.hip, stream_lstm.hip, stream_io.hip; streaming.StreamingDCCRN) ------------------------
 * One push runs the causal DCCRN over the k frames it completes for B lock-step streams.  Activations use the planar-J layout
 * with Tp = k + 1; a per-stream history column hist[2][C][F][B] supplies x[t-1] of each stream's first frame.  Exact fp32.
 *
 * Complex conv / transposed conv block (causal, kernel (5,2), stride (2,1)): sources x0 (C0 channels, history h0) and x1 (C1
 * skip channels, history h1; C1 = 0: none), then bias, the folded eval batch norm (fold[Cout][6] or NULL) and PReLU (slope or
 * NULL).  Writes out (planar [2][Cout][Fout][Jp]) and the last column of each stream to hist_out (or NULL); x0hist_out (or NULL)
 * receives the last column of x0.  nsplit = idv_stream_cconv_splits(...) K parts, work holds nsplit * 2 * Cout * Fout * B * k
 * floats when nsplit > 1; the parts are added in a fixed order.  w / bias from idv_stream_pack_cconv (w_*: conv [Cout][Cin][5][2],
 * transposed [Cin][Cout][5][2]; idv_stream_cconv_wfloats floats of w, 2 * Cout of bias). */
long long idv_stream_cconv_wfloats(int Cin, int Cout);
int idv_stream_pack_cconv(const float* w_re, const float* w_im, const float* b_re, const float* b_im, int Cin, int Cout,
                          int transposed, float* w, float* bias, void* stream);
int idv_stream_cconv_splits(int transposed, int Cin, int Cout, int Fin, int B);
int idv_stream_cconv(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                     const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist_out, float* x0hist_out,
                     float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k, int Tp, int Jp, void* stream);
/* Two-layer complex LSTM over k steps with carried state (H = 128 only; idv_stream_lstm_supported).  G: [2][k*B][8H] layer-0
 * projections from idv_pw_gemm (idv_pack_lstm_ih fragments, swap = 1, ldo = 8H); wt: [2 sets][W_hh0, W_ih1, W_hh1][H][4H]
 * (transposed torch weights, set 0 = lstm_re); b1: [2][4H] = b_ih1 + b_hh1; state: [4 runs][2 layers][h, c][B][H], read and
 * written back; hout: [4][k*B][H] scratch; out: planar [2][H][Jp] (real = rr - ii, imag = ir + ri). */
int idv_stream_lstm_supported(int H);
int idv_stream_clstm(const float* G, const float* wt, const float* b1, float* state, float* hout, float* out, int H, int B, int k,
                     int Tp, int Jp, void* stream);
/* Framing of frames t0 .. t0+k-1 into frames[win][Jp] (torch.stft centre / reflect convention): samples below n_prev from
 * ring[B][R] (sample s at s mod R), the others from x[B][n_new] (row stride ldx >= n_new); L_end >= 0 applies the end mirror of
 * a signal of L_end samples.  idv_stream_ring stores the last R samples of x into the ring. */
int idv_stream_frames(const float* ring, int R, const float* x, long long ldx, int n_new, long long n_prev, long long L_end, int B,
                      int n_fft, int win, int hop, long long t0, int k, float* frames, int Tp, int Jp, void* stream);
int idv_stream_ring(float* ring, int R, const float* x, long long ldx, int n_new, long long n_prev, int B, void* stream);
/* Overlap-add of the windowed inverse-DFT frames t0 .. t0+k-1 (frames[win][Jp], k may be 0) onto the carried partial sums
 * carry_in[B][cap] (padded positions n_fft/2 + e0 ...), emission of output samples e0 .. e1-1 divided by the istft envelope of
 * frames 0 .. T_total-1 (T_total < 0: no end yet) into y[b][y_off ...] (row stride ldy), and the partial sums of positions
 * n_fft/2 + e1 .. p_end-1 into carry_out. */
int idv_stream_ola(const float* frames, int Tp, int Jp, const float* carry_in, int carry_in_len, float* carry_out, int cap, int B,
                   int n_fft, int win, int hop, long long t0, int k, long long T_total, long long e0, long long e1, long long p_end,
                   float* y, int ldy, long long y_off, void* stream);

/* ---- streaming sessions: per-slot start, push length and end (stream_io.hip, stream_conv.hip, stream_lstm.hip;
 * streaming.StreamingSessions; additive entries: IDV_ABI_VERSION is unchanged).  Each entry takes a device table
 * rows[B][IDV_STREAM_ROW_FIELDS] of long long where the lock-step entry takes scalars; row b describes what slot b does in this
 * launch group.  k_launch = max_b k_b sizes the planar layout (Tp >= k_launch + 1) and the pointwise kernels; the columns of a
 * slot past its k_b hold zeros (frames) or values nobody reads.  A slot with k = 0 and e0 = e1 sits the group out: nothing of its
 * state is read or written.  hist / carry buffers are given whole ([2 parities][...]): slot b reads half parity_b and writes half
 * 1 - parity_b.  The arithmetic of a column is that of the lock-step entry, in the same order. */
#define IDV_STREAM_ROW_FIELDS 12
#define IDV_ROW_N_PREV 0    /* samples of the slot's signal before this call (held by the ring) */
#define IDV_ROW_COUNT 1     /* new samples x[b][0 .. count-1]; nothing at or past x[b][count] is read */
#define IDV_ROW_L_END 2     /* length of the signal when its end is known (end mirror), else -1 */
#define IDV_ROW_T0 3        /* first frame of the group */
#define IDV_ROW_K 4         /* frames of the group, 0 <= k <= k_launch */
#define IDV_ROW_PARITY 5    /* history / carry half read; 1 - parity is written */
#define IDV_ROW_E0 6        /* output samples e0 .. e1-1 become final */
#define IDV_ROW_E1 7
#define IDV_ROW_P_END 8     /* one past the last padded overlap-add position touched */
#define IDV_ROW_CARRY_IN 9  /* carried overlap-add positions */
#define IDV_ROW_T_TOTAL 10  /* frames of the whole signal when its end is known, else -1 */
#define IDV_ROW_Y_OFF 11    /* column of y that receives sample e0 */
int idv_stream_row_fields(void);   /* IDV_STREAM_ROW_FIELDS of the library */
/* Host only, launches nothing: validates a HOST copy of a group's table against what idv_stream_frames and idv_stream_ola check
 * for scalars: every sample a frame reads lies in the ring's reach or in x[b][0 .. count-1] (count <= n_x), the start mirror is
 * there, carry_in and the outgoing carry <= cap, k <= k_launch <= Tp - 1, y_off + e1 - e0 <= ldy, p_end - (n_fft/2 + e0) <=
 * span_max, parity in {0, 1}.  IDV_EINVAL otherwise.  Call it before the table is uploaded: the entries below cannot look. */
int idv_stream_rows_check(const long long* host_rows, int B, int R, int n_x, int n_fft, int win, int hop, int cap, int k_launch, int Tp,
                          long long ldy, long long span_max);
/* idv_stream_frames with n_prev, count, L_end, t0 and k of each slot; columns tl >= k_b are zeroed.  x may be NULL when every
 * count is 0. */
int idv_stream_frames_rows(const float* ring, int R, const float* x, long long ldx, const long long* rows, int B, int n_fft, int win,
                           int hop, int k_launch, float* frames, int Tp, int Jp, void* stream);
/* Appends the count_b samples x[b][0 .. count_b-1] (x: [B][n_x], row stride ldx) to the ring of slot b at position n_prev_b. */
int idv_stream_ring_rows(float* ring, int R, const float* x, long long ldx, int n_x, const long long* rows, int B, void* stream);
/* idv_stream_ola per slot: carry[2][B][cap] by parity_b, t0 / k / e0 / e1 / p_end / carry_in / T_total / y_off from the row; the
 * same order of sums (carry, then frames in increasing t) and the same double-precision envelope.  span_max >= the longest
 * p_end - (n_fft/2 + e0) of the slots that take part. */
int idv_stream_ola_rows(const float* frames, int Tp, int Jp, float* carry, int cap, const long long* rows, int B, int n_fft, int win,
                        int hop, int k_launch, long long span_max, float* y, long long ldy, void* stream);
/* idv_stream_cconv per slot: h0 / h1 / hist / x0hist are [2 parities][2][C][F][B]; x[t-1] of column 0 comes from half parity_b;
 * column k_b - 1 of out goes to hist (or NULL) and column k_b of x0 to x0hist (or NULL), half 1 - parity_b, only when k_b > 0.
 * nsplit and work as idv_stream_cconv with k = k_launch. */
int idv_stream_cconv_rows(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                          const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist, float* x0hist,
                          float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k_launch, int Tp, int Jp,
                          const long long* rows, void* stream);
/* idv_stream_clstm per slot (G: [2][k_launch*B][8H], hout: [4][k_launch*B][H]): steps t >= k_b leave h and c of both layers of
 * slot b as they are; its columns of out from k_b on are zero. */
int idv_stream_clstm_rows(const float* G, const float* wt, const float* b1, float* state, float* hout, float* out, int H, int B,
                          int k_launch, int Tp, int Jp, const long long* rows, void* stream);
/* buf viewed as [outer][B][inner]: zeroes the n_slots slots listed in the device array slots (each in [0, B)). */
int idv_stream_zero_rows(float* buf, long long outer, int B, long long inner, const long long* slots, int n_slots, void* stream);

/* ---- streaming conv on the fp32 matrix cores (stream_conv_mfma.hip; streaming.Streaming*(conv="mfma"); additive entries:
 * IDV_ABI_VERSION is unchanged).  The same function as idv_stream_cconv / idv_stream_cconv_rows and, bit for bit, the same
 * result: v_mfma_f32_32x32x2_f32 is fed the products of the vector-ALU kernel in its order, with the same K parts (nsplit from
 * idv_stream_cconv_splits, the same work layout and combine) and the same epilogue.  Blocks with Cout >= 16 only. */
/* Floats of the MFMA weight pack: [co tiles of 32][Cin][5][4 fragments][64 lanes]. */
long long idv_stream_cconv_mfma_wfloats(int Cin, int Cout);
/* Inputs and bias as idv_stream_pack_cconv; w in MFMA fragment order (lane = output channel and k; -w_im is formed here, rows
 * past Cout are zero). */
int idv_stream_pack_cconv_mfma(const float* w_re, const float* w_im, const float* b_re, const float* b_im, int Cin, int Cout,
                               int transposed, float* w, float* bias, void* stream);
/* Host only, launches nothing: 1 when the MFMA entries serve the block (Cin >= 1 and Cout >= 16), 0 when it stays on
 * idv_stream_cconv, -1 for a non-positive Cin or Cout. */
int idv_stream_cconv_mfma_supported(int transposed, int Cin, int Cout);
/* idv_stream_cconv with w from idv_stream_pack_cconv_mfma; IDV_EINVAL for an unsupported shape. */
int idv_stream_cconv_mfma(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                          const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist_out, float* x0hist_out,
                          float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k, int Tp, int Jp, void* stream);
/* idv_stream_cconv_rows with w from idv_stream_pack_cconv_mfma; IDV_EINVAL for an unsupported shape. */
int idv_stream_cconv_mfma_rows(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                               const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist, float* x0hist,
                               float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k_launch, int Tp, int Jp,
                               const long long* rows, void* stream);

/* ---- streaming conv in split-bf16 (bf16x3) arithmetic on the bf16 matrix cores (stream_conv_bf16.hip;
 * streaming.Streaming*(conv="bf16x3"); additive entries: IDV_ABI_VERSION is unchanged).  The same function, arguments, K parts,
 * work layout, combine and epilogue as idv_stream_cconv / idv_stream_cconv_rows; every product w x is replaced by
 * w_lo x_hi + w_hi x_lo + w_hi x_hi (hi = the fp32 value with its low 16 bits cleared, lo = the round-to-nearest-even bf16 of the
 * exact difference) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Sources, histories, outputs and work stay fp32; x is split
 * in registers, the weights by the pack.  Not bit-identical to the fp32 entries (about 1e-5 relative); the arithmetic of an
 * output position depends on the layer shape and nsplit alone, never on B, k or the row table. */
/* Floats (32-bit words of two bf16) of the bf16x3 weight pack: [co tiles of 32][ceil(Cin / 4)][5][4 fragments][64 lanes][4]. */
long long idv_stream_cconv_bf16_wfloats(int Cin, int Cout);
/* Inputs and bias as idv_stream_pack_cconv; w in bf16 A-fragment order, split here once (fragments: real tile hi, lo, imaginary
 * tile hi, lo; -w_im is formed before the split; channel slots past Cin and rows past Cout are zero). */
int idv_stream_pack_cconv_bf16(const float* w_re, const float* w_im, const float* b_re, const float* b_im, int Cin, int Cout,
                               int transposed, float* w, float* bias, void* stream);
/* Host only, launches nothing: 1 when the bf16x3 entries serve the block (Cin >= 4 and Cout >= 16), 0 when it stays on the fp32
 * entries, -1 for a non-positive Cin or Cout. */
int idv_stream_cconv_bf16_supported(int transposed, int Cin, int Cout);
/* idv_stream_cconv with w from idv_stream_pack_cconv_bf16; IDV_EINVAL for an unsupported shape. */
int idv_stream_cconv_bf16(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                          const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist_out, float* x0hist_out,
                          float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k, int Tp, int Jp, void* stream);
/* idv_stream_cconv_rows with w from idv_stream_pack_cconv_bf16; IDV_EINVAL for an unsupported shape. */
int idv_stream_cconv_bf16_rows(const float* x0, const float* h0, int C0, const float* x1, const float* h1, int C1, const float* w,
                               const float* bias, const float* fold, const float* prelu_slope, float* out, float* hist, float* x0hist,
                               float* work, int nsplit, int transposed, int Cout, int Fin, int B, int k_launch, int Tp, int Jp,
                               const long long* rows, void* stream);

/* ---- streaming I-DCCRN-VAE enhancement (stream_lstm.hip, stream_io.hip; streaming.StreamingVAE; additive entries:
 * IDV_ABI_VERSION is unchanged).  The noisy encoder runs at batch B, the decoder at batch B * ns with row b * ns + s, the order
 * of idv_reparam and idv_mask_apply(x_div = ns).  The three entries below are lock-step; each has a _rows twin for sessions
 * (streaming.StreamingVAESessions) further down. */
/* idv_stream_clstm for the hidden sizes of the VAE encoders: H % 16 == 0, 16 <= H <= 768 (idv_stream_clstm_wide_supported).
 * G, wt, b1, state and out as idv_stream_clstm.  hstep: idv_stream_clstm_wide_hstep_floats(H, B, k) = 8 * k * B * H floats of
 * scratch, [2 layers][4 runs][k*B][H]: the h of every step (h is never updated in place; the last rows go to state at the end).
 * One launch per layer per step (2k + 2 launches), no cooperative launch and no wait on another workgroup.  Every
 * pre-activation is one fmaf chain: G or b1 first, then the products in increasing k (layer 1: W_ih1 h0, then W_hh1 h1). */
int idv_stream_clstm_wide_supported(int H);
long long idv_stream_clstm_wide_hstep_floats(int H, int B, int k);
int idv_stream_clstm_wide(const float* G, const float* wt, const float* b1, float* state, float* hstep, float* out, int H, int B,
                          int k, int Tp, int Jp, void* stream);
/* The two Gaussian draws of idv_reparam for frames t0 .. t0+k-1: eps_r, eps_i [B][ns][k][zdim] (idv_reparam's layout with
 * T = k).  Philox4x32-10, key (seed low 32, seed high 32), counter (t low, t high, b*ns + s, u); words 0 and 1 through
 * Box-Muller: u1 = ((w0 >> 8) + 1) 2^-24, theta = 2 pi (w1 >> 8) 2^-24, r = sqrtf(-2 logf(u1)), eps_r = r cosf(theta),
 * eps_i = r sinf(theta).  A draw depends on (seed, b, s, t, u) alone. */
int idv_stream_eps(long long seed, long long t0, int k, int B, int ns, int zdim, float* eps_r, float* eps_i, void* stream);
/* A skip at batch B * ns: columns b*Tp + 1 .. b*Tp + k of x (planar [2][C][F][Jp]) go to columns (b*ns + s)*Tp + 1 .. of xn
 * (planar [2][C][F][Jpn]) for s < ns, and hist [2][C][F][B] (the history half the chunk reads; NULL with histn: none) to
 * histn [2][C][F][B*ns]. */
int idv_stream_repeat(const float* x, const float* hist, int C, int F, int B, int ns, int k, int Tp, int Jp, float* xn, float* histn,
                      int Jpn, void* stream);

/* ---- VAE sessions: the _rows twins of the three entries above (stream_lstm.hip, stream_io.hip;
 * streaming.StreamingVAESessions; additive entries: IDV_ABI_VERSION is unchanged).  rows[B][IDV_STREAM_ROW_FIELDS] is the table of
 * the other _rows entries, one row per slot of the ENCODER batch B; the decoder side takes a second table [B*ns] whose row
 * b*ns + s equals row b, with the existing idv_stream_cconv_rows / idv_stream_cconv_mfma_rows / idv_stream_ola_rows at B = B*ns.
 * Each kernel is the lock-step kernel's body compiled a second time: the arithmetic of a column and its order are one source. */
/* idv_stream_clstm_wide per slot.  G ([2][k_launch*B][8H]) and hstep (idv_stream_clstm_wide_hstep_floats(H, B, k_launch)) have
 * k_launch as the step stride; 2 * k_launch step launches, then the combine and the state copy.  Slot b takes part in the steps
 * t < k_b only: in a step t >= k_b nothing of it is written, neither c in state nor its hstep row, and since its hstep rows may
 * never have been written, zeros are staged in their place and the results dropped.  The fmaf chain of an active stream is the
 * lock-step one (G or b1 first, then increasing k) whatever its seven tile neighbours do; a workgroup whose 8 streams are all idle
 * at step t returns before its first barrier.  The state copy takes row k_b - 1 of slot b and nothing when k_b = 0; the combine
 * writes zeros to the columns t >= k_b of out, as idv_stream_clstm_rows does. */
int idv_stream_clstm_wide_rows(const float* G, const float* wt, const float* b1, float* state, float* hstep, float* out, int H, int B,
                               int k_launch, int Tp, int Jp, const long long* rows, void* stream);
/* idv_stream_eps per slot: eps_r, eps_i [B][ns][k_launch][zdim].  Frame tl < k_b of slot b is drawn with the counter
 * (t0_b + tl, b*ns + s, u), exactly as idv_stream_eps(seed, t0_b, ...) draws it; the entries with tl >= k_b are zero. */
int idv_stream_eps_rows(long long seed, const long long* rows, int B, int ns, int zdim, int k_launch, float* eps_r, float* eps_i,
                        void* stream);
/* idv_stream_repeat per slot: hist is [2 parities][2][C][F][B] and histn [2 parities][2][C][F][B*ns] (twice the lock-step
 * scratch: the _rows conv entries read h1 at half parity_b).  The columns tl < k_b of slot b and its history of half parity_b go
 * to the rows b*ns + s of xn and to half parity_b of histn; a slot with k_b = 0 is not touched, nor are the columns tl >= k_b. */
int idv_stream_repeat_rows(const float* x, const float* hist, int C, int F, int B, int ns, int k_launch, int Tp, int Jp,
                           const long long* rows, float* xn, float* histn, int Jpn, void* stream);

/* ---- streaming two-latent enhancement (stream_io.hip, elementwise.hip; streaming.StreamingVAETwoLatents; additive entries:
 * IDV_ABI_VERSION is unchanged).  The speech and the noise decoder both run at batch B * ns on one encoder pass; the estimator
 * takes the mean over the samples in front of the inverse DFT, which then runs at batch B. */
/* idv_stream_eps with the second pair of the same Philox block: words 0 and 1 give eps_sr, eps_si, bit for bit what
 * idv_stream_eps(seed, t0, k, B, ns, zdim, ...) writes; words 2 and 3 go through the same Box-Muller and give eps_nr, eps_ni, the
 * noise latent's draws.  All four are [B][ns][k][zdim]; a draw depends on (seed, b, s, t, u) alone. */
int idv_stream_eps_pair(long long seed, long long t0, int k, int B, int ns, int zdim, float* eps_sr, float* eps_si, float* eps_nr,
                        float* eps_ni, void* stream);
/* The estimators of idv_outtype_estimate (mode 0 real_imag_mask, 1 complex_mask, 2 phase_mask) on the planar streaming layout,
 * for the k columns of a launch group.  speech, noise: the last-block outputs of the two decoders, planar [2][F][Jpn], sample s of
 * stream b in column (b*ns + s)*Tp + t + 1; X: the noisy spectrum, planar [2][F][Jp], column b*Tp + t + 1.  recon_mask 1: each
 * sample is first turned into the masked spectrum with the arithmetic of idv_mask_apply (x_div = ns); 0 (real_imag): taken as it
 * is.  S and N are the means over s = 0 .. ns-1 summed in this order, as idv_outtype_estimate sums them.  out: planar [2][F][Jp],
 * column b*Tp + t + 1 for t < k; the guard columns are not written.  An output depends on its own column alone. */
int idv_stream_estimate(const float* speech, const float* noise, const float* X, int recon_mask, int mode, int ns, int F, int B,
                        int k, int Tp, int Jp, int Jpn, float* out, void* stream);

/* ---- two-latent sessions and per-slot seeds (stream_io.hip; streaming.StreamingVAETwoLatentsSessions and
 * streaming.StreamingVAESessions; an additive entry: IDV_ABI_VERSION is unchanged). */
/* idv_stream_eps_pair per slot, each slot with a seed of its own: seeds is a device array [B], rows the slots' table
 * [B][IDV_STREAM_ROW_FIELDS]; all four outputs are [B][ns][k_launch][zdim].  Frame tl < k_b of slot b is drawn with the key
 * seeds[b] and the counter (t0_b + tl, b*ns + s, u): words 0 and 1 through Box-Muller give eps_sr, eps_si, words 2 and 3 eps_nr,
 * eps_ni, bit for bit what idv_stream_eps_pair(seeds[b], t0_b, k_b, B, ns, zdim, ...) writes for slot b.  The entries with
 * tl >= k_b are zero in every output.  eps_nr == eps_ni == NULL selects the single-pair form, which writes the speech draws
 * alone (with equal seeds: what idv_stream_eps_rows writes); exactly one of the two NULL is IDV_EINVAL.  The same kernel source
 * as the three entries above it, compiled with the seed read from seeds[b]. */
int idv_stream_eps_pair_rows(const long long* seeds, const long long* rows, int B, int ns, int zdim, int k_launch, float* eps_sr,
                             float* eps_si, float* eps_nr, float* eps_ni, void* stream);

/* ---- save, load and move a slot's stream (stream_state.hip, stream_io.hip; streaming._Slots.save / load of every sessions
 * class; additive entries: IDV_ABI_VERSION is unchanged).
 *
 * The per-slot state of a sessions object lies in n_views device buffers of floats, view j an [outer_j][B][inner_j] array.  A
 * slot's RECORD is the concatenation of its [outer_j][inner_j] blocks in view order, per_slot = sum_j outer_j inner_j floats:
 * element (o, i) of view j sits at offset_j + o inner_j + i.  views is a table [n_views][IDV_STATE_VIEW_FIELDS] of long long,
 * slots a list of n_slots slot numbers; both are DEVICE arrays for gather / scatter and HOST arrays for the check. */
#define IDV_STATE_MAX_VIEWS 64
#define IDV_STATE_VIEW_FIELDS 4
#define IDV_STATE_VIEW_ADDR 0     /* device address of the buffer (floats) */
#define IDV_STATE_VIEW_OUTER 1
#define IDV_STATE_VIEW_INNER 2
#define IDV_STATE_VIEW_OFFSET 3   /* of the view inside a record, in floats */
/* Host only, touches no GPU: IDV_EINVAL unless 1 <= n_views <= 64, every address is non-zero, every outer and inner is
 * positive, the offsets start at 0, increase and tile [0, per_slot) exactly (offset_{j+1} = offset_j + outer_j inner_j, the last
 * view ends at per_slot: no overlap, no gap), 1 <= n_slots <= B, every slot lies in 0 .. B-1 and no slot appears twice.  Call it
 * on the host copies before they are uploaded: the two entries below cannot look.  That buffer j really holds outer_j B inner_j
 * floats is the caller's to guarantee. */
int idv_stream_state_check(const long long* views_host, int n_views, int B, const long long* slots_host, int n_slots,
                           long long per_slot);
/* out[n_slots][per_slot] (contiguous) <- the records of the named slots, in ONE launch whatever n_views and n_slots are.  The
 * view table is staged in LDS and every element finds its view by a bounded binary search over the offsets.  out is written
 * coalesced; the buffers are read contiguously for inner > 1 and at stride B for inner = 1.  Plain loads and stores, no atomics;
 * nothing but the named slots' elements is read, and nothing of the buffers is written.  IDV_EINVAL (nothing launched) for a
 * NULL pointer, n_views outside 1 .. 64, n_slots outside 1 .. B or per_slot <= 0. */
int idv_stream_state_gather(const long long* views, int n_views, int B, const long long* slots, int n_slots, float* out,
                            long long per_slot, void* stream);
/* The records in[n_slots][per_slot] -> the named slots: the same kernel with the copy turned round.  Every element of every
 * view of a named slot is written, nothing else; a slot named twice would be written twice in no defined order, which is why
 * idv_stream_state_check refuses it. */
int idv_stream_state_scatter(const long long* views, int n_views, int B, const long long* slots, int n_slots, const float* in,
                             long long per_slot, void* stream);
/* idv_stream_eps_pair_rows with a draw identity per slot: draw_slots is a device array [B], and slot b draws with the counter
 * (t0_b + tl, draw_slots[b]*ns + s, u) in place of (t0_b + tl, b*ns + s, u), so that a stream saved in slot draw_slots[b] and
 * loaded into slot b continues with the draws it would have had.  With draw_slots[b] = b for every b it writes the bits of
 * idv_stream_eps_pair_rows; everything else (seeds, rows, the outputs, the single-pair form, the refusals) is that entry's.
 * draw_slots[b] * ns + ns - 1 must fit in 32 bits.  The same kernel source, compiled with one more template flag whose pointer
 * is the last kernel argument; idv_stream_eps_pair_rows itself is unchanged. */
int idv_stream_eps_pair_rows_as(const long long* seeds, const long long* draw_slots, const long long* rows, int B, int ns, int zdim,
                                int k_launch, float* eps_sr, float* eps_si, float* eps_nr, float* eps_ni, void* stream);

/* ---- streaming at any sample rate: stateful polyphase resampler (stream_resample.hip; streaming.StreamingResampler,
 * StreamingResamplerSessions, AtRate, SessionsAtRate; additive entries: IDV_ABI_VERSION is unchanged).
 *
 * The definition is idv_resample's (scipy.signal.resample_poly with its default filter, not soxr) for a ratio ALREADY reduced by its
 * gcd, m = max(up, down) <= 640, half = 10 m, taps: device fp32[2 half + 1] as idv_resample takes them:
 *     y[n] = float(up * sum_j x[j] taps[half + n down - j up]),  max(0, ceil((n down - half) / up)) <= j <= min(L - 1, (n down + half) / up),
 * one double accumulator per output, j increasing, no atomics: the bits of idv_resample for the whole signal, however it is cut.
 * After P samples the outputs n < n_final(P) = max(0, ceil((P up - half) / down)) are final; a call that takes a stream from P0 to
 * P1 = P0 + count writes outputs n_final(P0) .. n_final(P1) - 1, the end of a signal of L = P1 samples writes n_final(P0) ..
 * ceil(L up / down) - 1.  State: hist[2 parities][B][H], H = 2 half / up + 1 = idv_stream_resample_hist(up, down) samples per
 * stream; a call reads half parity and, unless it ends the signal or brings no samples, writes the last H samples to half 1 -
 * parity (samples before the start of the signal as zeros), so that no workgroup reads what another one of the launch writes.
 * Positions are 64-bit (up to 2^50) and the cost of a call does not depend on them.  Row b reads nothing at or past x[b][count_b]
 * and nothing of another row; its bits do not depend on B, on the other rows, on the cut or on taps_mode.
 *
 * taps_mode: where the kernel reads the taps.  IDV_SR_TAPS_AUTO: from memory for up > 1 (an output touches the 2 half / up + 1
 * taps of its phase only), from LDS for up = 1 (every output reads every tap); the other two force one form (tests, measurements).
 *
 * idv_stream_resample_hist / idv_stream_resample_final: host only; H and n_final(P), -1 for refused arguments. */
#define IDV_SR_TAPS_AUTO 0
#define IDV_SR_TAPS_MEM 1
#define IDV_SR_TAPS_LDS 2
int idv_stream_resample_hist(int up, int down);
long long idv_stream_resample_final(long long P, int up, int down);
/* Lock-step: B streams at position P0 receive x[b][0 .. n_new-1] (row stride ldx; NULL for n_new = 0); y[b][0 .. m-1] (row stride
 * ldy) <- outputs n0 .. n0 + m - 1.  flush = 1: the signals end at L = P0 + n_new and no history is written.  n0 and m are the
 * caller's to know (they size y) and are held to the definition: IDV_EINVAL unless n0 = n_final(P0) and n0 + m = n_final(P1), at
 * flush ceil(L up / down).  IDV_EINVAL (before any GPU work) also for a ratio that is not reduced or has m > 640, H other than
 * idv_stream_resample_hist(up, down), parity outside {0, 1}, n_new outside 0 .. 2^27, ldx < n_new, ldy < m, B outside 1 .. 65535,
 * an unknown taps_mode and more than 2^31 - 257 positions B (m + H).  Nothing is launched for n_new = 0 and m = 0. */
int idv_stream_resample(float* hist, int H, int parity, const float* x, long long ldx, int n_new, long long P0, int flush, long long n0,
                        int m, int B, int up, int down, const float* taps, int taps_mode, float* y, long long ldy, void* stream);
/* Per slot: rows is a device table [B][IDV_SR_ROW_FIELDS] of long long, row b what slot b does in this call. */
#define IDV_SR_ROW_FIELDS 7
#define IDV_SR_ROW_P0 0      /* samples of the slot's signal before this call */
#define IDV_SR_ROW_COUNT 1   /* new samples x[b][0 .. count-1]; nothing at or past x[b][count] is read */
#define IDV_SR_ROW_N0 2      /* first output of this call, n_final(P0) */
#define IDV_SR_ROW_M 3       /* outputs of this call; columns m .. ldy-1 of y[b] are written as zeros */
#define IDV_SR_ROW_PARITY 4  /* history half read; 1 - parity is written unless the slot ends or is idle */
#define IDV_SR_ROW_END 5     /* 1: the signal ends at P0 + count */
#define IDV_SR_ROW_IDLE 6    /* 1: no samples and no end; nothing of the slot's state is read or written */
int idv_stream_resample_row_fields(void);   /* IDV_SR_ROW_FIELDS of the library */
/* Host only, launches nothing: validates a HOST copy of the table against what idv_stream_resample checks for scalars: count in
 * 0 .. n_x, parity / end / idle in {0, 1}, idle exactly when count = 0 and end = 0, n0 = n_final(P0), n0 + m = n_final(P0 + count)
 * or, for a slot that ends, ceil((P0 + count) up / down), m <= ldy.  IDV_EINVAL otherwise.  Call it before the table is uploaded:
 * idv_stream_resample_rows cannot look. */
int idv_stream_resample_rows_check(const long long* host_rows, int B, int n_x, int up, int down, int H, long long ldy);
/* x: [B][n_x] (row stride ldx; NULL for n_x = 0), y: [B][ldy], every column written.  The history of a slot that ends is left to
 * idv_stream_zero_rows (hist as [2][B][H]: outer 2, inner H). */
int idv_stream_resample_rows(float* hist, int H, const float* x, long long ldx, int n_x, const long long* rows, int B, int up, int down,
                             const float* taps, int taps_mode, float* y, long long ldy, void* stream);

/* ---- batches of utterances of different lengths (ragged.hip, reduce.hip; inference.enhance_* / compute_sisdr with `lengths`) ---
 * lens: device int32[], samples per utterance.  Utterance b has T_b = 1 + lens[b] / hop frames and hop * (T_b - 1) output samples;
 * the batch is laid out for Tmax = max_b T_b frames, Tp >= Tmax + 1.  A causal network computes frame t from frames <= t, so only
 * these signal ends and the metric need the lengths (additive entries: IDV_ABI_VERSION is unchanged).
 *
 * idv_stft_frames for x[B][ldx] (row pitch ldx): the end mirror of row b is taken at lens[b] and no sample at or past lens[b] is
 * read; the columns of frames t >= T_b and the guard column are zeros.  The _kimage form writes the split-bf16 K-major image
 * (idv_stft_frames_kimage) instead. */
int idv_stft_frames_ragged(const float* x, long long ldx, const int* lens, int B, int n_fft, int win, int hop, int Tmax, float* frames,
                           int Tp, int Jp, void* stream);
int idv_stft_frames_kimage_ragged(const float* x, long long ldx, const int* lens, int B, int n_fft, int win, int hop, int Tmax, void* img,
                                  long long lo_off_elems, int Tp, int Jp, void* stream);
/* idv_istft_ola per row: row b uses lens[b / len_div] (len_div = num_samples for the VAE decoders' B * num_samples rows).
 * Overlap-add of frames 0 .. T_b - 1 only, divided by the envelope of those frames (formed on the fly in double, as idv_make_dft
 * forms its table), into y[b][s] for s < hop * (T_b - 1); zeros from there to hop * (Tmax - 1).  y rows at pitch ldy. */
int idv_istft_ola_ragged(const float* frames, const int* lens, int len_div, int B, int n_fft, int win, int hop, int Tmax, int Tp, int Jp,
                         float* y, long long ldy, void* stream);
/* idv_sisdr over the first lens[b] samples of each row (clamped to the shorter row pitch); work: 3*B doubles. */
int idv_sisdr_ragged(const float* ref, int ref_ld, const float* est, int est_ld, const int* lens, int B, double* work, float* out,
                     void* stream);

/* ---- STOI / ESTOI and RMSE scoring of a padded batch (stoi.hip; inference.compute_stoi / compute_estoi / compute_rmse / score_list;
 * additive entries: IDV_ABI_VERSION is unchanged).  idv_stoi: the short-time objective intelligibility of Taal et al. 2011
 * (extended = 0) or its extended form of Jensen & Taal 2016 (extended = 1) with the constants and the framing of the pystoi package,
 * resampling of fs = 16000 input to 10 kHz (fs = 10000 skips it; nothing else is accepted), removal of the frames
 * more than 40 dB under the clean signal's loudest, 512-point DFT, 15 third-octave bands, 30-frame segments.  ref: the clean
 * signals, est: the processed ones, rows at pitch ref_ld / est_ld >= Lmax; lens: device int32[B], samples per row (clamped to
 * Lmax), or NULL: every row has Lmax (<= 2^27) samples.  Nothing at or past lens[b] is read and row b's result does not depend on
 * B, on the other rows or on the padding.  out[b]: the score, exactly 1e-5 when fewer than 30 frames remain; counts (may be
 * NULL): [B][3] = (frames, kept frames, segments).  work: idv_stoi_work_bytes(B, Lmax, fs) bytes (-1 for arguments idv_stoi
 * refuses), 16-byte aligned.  The tables are formed on the device once per device, on the stream of the first call.
 * idv_rmse_ragged: utils/eval_metrics.py:33-41 over the first lens[b] (required; clamped to the shorter pitch) samples of each
 * row, alpha = <est, ref> / <est, est>, out[b] = sqrt(mean((alpha est - ref)^2)), sums in double; work: 3*B doubles. */
long long idv_stoi_work_bytes(int B, int Lmax, int fs);
int idv_stoi(const float* ref, long long ref_ld, const float* est, long long est_ld, const int* lens, int B, int Lmax, int fs,
             int extended, void* work, long long work_bytes, float* out, int* counts, void* stream);
int idv_rmse_ragged(const float* ref, long long ref_ld, const float* est, long long est_ld, const int* lens, int B, double* work,
                    float* out, void* stream);

/* ---- corpus preparation (resample.hip, moments.hip, ragged.hip; inference.resample / resample_list, dataset/stats.py; additive
 * entries: IDV_ABI_VERSION is unchanged).
 *
 * idv_resample: scipy.signal.resample_poly(x, up, down) with its default filter for a padded batch x[B][ldx] -> y[B][ldy].  up / down
 * are reduced by their gcd inside; with m = max(up, down) and half = 10 m,
 *     y[b][n] = up * sum_j x[b][j] taps[half + n down - j up],  0 <= j < lens[b],  tap index in [0, 2 half],  n < ceil(lens[b] up / down).
 * taps: device fp32[idv_resample_ntaps(up, down) = 20 m + 1], formed by the caller in double: kaiser(2 half + 1, 5.0) * sinc(t / m) / m
 * for t = -half .. half, normalised to sum 1.  lens: device int32[B] (clamped to [0, L]) or NULL: every row has L samples.  Row b
 * reads nothing at or past lens[b] and nothing of another row; columns ceil(lens[b] up / down) .. ceil(L up / down) - 1 are written as
 * zeros; fp32 samples and taps, a double accumulator per output in increasing j, no atomics: a row's result does not depend on B, on
 * the other rows or on the padding.  IDV_EINVAL (before any GPU work) for up <= 0, down <= 0, m > 640 (8 / 11.025 / 22.05 / 24 / 32 /
 * 44.1 / 48 / 96 kHz to and from 16 kHz all fit), L <= 0, L > 2^27, ldx < L, ldy < ceil(L up / down) and an output row of 2^31 - 256
 * columns or more.  idv_resample_ntaps / idv_resample_len: host only; the tap count and ceil(L up / down), -1 for refused arguments. */
int idv_resample_ntaps(int up, int down);
long long idv_resample_len(long long L, int up, int down);
int idv_resample(const float* x, long long ldx, const int* lens, int B, int L, int up, int down, const float* taps, float* y,
                 long long ldy, void* stream);
/* idv_stft_frames_ragged with the padding of the signal ends as an argument.  IDV_PAD_REFLECT: that entry itself (torch.stft's
 * mirror; ldx > n_fft/2 and every lens[b] > n_fft/2).  IDV_PAD_CONSTANT: zeros before sample 0 and from lens[b] on, as
 * librosa.stft(center=True) of librosa >= 0.10 pads (pad_mode="constant"); any lens[b] >= 1 is valid.  In both modes row b has
 * T_b = 1 + lens[b] / hop frames, and the DFT is idv_pw_gemm with the idv_make_dft matrix (periodic hann(win) centred in n_fft). */
#define IDV_PAD_REFLECT 0
#define IDV_PAD_CONSTANT 1
int idv_stft_frames_ragged_pad(const float* x, long long ldx, const int* lens, int B, int n_fft, int win, int hop, int Tmax, int pad_mode,
                               float* frames, int Tp, int Jp, void* stream);
/* Running mean and sum of squared deviations (M2) of every row of planar spectra spec[rows = 2F][Jp] over their valid columns: frame
 * t < min(Tmax, 1 + lens[b] / hop) of utterance b sits in column b Tp + t + 1 (lens NULL: Tmax frames each); guard columns and frames
 * past a row's end are skipped, not counted as zeros.  state: device double[1 + 2 rows] = (n, mean[rows], M2[rows]), zeroed by the
 * caller before the first update; var = M2 / (n - 1).  Each workgroup forms (n, mean, M2) of its 2048-column tile about the tile's own
 * mean (two passes over registers), and one workgroup folds the tiles and then the state by Chan's formula in a fixed order: no
 * atomics, the same sequence of calls gives the same bits.  work: idv_spec_moments_work_bytes(rows, B, Tp) bytes (-1 for refused
 * arguments), 8-byte aligned.  idv_spec_moments_merge: state <- Chan merge of state and other (another state of the same rows, e.g.
 * of another rank or loader shard). */
long long idv_spec_moments_work_bytes(int rows, int B, int Tp);
int idv_spec_moments_update(const float* spec, const int* lens, int B, int hop, int Tmax, int Tp, int Jp, int rows, double* state,
                            void* work, long long work_bytes, void* stream);
int idv_spec_moments_merge(double* state, const double* other, int rows, void* stream);

/* ---- silence trimming (trim.hip; inference.trim / trim_list, the trimmed segment index of dataset/dataload.py; additive entries:
 * IDV_ABI_VERSION is unchanged).  The definition is librosa.effects.trim(y, top_db, ref=np.max, frame_length=frame,
 * hop_length=hop) of librosa 0.10 restated (tests/trim_ref.py; parity with the package itself is unpinned).  For row b of n = lens[b]
 * samples (lens: device int32[B], clamped to [0, L], or NULL: every row has L samples) of the padded batch x[B][ldx]:
 *     T = 1 + n / hop frames; frame t covers samples [t hop - frame/2, t hop + frame/2), zeros outside [0, n);
 *     P[t] = mean of the squares over the frame;  db[t] = 10 log10(max(1e-10, P[t])) - 10 log10(max(1e-10, max_t P[t]));
 *     t0 / t1 the first / last frame with db[t] > -top_db:  bounds[b] = {t0 hop, min(n, (t1 + 1) hop)};  no such frame: {0, 0}.
 * So a row of zeros (or wholly below 1e-10 in power) comes back untrimmed as {0, n}, and n = 0 gives {0, 0}.
 * idv_trim_bounds: one wave sums the squares of one hop-sample block in double (fp32 squares are exact in double; 16-byte loads at
 * any row pitch; the order of the sum depends on the sample's index in its block alone), one workgroup per row adds the frame / hop
 * blocks of each frame in increasing order, divides by frame and compares in double.  Nothing at or past lens[b] and nothing of
 * another row is read, no atomics: a row's result does not depend on B, the other rows, the padding or ldx.  work:
 * idv_trim_work_bytes(B, L, hop) = 8 B ceil(L / hop) bytes, 8-byte aligned (host only; -1 for refused arguments).  bounds: device
 * int32[B][2].  power: NULL, or device double[B][ldp] that receives P[b][0 .. T_b - 1] and zeros up to column L / hop.
 * idv_trim_gather: y[b][i] = x[b][bounds[b][0] + i] for i < bounds[b][1] - bounds[b][0], zeros from there to Lout - 1; bounds are read
 * on the device and must lie inside the row.
 * IDV_EINVAL (before any GPU work) for a NULL pointer (lens and power may be NULL), B <= 0 or B > 65535, L <= 0 or L > 2^27, ldx < L,
 * hop <= 0, hop > 2^27 or hop % 4 != 0, frame % (2 hop) != 0 or frame / hop > 64, top_db <= 0 or not finite, work_bytes too small,
 * ldp < 1 + L / hop when power is given; for the gather Lout <= 0 or Lout > 2^27 and ldy < Lout. */
long long idv_trim_work_bytes(int B, int L, int hop);
int idv_trim_bounds(const float* x, long long ldx, const int* lens, int B, int L, int frame, int hop, double top_db, void* work,
                    long long work_bytes, int* bounds, double* power, long long ldp, void* stream);
int idv_trim_gather(const float* x, long long ldx, const int* bounds, int B, int Lout, float* y, long long ldy, void* stream);

/* ---- latent-space report (latent.hip; latent.py; additive entries: IDV_ABI_VERSION is unchanged).  A latent is read
 * in place from a planar buffer q[2][H][Jp] with F = 1: channel off + h of frame t of row b is q[(ri H + off + h) Jp + b Tp + t + 1].
 * frames: device int32[B], the valid frames of each row, clamped to [1, T] (NULL: T each); nothing at or past frame frames[b] and no
 * guard column is read.  Elementwise arithmetic is fp32 as the reference's, every sum is double in a fixed order, no atomics.
 *
 * idv_latent_row_stats: out[b][13] = kl, then (min, max, mean, norm) of vrr, of vri and of vii (pretrained_vaes/test_prevae.py:25-74,
 * 171-197 per row).  idv_latent_pair_dist: out[b][3] = dis_mean, dis_sigma, dis_delta between two posteriors
 * (nsvae_dccrn/test_nsvae_se.py:27-35).  One wave per (row, channel), its lanes the frames t = lane, lane + 64, ..., then the xor
 * butterfly; a second kernel, one wave per row, adds the channels h = lane, lane + 64 and runs the butterfly again.  A row's value
 * depends on frames[b] and zdim alone, bit for bit.  work: device double[B zdim 10] (row_stats) / [B zdim 3] (pair_dist).
 * zdim % 16 == 0, 16 <= zdim <= 128, B <= 65535. */
int idv_latent_row_stats(const float* q, int H, int Jp, int Tp, int off_miu, int off_ls, int off_dl, int zdim, const int* frames, int B,
                         int T, double* work, double* out, void* stream);
int idv_latent_pair_dist(const float* qa, int Ha, int Jpa, int Tpa, int oa_miu, int oa_ls, int oa_dl, const float* qb, int Hb, int Jpb,
                         int Tpb, int ob_miu, int ob_ls, int ob_dl, int zdim, const int* frames, int B, int T, double* work, double* out,
                         void* stream);
/* Running mean and co-moments of the 2 zdim rows (real channels, then imaginary channels) of miu over the valid frames.
 * state: device double[1 + 2 zdim + (2 zdim)^2] = (n, mean[2 zdim], C[2 zdim][2 zdim]), zeroed by the caller; cov = C / n.  Only the
 * 32 x 32 blocks on and above the block diagonal of C are written (the rest stays as the caller left it).  The frames are numbered
 * b T + t and cut into chunks of idv_miu_moments_chunk() numbers, whatever Tp and Jp are.  Per chunk: the count and mean of the valid
 * frames, then X X^T of the values centred on that mean (invalid columns zero) on v_mfma_f64_16x16x4_f64 through LDS; the chunks and then
 * the state are folded in increasing order by Chan's formula C = Ca + Cb + (na nb / n) d d^T.  work: idv_miu_moments_work_bytes bytes
 * (-1 for refused arguments), 8-byte aligned.  idv_miu_moments_merge: state <- Chan merge of state and another state. */
int idv_miu_moments_chunk(void);
long long idv_miu_moments_work_bytes(int zdim, int B, int T);
int idv_miu_moments_update(const float* q, int H, int Jp, int Tp, int off_miu, int zdim, const int* frames, int B, int T, double* state,
                           void* work, long long work_bytes, void* stream);
int idv_miu_moments_merge(double* state, const double* other, int zdim, void* stream);
/* Sets of latent vectors x[N][D] (D = 2 zdim floats each, contiguous).  idv_latent_set_moments: mom[2 D] = the mean and the population
 * variance of every column.  idv_latent_silhouette (test_nsvae_se.py:39-50, 482-500): out[6] = sc, mean_dis, then the variance averaged
 * over the even (real) and the odd (imaginary) columns of set 1 and of set 2; work: double[N1 + N2], the score of every vector. */
int idv_latent_set_moments(const float* x, int N, int D, double* mom, void* stream);
int idv_latent_silhouette(const float* x1, int N1, const float* x2, int N2, int D, const double* mom1, const double* mom2, double* work,
                          double* out, void* stream);

/* ---- mixture synthesis (mix.hip; dataset/mix.py snr_mix / DynamicMixtures; additive entries: IDV_ABI_VERSION is unchanged; DESIGN.md
 * 3.12).  The definition is normalize / snr_mixer / segmental_snr_mixer of the DNS-Challenge synthesizer restated (tests/mix_ref.py;
 * parity with the package itself is unpinned), except that a window's level is the true dB of its mean square.  EPS = 2^-52.  Row b:
 * n = lens[b] clean samples c (lens: device int32[B], clamped to [0, L], or NULL: L each) at clean + clean_off[b] (device int64[B]
 * sample offsets: rows in place in a packed pool) or, clean_off == NULL, at clean + b ldc; the noise row likewise with m = noise_lens[b]
 * samples (clamped to [1, Ln]; NULL: Ln each), read cyclically from phase[b] (taken mod m; NULL: 0): v[i] = noise_b[(phase + i) mod m].
 *     c1 = c / (max|c| + EPS), c2 = c1 10^(target_db / 20) / (rms(c1) + EPS), the same for v1, v2 (rms over the n samples);
 *     rc, rv = rms(c2), rms(v2); segmental: over the samples of the windows [k win, min(n, (k + 1) win)) with
 *     10 log10(mean(v2^2) + EPS) > thresh_db (both EPS if there is none);
 *     v3 = v2 rc / 10^(snr_db / 20) / (rv + EPS), y = c2 + v3;  y, c2, v3 are scaled by 10^(level_db / 20) / (rms(y) + EPS) and, where
 *     max|y| > clip then, divided by max|y| / (clip - EPS).
 * par: device double[B][2] = (snr_db, level_db) of every row.  Everything being linear, idv_mix_gains reduces each row to
 * rows[b][IDV_MIX_ROW_FIELDS] (device doubles, the indices below): one wave per window writes max|c|, sum c^2, max|v|, sum v^2 in double
 * (fp32 squares are exact in double; 16-byte loads at any base alignment and row pitch), one workgroup per row combines them and decides
 * the active windows, a second window pass forms sum y0^2 and max|y0| of y0 = a c + b v from the samples themselves, a second row
 * kernel applies level and clip rule.  work: idv_mix_work_bytes(B, L, win) = 8 IDV_MIX_WIN_FIELDS B ceil(L / win) bytes, 8-byte aligned
 * (host only; -1 for refused arguments); afterwards it holds per row and window max|c|, sum c^2, max|v|, sum v^2, max|y0|, sum y0^2 (zeros
 * for the windows past a row's end).  idv_mix_write: noisy = float(g_clean c + g_noise v), clean_out = float(g_clean c), noise_out =
 * float(g_noise v), each ONE fp32 rounding of a double expression of the input samples, zeros from n to L - 1; the three outputs are
 * [B][ldy].  The place of a sample in every sum depends on its index in its window alone, nothing at or past lens[b] is read, no atomics:
 * a row's result does not depend on B, the other rows, the padding, the pitch or the alignment.
 * IDV_EINVAL (before any GPU work) for a NULL pointer (clean_off, noise_off, lens, noise_lens, phase may be NULL), B <= 0 or B > 65535,
 * L or Ln <= 0 or > 2^27, ldc < L / ldn < Ln where the offsets are NULL, win < 4, win > 2^27 or win % 4 != 0, a parameter that is not
 * finite, clip <= 2 EPS, segmental not 0 or 1, work_bytes too small, ldy < L, a misaligned pointer. */
#define IDV_MIX_WIN_FIELDS 6
#define IDV_MIX_ROW_FIELDS 16
#define IDV_MIX_MAX_C 0      /* max|c|, sum c^2, max|v|, sum v^2 over the row */
#define IDV_MIX_SUM_C2 1
#define IDV_MIX_MAX_V 2
#define IDV_MIX_SUM_V2 3
#define IDV_MIX_ACT_C2 4     /* sum c^2, sum v^2 and the number of samples of the active windows (the whole row in plain mode) */
#define IDV_MIX_ACT_V2 5
#define IDV_MIX_ACTIVE 6
#define IDV_MIX_A 7          /* y0 = a c + b v, the mixture before the level step */
#define IDV_MIX_B 8
#define IDV_MIX_SUM_Y2 9     /* sum y0^2, max|y0| */
#define IDV_MIX_MAX_Y 10
#define IDV_MIX_G_CLEAN 11   /* clean_out = g_clean c, noise_out = g_noise v */
#define IDV_MIX_G_NOISE 12
#define IDV_MIX_LEVEL_DB 13  /* 20 log10(rms(y) + EPS) of the final y */
#define IDV_MIX_CLIPPED 14   /* 1.0 where the clip rule applied */
#define IDV_MIX_LEN 15       /* n */
long long idv_mix_work_bytes(int B, int L, int win);
int idv_mix_gains(const float* clean, const long long* clean_off, long long ldc, const float* noise, const long long* noise_off,
                  long long ldn, const int* lens, const int* noise_lens, const int* phase, int B, int L, int Ln, const double* par,
                  int segmental, double target_db, double clip, int win, double thresh_db, void* work, long long work_bytes, double* rows,
                  void* stream);
int idv_mix_write(const float* clean, const long long* clean_off, long long ldc, const float* noise, const long long* noise_off,
                  long long ldn, const int* lens, const int* noise_lens, const int* phase, int B, int L, int Ln, const double* rows,
                  float* noisy, float* clean_out, float* noise_out, long long ldy, void* stream);

/* ---- reverberation (reverb.hip; dataset/reverb.py reverb / reverb_draw; an additive entry: IDV_ABI_VERSION is unchanged; DESIGN.md
 * 3.13).  Every row convolved with its own impulse response, the scipy.signal.fftconvolve(x, h)[:n] of the DNS-Challenge synthesizer's
 * add_pyreverb (tests/reverb_ref.py).  Row b: n = lens[b] samples (device int32[B], clamped to [0, L]; NULL: L each) at x + x_off[b]
 * (device int64[B] sample offsets: rows in place in a packed pool) or, x_off == NULL, at x + b ldx; K = taps[b] taps (device int32[B],
 * clamped to [1, Kmax]) at h + h_off[b] or, h_off == NULL, at h + b ldh; H = hist[b] (device int32[B], clamped to [0, 65535]; NULL: 0)
 * real samples x[-H .. -1] in front of the row's start, read in place: a segment cut from a longer recording carries the tail of what
 * precedes it, as if the whole recording had been convolved and then cut.
 *     y[b][i] = float( sum_{k < K} (double)h[k] (double)x[i - k] ),  x[j] = 0 for j < -H,   0 <= i < n;      y[b][i] = 0,  n <= i < L
 * Every product is exact in double, the sum is double, the result ONE fp32 rounding of it; y is [B][ldy].  Nothing at or past x[n],
 * before x[-H] or at or past h[K] is read.  A block-Toeplitz product on v_mfma_f64_16x16x4_f64: the place of a term in the sum of
 * output i follows from (i, K, H) of its row alone, not from B, the other rows, L, the pitches, the offsets or the alignment; no
 * atomics, no work buffer.
 * IDV_EINVAL (before any GPU work) for a NULL pointer (x_off, h_off, lens, hist may be NULL), B <= 0 or B > 65535, L <= 0 or L > 2^27,
 * Kmax <= 0 or Kmax > 65536, ldx < L / ldh < Kmax where the offsets are NULL, ldy < L, a misaligned pointer. */
int idv_reverb(const float* x, const long long* x_off, long long ldx, const float* h, const long long* h_off, long long ldh,
               const int* lens, const int* taps, const int* hist, int B, int L, int Kmax, float* y, long long ldy, void* stream);

/* ---- time-Winograd convs with two co tiles per workgroup (cgemm_tw.hip, cgemm_tw2.hip; additive entries: IDV_ABI_VERSION is
 * unchanged).  A layer with an even number of 32-channel co tiles runs workgroups of eight waves that stage the raw input rows once
 * for two co tiles; the outputs are bit-identical to the one-co-tile kernels (the train-mode moment sums within the rounding of a
 * reordered double sum).  The switch is a bit mask, read once from IDV_TW_PAIR in the environment. */
#define IDV_TW_PAIR_T_EVEN 1   /* transposed conv (idv_ctconv2d_tw_fwd), even-row phase */
#define IDV_TW_PAIR_T_ODD 2    /* transposed conv, odd-row phase */
#define IDV_TW_PAIR_CONV 4     /* conv (idv_cconv2d_tw_fwd) */
#define IDV_TW_PAIR_ALL 7
#define IDV_TW_PAIR_DEFAULT 7   /* the paired form is faster in all three */
/* mask >= 0: sets the switch (atomically; launches issued afterwards see it) and returns the previous value; mask < 0: returns it. */
int idv_tw_pair(int mask);
/* Number of paired kernel launches of this process so far; reset != 0 also sets the count back to 0. */
long long idv_tw_pair_launches(int reset);

/* ---- distinguisher of the adversarial decoder fine-tune (dis.hip; model/pvae_module.py distinguisher, model/nsvae_loss.py
 * adversarial_second_phase_loss, adversarial.py; additive entries: IDV_ABI_VERSION is unchanged).
 *
 * The real two-layer nn.LSTM(2 C F, hidden_size 1) of model/pvae_module.py:2319-2346 with h0 = c0 = 0, gate order i, f, g, o.  x is
 * the last dis_Encoder block's planar activation act[2][C][F][Jp], read in place: feature k = (c F + f) 2 + d of the reference's
 * [T, B, 2 C F] input is plane (d, c, f), frame t of row b is column b Tp + 1 + t; no other column is read.  wih0 [4][2 C F],
 * whh0 / wih1 / whh1 / b* [4]: the eight nn.LSTM tensors as they are.  y [B][T] fp32 = the layer-1 hidden state (the reference's
 * [B, T, 1] output).  Every sum is double in an order fixed by (k, t): y of a row does not depend on the other rows; no atomics.
 * save: idv_rlstm1_save_doubles(B, T) doubles that idv_rlstm1_bwd reads (activated gates, cell states, tanh(c) of both layers), or
 * NULL when no backward follows; scratch: idv_rlstm1_fwd_scratch_doubles(2 C F, Jp) doubles, free again when the call has run.
 * IDV_EINVAL (before any GPU work) for a NULL pointer (save may be NULL), C, F <= 0 or C F > 32768, B <= 0 or B > 65535, T <= 0 or
 * T > 2^20, Tp < T + 1, Jp < B Tp or not a multiple of 4, x not 16-byte aligned, another pointer not aligned to its element. */
long long idv_rlstm1_save_doubles(int B, int T);
long long idv_rlstm1_fwd_scratch_doubles(int K, int Jp);
long long idv_rlstm1_bwd_scratch_doubles(int K, int B, int Jp);
int idv_rlstm1_fwd(const float* x, int C, int F, int B, int T, int Tp, int Jp, const float* wih0, const float* whh0,
                   const float* bih0, const float* bhh0, const float* wih1, const float* whh1, const float* bih1,
                   const float* bhh1, double* save, double* scratch, float* y, void* stream);
/* Back-propagation through time of idv_rlstm1_fwd.  dy [B][T]; save: what the forward left; scratch:
 * idv_rlstm1_bwd_scratch_doubles(2 C F, B, Jp) doubles.  dx (may be NULL): act[2][C][F][Jp] gradient, every column of [0, Jp) written,
 * zeros wherever the column is not a frame (the planar invariant); dwih0 (may be NULL: a frozen distinguisher) [4][2 C F];
 * dsmall[28] = dW_hh0[4], db_ih0[4], db_hh0[4], dW_ih1[4], dW_hh1[4], db_ih1[4], db_hh1[4].  Per-row partial sums in double, added
 * over the rows b = 0, 1, ...; dW_ih0 summed along j in double, 1024-column tiles in ascending order.  Refusals as idv_rlstm1_fwd
 * (dx 16-byte aligned). */
int idv_rlstm1_bwd(const float* x, int C, int F, int B, int T, int Tp, int Jp, const float* dy, const float* wih0,
                   const float* whh0, const float* wih1, const float* whh1, const double* save, double* scratch,
                   float* dx, float* dwih0, float* dsmall, void* stream);
/* LSGAN terms of model/nsvae_loss.py:957-962, :982: out[0] = (sum_i (a[i] - 1)^2 + sum_i b[i]^2) / n, b == NULL: the first sum
 * alone.  Double sums in a fixed order, one fp32 rounding.  idv_lsgan_bwd: da[i] = gout[0] 2 (a[i] - 1) / n, db[i] = gout[0] 2 b[i] / n
 * (gout: device scalar; da or db may be NULL, not both).  IDV_EINVAL for a NULL a / out / gout, n <= 0 or n > 2^28, a misaligned
 * pointer. */
int idv_lsgan(const float* a, const float* b, long long n, float* out, void* stream);
int idv_lsgan_bwd(const float* a, const float* b, long long n, const float* gout, float* da, float* db, void* stream);

/* ---- clip assembly (assemble.hip; dataset/assemble.py assemble / activity / SignalPool.stats; additive entries: IDV_ABI_VERSION is
 * unchanged).  The definition is build_audio / activitydetector of the DNS-Challenge synthesizer restated
 * (tests/assemble_ref.py; parity with the package itself is unpinned).
 *
 * A candidate row r = b tries + t is count[r] <= IDV_ASM_MAX_PIECES pieces first[r] .. first[r] + count[r] - 1 of the piece arrays
 * (device, npieces entries each): piece i copies len[i] samples from pool + src[i] (int64 sample offsets) to positions dst[i] ..
 * dst[i] + len[i] - 1 of the row.  The pieces of a row are sorted by dst and do not overlap; positions no piece covers are +0.  A row
 * holds n = rowlen[r] positions (device int32, clamped to [0, samples]; NULL: samples each).  A piece that does not lie inside
 * [0, pool_n) or inside [0, n) is dropped whole: nothing outside a named piece, and nothing outside the pool, is ever read.
 *
 * idv_asm_activity, three launches: (a) one wave per win-sample window of every candidate: max|x| and sum x^2 in double into work
 * (idv_asm_work_bytes(B tries, samples, win) = 16 B tries ceil(samples / win) bytes, 8-byte aligned); (b) one workgroup per row b, for
 * each candidate in double: k = 10^(target_db / 20) / (sqrt(sum x^2 / n) + EPS), per window db = 20 log10(k^2 sum x^2 + EPS),
 * p = 1 / (1 + exp(1 - 0.2 db)), s_j = 0.8 p_j + 0.2 p_(j-1) where p_j > p_(j-1), else 0.05 p_j + 0.95 p_(j-1), p_(-1) = 0; the window is
 * active when s_j > energy_thresh.  rowstat[r][2] = max|x|, sum x^2; active[r], windows[r] = ceil(n / win) (int32);
 * activity[r] = active / windows (double, 0 for n = 0); chosen[b] = the first t with activity > min_activity and accepted[b] = 1, or,
 * when there is none, the t with the most active windows (the lowest on a tie) and accepted[b] = 0.
 * idv_asm_write: out[b][0 .. samples) = candidate chosen[b] (read on the device, clamped to [0, tries)) of row b, its pieces copied
 * bit for bit, +0 elsewhere; out is [B][ldo].
 * The order of every sum follows from a sample's index in its window and a window's index in its row alone; no atomics.
 * IDV_EINVAL (before any GPU work) for a NULL pointer (rowlen may be NULL), B <= 0, tries outside 1 .. IDV_ASM_MAX_TRIES, B tries >
 * 65535, samples <= 0 or > 2^27, win < 4, > 2^27 or no multiple of 4 (a window starts on a quad of its row), npieces <= 0 or > 2^30,
 * pool_n <= 0, work_bytes too small, ldo < samples, a non-finite parameter, a pointer not aligned to its element. */
#define IDV_ASM_MAX_PIECES 64
#define IDV_ASM_MAX_TRIES 16
#define IDV_ASM_WIN_FIELDS 2
long long idv_asm_work_bytes(int R, int samples, int win);
int idv_asm_activity(const float* pool, long long pool_n, const long long* src, const int* len, const int* dst, const int* first,
                     const int* count, int npieces, const int* rowlen, int B, int tries, int samples, int win, double target_db,
                     double energy_thresh, double min_activity, void* work, long long work_bytes, double* rowstat, int* active,
                     int* windows, double* activity, int* chosen, int* accepted, void* stream);
int idv_asm_write(const float* pool, long long pool_n, const long long* src, const int* len, const int* dst, const int* first,
                  const int* count, int npieces, const int* chosen, int B, int tries, int samples, float* out, long long ldo,
                  void* stream);

/* ---- real 3x3 convolution on the fp32 matrix cores and DNSMOS P.835 (dnsmos.hip; dnsmos.py, inference.compute_dnsmos / dnsmos_list;
 * additive entries: IDV_ABI_VERSION is unchanged).
 *
 * idv_conv3x3_fwd: y = ReLU(conv3x3(x, w) + bias), stride 1, zero padding 1, on v_mfma_f32_32x32x2_f32.  x is [N][H][W][Cin], y is
 * [N][H][W][Cout], or with pool != 0 the 2x2 / stride-2 maximum of that map, [N][H / 2][W / 2][Cout] (floor: an odd last row / column is
 * dropped); the un-pooled map is never written.  wp: idv_conv3x3_wfloats(Cin, Cout) floats that idv_conv3x3_pack made of w
 * [Cout][Cin][3][3].  One accumulator per output sums k = (chunk of 32 channels, tap ky 3 + kx, channel) in ascending order, starting
 * from 0; the bias is added last.  An output depends on its own image alone.  idv_conv3x3_tile(0 / 1): the rows / columns of output
 * pixels one workgroup owns.
 * idv_conv3x3_c1_fwd: the 1 -> C first layer on the vector ALU: f [N][H][W] -> y [N][H][W][C], w1 [C][9], one fmaf chain over the taps.
 * idv_conv3x3_c1_pool_fwd: the same layer with the 2x2 / stride-2 floor maximum behind it, y [N][H / 2][W / 2][C]: the bits of the pool of
 * idv_conv3x3_c1_fwd's map (the same device function), which is never written; H, W >= 2.
 * idv_conv3x3_c1_fused_fwd: idv_conv3x3_fwd applied to idv_conv3x3_c1_fwd(f) (C1 = its Cin) without the C1-channel map in memory: the
 * first layer is evaluated while a chunk is staged; the same bits as the two calls.
 * idv_conv3x3_gmax: x [N][P][C] -> out [N][C], the maximum over the P pixels.
 * IDV_EINVAL (before any GPU work) for a NULL pointer, N, H, W <= 0, H or W > 32768, Cin not in {32, 64, 128}, Cout not in {32, 64},
 * pool with H < 2 or W < 2, C outside 1 .. 1024 (c1) or no divisor of 256 (gmax), x not 16-byte aligned (idv_conv3x3_fwd), another pointer
 * not aligned to its element. */
int idv_conv3x3_tile(int which);
long long idv_conv3x3_wfloats(int Cin, int Cout);
int idv_conv3x3_pack(const float* w, int Cin, int Cout, float* packed, void* stream);
int idv_conv3x3_fwd(const float* x, const float* wp, const float* bias, int N, int H, int W, int Cin, int Cout, int pool, float* y,
                    void* stream);
int idv_conv3x3_c1_fwd(const float* f, const float* w1, const float* b1, int N, int H, int W, int C, float* y, void* stream);
int idv_conv3x3_c1_pool_fwd(const float* f, const float* w1, const float* b1, int N, int H, int W, int C, float* y, void* stream);
int idv_conv3x3_c1_fused_fwd(const float* f, const float* w1, const float* b1, int C1, const float* wp, const float* bias, int N, int H,
                             int W, int Cout, int pool, float* y, void* stream);
int idv_conv3x3_gmax(const float* x, int N, long long P, int C, float* out, void* stream);
/* idv_dnsmos_frontend: segment s = (row, start) = seg[2 s], seg[2 s + 1] (device int32) of the padded batch x [B][ldx]; its sample j is
 * x[row][(start + j) mod lengths[row]], so nothing at or past a row's length is read and the tiled clip is never built.  Frame t (900
 * of them) is samples 160 t .. 160 t + 319; re / im = frame x the two [161][320] matrices (mats: idv_dnsmos_frontend_wfloats() floats
 * made by idv_dnsmos_frontend_pack) on the fp32 matrix cores, k ascending; p = (sqrt(re re + im im))^2 with one fp32 rounding per
 * operation; feat [nseg][900][161] = float(ln(max(floor_p, p)) / ln_div), the logarithm and the quotient in double.  A segment whose row
 * is outside [0, B) or whose length is < 1 is all floor.
 * idv_dnsmos_head: g [N][64] -> raw [N][3]: dense 64 -> 128 ReLU, 128 -> 64 ReLU, 64 -> 3 (weights [in][out]), k-ascending fmaf chains.
 * idv_dnsmos_clip: out [B][6] (double) = the means over the segments first[b] .. first[b] + count[b] - 1 of raw [nseg][3] and of
 * poly_j(raw_j) (poly [3][4] double, highest power first, Horner in double); double sums in segment order.
 * IDV_EINVAL for a NULL pointer, B, nseg, N <= 0, nseg > 2^20, ldx <= 0, floor_p or ln_div not > 0, a pointer not aligned to its element. */
long long idv_dnsmos_frontend_wfloats(void);
int idv_dnsmos_frontend_pack(const float* re, const float* im, float* packed, void* stream);
int idv_dnsmos_frontend(const float* x, long long ldx, const int* lengths, int B, const int* seg, int nseg, const float* mats,
                        float floor_p, float ln_div, float* feat, void* stream);
int idv_dnsmos_head(const float* g, int N, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* raw, void* stream);
int idv_dnsmos_clip(const float* raw, int nseg, const int* first, const int* count, int B, const double* poly, double* out, void* stream);

/* ---- DNSMOS P.808, the P808_MOS column (p808.hip; dnsmos.py P808; additive entries: IDV_ABI_VERSION is unchanged).
 *
 * idv_p808_mel: segment s = (row, start) = seg[2 s], seg[2 s + 1] (device int32) of the padded batch x [B][ldx]; a[j] =
 * x[row][(start + j) mod lengths[row]] for 0 <= j < 144000, so nothing at or past a row's length is read.  Frame t (900 of them) is
 * a[160 t - 160 .. 160 t + 160], zero outside [0, 144000).  dft: [2][161][324] doubles, the windowed cosine table and the windowed
 * negated sine table, element [k][n], n = 321 .. 323 zero.  mel: [120][161] doubles.  re / im = frame x table, p = re re + im im,
 * S [nseg][900][120] = sum_k mel[m][k] p[t][k], all in double on v_mfma_f64_16x16x4_f64, k ascending in steps of 4; smax [nseg] = the
 * maximum of the segment's S.  work: idv_p808_mel_work_doubles(nseg) doubles (per-workgroup maxima; -1 for nseg outside 1 .. 2^20).
 * No atomics; a segment's bits do not depend on the other segments.  A segment whose row is outside [0, B) or whose length is < 1
 * is all zero.
 * idv_p808_db: feat [nseg][per] (float) = ((max(ls, -80) + 40) / 40), ls = 10 log10(max(1e-10, S)) - 10 log10(max(1e-10, smax[s])) in
 * double, rounded once (librosa power_to_db with ref = max, top_db = 80: the largest ls is 0).
 * idv_p808_head: g [N][64] -> raw [N]: dense 64 -> 64 ReLU, 64 -> 64 ReLU, 64 -> 1 (weights [in][out]), k-ascending fmaf chains.
 * idv_p808_clip: out [B] (double) = the mean over the segments first[b] .. first[b] + count[b] - 1 of raw [nseg], a double sum in order.
 * IDV_EINVAL (before any GPU work) for a NULL pointer, B, nseg, N <= 0, nseg > 2^20, ldx <= 0, per outside 1 .. 2^31, a pointer not
 * aligned to its element. */
long long idv_p808_mel_work_doubles(int nseg);
int idv_p808_mel(const float* x, long long ldx, const int* lengths, int B, const int* seg, int nseg, const double* dft, const double* mel,
                 double* S, double* smax, double* work, void* stream);
int idv_p808_db(const double* S, const double* smax, int nseg, long long per, float* feat, void* stream);
int idv_p808_head(const float* g, int N, const float* w0, const float* b0, const float* w1, const float* b1, const float* w2,
                  const float* b2, float* raw, void* stream);
int idv_p808_clip(const float* raw, int nseg, const int* first, const int* count, int B, double* out, void* stream);

/* ---- BSS-eval SDR of a padded batch (sdr.hip; inference.compute_sdr / score_list; additive entries: IDV_ABI_VERSION is unchanged;
 * DESIGN.md 3.18).  The signal-to-distortion ratio of bss_eval_sources for one source with a K-tap distortion filter: with s = ref row,
 * e = est row, both zero outside [0, n), n = lens[b]:
 *   r[k] = sum_i s[i] s[i + k], d[k] = sum_i s[i] e[i + k] (k < K);  G c = d, G[i][j] = r[|i - j|];
 *   p[i] = sum_k c[k] s[i - k], err[i] = e[i] - p[i] (i < n + K - 1);  out[b] = float(10 log10(sum p^2 / sum err^2)),
 * every sum in double.  ref, est: rows at pitch ref_ld / est_ld >= Lmax; lens: device int32[B], samples per row (clamped to Lmax), or
 * NULL: every row has Lmax (<= 2^27) samples.  K: a multiple of 16 in 16 .. 512.  Nothing at or past lens[b] is read and row b's
 * result does not depend on B, on the other rows, on the pitches or on the padding.  Special rows: NaN for a silent reference
 * (r[0] == 0) and for a solve that meets a non-positive prediction error (a numerically singular G); -inf for sum p^2 == 0 (a silent
 * estimate); +inf for sum err^2 == 0.  details (may be NULL): double [B][2] = (sum p^2, sum err^2), NaN for a NaN row; filt (may be NULL):
 * double [B][K] = c, NaN for a NaN row.  work: idv_sdr_work_bytes(B, Lmax, K) bytes, 16-byte aligned:
 *   8 B (2 K T1 + K + 1 + 2 T3),  T1 = ceil(((Lmax + 14) / 16 + 1) / 256),  T3 = ceil((Lmax + K - 1) / 4096)
 * (the per-tile lag sums, c, a status word and the per-tile energies of each row); -1 for what idv_sdr refuses.  No allocation, no
 * atomics.  IDV_EINVAL (before any GPU work) for a NULL ref / est / work / out, B outside 1 .. 65535, Lmax outside 1 .. 2^27, a K as
 * above, a pitch below Lmax, work_bytes too small, work not 16-byte aligned, details / filt not 8-byte aligned. */
long long idv_sdr_work_bytes(int B, int Lmax, int K);
int idv_sdr(const float* ref, long long ref_ld, const float* est, long long est_ld, const int* lens, int B, int Lmax, int K, void* work,
            long long work_bytes, float* out, double* details, double* filt, void* stream);

/* ---- BSS-eval SDR, SIR and SAR of a padded batch with two sources (bss.hip; inference.compute_bss / score_list; additive entries:
 * IDV_ABI_VERSION is unchanged).  bss_eval_sources for the target s = ref row and ONE interferer v = interf row, read
 * for the target, with K-tap distortion filters; y = est row, all zero outside [0, n), n = lens[b]:
 *   x_ab[k] = sum_i a[i] b[i + k] (a, b in {s, v}, |k| < K),  d_a[k] = sum_i a[i] y[i + k] (0 <= k < K)
 *   G_ss c = d_s;   [G_ss G_sv; G_vs G_vv] [C_s; C_v] = [d_s; d_v],   G_ab[i][j] = x_ab[i - j]
 *   p1 = c * s,  pall = C_s * s + C_v * v  (i < n + K - 1)
 *   out[b] = float(10 log10 of) ( sum p1^2 / sum (y - p1)^2,  sum p1^2 / sum (pall - p1)^2,  sum pall^2 / sum (y - pall)^2 ) = (SDR, SIR, SAR),
 * every sum in double.  The SDR column, c and its two sums are idv_sdr's, bit for bit.  ref, interf, est: rows at pitch ref_ld /
 * interf_ld / est_ld >= Lmax; lens: device int32[B], samples per row (clamped to Lmax), or NULL: every row has Lmax (<= 2^27) samples.
 * K: a multiple of 16 in 16 .. 512.  Nothing at or past lens[b] is read and row b's result does not depend on B, on the other rows, on
 * the pitches or on the padding.  Each ratio: -inf for a zero numerator, otherwise +inf for a zero denominator.  Special rows: all
 * three NaN for a silent reference (and where idv_sdr gives NaN); SDR as idv_sdr gives it and SIR = SAR = NaN for a silent interferer
 * (x_vv[0] == 0), for n <= K (2 K unknowns, n + K - 1 equations: G is singular whatever the signals) and for a solve that meets an
 * error matrix that is not positive definite (a numerically singular G, e.g. v = 2 s).  Rows shorter than about 2 K are overfitted:
 * the joint filter explains nearly everything.  details (may be NULL): double [B][5] = (sum p1^2, sum (y - p1)^2, sum (pall - p1)^2,
 * sum pall^2, sum (y - pall)^2), the first two as idv_sdr gives them, the last three NaN where SIR and SAR are NaN by the special
 * rows; filt (may be NULL): double [B][2][K] = C_s, C_v, NaN for such a row.  work: idv_bss_work_bytes(B, Lmax, K) bytes, 16-byte aligned:
 *   8 (B (8 K T1 + 4 K + 4 + 5 T3) + (B + 1) / 2),  T1 = ceil(((Lmax + 14) / 16 + 1) / 256),  T3 = ceil((Lmax + K - 1) / 4096)
 * (idv_sdr's own work, its values, sums and filter, the six per-tile lag sums, C, a status word and the three per-tile energies of
 * each row); -1 for what idv_bss refuses.  No allocation, no atomics.  IDV_EINVAL (before any GPU work) for a NULL ref / interf / est /
 * work / out, B outside 1 .. 65535, Lmax outside 1 .. 2^27, a K as above, a pitch below Lmax, work_bytes too small, work not 16-byte
 * aligned, details / filt not 8-byte aligned, ref / interf / est / lens / out not 4-byte aligned. */
long long idv_bss_work_bytes(int B, int Lmax, int K);
int idv_bss(const float* ref, long long ref_ld, const float* interf, long long interf_ld, const float* est, long long est_ld,
            const int* lens, int B, int Lmax, int K, void* work, long long work_bytes, float* out, double* details, double* filt,
            void* stream);

/* ---- image-source impulse responses of rectangular rooms (ism.hip; dataset/rir.py shoebox_rir, RirPool.shoebox; additive entries:
 * IDV_ABI_VERSION is unchanged).  Allen & Berkley's method as tests/ism_ref.py restates it.  Room b is the record
 * geom[b][IDV_ISM_FIELDS] (device doubles, the indices below): image (m, q) of axis a lies at p = 2 m L + (1 - 2 q) s - r, was
 * reflected e0 = |m - q| times at the wall at 0 and e1 = |m| times at the wall at L, g = beta0^e0 beta1^e1 (x^0 = 1); d = |p|,
 * A = gx gy gz / (4 pi d), tau = d fs / c, n_i = rint(tau), f = tau - n_i, u = n - tau:
 *   h[b][n] = float( sum_i A sinc(u) (1 + cos(2 pi u / 81)) / 2 ),  |u| < 40.5,  0 <= n < taps[b]
 *   sinc(0) = 1,  sinc(u) = (-1)^(n - n_i + 1) sin(pi f) / (pi u)
 * over the images with sum_a (e0 + e1) <= max_order[b] (device int32[B]; NULL: every image) and A != 0, every sum in double in an
 * order that follows from the room and n alone.  taps: device int32[B], clamped to 1 .. Kmax; row b gets its taps[b] samples and
 * zeros from there to Kmax; nothing else of h is written.  Row b does not depend on B, on the other rooms, on Kmax, on taps[b] (a
 * shorter response is the beginning of a longer one) or on ldh.  A record that cannot be walked (a value that is not finite, L, fs or
 * c not positive, more than 8192 images along an axis within a tile's reach) gives a row of NaN.  work: idv_ism_work_bytes(B, Kmax) =
 * 16 B ceil(Kmax / 64) bytes, 8-byte aligned: long long [B][ceil(Kmax / 64)][2], per tile of 64 samples the images summed into it and
 * those of them it owns (rint(tau) in the tile, or past it for the row's last tile: the sum over a row's tiles is the row's image
 * count); zeros for the tiles at or past taps[b]; -1 for what idv_ism_rir refuses.  No allocation, no atomics.
 * IDV_EINVAL (before any GPU work) for a NULL geom / taps / h / work, B outside 1 .. 65535, Kmax outside 1 .. 65536, ldh < Kmax,
 * work_bytes too small, geom / work not 8-byte aligned, taps / max_order / h not 4-byte aligned.
 * idv_ism_peaks: peaks[b] (device int32) = the index of max|h[b][n]| over n < taps[b] (clamped to 1 .. min(ldh, 65536)), the first on
 * ties.  IDV_EINVAL for a NULL h / taps / peaks, B outside 1 .. 65535, ldh < 1, a pointer not 4-byte aligned. */
#define IDV_ISM_FIELDS 17
#define IDV_ISM_LX 0         /* the room's size, metres */
#define IDV_ISM_LY 1
#define IDV_ISM_LZ 2
#define IDV_ISM_SX 3         /* the source */
#define IDV_ISM_SY 4
#define IDV_ISM_SZ 5
#define IDV_ISM_RX 6         /* the microphone */
#define IDV_ISM_RY 7
#define IDV_ISM_RZ 8
#define IDV_ISM_BETA 9       /* beta[a][w] at IDV_ISM_BETA + 2 a + w: the wall at 0 (w = 0) and at L (w = 1) of axis a */
#define IDV_ISM_FS 15        /* samples per second */
#define IDV_ISM_C 16         /* metres per second */
long long idv_ism_work_bytes(int B, int Kmax);
int idv_ism_rir(const double* geom, const int* taps, const int* max_order, int B, int Kmax, float* h, long long ldh, void* work,
                long long work_bytes, void* stream);
int idv_ism_peaks(const float* h, long long ldh, const int* taps, int B, int* peaks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
