"""The adversarial decoder fine-tune step (reference: i_dccrn_vae/nsvae_dccrn/train_second_phase_adversarial.py:290-320 and its
validation pass :351-370) on the drop-in modules: frozen noisy encoder (eval), decoder with repeated real skips (train), the LSGAN
distinguisher of model/pvae_module.py and the losses of model/nsvae_loss.adversarial_second_phase_loss.

    step = AdversarialFineTune(noisy_encoder, decoder, speech_distin, optimizer_noisy_clean_de, optimizer_speech_dis, d_step=2)
    gen_loss, loss_recon, loss_dis_gen, dist_loss = step.step(noisy_batch, clean_batch)

The trainer loop, logging, schedulers and checkpoints stay the caller's (utils/checkpoint.py is role-generic).
"""
from __future__ import annotations

import torch

from .model.nsvae_loss import adversarial_second_phase_loss


class AdversarialFineTune:
    """One object per training run; ``step`` counts the iterations, so the distinguisher is updated on every ``d_step``-th call
    (iteration 0 included) and the decoder on every call.

    ``skip_dis_grads_in_g``: the generator update back-propagates THROUGH the distinguisher into the decoder.  The reference also
    accumulates that loss's gradients of the distinguisher's own parameters, and zeroes them before they are ever used (the next
    distinguisher update starts with ``zero_grad``).  With the switch on the distinguisher's parameters are frozen for the duration
    of the generator's forward and backward, so its weight-gradient contractions -- the most expensive backward kernels of a conv
    block, and dW_ih0 of the LSTM -- are skipped through the frozen-layer path; the decoder's gradients and every distinguisher
    update are bit-identical either way."""

    def __init__(self, noisy_encoder, decoder, distinguisher, opt_decoder, opt_dis, d_step=2, skip_dis_grads_in_g=True):
        if int(d_step) < 1:
            raise ValueError("d_step must be >= 1")
        self.noisy_encoder, self.decoder, self.distinguisher = noisy_encoder, decoder, distinguisher
        self.opt_decoder, self.opt_dis = opt_decoder, opt_dis
        self.d_step = int(d_step)
        self.skip_dis_grads_in_g = bool(skip_dis_grads_in_g)
        self.loss = adversarial_second_phase_loss(getattr(noisy_encoder, "latent_num", 1))
        self.iteration = 0
        self.dist_loss = None                      # the last computed one, as the script logs it
        self.last_recon = None                     # recon_sig_clean [B * ns, L'] of the last step, detached

    def _generate(self, noisy, clean, eps, train):
        with torch.no_grad():
            r = self.noisy_encoder(noisy, train=False, eps=eps)
        z, skiper, C, F, stft_x = r[0], r[8], r[9], r[10], r[11]
        recon, _ = self.decoder(stft_x, z, skiper, C, F, train=train, pad='sig')
        bs, time_len = clean.shape
        ns = recon.shape[0] // bs
        clean_rep = clean.float().unsqueeze(1).repeat(1, ns, 1).view(bs * ns, time_len)
        return recon, clean_rep

    def step(self, noisy, clean, eps=None):
        """-> (gen_loss, loss_recon, loss_dis_gen, dist_loss), detached device scalars."""
        D = self.distinguisher
        with torch.enable_grad():
            recon, clean_rep = self._generate(noisy, clean, eps, True)
            self.last_recon = recon.detach()
            if self.iteration % self.d_step == 0:
                dist_true = D(clean_rep, train=True)
                dist_est = D(recon.detach(), train=True)
                dist_loss = self.loss.distinguisher_loss(dist_true, dist_est, None, None)
                self.opt_dis.zero_grad()
                dist_loss.backward()
                self.opt_dis.step()
                self.dist_loss = dist_loss.detach()
            frozen = [q for q in D.parameters() if q.requires_grad] if self.skip_dis_grads_in_g else []
            try:
                for q in frozen:
                    q.requires_grad_(False)
                dist_gen = D(recon, train=True)
                gen_loss, loss_recon, loss_dis_gen = self.loss.generator_loss(clean_rep, recon, dist_gen, None, None, None)
                self.opt_decoder.zero_grad()
                gen_loss.backward()
            finally:
                for q in frozen:
                    q.requires_grad_(True)
            self.opt_decoder.step()
        self.iteration += 1
        return gen_loss.detach(), loss_recon.detach(), loss_dis_gen.detach(), self.dist_loss

    @torch.no_grad()
    def validate(self, noisy, clean, eps=None):
        """The validation pass of the script: decoder in eval mode, the distinguisher still with train=True (batch moments, running
        buffers overwritten), no graph -> (gen_loss, loss_recon, loss_dis_gen, dist_loss)."""
        D = self.distinguisher
        recon, clean_rep = self._generate(noisy, clean, eps, False)
        dist_true = D(clean_rep, train=True)
        dist_est = D(recon, train=True)
        dist_loss = self.loss.distinguisher_loss(dist_true, dist_est, None, None)
        gen_loss, loss_recon, loss_dis_gen = self.loss.generator_loss(clean_rep, recon, dist_est, None, None, None)
        return gen_loss, loss_recon, loss_dis_gen, dist_loss
