"""``snn_model.vae_model`` of the MI355X build: the spiking VQ-VAE inference path.

Counterpart of R/snn_model/vae_model.py:22-196 -- same class names, constructor signatures, attribute paths
(``model.encoder``, ``model.vq_layer.quantize/poisson``, ``model.decoder``, ``model.memout``) and ``state_dict``
keys, so R/main.py's test/sampling section runs against it unchanged.  The eval branches run on
``libspkdiff.so`` (fused Conv+BN+LIF kernels, VQ argmin kernel).  The training branches (VQ / commitment / PSP /
reconstruction losses, straight-through estimator: vae_model.py:61-85,189-196) run in train()
mode with autograd: native convolutions forward and backward (``csrc/conv_train.hip``, fp32 matrix cores; shapes it does not
cover take the framework's operator), native BatchNorm+LIF block tails (``spk_bn_lif_train_*``), and the VectorQuantizer's
read-out / code search / losses, the PSP losses and the reconstruction loss as fused operators (``csrc/vq_train.hip``).

``SNN_VAE`` (R/snn_model/vae_model.py:198-546, the FSVAE-style baseline) runs its eval forward, ``encode``, ``decode`` and
``sample`` on ``csrc/svae.hip``: Linear + LIF pairs fused, each autoregressive Bernoulli loop one launch.  Its training
branch (MMD + reconstruction losses) runs with autograd on ``csrc/svae_train.hip``: Linear + surrogate LIF forward and
backward, the no-grad prefix passes of each Bernoulli loop in one launch, the gather and MMD loss fused; the encoder and
decoder take SNN_VQVAE's training path.

``SNN_VQVAE_uni`` (R/snn_model/vae_model.py:674-801) is SNN_VQVAE with ``VectorQuantizer_uni``: the same kernels, plus the
codebook-usage statistic the quantizer computes and prints on every call, one launch of ``csrc/vq_usage.hip``.

``VQVAE`` (R/snn_model/vae_model.py:548-672, the plain-CNN baseline) runs its eval forward, ``encode_images`` and
``decode_tokens`` on ``csrc/ann_vqvae.hip``: encoder and code search one launch, decoder two.  In train() mode the iteration runs
on ``csrc/conv_train.hip`` (the six convolutions, the ReLU an epilogue of the launches around it) and
``csrc/ann_vqvae_train.hip`` (quantiser and losses) as one autograd node.  Its modules are the reference's torch operators; they
serve CPU tensors, hooks, other dtypes and shapes, codebooks beyond the training quantiser's (K > 862), images that want a
gradient, and ``fused_train = False``.

Re-exported names match what ``from snn_model.vae_model import *`` gives R/main.py (``functional`` in particular,
R/main.py:101-107,317).
"""
import random

import torch
import torch.nn as nn
import torch.nn.functional as F

from spikingjelly.activation_based import neuron, functional, layer, surrogate, monitor  # noqa: F401
from spikingjelly import visualizing  # noqa: F401

from spkdiff import ops
from spkdiff.fused import FusedSequential, conv_geometry, has_hooks, derived_epoch
from spkdiff.ops import IN_PTC, IN_SEQ, IN_TINV

from .snn_layers import *  # noqa: F401,F403
from .snn_layers import MembraneOutputLayer, PSP


def _training_oos(what):
    raise NotImplementedError(f'spkdiff: {what} is a training branch of the reference, outside the inference hot '
                              'path (SURVEY.md §8f); call .eval()')


class VectorQuantizer(nn.Module):
    def __init__(self, embedding_dim, num_embeddings, commitment_cost, n_steps: int = 16):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings
        self.commitment_cost = commitment_cost
        self.memout = MembraneOutputLayer(n_steps)
        self.num_step = n_steps
        self.psp = PSP()
        self.alpha = nn.Parameter(torch.tensor(0.5))
        self.embeddings = nn.Embedding(self.num_embeddings, self.embedding_dim)
        self.fused_train = True              # training branch: ops.VQTrainFunction (False: the same algebra op by op through autograd)
        self.poisson = FusedSequential(
            layer.Conv2d(in_channels=embedding_dim, out_channels=embedding_dim, kernel_size=1),
            layer.BatchNorm2d(embedding_dim),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),
        )

    # -- fused pieces, shared with SNN_VQVAE's end-to-end path ------------------------------------------------
    def _quantize_ptc(self, z_ptc, want_xm=False, want_zq=True):
        """z_ptc u8 [B,h,w,T,D] -> (indices int64 [B*h*w], quantized fp32 [B,D,h,w] or None)."""
        idx, zq, xm = ops.vq_readout_argmin(z_ptc, self.memout.coef.flatten(), self.alpha, self.embeddings.weight,
                                            want_zq=want_zq, want_xm=want_xm)
        return (idx, zq, xm) if want_xm else (idx, zq)

    def _spike_generator(self, zq, T, final='f32'):
        """'adaptive spike generator': repeat(T) + poisson, the repeat folded into the kernel (same frame each step)."""
        return self.poisson.run(zq, IN_TINV, final=final, T=T)

    def forward(self, x):
        # x: (T,N,C,H,W) spikes of the encoder
        if self.training:
            return self._train_forward(x)
        T = x.shape[0]
        idx, zq = self._quantize_ptc(ops.spikes_to_ptc(x))
        if has_hooks(self.poisson):                   # hooks on the spike generator's layers: run it child by child
            return self.poisson(torch.unsqueeze(zq, dim=0).repeat(T, 1, 1, 1, 1)), idx
        quantized = self._spike_generator(zq, T)['f32']
        return quantized, idx

    def _train_forward(self, x):
        """Training branch, R/snn_model/vae_model.py:40-47,61-85: read-out, nearest code, VQ and
        commitment losses, straight-through estimator, spike generator, PSP losses.  Native pieces: the membrane read-out
        (spk_memout_fwd), the code search (spk_vq_argmin), the spike generator's BatchNorm+LIF (spk_bn_lif_train_*) and
        the PSP filter (spk_psp); the remaining element-wise algebra and the embedding gradient are torch plumbing."""
        quantized, loss, _ = self._train_forward_idx(x)
        return quantized, loss

    def _train_forward_idx(self, x):
        """_train_forward, also returning the code indices int64 [B*h*w]."""
        if not torch.is_grad_enabled():
            _training_oos('VectorQuantizer.forward in train() mode without autograd')
        T = x.shape[0]
        if (self.fused_train and x.is_cuda and x.dtype == torch.float32 and x.dim() == 5 and T == self.memout.coef.numel()
                and self.embedding_dim <= ops.VQ_TRAIN_MAX_D):       # (spk_vq_train_bwd keeps a code vector in registers: D <= 64)
            # read-out, code search, q / e latent losses, straight-through value: three native launches forward, one backward
            # (ops.VQTrainFunction; the module-by-module algebra below is the same arithmetic through autograd)
            quantized, loss_1 = ops.VQTrainFunction.apply(x, self.memout.coef, self.alpha, self.embeddings.weight,
                                                          self.commitment_cost)
            encoding_indices = getattr(quantized.grad_fn, "indices", None)     # (the code search's result, kept on the autograd node)
        else:
            x_memout = (1 - self.alpha) * self.memout(x) + self.alpha * torch.sum(x, dim=0) / self.num_step
            x_memout = x_memout.permute(0, 2, 3, 1).contiguous()
            flat_x = x_memout.reshape(-1, self.embedding_dim)
            encoding_indices = self.get_code_indices(flat_x.detach())
            quantized = F.embedding(encoding_indices, self.embeddings.weight).view_as(x_memout)
            q_latent_loss = F.mse_loss(quantized, x_memout.detach())
            e_latent_loss = F.mse_loss(x_memout, quantized.detach())
            loss_1 = q_latent_loss + self.commitment_cost * e_latent_loss
            quantized = x_memout + (quantized - x_memout).detach()           # straight-through estimator
            quantized = quantized.permute(0, 3, 1, 2).contiguous()
        quantized = torch.unsqueeze(quantized, dim=0).repeat(T, 1, 1, 1, 1)
        quantized = self.poisson(quantized)
        if self.fused_train and quantized.is_cuda and quantized.shape == x.shape and T <= 16:
            # both PSP filters, both mean squares and their backward: one launch each way (ops.PSPLossFunction)
            loss_2 = ops.PSPLossFunction.apply(quantized, x, self.commitment_cost, float(self.psp.tau_s))
        else:
            # psp(x.detach()) and psp(x).detach() are the same numbers: each filter runs once
            pq, px = self.psp(quantized), self.psp(x)
            q_latent_loss_2 = torch.mean((pq - px.detach()) ** 2)
            e_latent_loss_2 = torch.mean((pq.detach() - px) ** 2)
            loss_2 = q_latent_loss_2 + self.commitment_cost * e_latent_loss_2
        return quantized, loss_1 + loss_2, encoding_indices

    def get_code_indices(self, flat_x):
        """argmin_k ||x - e_k||^2 for rows of flat_x [N, D] (R/snn_model/vae_model.py:87-95)."""
        return ops.vq_argmin(flat_x, self.embeddings.weight)

    def quantize(self, encoding_indices):
        """Returns embedding tensor for a batch of indices."""
        return ops.embedding(encoding_indices, self.embeddings.weight)


class Encoder(nn.Module):
    """Encoder of VQ-VAE"""

    def __init__(self, in_dim=1, latent_dim=16):
        super().__init__()
        self.in_dim = in_dim
        self.latent_dim = latent_dim
        self.snn_convs = FusedSequential(
            layer.Conv2d(in_channels=in_dim, out_channels=32, kernel_size=3, stride=2, padding=1),
            layer.BatchNorm2d(32),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),

            layer.Conv2d(in_channels=32, out_channels=64, kernel_size=3, stride=2, padding=1),
            layer.BatchNorm2d(64),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),

            layer.Conv2d(in_channels=64, out_channels=latent_dim, kernel_size=1, stride=1, padding=0),
            layer.BatchNorm2d(latent_dim),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),
        )

    def forward(self, x):
        # [t, b, c, h, w]
        return self.snn_convs(x)


class Decoder(nn.Module):
    """Decoder of VQ-VAE"""

    def __init__(self, out_dim=1, latent_dim=16):
        super().__init__()
        self.out_dim = out_dim
        self.latent_dim = latent_dim
        self.snn_convs = FusedSequential(
            layer.ConvTranspose2d(in_channels=latent_dim, out_channels=64, kernel_size=3, stride=2, padding=1,
                                  output_padding=1),
            layer.BatchNorm2d(64),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),

            layer.ConvTranspose2d(in_channels=64, out_channels=32, kernel_size=3, stride=2, padding=1,
                                  output_padding=1),
            layer.BatchNorm2d(32),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),

            layer.ConvTranspose2d(in_channels=32, out_channels=out_dim, kernel_size=3, stride=1, padding=1,
                                  output_padding=0),
        )

    def forward(self, x):
        # [t, b, c, h, w]
        return self.snn_convs(x)


SPIKEGEN_BY_TOKEN = True     # decode_tokens: the spike generator as a per-token pattern table (False: embedding + generator + packing launches)


class SNN_VQVAE(nn.Module):
    """VQ-VAE"""

    def __init__(self, in_dim, embedding_dim, num_embeddings, data_variance, commitment_cost=0.25,
                 n_steps: int = 16):
        super().__init__()
        self.in_dim = in_dim
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings
        self.data_variance = data_variance

        self.encoder = Encoder(in_dim, embedding_dim)
        self.vq_layer = VectorQuantizer(embedding_dim, num_embeddings, commitment_cost, n_steps)
        self.decoder = Decoder(in_dim, embedding_dim)
        self.memout = MembraneOutputLayer(n_steps)

    def forward(self, x, image):
        # x: [t, B, C, H, W]
        if self.training:
            # training branch, R/snn_model/vae_model.py:189-196
            if not torch.is_grad_enabled():
                _training_oos('SNN_VQVAE.forward in train() mode without autograd')
            z = self.encoder(x)
            e, e_q_loss = self.vq_layer(z)
            real_recon_loss = self._train_recon_loss(self.decoder(e), image)
            return e_q_loss, real_recon_loss / self.data_variance, real_recon_loss
        T = x.shape[0]
        enc = self.encoder.snn_convs
        dec = self.decoder.snn_convs
        if enc._fusable(enc._blocks()) and dec._fusable(dec._blocks()) and T <= ops.MAX_T and not has_hooks(self):
            # end-to-end fused: spikes stay u8 PTC between encoder, VQ, spike generator and decoder
            z_ptc = enc.run(x, IN_SEQ, final='ptc')['ptc']
            idx, zq = self.vq_layer._quantize_ptc(z_ptc)
            e = self.vq_layer._spike_generator(zq, T, final='both')
            x_recon = dec.run(e['ptc'], IN_PTC, final='memout', coef=self.memout.coef.flatten(),
                              apply_tanh=True)['f32']
            return e['f32'], x_recon, idx
        z = self.encoder(x)
        e, enco = self.vq_layer(z)
        x_recon = self.decoder(e)
        x_recon = torch.tanh(self.memout(x_recon))
        return e, x_recon, enco

    def _train_recon_loss(self, y, image):
        """mse_loss(tanh(memout(decoder output y)), image) of the training branch (R/snn_model/vae_model.py:192-194)."""
        if self.vq_layer.fused_train and y.is_cuda and y.shape[1:] == image.shape and image.dtype == torch.float32:
            return ops.ReconLossFunction.apply(y, self.memout.coef, image)      # read-out + tanh + mse: one launch
        x_recon = torch.tanh(self.memout(y))
        return F.mse_loss(x_recon, image)

    # ---- convenience entry points of the MI355X build (not in the reference) -----------------------------------
    @torch.no_grad()
    def encode_images(self, images, T=16):
        """images [B,C,H,W] already normalised (images - 0.5) -> code indices [B,h,w]; the T-fold repeat of
        R/main.py:309 / vq_diffusion.py:30 is folded into the first kernel (time-invariant input)."""
        z_ptc = self.encoder.snn_convs.run(images, IN_TINV, final='ptc', T=T, stateful=False)['ptc']
        idx, _ = self.vq_layer._quantize_ptc(z_ptc, want_zq=False)      # (indices only: no [B,D,h,w] gather)
        L = images.shape[-1] // 4
        return idx.reshape(images.shape[0], L, L)

    @torch.no_grad()
    def encode_features(self, images, T=16):
        """images [B,C,H,W] already normalised (images - 0.5) -> fp32 [B, h*w*D]: the encoder's read-out the quantiser searches
        on (``_quantize_ptc(want_xm=True)``: position-major, D values per position), flattened per image -- the feature space of
        ``spkdiff.evaluate.sample_quality_eval``.  Same launches as ``encode_images``."""
        z_ptc = self.encoder.snn_convs.run(images, IN_TINV, final='ptc', T=T, stateful=False)['ptc']
        _, _, xm = self.vq_layer._quantize_ptc(z_ptc, want_xm=True, want_zq=False)
        return xm.reshape(images.shape[0], -1)

    def _decoder_takes_s32(self, T, h, w):
        """Will the decoder's first layer take nibble-packed spikes (the fp6 transposed-convolution kernel, csrc/vae_fp6.hip)?"""
        blocks = self.decoder.snn_convs._blocks()
        if blocks is None or len(blocks) != 3 or T != 16:
            return False
        conv = blocks[0][0]
        return FusedSequential._vae_kind(conv, conv_geometry(conv), T, h, w) == ops.VAE_OUT_S32

    @torch.no_grad()
    def decode_tokens(self, tokens, T=16, want_u8=True):
        """tokens int64 [B,h,w] -> (pred fp32 [B,C,H,W] in (-1,1), uint8 image): the glue of R/main.py:388-401 as
        three launches (embedding gather, spike generator, fused decoder + read-out + tanh + uint8)."""
        B, h, w = tokens.shape
        e_ptc = None
        if SPIKEGEN_BY_TOKEN and self._decoder_takes_s32(T, h, w):
            # embedding + spike generator + nibble packing as a per-token pattern table (csrc/conv_direct.hip, spk_spikegen_tokens_s32)
            e_ptc = self.vq_layer.poisson.tokens_to_s32(tokens, self.vq_layer.embeddings.weight, T=T,
                                                        epoch=derived_epoch(self.vq_layer))
        if e_ptc is None:
            zq = ops.embedding(tokens, self.vq_layer.embeddings.weight, nchw_hw=(h, w))
            e_ptc = self.vq_layer.poisson.run(zq, IN_TINV, final='ptc', T=T, stateful=False)['ptc']
        r = self.decoder.snn_convs.run(e_ptc, IN_PTC, final='memout', coef=self.memout.coef.flatten(), apply_tanh=True,
                                       want_u8=want_u8, stateful=False)
        return r['f32'], r['u8']


# ---- SNN_VAE: the FSVAE-style baseline (R/snn_model/vae_model.py:198-546) --------------------------------------------------
# Every Linear + LIFNode pair runs fused (spk_linear_lif_fwd) and each autoregressive Bernoulli loop is ONE launch
# (spk_svae_ar_fwd); the modules keep the reference's children, state_dict keys and LIFNode states, so reset_net and
# load_state_dict behave as there.  The random indices are drawn on the host with the reference's calls in its order.

def _svae_node_v(node, B, n, device):
    """The LIFNode's state as the [B, n] fp32 buffer the kernels update in place (the float reset value expanded on first
    use, SJ/activation_based/neuron.py:260-263)."""
    if not (node.v_reset == 0.0 and node.v_threshold == 1.0 and node.tau == 2.0 and node.decay_input
            and not node.store_v_seq):
        raise NotImplementedError('spkdiff: the SNN_VAE kernels implement the default LIFNode (tau 2, v_th 1, hard reset 0, '
                                  'decay_input)')
    v = node.v
    if isinstance(v, float):
        v = torch.full((B, n), v, dtype=torch.float32, device=device)
    elif v.shape != (B, n) or v.dtype != torch.float32 or v.device != device or not v.is_contiguous():
        raise ValueError(f'spkdiff: LIFNode state {tuple(v.shape)} on {v.device} does not fit a batch of {B} x {n} on '
                         f'{device}; call functional.reset_net between batches of different sizes')
    node.v = v
    return v


def _svae_linear_lif(seq, x, **kw):
    """nn.Sequential(layer.Linear, LIFNode) on x (fp32 / u8 [T,B,in] or u8 PTC [B,H,W,T,C]) -> u8 spikes (or PTC / None)."""
    lin, node = seq[0], seq[1]
    B = x.shape[0] if x.dim() == 5 else x.shape[1]
    return ops.linear_lif(x, lin.weight, lin.bias, _svae_node_v(node, B, lin.out_features, x.device), **kw)


def _svae_linear_lif_train(seq, x, x2=None):
    """nn.Sequential(layer.Linear, LIFNode) in training on fp32 [T,B,in] (+ optional concat x2): fp32 spikes with autograd."""
    lin, node = seq[0], seq[1]
    v = _svae_node_v(node, x.shape[1], lin.out_features, x.device)
    return ops.LinearLIFTrainFunction.apply(x, x2, lin.weight, lin.bias, v, True)


def _train_guard(what, t):
    if not torch.is_grad_enabled():
        _training_oos(f'{what} in train() mode without autograd')
    if not t.is_cuda:
        raise NotImplementedError(f"spkdiff: {what} in train() mode needs a ROCm device; there is no CPU path")


def _require_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"spkdiff: {what} is on '{t.device}'; there is no CPU path (move the module and tensors to a "
                           "ROCm device)")


class _BernoulliSTBP(nn.Module):
    """The 3-layer spiking MLP shared by the prior (input z) and the posterior (input [x, z]) of R/snn_model/vae_model.py."""

    def __init__(self, in_mult, k):
        super().__init__()
        self.channels = 28 * 2
        self.k = k
        self.n_steps = 16
        self.layers = nn.Sequential(
            layer.Linear(self.channels * in_mult, self.channels * 2),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),
            layer.Linear(self.channels * 2, self.channels * 4),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),
            layer.Linear(self.channels * 4, self.channels * k),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),
        )
        self.register_buffer('initial_input', torch.zeros(1, 1, self.channels))

    def _draw_indices(self, batch_size, device):
        """The n_steps draws torch.randint(0, k, (B*C,)) of the reference, in its order, on the CPU default generator."""
        idx = torch.stack([torch.randint(0, self.k, (batch_size * self.channels,)) for _ in range(self.n_steps)])
        return idx.view(self.n_steps, batch_size, self.channels).to(torch.int32).to(device)

    def _ar(self, x, batch_size, want_q_z=False):
        dev = self.initial_input.device
        _require_device(self.initial_input, f'{type(self).__name__}')
        idx = self._draw_indices(batch_size, dev)
        lins = [self.layers[i] for i in (0, 2, 4)]
        vs = [_svae_node_v(self.layers[i + 1], batch_size, lins[j].out_features, dev) for j, i in enumerate((0, 2, 4))]
        return ops.svae_ar(x, self.initial_input, [(m.weight, m.bias) for m in lins], vs, idx, want_q_z=want_q_z)

    def _state(self, B, dev):
        lins = [self.layers[i] for i in (0, 2, 4)]
        vs = [_svae_node_v(self.layers[i + 1], B, lins[j].out_features, dev) for j, i in enumerate((0, 2, 4))]
        return [(m.weight.detach(), m.bias.detach()) for m in lins], vs

    def _grad_pass(self, x, x2=None):
        """The one pass with grad of a training loop: the three Linear + LIF layers on [x | x2] -> fp32 spikes [T,B,C*k]."""
        h = _svae_linear_lif_train(self.layers[0:2], x, x2)
        h = _svae_linear_lif_train(self.layers[2:4], h)
        return _svae_linear_lif_train(self.layers[4:6], h)

    def _teacher_forced(self, z, want_out=True):
        """The eval pass over [initial_input, z_0 .. z_{T-2}] (one multi-step pass, state carried): u8 [T,B,C*k] or None."""
        _require_device(z, 'z')
        B = z.shape[1]
        z_prev = torch.cat([self.initial_input.to(torch.float32).expand(1, B, self.channels), z[:-1].to(torch.float32)], 0)
        h = _svae_linear_lif(self.layers[0:2], z_prev.contiguous())
        h = _svae_linear_lif(self.layers[2:4], h)
        return _svae_linear_lif(self.layers[4:6], h, want_out=want_out)


class PriorBernoulliSTBP(_BernoulliSTBP):
    """p(z_t | z_<t), R/snn_model/vae_model.py:306-423."""

    def __init__(self, k=20) -> None:
        super().__init__(1, k)

    def forward(self, z, scheduled=True, p=None):
        """Eval: p_z (T,B,C,k) of the pass over [initial_input, z_0 .. z_{T-2}] (both branches of the reference compute this
        pass outside training, :338-403).  Advances the layers' LIF state."""
        if self.training:
            p_z, _ = self._train_forward(z, scheduled, p)
            return p_z.view(self.n_steps, z.shape[1], self.channels, self.k)
        out = self._teacher_forced(z)
        return out.to(torch.float32).view(self.n_steps, z.shape[1], self.channels, self.k)

    def _train_forward(self, z, scheduled=True, p=None):
        """Training (:338-403): the scheduled-sampling prefix passes without grad (one launch, skipped when no step is
        scheduled), then one pass with grad over z_t_minus.  Returns (p_z fp32 [T,B,C*k], z_t_minus fp32 [T,B,C]).
        Host draws as the reference's: random.random() for t = 5..T-2, torch.randn_like([B,C]) per scheduled step."""
        _train_guard('PriorBernoulliSTBP.forward', z)
        z = z.detach().to(torch.float32)
        T, B = z.shape[0], z.shape[1]
        dev = z.device
        sched = [False] * (self.n_steps - 1)
        noise = []
        if scheduled:
            for t in range(self.n_steps - 1):
                if t >= 5 and random.random() < p:
                    sched[t] = True
                    noise.append(torch.randn_like(torch.empty((B, self.channels), dtype=torch.float32, device=dev)))
        z0 = self.initial_input.to(torch.float32)
        if noise:
            layers, vs = self._state(B, dev)
            z_t_minus = ops.svae_ar_prefix(None, z0, layers, vs, sched=torch.tensor(sched, dtype=torch.uint8, device=dev),
                                           noise=torch.stack(noise), z_teacher=z.contiguous())
        else:
            z_t_minus = torch.cat([z0.expand(1, B, self.channels), z[:-1]], 0).contiguous()
        return self._grad_pass(z_t_minus), z_t_minus

    def sample(self, batch_size=64):
        """Autoregressive sampling of z (T,B,C): n_steps passes over the growing prefix, one launch (spk_svae_ar_fwd)."""
        z, _ = self._ar(None, batch_size)
        return z


class PosteriorBernoulliSTBP(_BernoulliSTBP):
    """q(z_t | x_<=t, z_<t), R/snn_model/vae_model.py:425-546."""

    def __init__(self, k=20) -> None:
        super().__init__(2, k)
        self.is_true_scheduled_sampling = True

    def forward(self, x, want_q_z=True):
        """x: (T,B,C) spikes of before_latent_layer (u8 / bool, or fp32 0/1).  Returns (sampled_z (T,B,C) fp32,
        q_z (T,B,C,k) fp32 -- the spikes of the final pass -- or None with want_q_z=False).  One launch."""
        if self.training:
            q, idx = self._train_forward(x)
            sz, _ = ops.LatentLossFunction.apply(q, None, idx, 2.0)
            return sz, q.view(x.shape[0], x.shape[1], self.channels, self.k)
        _require_device(x, 'x')
        if x.dtype != torch.uint8 and x.dtype != torch.bool:
            x = x.to(torch.uint8)
        T, B = x.shape[0], x.shape[1]
        z, q = self._ar(x.contiguous(), B, want_q_z=want_q_z)
        if q is not None:
            q = q.to(torch.float32).view(T, B, self.channels, self.k)
        return z, q


    def _train_forward(self, x):
        """Training (:470-546): the T-1 prefix passes without grad in one launch, then one pass with grad over
        [x, z_t_minus] (gradient into x only).  x fp32 [T,B,C] (with autograd).  Returns (q_z fp32 [T,B,C*k], idx int32
        [T,B,C]); sampled_z is the gather of q_z at idx (ops.LatentLossFunction)."""
        _train_guard('PosteriorBernoulliSTBP.forward', x)
        T, B = x.shape[0], x.shape[1]
        dev = x.device
        idx = self._draw_indices(B, dev)
        layers, vs = self._state(B, dev)
        z_t_minus = ops.svae_ar_prefix(x.detach().to(torch.uint8), self.initial_input.to(torch.float32), layers, vs, idx=idx)
        x = x if x.dtype == torch.float32 else x.to(torch.float32)
        return self._grad_pass(x, z_t_minus), idx


class SNN_VAE(nn.Module):
    """The spiking VAE baseline, R/snn_model/vae_model.py:198-305 -- eval forward, encode, decode and sample on HIP."""

    def __init__(self):
        super().__init__()
        latent_dim = 28 * 2
        self.latent_dim = latent_dim
        self.n_steps = 16
        self.k = 20
        self.encoder = Encoder()
        self.before_latent_layer = nn.Sequential(
            layer.Linear(in_features=784, out_features=latent_dim),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),
        )
        self.prior = PriorBernoulliSTBP(self.k)
        self.posterior = PosteriorBernoulliSTBP(self.k)
        self.decoder_input = nn.Sequential(
            layer.Linear(in_features=latent_dim, out_features=16 * 7 * 7),
            neuron.LIFNode(surrogate_function=surrogate.ATan()),
        )
        self.decoder = Decoder()
        self.p = 0
        self.membrane_output_layer = MembraneOutputLayer()
        self.psp = PSP()

    def _train_latent(self, x, scheduled=True):
        """Training encode: encoder (batch-statistics BN, surrogate LIF), before_latent_layer, posterior, prior and the
        fused gather + MMD loss.  Returns (sampled_z, mmd_loss, q_z flat, p_z flat, prior's z_t_minus, latent_x)."""
        z = self.encoder(x)                                                           # (T,B,16,7,7) fp32
        latent_x = _svae_linear_lif_train(self.before_latent_layer, torch.flatten(z, 2).contiguous())
        return self._latent_from(latent_x, scheduled) + (latent_x,)

    def _latent_from(self, latent_x, scheduled=True):
        """posterior -> prior -> (sampled_z, mmd_loss, q_z [T,B,C*k], p_z [T,B,C*k], the prior's z_t_minus [T,B,C]) from
        before_latent_layer's spikes [T,B,C]."""
        q_z, idx = self.posterior._train_forward(latent_x)
        sampled_vals, _ = ops.LatentLossFunction.apply(q_z.detach(), None, idx, float(self.psp.tau_s))   # prior input: no grad
        p_z, z_t_minus = self.prior._train_forward(sampled_vals, scheduled, self.p)
        sampled_z, mmd = ops.LatentLossFunction.apply(q_z, p_z, idx, float(self.psp.tau_s))
        return sampled_z, mmd, q_z, p_z, z_t_minus

    def _train_decode(self, z):
        """decoder_input + view + decoder in training: the decoder's output (T,B,1,28,28) before the read-out."""
        result = _svae_linear_lif_train(self.decoder_input, z.to(torch.float32).contiguous())
        return self.decoder(result.view(self.n_steps, result.shape[1], 16, 7, 7))

    def _encode(self, x, scheduled=True, full=True):
        if self.training:
            _train_guard('SNN_VAE.encode', x)
            sampled_z, _, q_z, p_z, _, _ = self._train_latent(x, scheduled)
            T, B = q_z.shape[0], q_z.shape[1]
            return (sampled_z, q_z.view(T, B, self.latent_dim, self.k), p_z.view(T, B, self.latent_dim, self.k))
        _require_device(x, 'x')
        z_ptc = self.encoder.snn_convs.run(x, IN_SEQ, final='ptc')['ptc']            # u8 [B,7,7,T,16]
        latent_x = _svae_linear_lif(self.before_latent_layer, z_ptc)                 # u8 [T,B,56], flatten(C,H,W) order
        sampled_z, q_z = self.posterior(latent_x, want_q_z=full)
        if full:
            p_z = self.prior(sampled_z, scheduled, self.p)
        else:
            self.prior._teacher_forced(sampled_z, want_out=False)                    # output unused; advances the state
            p_z = None
        return sampled_z, q_z, p_z

    def encode(self, x, scheduled=True):
        """x (T,B,1,28,28) -> (sampled_z (T,B,C), q_z (T,B,C,k), p_z (T,B,C,k))."""
        return self._encode(x, scheduled, full=True)

    def decode(self, z):
        """z (T,B,C) -> tanh(membrane read-out) (B,1,28,28): decoder_input writes the PTC spikes the fused decoder reads."""
        if self.training:
            _train_guard('SNN_VAE.decode', z)
            return torch.tanh(self.membrane_output_layer(self._train_decode(z)))
        _require_device(z, 'z')
        ptc = _svae_linear_lif(self.decoder_input, z.to(torch.float32).contiguous(), out_ptc=(16, 7, 7))
        return self.decoder.snn_convs.run(ptc, IN_PTC, final='memout', coef=self.membrane_output_layer.coef.flatten(),
                                          apply_tanh=True)['f32']

    def sample(self, batch_size=64):
        sampled_z = self.prior.sample(batch_size)
        sampled_x = self.decode(sampled_z)
        return sampled_x, sampled_z

    def loss_function_mmd(self, input_img, recons_img, q_z, p_z):
        """q_z, p_z: (T,N,latent_dim,k) -> (mmd_loss, recons_loss)."""
        recons_loss = F.mse_loss(recons_img, input_img)
        q_z_ber = torch.mean(q_z, dim=-1)
        p_z_ber = torch.mean(p_z, dim=-1)
        mmd_loss = torch.mean((self.psp(q_z_ber) - self.psp(p_z_ber)) ** 2)
        return mmd_loss, recons_loss

    def weight_clipper(self):
        with torch.no_grad():
            for prm in self.parameters():
                prm.data.clamp_(-4, 4)

    def update_p(self, epoch, max_epoch):
        init_p, last_p = 0.1, 0.3
        self.p = (last_p - init_p) * epoch / max_epoch + init_p

    def forward(self, x, image, scheduled=True):
        """Eval: (sampled_z (T,B,C), x_recon (B,1,28,28)).  Training: (mmd_loss, recons_loss) with autograd, the
        reconstruction loss not divided by the data variance (R/snn_model/vae_model.py:299-305)."""
        if self.training:
            _train_guard('SNN_VAE.forward', x)
            sampled_z, mmd, _, _, _, _ = self._train_latent(x, scheduled)
            y = self._train_decode(sampled_z)
            return mmd, ops.ReconLossFunction.apply(y, self.membrane_output_layer.coef, image)      # read-out + tanh + mse
        sampled_z, _, _ = self._encode(x, scheduled, full=False)
        return sampled_z, self.decode(sampled_z)


# ---- SNN_VQVAE_uni: SNN_VQVAE with a codebook-usage statistic (R/snn_model/vae_model.py:674-801) ----------------------------
# The modules, state_dict keys and the arithmetic of e, x_recon, the indices and the training losses are SNN_VQVAE's; the
# quantizer also computes, on every call, the histogram of the codes, the number of codes used, the most used code and the
# "FID_loss" (:705-718, one launch: spk_vq_code_usage) and prints them.  In train() mode the printed FID_loss is replaced by a
# CPU int64 zero (:752), so the gradients are SNN_VQVAE's.  (The reference file defines SNN_VQVAE_uni's __init__ and forward a
# second time at :806-879, after the class's forward; those definitions shadow the ones at :772-801, and with them
# R/main.py:101 fails at construction.  This class is the :674-801 model that R/main.py's snn-vq-vae-uni branches call.)

def _device_repr(t, device):
    """repr of the host tensor t as torch prints the same values on ``device`` (the device suffix, torch's line rule)."""
    s, suffix = repr(t)[:-1], f"device='{device}'"
    last_line_len = len(s) - s.rfind('\n') + 1
    if last_line_len + len(suffix) + 2 > torch._tensor_str.PRINT_OPTS.linewidth:
        return s + ',\n       ' + suffix + ')'
    return s + ', ' + suffix + ')'


def print_code_usage(usage, n, device):
    """The four lines R/snn_model/vae_model.py:714-718 prints, from ONE device-to-host copy of the statistic (the reference
    synchronises at the same place: its prints read device tensors)."""
    hist, used, m, fid = ops.unpack_code_usage(usage.packed.cpu())
    K = hist.numel()
    keep = torch.ne(torch.arange(K), m)
    print(n)
    print(_device_repr(torch.masked_select(hist, keep), device))
    print(_device_repr(torch.masked_select(torch.ones(K) * n / K, keep), device))
    print(torch.Size([used]), fid)


class VectorQuantizer_uni(VectorQuantizer):
    """VectorQuantizer plus the codebook-usage statistic (R/snn_model/vae_model.py:674-766).  ``print_usage`` (not in the
    reference; default True) prints it as the reference does, one synchronising copy per call; False skips the prints and
    the copy, so the call stays asynchronous and capturable.  ``usage`` holds the last statistic (ops.CodeUsage, device
    tensors) either way."""

    def __init__(self, embedding_dim, num_embeddings, commitment_cost):
        super().__init__(embedding_dim, num_embeddings, commitment_cost)
        self.print_usage = True
        self.usage = None

    def code_usage(self, encoding_indices):
        """The statistic of :705-718 on encoding_indices (device) -> ops.CodeUsage; printed when print_usage is set."""
        self.usage = ops.vq_code_usage(encoding_indices, self.num_embeddings)
        if self.print_usage:
            print_code_usage(self.usage, encoding_indices.numel(), encoding_indices.device)
        return self.usage

    def forward(self, x):
        # x: (T,N,C,H,W) spikes of the encoder
        if self.training:
            quantized, loss, encoding_indices = self._train_forward_idx(x)
            if encoding_indices is None:
                raise NotImplementedError('spkdiff: VectorQuantizer_uni in train() mode needs the codebook or alpha to '
                                          'require grad (the code indices come from the autograd node)')
            self.code_usage(encoding_indices)
            return quantized, loss, torch.tensor(0)          # the reference's FID_loss in train() mode (:752)
        quantized, encoding_indices = super().forward(x)
        self.code_usage(encoding_indices)
        return quantized, encoding_indices


class SNN_VQVAE_uni(SNN_VQVAE):
    """VQ-VAE (R/snn_model/vae_model.py:768-801): SNN_VQVAE with VectorQuantizer_uni."""

    def __init__(self, in_dim, embedding_dim, num_embeddings, data_variance, commitment_cost=0.25):
        super().__init__(in_dim, embedding_dim, num_embeddings, data_variance, commitment_cost)
        self.vq_layer = VectorQuantizer_uni(embedding_dim, num_embeddings, commitment_cost)

    def forward(self, x, image):
        # x: [t, B, C, H, W]
        if self.training:
            if not torch.is_grad_enabled():
                _training_oos('SNN_VQVAE_uni.forward in train() mode without autograd')
            z = self.encoder(x)
            e, e_q_loss, FID_loss = self.vq_layer(z)
            real_recon_loss = self._train_recon_loss(self.decoder(e), image)
            return e_q_loss + FID_loss, real_recon_loss / self.data_variance, real_recon_loss
        vq = self.vq_layer
        vq.usage = None
        e, x_recon, encoding_indices = super().forward(x, image)
        if vq.usage is None:            # the fused end-to-end path runs the quantizer's pieces, not its forward
            vq.code_usage(encoding_indices)
        return e, x_recon, encoding_indices


# ---- VQVAE: the plain-CNN baseline (R/snn_model/vae_model.py:548-672, main.py --model vq-vae) --------------------------------
# The ANN the paper's tables set the spiking model against.  The modules, children and state_dict keys are the reference's.  In
# eval() on a ROCm device the forward is three launches of csrc/ann_vqvae.hip (encoder + code search: one; decoder: two); CPU
# tensors, other dtypes, unsupported shapes and modules with hooks take the modules below, which are the reference's operators
# in the reference's order.  In train() the same test sends the iteration to csrc/conv_train.hip (the six convolutions with the ReLU
# as an epilogue) and csrc/ann_vqvae_train.hip (quantiser, commitment cost, straight-through value, mse) as one autograd node;
# ``fused_train = False`` or any of the conditions above runs the modules under autograd.

class CNN_VectorQuantizer(nn.Module):
    """VQ-VAE layer of the ANN baseline (R/snn_model/vae_model.py:548-605)."""

    def __init__(self, embedding_dim, num_embeddings, commitment_cost):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings
        self.commitment_cost = commitment_cost
        self.embeddings = nn.Embedding(self.num_embeddings, self.embedding_dim)

    def forward(self, x):
        x = x.permute(0, 2, 3, 1).contiguous()                      # [B, C, H, W] -> [B, H, W, C]
        flat_x = x.reshape(-1, self.embedding_dim)
        encoding_indices = self.get_code_indices(flat_x)
        quantized = self.quantize(encoding_indices)
        quantized = quantized.view_as(x)
        if not self.training:
            quantized = quantized.permute(0, 3, 1, 2).contiguous()
            return quantized, encoding_indices
        q_latent_loss = F.mse_loss(quantized, x.detach())           # moves the embeddings towards the encoder's output
        e_latent_loss = F.mse_loss(x, quantized.detach())           # commitment loss
        loss = q_latent_loss + self.commitment_cost * e_latent_loss
        quantized = x + (quantized - x).detach()                    # straight-through estimator
        quantized = quantized.permute(0, 3, 1, 2).contiguous()
        return quantized, loss

    def get_code_indices(self, flat_x):
        distances = (
            torch.sum(flat_x ** 2, dim=1, keepdim=True) +
            torch.sum(self.embeddings.weight ** 2, dim=1) -
            2. * torch.matmul(flat_x, self.embeddings.weight.t())
        )
        return torch.argmin(distances, dim=1)

    def quantize(self, encoding_indices):
        """Returns embedding tensor for a batch of indices."""
        return self.embeddings(encoding_indices)


class CNN_Encoder(nn.Module):
    """Encoder of VQ-VAE"""

    def __init__(self, in_dim=3, latent_dim=16):
        super().__init__()
        self.in_dim = in_dim
        self.latent_dim = latent_dim
        self.convs = nn.Sequential(
            nn.Conv2d(in_dim, 32, 3, stride=2, padding=1),
            nn.ReLU(inplace=True),
            nn.Conv2d(32, 64, 3, stride=2, padding=1),
            nn.ReLU(inplace=True),
            nn.Conv2d(64, latent_dim, 1),
        )

    def forward(self, x):
        return self.convs(x)


class CNN_Decoder(nn.Module):
    """Decoder of VQ-VAE"""

    def __init__(self, out_dim=1, latent_dim=16):
        super().__init__()
        self.out_dim = out_dim
        self.latent_dim = latent_dim
        self.convs = nn.Sequential(
            nn.ConvTranspose2d(latent_dim, 64, 3, stride=2, padding=1, output_padding=1),
            nn.ReLU(inplace=True),
            nn.ConvTranspose2d(64, 32, 3, stride=2, padding=1, output_padding=1),
            nn.ReLU(inplace=True),
            nn.ConvTranspose2d(32, out_dim, 3, padding=1),
        )

    def forward(self, x):
        return self.convs(x)


def _ann_conv_is(m, cls, cin, cout, k, stride, pad, out_pad=None):
    return (type(m) is cls and (m.in_channels, m.out_channels) == (cin, cout) and m.kernel_size == (k, k)
            and m.stride == (stride, stride) and m.padding == (pad, pad) and m.dilation == (1, 1) and m.groups == 1
            and m.bias is not None and (out_pad is None or m.output_padding == (out_pad, out_pad))
            and m.padding_mode == 'zeros')


class VQVAEConstructorError(TypeError, NotImplementedError):
    """``VQVAE(in_dim, embedding_dim, num_embeddings)`` without ``data_variance``.  The reference's constructor raises TypeError for
    that call (a missing positional argument), and so does this one; while the class was a stub the same call raised
    NotImplementedError, which callers written against it catch, so the error is both."""


_REQUIRED = object()


class VQVAE(nn.Module):
    """VQ-VAE"""

    def __init__(self, in_dim, embedding_dim, num_embeddings, data_variance=_REQUIRED, commitment_cost=0.25):
        if data_variance is _REQUIRED:
            raise VQVAEConstructorError("VQVAE.__init__() missing 1 required positional argument: 'data_variance' -- it takes the "
                                        "four arguments of SNN_VQVAE and SNN_VQVAE_uni (R/main.py:107: in_dim, embedding_dim, "
                                        "num_embeddings, train_data_variance)")
        super().__init__()
        self.in_dim = in_dim
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings
        self.data_variance = data_variance

        self.encoder = CNN_Encoder(in_dim, embedding_dim)
        self.vq_layer = CNN_VectorQuantizer(embedding_dim, num_embeddings, commitment_cost)
        self.decoder = CNN_Decoder(in_dim, embedding_dim)
        # training: ops.ANNVQVAETrainFunction on the HIP training kernels (False: the modules below under autograd)
        self.fused_train = True

    # -- the fused path -------------------------------------------------------------------------------------------
    def _is_reference_net(self):
        """Are the children the reference's layers (what csrc/ann_vqvae.hip implements)?"""
        enc, dec, D = self.encoder.convs, self.decoder.convs, self.embedding_dim
        return (len(enc) == 5 and len(dec) == 5 and all(type(m) is nn.ReLU for m in (enc[1], enc[3], dec[1], dec[3]))
                and _ann_conv_is(enc[0], nn.Conv2d, self.in_dim, 32, 3, 2, 1) and _ann_conv_is(enc[2], nn.Conv2d, 32, 64, 3, 2, 1)
                and _ann_conv_is(enc[4], nn.Conv2d, 64, D, 1, 1, 0)
                and _ann_conv_is(dec[0], nn.ConvTranspose2d, D, 64, 3, 2, 1, 1)
                and _ann_conv_is(dec[2], nn.ConvTranspose2d, 64, 32, 3, 2, 1, 1)
                and _ann_conv_is(dec[4], nn.ConvTranspose2d, 32, self.in_dim, 3, 1, 1, 0)
                and type(self.vq_layer.embeddings) is nn.Embedding
                and tuple(self.vq_layer.embeddings.weight.shape) == (self.num_embeddings, D))

    def _fused(self, t, hw):
        """Does a call on tensor ``t`` for images of size ``hw`` take csrc/ann_vqvae.hip?  ROCm device, the library supports
        the shape, fp32 parameters on that device, the reference's layers, no hooks anywhere below (syops, monitors)."""
        cb = self.vq_layer.embeddings.weight
        return (t.is_cuda and cb.device == t.device and all(p.dtype == torch.float32 and p.device == t.device
                                                            for p in self.parameters())
                and ops.ann_vqvae_supported(self.in_dim, hw[0], hw[1], self.embedding_dim, self.num_embeddings)
                and not has_hooks(self) and self._is_reference_net())

    def _images_fused(self, x):
        return (x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous() and x.shape[1] == self.in_dim
                and self._fused(x, x.shape[2:]))

    def _enc_params(self):
        c = self.encoder.convs
        return (c[0].weight, c[0].bias, c[2].weight, c[2].bias, c[4].weight, c[4].bias)

    def _dec_params(self):
        c = self.decoder.convs
        return (c[0].weight, c[0].bias, c[2].weight, c[2].bias, c[4].weight, c[4].bias)

    def _train_fused(self, x):
        """Does a train() call on ``x`` take the HIP training kernels (csrc/conv_train.hip, csrc/ann_vqvae_train.hip)?  Not an
        image that wants a gradient (the node gives it none), nor a codebook beyond the quantiser kernel's (K > 862 at D = 16)."""
        return (self.fused_train and not x.requires_grad and self._images_fused(x)
                and ops.ann_vqvae_train_supported(x.shape, self._enc_params(), self._dec_params(), self.vq_layer.embeddings.weight))

    def _data_variance_on(self, device):
        """data_variance as the fp32 device scalar the loss kernels read, converted once per value and device (a tensor's in-place
        update or replacement converts again): an iteration reads nothing back and uploads nothing."""
        dv = self.data_variance
        key = ((id(dv), dv._version) if isinstance(dv, torch.Tensor) else float(dv), str(device))
        if getattr(self, "_dv_key", None) != key:
            self._dv_dev, self._dv_key = ops.ann_data_variance(dv, device), key
        return self._dv_dev

    def forward(self, x):
        if not self.training and self._images_fused(x):
            B, _, H, W = x.shape
            cb = self.vq_layer.embeddings.weight
            enco, _, e = ops.ann_vqvae_encode(x, self._enc_params(), cb, want_e=True)
            x_recon, _ = ops.ann_vqvae_decode(enco.view(B, H // 4, W // 4), self._dec_params(), cb)
            return e, x_recon, enco
        if self.training and self._train_fused(x):
            params = self._enc_params() + self._dec_params() + (self.vq_layer.embeddings.weight,)
            beta, dv = self.vq_layer.commitment_cost, self._data_variance_on(x.device)
            if not torch.is_grad_enabled():               # the three values; nothing is kept
                return ops.ann_vqvae_train_forward(x, params[:6], params[6:12], params[12], beta, dv)[0]
            return ops.ANNVQVAETrainFunction.apply(x, beta, dv, *params)
        z = self.encoder(x)
        if not self.training:
            e, enco = self.vq_layer(z)
            x_recon = self.decoder(e)
            return e, x_recon, enco

        e, e_q_loss = self.vq_layer(z)
        x_recon = self.decoder(e)
        recon_loss = F.mse_loss(x_recon, x) / self.data_variance
        return e_q_loss, recon_loss, F.mse_loss(x_recon, x)

    # ---- convenience entry points of the MI355X build (not in the reference), SNN_VQVAE's call shapes ----------------
    @torch.no_grad()
    def encode_images(self, images, T=16):
        """images [B,C,H,W] already normalised (images - 0.5) -> code indices [B,h,w].  ``T`` is accepted and ignored (the
        spiking models' callers pass it)."""
        B, _, H, W = images.shape
        if self._images_fused(images):
            idx, _, _ = ops.ann_vqvae_encode(images, self._enc_params(), self.vq_layer.embeddings.weight)
        else:
            z = self.encoder(images).permute(0, 2, 3, 1).contiguous()
            idx = self.vq_layer.get_code_indices(z.reshape(-1, self.embedding_dim))
        return idx.reshape(B, H // 4, W // 4)

    @torch.no_grad()
    def decode_tokens(self, tokens, T=16, want_u8=True):
        """tokens int64 [B,h,w] -> (pred fp32 [B,C,H,W], uint8 image = clip(pred + 0.5, 0, 1) * 255 truncated, R/main.py:400,
        or None).  ``T`` is accepted and ignored."""
        B, h, w = tokens.shape
        if tokens.dtype == torch.int64 and self._fused(tokens, (4 * h, 4 * w)):
            return ops.ann_vqvae_decode(tokens, self._dec_params(), self.vq_layer.embeddings.weight, want_u8=want_u8)
        pred = self.decoder(self.vq_layer.quantize(tokens).permute(0, 3, 1, 2).contiguous())
        u8 = ((pred + 0.5).clamp(0, 1) * 255).to(torch.uint8) if want_u8 else None
        return pred, u8
