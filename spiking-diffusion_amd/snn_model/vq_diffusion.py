"""``snn_model.vq_diffusion`` of the MI355X build: spiking denoiser + absorbing-state reverse diffusion sampler.

Counterpart of R/snn_model/vq_diffusion.py -- ``DummyModel`` (:150-208), ``AbsorbingDiffusion`` (:43-147, only
``sample`` is on the hot path) and ``get_data_for_diff`` (:23-36) -- with the same names, constructor arguments,
attributes (``num_embeddings``, ``n_samples``, ``mask_id``, ``shape``...) and ``state_dict`` keys.

The denoiser runs as fused Conv+BN+LIF kernels (conv1 sees a time-invariant input, conv6 + the time mean are one
kernel), the per-step token update is one ``spk_psample_step`` launch, and ``sample()`` enqueues the whole
reverse process without any host synchronisation.  ``score()`` runs the same loop teacher-forced on given tokens (the token
update is one ``spk_pscore_step`` launch) and returns the sampler's likelihood bound for them.  Latent size and T are parameters (the reference hard-codes
7x7 and 16: vq_diffusion.py:47-48,106,198,206).
"""
import contextlib
import math
import os
from typing import NamedTuple

import torch
import torch.nn as nn

from spikingjelly.activation_based import neuron, functional, layer, surrogate, monitor  # noqa: F401
from spikingjelly import visualizing  # noqa: F401

from spkdiff import ops
from spkdiff.fused import (FusedSequential, invalidate_derived, has_hooks, derived_epoch, derived_refs, exact_spike_conv,
                           keep_channels_last)
from spkdiff.ops import IN_PTC, IN_TINV

from .vae_model import *  # noqa: F401,F403  (R/snn_model/vq_diffusion.py:21)


def get_data_for_diff(train_loader, model, T: int = 16, carry_state: bool = True):
    """Encode a data set to code indices (R/snn_model/vq_diffusion.py:23-36).

    The reference calls ``model(images_spike, images)`` batch after batch with no ``reset_net`` inside the loop, so every
    LIF layer starts a batch from the membrane potentials the previous batch left (its loaders drop the ragged last
    batch, R/load_dataset_snn.py:65-66).  ``carry_state=True`` (default) is that call sequence on the fused module path
    -- same indices as the reference (fixture F12), same module state afterwards; a batch of another size raises, as it
    does there.  ``carry_state=False`` encodes every batch from the reset state with the encoder alone (time-invariant
    input folded into the first kernel; nothing of the module state is read or written).

    The plain-CNN ``VQVAE`` (main.py --model vq-vae) has no state to carry and takes one argument -- the reference's
    two-argument call raises TypeError for it --: it is encoded with ``encode_images`` whatever ``carry_state`` says."""
    print('prepare data for train diffusion...')
    model.eval()
    train_indices = []
    dev = next(model.parameters()).device
    stateless = isinstance(model, VQVAE)
    for images, labels in train_loader:
        images = (images - 0.5).to(dev).float().contiguous()  # normalize to [-0.5, 0.5]
        with torch.inference_mode():
            if carry_state and not stateless:
                images_spike = images.unsqueeze(0).repeat(T, 1, 1, 1, 1)
                _, _, encoding_indices = model(images_spike, images)
                L = images.shape[-1] // 4
                idx = encoding_indices.reshape(images.shape[0], L, L)
            else:
                idx = model.encode_images(images, T)
            train_indices.append(idx.cpu())
    return train_indices


class Sampler(nn.Module):
    def __init__(self):
        super().__init__()


class SampleForm(NamedTuple):
    """Launch form of one ``sample()`` call, decided by ``AbsorbingDiffusion._form`` (same tokens in every form)."""
    skip: bool          # elimination: the denoiser runs on the images spk_select_active lists for the step
    lists: bool         # ... and its MFMA layers on the positions spk_select_needed lists
    tail: bool          # dense: conv6 + token update + the next step's first layer as one launch (spk_den_step_tail)
    tail_act: bool      # elimination: conv6 + token update of the active images as one launch (step_tail_in_elimination)


class _Noise(NamedTuple):
    """u / q of a reverse step: ``draw`` t -> (u, q) (injected, or the host's); without it Philox on the device, keyed by ``seed``
    or, with ``state``, by the 2-word device buffer {seed, counter base} a captured graph reads; counters at the step's offset."""
    draw: object = None
    seed: int = 0
    state: object = None


class Score(NamedTuple):
    """Result of ``AbsorbingDiffusion.score``: per reveal order o, image b and position (i, j) the log-probability (nats) of the
    given token at the step the order revealed it, and that step; 0 / 0 at the positions given as known."""
    position_log_prob: torch.Tensor     # fp64 [orders,B,h,w]
    reveal_step: torch.Tensor           # int32 [orders,B,h,w]
    log_prob: torch.Tensor              # fp64 [orders,B]: sum over the positions -- one estimate of the bound on log p(x_0) each

    def bits_per_dim(self, n_dims=None):
        """-mean over orders and images of ``log_prob`` / (ln 2 * n_dims) as a 0-dim device tensor; ``n_dims`` defaults to h * w
        (the unit of the reference's training loss, R/snn_model/vq_diffusion.py:85-101)."""
        if n_dims is None:
            n_dims = self.position_log_prob.shape[-2] * self.position_log_prob.shape[-1]
        return -self.log_prob.mean() / (math.log(2) * int(n_dims))


class _SamplerGraph:
    """One captured reverse process: the graph, its inputs (``steps`` = int32 [B] of a per-image-steps graph; ``state`` = {seed, counter base}; ``start_in`` = (codes, keep) of the
    conditional form; ``temps`` = fp32 [B] of a per-image-temperature graph; ``topk`` = int32 [B] of a truncating graph (which always has ``temps`` too); ``topp`` = fp32 [B] of a nucleus graph (which always has both); ``target[0]`` = the tokens a score graph is forced to, which are also its ``codes``), its result ``x_t`` (a
    score graph: ``target[1:]`` = (logp, step), zeroed inside the graph), and every other buffer the captured launches address by raw pointer: freed earlier,
    its block would go to the next allocation while replays keep writing to it.  That includes the denoiser's derived tensors
    (``derived``: an invalidation re-keys the graph, but until the stale entry is evicted their memory must not be recycled)
    and the flag workspaces of the certified kernels (``flag_ws``)."""

    def __init__(self, dev, b, h, w, form, radii, conditional, score=False, per_image_temp=False, top_k=False, top_p=False,
                 confident=False, per_image_steps=False, sched_steps=0, remask=False):
        self.graph = self.derived = None                            # set by the capture
        # remasking: the table is one more INPUT [B][S + 1] beside the two of the schedule; commit_conf is a buffer
        # of the graph, re-initialised from the start state by every replay (set by the capture)
        self.remask = torch.zeros((b, sched_steps + 1), dtype=torch.int32, device=dev) if remask else None
        self.commit_conf = None
        # a reveal schedule and annealed selection noise are two more INPUTS of fixed shape [B][S + 1]: the captured
        # `_sched` token updates read these buffers, so one graph serves every schedule and every noise scale
        self.sched = (torch.zeros((b, sched_steps + 1), dtype=torch.int32, device=dev),
                      torch.zeros((b, sched_steps + 1), dtype=torch.float32, device=dev)) if sched_steps else None
        self.confident = bool(confident)                            # the captured token updates are the confidence-ordered ones (§4.15)
        # per-image step counts are one more INPUT: the captured select_pending / listed updates read this buffer
        self.steps = torch.ones(b, dtype=torch.int32, device=dev) if per_image_steps else None
        self.state = torch.zeros(2, dtype=torch.int64, device=dev)
        # per-image temperatures are one more INPUT: the captured token updates read this buffer, filled before each replay
        self.temps = torch.ones(b, dtype=torch.float32, device=dev) if per_image_temp or top_k or top_p else None
        # ... and so is the per-image k of a truncating graph
        self.topk = torch.zeros(b, dtype=torch.int32, device=dev) if top_k or top_p else None
        # ... and the per-image p of a nucleus graph
        self.topp = torch.ones(b, dtype=torch.float32, device=dev) if top_p else None
        self.x_t = torch.empty((b, 1, h, w), dtype=torch.int64, device=dev)
        self.unmasked = torch.empty((b, 1, h, w), dtype=torch.bool, device=dev)
        self.start_in = (torch.empty((b, h, w), dtype=torch.int64, device=dev),
                         torch.empty((b, h, w), dtype=torch.uint8, device=dev)) if conditional else None
        self.target = None
        if score:
            x0 = self.start_in[0] if conditional else torch.empty((b, h, w), dtype=torch.int64, device=dev)
            self.target = (x0, torch.empty((b, h, w), dtype=torch.float64, device=dev),
                           torch.empty((b, h, w), dtype=torch.int32, device=dev))
        self.act = (torch.zeros(b, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)) if form.skip else None
        self.need = ops.NeedLists(b, radii, dev) if form.lists else None
        # dense form without the fused step tail: every spk_psample_step also writes the next step's denoiser input
        self.inp = None if (form.skip or form.tail) else torch.empty((b, 2, h, w), dtype=torch.float32, device=dev)
        self.flag_ws = {}


class AbsorbingDiffusion(Sampler):
    def __init__(self, denoise_fn, mask_id, latent_shape=(7, 7)):
        super().__init__()
        self.num_classes = denoise_fn.num_embeddings
        self.shape = list(latent_shape)
        self.num_timesteps = latent_shape[0] * latent_shape[1]
        self.mask_id = mask_id
        self._denoise_fn = denoise_fn
        self.n_samples = 16
        self.mask_schedule = 'random'
        self.loss_type = 'reweighted_elbo'
        # 'philox': on-device counter-based noise (throughput); 'host': u and q drawn per step from torch's global
        # CPU generator in the reference's order (rand_like, then multinomial's exponential draw), which reproduces the
        # reference CPU path token for token under the same torch.manual_seed.
        self.noise_source = 'philox'
        # Philox contract ('philox' mode): every sample() call takes ONE 62-bit draw from torch's global CPU generator as
        # its key, so ``torch.manual_seed(s); sample(); sample()`` gives two different batches and re-seeding repeats
        # them -- the reference's behaviour -- and two samplers in one process never share a stream.
        # ``noise_layout`` says how the counters are laid out (csrc/psample_common.h; include/spkdiff.h, spk_psample_step):
        #   'global' (default): counter = step * 2^40 + (GLOBAL image index * h*w + position) * K + class.  The draws of
        #       image i at step s depend on (key, s, i, position, class) only -- not on the batch size, not on how the batch
        #       is split over processes: an 8-GPU job, a 1-GPU job and the oracle on the dumped noise give the same tokens for
        #       the same images (SURVEY.md §8e "parity mode => result independent of G"; the reference draws one batch from
        #       one stream, R/snn_model/vq_diffusion.py:103-142).  A shard sets ``global_first`` (index of its first image,
        #       see ``set_shard``); ranks must use the SAME key: seed them alike, or let ``sync_key`` broadcast rank 0's draw.
        #   'rank': the rounds 1-3 form -- local image index, step stride b*h*w*K, the RANK folded into the key
        #       (``philox_stream``): ranks seeded alike draw distinct noise, but the sample depends on the split.
        self.noise_layout = 'global'
        self.global_first = 0
        # The key broadcast is a COLLECTIVE, so it is opt-in: it happens only in a sampler that ``set_shard`` declared a shard of a
        # multi-rank job (every rank of the job then calls sample()).  A sampler that never called set_shard inside an initialised
        # process group (a preview on rank 0 during DDP training, or old-style per-rank sampling) takes no collective and folds the
        # rank into its key, as rounds 1-3 did: no deadlock, and ranks seeded alike still draw distinct images (one warning).
        self.sync_key = True                 # set_shard + 'global' layout + world_size > 1: broadcast the key from rank 0
        self._shard_set = False
        self._warned_unsharded = False
        self.last_key = None
        self.philox_stream = int(os.environ.get('RANK', '0'))
        # Replay the whole reverse process as ONE hipGraph (philox mode, no hooks): the ~800 kernel launches of a
        # 100-step sample are captured once per (batch, steps, temp) and replayed; fresh noise per replay comes from a
        # 2-word device buffer {seed, counter base} the kernels read (spk_psample_step philox_state).
        self.use_graph = True
        self._graphs = {}
        # Reverse step t only writes the positions in `changes` (computed before the denoiser call, :113-124,140): an
        # image without a change at step t never has its denoiser output read.  True = evaluate the denoiser only for the
        # images spk_select_active lists for the step (61 % of (image, step) pairs drop out at 100 steps x 49 positions);
        # the sampled tokens are those of the dense loop, draw for draw.
        self.skip_untouched = True
        # ... and, of a touched image, the logits are read only at the positions that change: with 3x3 layers below them a
        # layer r levels down is needed within distance r of a change.  True = the MFMA layers of the denoiser compute the
        # positions spk_select_needed lists for the step (7x7 latents; again the same tokens, draw for draw).
        self.list_positions = True
        # ... from this batch size on: below it every launch of a reverse step is latency bound and the list bookkeeping (one more
        # launch per step, per-class item division) costs more than the skipped positions save -- R/main.py's own n_samples = 16:
        # 7.04 ms per 49-step sample without lists, 7.75 with; B = 32: 8.9 / 8.25 (tools/small_batch_time.py, profiles/r6_ab_kernel_variants.txt (1))
        self.list_min_batch = 24
        # elimination forms: conv6 on the spike counts + the token update of the ACTIVE images as one launch per slot (spk_den_step_tail with
        # the active list) instead of two (spk_den_conv3x3_counts_mfma, spk_psample_step).  Same tokens -- and measured SLOWER (round 6, one
        # box: B = 256 x 100 steps 35.30 against 34.88 ms, B = 64 18.70 / 17.58, B = 16 x 49 steps 7.93 / 7.13: a workgroup of the step tail
        # is one image's 90-iteration weight stream, ~30 us whatever the number of slots, where the counts kernel spreads the active images'
        # rows over the chip).  Off; kept as an opt-in with its test (profiles/r6_ab_kernel_variants.txt (6)).
        self.step_tail_in_elimination = False
        self.list_radii = 3                 # layers below the logits that take lists (1: conv5 only ... 4: conv2..conv5;
                                            # conv2 needs nearly every position anyway: 3 measured fastest)
        # Derived weight forms (digit planes, folded BN terms, captured graphs) are keyed on (data_ptr, _version), which
        # writes through ``.data`` and graph-replayed optimizer steps do not change.  True = every sample() call compares
        # a content checksum of the denoiser's parameters and buffers (one launch + one 8-byte read-back, ~30 us) with the
        # one the derived forms were built from and rebuilds them when it differs.
        self.verify_weights = True
        self._wsum = None
        self._pinned_key = None             # see _one_key()

    # ---- training step (R/snn_model/vq_diffusion.py:56-101,144-147) -------------------------
    def sample_time(self, b, device):
        t = torch.randint(1, self.num_timesteps + 1, (b,), device=device).long()
        pt = torch.ones_like(t).float() / self.num_timesteps
        return t, pt

    def q_sample(self, x_0, t):
        """Mask each token of x_0 [B,1,h,w] with probability t/T.  Returns (x_t, x_0_ignore, mask): masked positions
        hold ``mask_id`` in x_t, unmasked positions hold -1 (the loss's ignore index) in x_0_ignore."""
        b = x_0.shape[0]
        if x_0.is_cuda and x_0.dtype == torch.float32 and t.is_cuda and t.dtype == torch.int64 and x_0.dim() == 4:
            # one native launch after the framework's draw (same RNG call, same order as the reference's rand_like)
            return ops.q_sample(x_0, t, torch.rand_like(x_0), self.num_timesteps, self.mask_id)
        t_mask = t.reshape(b, 1, 1, 1).expand(b, 1, x_0.shape[2], x_0.shape[3])
        mask = torch.rand_like(x_0.float()) < (t_mask.float() / self.num_timesteps)
        x_t = torch.where(mask, torch.full_like(x_0, self.mask_id), x_0)
        x_0_ignore = torch.where(mask, x_0, torch.full_like(x_0, -1))
        return x_t, x_0_ignore, mask

    def _loss_from_logits(self, x_0_hat_logits, x_0_ignore, t):
        """Loss tail of _train_loss (:85-101): masked cross-entropy summed over positions, weighted per sample, in bits
        per latent dimension, mean over the batch.  Cross-entropy and its gradient: one spk_masked_ce launch."""
        b = x_0_hat_logits.shape[0]
        denom = math.log(2) * x_0_ignore.shape[1:].numel()
        if self.loss_type == 'elbo':
            pt = torch.ones_like(t).float() / self.num_timesteps
            coef = 1.0 / t.float() / pt / denom
        elif self.loss_type == 'reweighted_elbo':
            coef = (1 - (t / self.num_timesteps)).float() / denom
        else:
            raise ValueError
        return ops.MaskedCEFunction.apply(x_0_hat_logits, x_0_ignore.float(), coef / b)

    def _train_loss(self, x_0):
        b, device = x_0.size(0), x_0.device
        t, pt = self.sample_time(b, device)
        x_t, x_0_ignore, mask = self.q_sample(x_0=x_0, t=t)
        x_0_hat_logits = self._denoise_fn(x_t, t=t)
        return self._loss_from_logits(x_0_hat_logits, x_0_ignore, t)

    def train_iter(self, x):
        loss = self._train_loss(x)
        stats = {'loss': loss}
        return stats

    @torch.no_grad()
    def sample(self, temp=1.0, sample_steps=None, noise=None, record=None, x_init=None, known=None):
        """Reverse absorbing diffusion (R/snn_model/vq_diffusion.py:103-142).  Returns x_t int64 [B,1,h,w].

        ``noise``: optional callable t -> (u [B,1,h,w], q [B*h*w, K]) of device tensors (tests inject fixtures).
        ``record``: optional list receiving (t, x_t.clone(), unmasked.clone(), logits.clone()) per step.
        ``x_init`` / ``known`` (both or neither): complete a partly given latent.  ``x_init`` integer device tensor [B,1,h,w] or
        [B,h,w], ``known`` bool / uint8 of the same shape, true where the token is given.  The loop above runs unchanged from
        ``unmasked = known & (0 <= x_init < num_classes)``, ``x_t = where(unmasked, x_init, mask_id)`` instead of the
        all-masked state (a "known" token outside the codebook counts as not known: decided on the device).  The batch is
        ``x_init.shape[0]``; ``n_samples`` is neither read nor changed.  Same noise contract: one key draw, counters on the
        global image index -- with ``known`` all false the tokens are those of ``sample(temp, sample_steps)`` at
        ``n_samples = B`` under the same seed, and a shard (``set_shard``) gives the tokens the whole job gives.
        ``temp``: a number, or one temperature per image of the call's batch (``_temp_arg``): image i is
        sampled as ``sample(temp[i])`` samples it -- the same tokens under the same key and global image index, in every launch
        form, and one captured graph serves every vector.  Top-k truncation: ``sample_top_k``; nucleus truncation:
        ``sample_top_p``."""
        return self._sample_call(temp, sample_steps, noise, record, x_init, known, None)

    @torch.no_grad()
    def sample_top_k(self, top_k, temp=1.0, sample_steps=None, noise=None, record=None, x_init=None, known=None):
        """``sample()`` with top-k truncation: every token is drawn from its position's ``k`` likeliest codes,
        renormalised -- the classes below the k-th largest temperature-scaled logit are dropped ahead of the unchanged draw
        (classes that tie with the k-th all stay).  ``top_k``: None (``sample()`` itself: the same calls with the same arguments),
        an int >= 1 for every image, or one entry per image of the call (``_topk_arg``): integers >= 0, where 0 -- like any k >=
        num_classes -- leaves that image untruncated; a device tensor is int32 [B] and taken as given.  Every other argument is
        sample()'s; same noise contract (a dropped class's draw is simply not used: no other draw moves), so the tokens do not
        depend on the launch form, on the split (``set_shard``) or on eager / captured, and with k = 1 an image gets its arg max
        at every position.  In a captured graph ``top_k`` and the temperatures are inputs: one graph per (batch, steps, form,
        conditional) serves every k and every temperature.  ``score()`` takes no ``top_k``: a given token outside the kept set
        would score -inf, which bounds nothing."""
        return self._sample_call(temp, sample_steps, noise, record, x_init, known, top_k)

    @torch.no_grad()
    def sample_top_p(self, top_p, temp=1.0, sample_steps=None, noise=None, record=None, x_init=None, known=None, top_k=None):
        """``sample()`` with nucleus (top-p) truncation: every token is drawn from the likeliest codes of its
        position whose probability mass reaches ``p`` of the row's, renormalised -- the smallest such set of top classes, closed
        under ties; the cut is made on integer masses inside the kernels, so it does not depend on a summation order.  ``top_p``:
        None (``sample_top_k(top_k, ...)`` itself: the same calls with the same arguments), a number in (0, 1] for every image,
        or one entry per image of the call (``_topp_arg``): finite numbers in (0, 1], where 1 leaves that image untruncated; a
        device tensor is fp32 [B] and taken as given.  ``top_k``: as ``sample_top_k`` takes it; it is applied first.  Every other
        argument is sample()'s; same noise contract (a dropped class's draw is simply not used), so the tokens do not depend on the
        launch form, on the split (``set_shard``) or on eager / captured; the row maximum always stays, and as p -> 0+ an image
        gets its arg max at every position.  In a captured graph ``top_p``, ``top_k`` and the temperatures are inputs: one graph
        per (batch, steps, form, conditional) serves every p, k and temperature.  ``score()`` takes no ``top_p``, for the reason it
        takes no ``top_k``."""
        return self._sample_call(temp, sample_steps, noise, record, x_init, known, top_k, top_p)

    @torch.no_grad()
    def sample_confident(self, sample_steps=None, temp=1.0, noise=None, record=None, x_init=None, known=None, top_k=None, top_p=None,
                         schedule=None, selection_noise=None, remask=None):
        """Confidence-ordered decoding: ``sample()`` with another rule for WHERE a step reveals.  At step t every
        still-masked position of an image draws a candidate token -- the draw of ``sample_top_p(top_p, top_k=top_k)``, same noise
        counters -- and the ceil(m / t) candidates the denoiser is surest of (m = positions masked at entry; the order is the
        log-probability of the candidate under the truncated, renormalised row as the draw itself computes it in fp32, ties to the
        lower position) are committed; the others stay masked and draw again at the next step.  t = 1 reveals what is left, so the
        result holds no ``mask_id`` at any ``sample_steps``; the coin of sample() (``u < 1/t``) is not drawn, and there is no
        selection noise and no other schedule.  ``temp`` / ``top_k`` / ``top_p``: as sample_top_p() takes them (numbers are broadcast:
        the kernels read all three per image; None: no truncation); ``top_k = 1`` is greedy decoding, the same tokens under every
        key.  ``noise`` / ``record`` / ``x_init`` / ``known``: sample()'s (of an injected (u, q) only q is read).  Same noise contract
        -- one key draw, counters on the global image index -- so ``set_shard`` works unchanged, eager and captured give the same
        tokens, and one captured graph per (batch, steps, conditional) serves every temperature, k and p.  The launch form is the
        dense one whatever ``skip_untouched`` says (fused step tail where the denoiser allows it): which positions change depends
        on the logits, so no image and no position can be ruled out before the denoiser ran.  Latents of more than 64 positions:
        NotImplementedError before anything is launched.  ``score()`` has no such form.

        Per-image step counts: ``sample_steps`` may be a sequence or 1-D tensor of B integers >= 1, one per image
        of the call (``_steps_arg``; a device tensor is read back once, before the key is drawn).  The loop runs S = max of them
        steps; image i joins at t = s_i and is revealed by the ceil(m / t) rule from there, with the noise counters of its own run
        (step index s_i - t): under the 'global' layout image i equals, bit for bit, image i of ``sample_confident(s_i, ...)`` with
        the same key, global index, temperature / k / p and start state, whatever the other images' counts are -- so the result
        depends neither on the batch nor on the split.  Every step runs on the device-side list of PENDING images (t <= s_i and
        something still masked: spk_select_pending) -- the denoiser on the list, spk_psample_step_conf_listed for the update -- so
        the work is proportional to the sum of the s_i (an image with nothing masked is never evaluated).  In a captured graph the
        vector is an input: one graph per (batch, S, conditional) serves every vector with that maximum.  Refused before a key is
        drawn: ``record=``, the 'rank' layout, a wrong length, an entry < 1 (ValueError).  An int takes the path above unchanged.

        Reveal schedules and annealed selection noise.  ``schedule`` says HOW MANY positions a step commits:
        None (the ceil(m / t) count above, the calls made before), 'linear' (the same counts from a weight table), 'cosine' (few
        tokens on the empty context, most at the end: the masked fraction after progress r is cos(pi r / 2)), a sequence of
        sample_steps + 1 integer weights w[0 .. S] in 0 .. 2^24 -- step t keeps min(m, floor(m w[t - 1] / w[t])) of its m masked
        positions masked, reveals the rest and at least one (``spkdiff.schedules.reveal_counts`` lists the counts) -- or one of
        these per image of the call (a list of B entries, or a 2-D array / tensor [B, S + 1]).  ``selection_noise`` says IN WHAT
        ORDER: tau >= 0, finite, a number or one per image; the candidates are ranked by confidence + a * Gumbel(0, 1) with a =
        tau * (t - 1) / e annealed linearly to zero at the image's last step (e: the image's step count), the Gumbel from the
        position's stream-0 counter -- the coin's, free under this rule (of an injected (u, q), u is that uniform).  The candidates
        themselves do not change, and ``top_k = 1`` with tau > 0 commits the arg max tokens in a key-dependent order.  With both at
        None the call is the one above, launch for launch; anything else runs the ``_sched`` kernels (``schedule='linear'`` with
        tau = 0: the same tokens).  Under per-image step counts row i is built for the image's own e_i steps, so image i still
        equals image i of ``sample_confident(s_i, schedule=its row, selection_noise=tau_i)``.  In a captured graph both tables are
        inputs [B][S + 1]: one graph per (batch, S, conditional, per-image steps) serves every schedule and every tau.  Refused
        before a key is drawn (ValueError): tau negative or not finite, an unknown name, a table of the wrong length, a weight
        outside 0 .. 2^24 or no integer, a per-image list of the wrong length.

        Remasking.  ``remask`` lets the sampler change its mind: at the end of a step, after the reveal, the
        least trusted of the tokens EARLIER steps of this call committed -- smallest confidence at commit, ties to the higher
        position -- return to the masked state and draw again at the next step, when a denoiser call has seen them masked.  The
        step count, and so the cost, does not change.  A committed token is never re-scored from the current logits (the denoiser
        is not trained at unmasked positions): its trust is the confidence it was committed with.  None: the calls made without
        the argument, launch for launch.  An int r >= 0: up to r tokens per image at every step 2 <= t <= e.  A sequence of e + 1
        non-negative integers indexed by t (entries 0 and 1 must be 0: the last step remasks nothing, so no ``mask_id`` is
        left).  Or one of these per image: a list of B entries, or a 2-D array / tensor [B, S + 1].  ``known`` tokens are never
        remasked.  Anything but None runs the ``_remask`` kernels on top of the ``_sched`` family (``schedule`` None is then the
        linear table, ``selection_noise`` None no noise: ``remask=0`` gives the tokens of ``schedule='linear'``).  Under per-image
        step counts row i is built for e_i and image i equals image i of its one-count call.  In a captured graph the table is one
        more input [B][S + 1]: one graph per (batch, S, conditional, per-image steps) serves every table.  No new noise counters:
        ``set_shard`` works unchanged.  Refused before a key is drawn (ValueError): a negative or non-integer entry, a non-zero
        entry at t <= 1, a wrong length.  ``spkdiff.schedules.run_counts_remask`` lists the (revealed, remasked) counts of a run."""
        h, w = self.shape
        if h * w > 64:
            raise NotImplementedError(f'spkdiff: sample_confident() ranks an image\'s positions in one wave: h * w <= 64, got {h} x {w}')
        return self._sample_call(temp, sample_steps, noise, record, x_init, known, top_k, top_p, confident=True,
                                 **({} if schedule is None and selection_noise is None and remask is None else
                                    {'schedule': schedule, 'selection_noise': selection_noise, 'scheduled': True}),
                                 **({} if remask is None else {'remask': remask}))

    @staticmethod
    def _remask_arg(remask, b, steps, S):
        """The remask table of a sample_confident(remask=) call for a batch of ``b``, checked and built on the
        host: ``steps`` = the b per-image step counts e_i <= S (a list) -> int32 [b, S + 1] CPU tensor, row i built for e_i and
        placed as ``spkdiff.schedules.weights_row`` places a schedule row."""
        from spkdiff import schedules as sch
        what = 'spkdiff: sample_confident(remask=)'
        if hasattr(remask, 'detach'):
            remask = remask.detach().cpu()
        if hasattr(remask, 'tolist') and getattr(remask, 'ndim', 0) >= 1:
            integers = (not remask.is_floating_point() and remask.dtype != torch.bool) if isinstance(remask, torch.Tensor) \
                else getattr(remask.dtype, 'kind', 'i') in 'iu'
            if not integers:
                raise ValueError(f'{what}: counts are integers, got an array of {remask.dtype}')
            if remask.ndim > 2:
                raise ValueError(f'{what}: a table is 1-D, per-image tables are [B, S + 1], got {tuple(remask.shape)}')
            remask = remask.tolist()
        elif hasattr(remask, 'item') and getattr(remask, 'ndim', 1) == 0:
            remask = remask.item()
        per_image = isinstance(remask, (list, tuple)) and len(remask) > 0 and \
            any(v is None or isinstance(v, (list, tuple)) or getattr(v, 'ndim', 0) >= 1 for v in remask)
        if per_image and len(remask) != b:
            raise ValueError(f'{what}: per-image tables take one entry per image of the call ({b}), got {len(remask)}')
        built, rows = {}, []
        for i in range(b):
            ri = remask[i] if per_image else remask
            ri = tuple(ri.tolist() if hasattr(ri, 'tolist') else ri) if isinstance(ri, (list, tuple)) or getattr(ri, 'ndim', 0) >= 1 else ri
            try:
                key = (ri, steps[i])
                hash(key)
            except TypeError:
                raise ValueError(f'{what}: an integer >= 0 or a table of integers >= 0, got {ri!r}') from None
            if key not in built:
                built[key] = sch.remask_row(ri, steps[i], S, what)
            rows.append(built[key])
        return torch.tensor(rows, dtype=torch.int32).reshape(b, S + 1)

    @staticmethod
    def _sched_arg(schedule, selection_noise, b, steps, S):
        """The two tables of a scheduled sample_confident() call for a batch of ``b``, checked and built on the
        host: ``steps`` = the b per-image step counts e_i <= S (a list) -> (w int32 [b, S + 1], a fp32 [b, S + 1]) CPU tensors;
        a = fp32(tau_i * (t - 1) / e_i) computed in fp64."""
        from spkdiff import schedules as sch
        what = 'spkdiff: sample_confident(schedule=)'
        if hasattr(schedule, 'detach'):
            schedule = schedule.detach().cpu()
        if hasattr(schedule, 'tolist') and getattr(schedule, 'ndim', 0) >= 1:
            integers = (not schedule.is_floating_point() and schedule.dtype != torch.bool) if isinstance(schedule, torch.Tensor) \
                else getattr(schedule.dtype, 'kind', 'i') in 'iu'
            if not integers:
                raise ValueError(f'{what}: weights are integers, got an array of {schedule.dtype}')
            if schedule.ndim > 2:
                raise ValueError(f'{what}: a table is 1-D, per-image tables are [B, S + 1], got {tuple(schedule.shape)}')
            schedule = schedule.tolist()
        if not (schedule is None or isinstance(schedule, (str, list, tuple))):
            raise ValueError(f"{what}: None, 'linear', 'cosine', a table of integer weights or one of these per image, got {schedule!r}")
        per_image = isinstance(schedule, (list, tuple)) and len(schedule) > 0 and \
            any(v is None or isinstance(v, (str, list, tuple)) or getattr(v, 'ndim', 0) >= 1 for v in schedule)
        if per_image and len(schedule) != b:
            raise ValueError(f'{what}: per-image schedules take one entry per image of the call ({b}), got {len(schedule)}')
        # every distinct (schedule, step count) builds its row once: a batch of 256 with one schedule is one row, not 256
        built, index = {}, []
        shared = tuple(schedule) if isinstance(schedule, list) and not per_image else schedule      # (a hashable key)
        for i in range(b):
            si = shared
            if per_image:
                si = schedule[i]
                si = tuple(si.tolist() if hasattr(si, 'tolist') else si) if not (si is None or isinstance(si, str)) else si
            key = (si, steps[i])
            if key not in built:
                built[key] = (len(built), sch.weights_row(si, key[1], S, what))
            index.append(built[key][0])
        rows = torch.tensor([r for _, r in built.values()], dtype=torch.int32).reshape(len(built), S + 1)
        rows = rows.expand(b, S + 1).contiguous() if len(built) == 1 else rows[torch.tensor(index)]
        tau = selection_noise
        if tau is None:
            taus = [0.0] * b
        elif isinstance(tau, (list, tuple)) or getattr(tau, 'ndim', 0) >= 1:
            tl = tau.detach().cpu().tolist() if hasattr(tau, 'detach') else (tau.tolist() if hasattr(tau, 'tolist') else list(tau))
            if getattr(tau, 'ndim', 1) != 1 or len(tl) != b:
                raise ValueError(f'spkdiff: per-image selection_noise takes one number per image of the call ({b}), got {tau!r}')
            taus = [sch.check_tau(v, 'spkdiff: selection_noise') for v in tl]
        else:
            taus = [sch.check_tau(tau.item() if hasattr(tau, 'item') else tau, 'spkdiff: selection_noise')] * b
        # a[i][t] = tau_i * (t - 1) / e_i for 1 <= t <= e_i (spkdiff.schedules.noise_scales, all rows at once: the same two fp64
        # operations), 0 elsewhere; rounded to fp32 once
        t = torch.arange(S + 1, dtype=torch.float64)[None, :]
        e = torch.tensor(steps, dtype=torch.float64)[:, None]
        a = torch.tensor(taus, dtype=torch.float64)[:, None] * (t - 1) / e
        a = torch.where((t >= 1) & (t <= e), a, torch.zeros((), dtype=torch.float64)).to(torch.float32)
        if not bool(torch.isfinite(a).all()):
            raise ValueError('spkdiff: selection_noise is too large for fp32')
        return rows, a.reshape(b, S + 1)

    @staticmethod
    def _steps_arg(sample_steps, b):
        """The ``sample_steps`` of sample_confident() for a batch of ``b``: None or anything that is one integer (a Python or numpy
        integer, a 0-dim tensor or array) is the one-count call -- returned as it came; a list / tuple or a 1-D tensor / array is one
        count per image -- ``b`` integers >= 1 (ValueError otherwise), returned as a CPU int32 tensor [b] (a device tensor: its one
        read-back)."""
        if sample_steps is None or not (isinstance(sample_steps, (list, tuple)) or getattr(sample_steps, 'ndim', 0) >= 1):
            return sample_steps
        on_device = isinstance(sample_steps, torch.Tensor) and sample_steps.is_cuda
        got = f'a device tensor {sample_steps.dtype} {tuple(sample_steps.shape)}' if on_device else repr(sample_steps)
        bad = ValueError(f'spkdiff: per-image sample_steps takes one integer >= 1 per image of the call ({b}), got {got}')
        try:
            v = sample_steps.detach().cpu() if isinstance(sample_steps, torch.Tensor) else torch.as_tensor(sample_steps)
        except (TypeError, ValueError, RuntimeError):
            raise bad from None
        if v.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise bad
        if v.dim() != 1 or int(v.numel()) != b or bool((v < 1).any()) or bool((v > 0x7FFFFFFF).any()):
            raise bad
        return v.to(torch.int32)

    def _sample_call(self, temp, sample_steps, noise, record, x_init, known, top_k, top_p=None, confident=False, schedule=None,
                     selection_noise=None, scheduled=False, remask=None):
        start = self._start_state_args(x_init, known)
        b = int(self.n_samples) if start is None else int(start[0].shape[0])
        steps_b = None
        if confident:
            sample_steps = self._steps_arg(sample_steps, b)
            if isinstance(sample_steps, torch.Tensor) and sample_steps.dim() == 1:
                # per-image step counts: the loop runs the largest, every image its own
                if record is not None:
                    raise ValueError('spkdiff: sample_confident() with per-image sample_steps takes no record= (a record holds the '
                                     'logits of every image at every step; the steps run on the pending images only)')
                if self.noise_layout != 'global':
                    raise ValueError("spkdiff: per-image sample_steps needs the 'global' noise layout (one counter stride per step)")
                steps_b, sample_steps = sample_steps, int(sample_steps.max())
        sched = None
        if scheduled:
            # a reveal schedule / selection noise: both tables built on the host before anything is drawn
            S = int(self.num_timesteps if sample_steps is None else sample_steps)
            if S < 1:
                raise ValueError(f'spkdiff: sample_confident(schedule=, selection_noise=) takes sample_steps >= 1, got {S}')
            sched = self._sched_arg(schedule, selection_noise, b, [S] * b if steps_b is None else steps_b.tolist(), S)
            if remask is not None:
                # remasking: one more host-built table, on top of the scheduled family
                remask = self._remask_arg(remask, b, [S] * b if steps_b is None else steps_b.tolist(), S)
        temp = self._temp_arg(temp, b)
        top_k = self._topk_arg(top_k, b)
        top_p = self._topp_arg(top_p, b)
        dn = self._denoise_fn
        dev = next(dn.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('spkdiff: the sampler runs on a ROCm device; move the denoiser with .cuda()')
        temp = self._temp_on(temp, dev)
        if confident:
            # the confidence-ordered kernels exist on top of the most general family only: k = 0 / p = 1 are "untruncated"
            if not isinstance(temp, torch.Tensor) and not (temp > 0 and math.isfinite(temp)):
                raise ValueError(f'spkdiff: temp must be finite and > 0, got {temp!r}')
            top_p = 1.0 if top_p is None else top_p
        if top_p is not None:
            # a nucleus call takes all three per image (the `_topp` kernels read three arrays): no top_k is k = 0 everywhere
            top_p = self._topp_on(top_p, dev, b)
            top_k = 0 if top_k is None else top_k
        if top_k is not None:
            # a truncating call takes both per image: the `_topk` kernels read two arrays, and its graph two inputs
            top_k = self._topk_on(top_k, dev, b)
            if not isinstance(temp, torch.Tensor):
                temp = torch.full((b,), temp, dtype=torch.float32, device=dev)
        h, w = self.shape
        if start is not None and (start[0].device != dev or start[1].device != dev):
            raise ValueError(f'spkdiff: x_init / known must be on the denoiser\'s device {dev}')
        if sample_steps is None:
            sample_steps = self.num_timesteps
        if steps_b is not None:
            steps_b = steps_b.to(dev)
        seed = 0
        if noise is None and self.noise_source == 'philox':
            seed = self._philox_key()
            self.last_key = seed               # (read-only record: bench.py compares it across ranks after a timed region)
        self._check_weights(dn)
        form = self._form(b, h, w, record is not None)
        if confident:
            form = SampleForm(skip=False, lists=False, tail=dn.tail_fusable(h, w), tail_act=False)
        if steps_b is not None:
            # the pending images as an active list; no position lists (which positions change depends on the logits), no step tail
            form = SampleForm(skip=True, lists=False, tail=False, tail_act=False)
        return self._reverse_process(dev, b, h, w, form, temp, int(sample_steps), noise, seed, start, record, top_k=top_k,
                                     **({} if top_p is None else {'top_p': top_p}), **({'confident': True} if confident else {}),
                                     **({} if steps_b is None else {'steps_b': steps_b}),
                                     **({} if sched is None else {'sched': sched}), **({} if remask is None else {'remask': remask}))

    def _topp_arg(self, top_p, b):
        """The ``top_p`` of sample_top_p() for a batch of ``b``, checked before anything is drawn or launched.  None: no nucleus
        truncation.  A number in (0, 1] (anything ``float()`` takes that is no bool: a Python or numpy number, a 0-dim tensor or
        array): that p for every image -- returns the float.  Otherwise one entry per image: host data (a list / tuple, a numpy
        array, a CPU tensor) must be ``b`` finite numbers in (0, 1] (1: that image is not truncated; ValueError for a wrong length,
        an entry outside (0, 1], a NaN or a bool) and comes back as a CPU fp32 tensor [b]; a device tensor is taken as given --
        fp32 [b], its values are not read (the kernels leave an image whose p is outside (0, 1) untruncated)."""
        if top_p is None:
            return None
        # (a device tensor first: the message below prints its argument, which for a device tensor is a read-back of every entry)
        if isinstance(top_p, torch.Tensor) and top_p.is_cuda:
            if top_p.dim() != 1 or int(top_p.numel()) != b or top_p.dtype != torch.float32:
                raise ValueError(f'spkdiff: a per-image top_p on the device must be fp32 [{b}] (one entry per image of the call), '
                                 f'got {top_p.dtype} {tuple(top_p.shape)}')
            return top_p.contiguous()
        bad = ValueError(f'spkdiff: top_p must be None, a number in (0, 1] or one such number per image of the call ({b}), '
                         f'got {top_p!r}')
        if isinstance(top_p, bool):
            raise bad
        try:
            v = top_p.detach() if isinstance(top_p, torch.Tensor) else torch.as_tensor(top_p)
            if v.dtype in (torch.bool, torch.complex64, torch.complex128) or v.dim() > 1 or (v.dim() == 1 and int(v.numel()) != b):
                raise bad
            # (host numbers are read in fp64: as_tensor alone would round a Python float to fp32 before the range check)
            v = v.to(torch.float64) if isinstance(top_p, torch.Tensor) else torch.as_tensor(top_p, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise bad from None
        if not bool(torch.isfinite(v).all()) or not bool(((v > 0) & (v <= 1)).all()):
            raise bad
        # (what the kernels compare is the fp32 value: a p that rounds to 0 in fp32 would switch the truncation off)
        if not bool((v.to(torch.float32) > 0).all()):
            raise bad
        return float(v) if v.dim() == 0 else v.to(torch.float32)

    @staticmethod
    def _topp_on(top_p, dev, b):
        """``_topp_arg``'s result for the kernels: fp32 [b] on the denoiser's device (a number: broadcast; host data: its one copy)."""
        if not isinstance(top_p, torch.Tensor):
            return torch.full((b,), float(top_p), dtype=torch.float32, device=dev)
        if top_p.is_cuda and top_p.device != dev:
            raise ValueError(f'spkdiff: a per-image top_p must be on the denoiser\'s device {dev}, got {top_p.device}')
        return top_p.to(dev)

    def _topk_arg(self, top_k, b):
        """The ``top_k`` of sample_top_k() for a batch of ``b``, checked before anything is drawn or launched.  None: no
        truncation.  An int >= 1 (a Python or numpy integer, a 0-dim integer tensor or array; not a bool): that k for every image
        -- returns the int.  Otherwise one entry per image: host data (a list / tuple, a numpy array, a CPU tensor) must be ``b``
        integers >= 0 (0: that image is not truncated; ValueError for a wrong length, a negative entry, a non-integer or a bool)
        and comes back as a CPU int32 tensor [b]; a device tensor is taken as given -- int32 [b], its values are not read."""
        if top_k is None:
            return None
        # (a device tensor first: the message below prints its argument, which for a device tensor is a read-back of every entry)
        if isinstance(top_k, torch.Tensor) and top_k.is_cuda:
            if top_k.dim() != 1 or int(top_k.numel()) != b or top_k.dtype != torch.int32:
                raise ValueError(f'spkdiff: a per-image top_k on the device must be int32 [{b}] (one entry per image of the call), '
                                 f'got {top_k.dtype} {tuple(top_k.shape)}')
            return top_k.contiguous()
        bad = ValueError(f'spkdiff: top_k must be None, an int >= 1 or one integer >= 0 per image of the call ({b}), got {top_k!r}')
        if isinstance(top_k, bool):
            raise bad
        try:
            v = top_k.detach() if isinstance(top_k, torch.Tensor) else torch.as_tensor(top_k)
        except (TypeError, ValueError, RuntimeError):
            raise bad from None
        if v.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
            raise bad                          # (floats, bools, complex: not a count)
        if v.dim() == 0:
            if int(v) < 1:
                raise bad
            return int(v)
        if v.dim() != 1 or int(v.numel()) != b or bool((v < 0).any()) or bool((v > 0x7FFFFFFF).any()):
            raise bad
        return v.to(torch.int32)

    @staticmethod
    def _topk_on(top_k, dev, b):
        """``_topk_arg``'s result for the kernels: int32 [b] on the denoiser's device (an int: broadcast; host data: its one copy)."""
        if not isinstance(top_k, torch.Tensor):
            return torch.full((b,), int(top_k), dtype=torch.int32, device=dev)
        if top_k.is_cuda and top_k.device != dev:
            raise ValueError(f'spkdiff: a per-image top_k must be on the denoiser\'s device {dev}, got {top_k.device}')
        return top_k.to(dev)

    def _temp_arg(self, temp, b):
        """The ``temp`` of sample() / score() for a batch of ``b``, checked before anything is drawn or launched.  Anything
        ``float()`` takes -- a number, a 0-dim or one-element tensor or array -- is the scalar call, as ever: returns the float.
        Otherwise one entry per image: host data (a list / tuple, a numpy array, a CPU tensor) must have ``b`` finite entries
        > 0 (ValueError otherwise) and comes back as a CPU fp32 tensor [b]; a device tensor is taken as given -- fp32 [b], its
        values are not read (the kernels divide by whatever is there: include/spkdiff.h)."""
        if isinstance(temp, torch.Tensor):
            if temp.dim() == 0 or (temp.numel() == 1 and b != 1):
                return float(temp)
            if temp.is_cuda:
                if temp.dim() != 1 or int(temp.numel()) != b or temp.dtype != torch.float32:
                    raise ValueError(f'spkdiff: a per-image temp on the device must be fp32 [{b}] (one entry per image of the '
                                     f'call), got {temp.dtype} {tuple(temp.shape)}')
                return temp.contiguous()
            v = temp.detach().to(torch.float64)
        elif isinstance(temp, (list, tuple)) or (hasattr(temp, '__array__') and getattr(temp, 'ndim', 0) > 0 and
                                                 not (getattr(temp, 'size', 0) == 1 and b != 1)):
            v = torch.as_tensor(temp, dtype=torch.float64)
        else:
            return float(temp)
        if v.dim() != 1 or int(v.numel()) != b:
            raise ValueError(f'spkdiff: a per-image temp takes one entry per image of the call: {b}, got shape {tuple(v.shape)}')
        if not bool(torch.isfinite(v).all()) or not bool((v > 0).all()):
            raise ValueError('spkdiff: every per-image temperature must be finite and > 0')
        return v.to(torch.float32)

    @staticmethod
    def _temp_on(temp, dev):
        """``_temp_arg``'s result for the kernels: the float, or the vector on the denoiser's device (host data: its one copy)."""
        if not isinstance(temp, torch.Tensor):
            return temp
        if temp.is_cuda and temp.device != dev:
            raise ValueError(f'spkdiff: a per-image temp must be on the denoiser\'s device {dev}, got {temp.device}')
        if temp.numel() == 1:                  # (a batch of one: the scalar call)
            return float(temp)
        return temp.to(dev)

    @torch.no_grad()
    def score(self, x_0, temp=1.0, sample_steps=None, orders=1, noise=None, record=None, known=None):
        """The reverse process of ``sample(temp, sample_steps)`` run teacher-forced on the tokens ``x_0``: a lower bound on
        log p(x_0) under the sampler.  Same unmask draws and denoiser calls as sample(); the token written at a
        revealed position is x_0's, and its log-probability under softmax(logits / temp) is kept (spk_pscore_step).  Returns
        ``Score(position_log_prob fp64 [orders,B,h,w] nats, reveal_step int32 [orders,B,h,w], log_prob fp64 [orders,B])``, all on
        the device, no host synchronisation; every order is one unbiased estimate of the bound (averaging orders tightens the
        estimate, not the bound).

        ``x_0``: integer device tensor [B,1,h,w] or [B,h,w]; the batch is its first dimension (``n_samples`` is neither read nor
        changed).  A token outside [0, num_classes) scores -inf.  ``known`` (bool / uint8, x_0's shape): the loop starts from the
        completion start state of sample(x_init=x_0, known=known) and bounds log p(x_unknown | x_known); known positions hold 0 / 0.
        Noise: sample()'s contract -- one key draw per order from torch's global CPU generator ('philox' mode; ``last_key`` keeps
        the last), counters on the global image index (``set_shard``), the same key broadcast rule; ``noise`` = t -> (u, q) injects
        (only u is read); ``noise_source = 'host'`` draws u only.  ``record`` receives (t, x_t, unmasked, logits) per step as in
        sample() (dense form).  With ``use_graph`` and neither ``noise`` nor ``record`` an order is one replay of a captured graph
        that takes x_0 and ``known`` as inputs (a key of its own; sample()'s graphs and keys are untouched).
        ``temp``: a number or one temperature per image, as in sample() (every order scores image i at ``temp[i]``).  There is no
        ``top_k`` here (sample_top_k): under truncation a given token outside the kept set scores -inf, not a useful bound.  Nor is there a
        ``confident`` flag (sample_confident): the bound is derived for the coin's reveal order, which does not look at the logits;
        an order chosen from them is another process, whose likelihood this loop does not bound."""
        if isinstance(x_0, torch.Tensor) and x_0.dim() in (3, 4):      # (host checks of a per-image temp: before the device is looked at)
            temp = self._temp_arg(temp, int(x_0.shape[0]))
        start = self._start_state_args(x_0, known, what='x_0', call='score()', alone=True)
        orders = int(orders)
        if orders < 1:
            raise ValueError(f'spkdiff: score() takes orders >= 1, got {orders}')
        dn = self._denoise_fn
        dev = next(dn.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('spkdiff: the sampler runs on a ROCm device; move the denoiser with .cuda()')
        if any(t is not None and t.device != dev for t in start):
            raise ValueError(f'spkdiff: x_0 / known must be on the denoiser\'s device {dev}')
        x0 = start[0]
        b = int(x0.shape[0])
        temp = self._temp_on(temp, dev)
        h, w = self.shape
        if sample_steps is None:
            sample_steps = self.num_timesteps
        self._check_weights(dn)
        # (a score call never takes the fused-tail forms: their launch samples the token itself)
        form = self._form(b, h, w, record is not None)._replace(tail=False, tail_act=False)
        logp = torch.zeros((orders, b, h, w), dtype=torch.float64, device=dev)
        step = torch.zeros((orders, b, h, w), dtype=torch.int32, device=dev)
        for o in range(orders):
            seed = 0
            if noise is None and self.noise_source == 'philox':
                seed = self._philox_key()
                self.last_key = seed
            self._reverse_process(dev, b, h, w, form, temp, int(sample_steps), noise, seed,
                                  None if known is None else start, record, target=(x0, logp[o], step[o]))
        return Score(logp, step, logp.sum(dim=(2, 3)))

    def _reverse_process(self, dev, b, h, w, form, temp, sample_steps, noise, seed, start, record, target=None, top_k=None,
                         top_p=None, confident=False, steps_b=None, sched=None, remask=None):
        """One reverse process of sample() / score(): a replay of its captured graph where the call allows one, else eager."""
        if self.use_graph and noise is None and record is None and self.noise_source == 'philox':
            self._capturing = False
            try:
                return self._sample_graphed(dev, b, h, w, form, temp, sample_steps, seed, start=start, target=target, top_k=top_k,
                                            **({} if top_p is None else {'top_p': top_p}),
                                            **({'confident': True} if confident else {}),
                                            **({} if steps_b is None else {'steps_b': steps_b}),
                                            **({} if sched is None else {'sched': sched}),
                                            **({} if remask is None else {'remask': remask}))
            except (NotImplementedError, ValueError, TypeError):
                raise                          # an argument / support error of a kernel, not a capture problem
            except RuntimeError as e:
                # Only a failure raised while the capture block was open is a capture problem (the runtime refused an
                # operation on a capturing stream, another thread touched the device, ...): same kernels, launched one by
                # one.  The kernels' own return codes surface as ValueError / NotImplementedError / SpkdiffError with the
                # entry point's name and propagate.
                from spkdiff._lib import SpkdiffError
                if not self._capturing or isinstance(e, SpkdiffError):
                    raise
                import warnings
                warnings.warn(f'spkdiff: hipGraph capture of the sampler failed ({e}); launching eagerly')
                self.use_graph = False
                self._graphs.clear()
                torch.cuda.synchronize(dev)
            finally:
                self._capturing = False
        return self._sample_eager(dev, b, h, w, form, temp, sample_steps, noise, seed, start, record, target, top_k,
                                  **({} if top_p is None else {'top_p': top_p}), **({'confident': True} if confident else {}),
                                  **({} if steps_b is None else {'steps_b': steps_b}), **({} if sched is None else {'sched': sched}),
                                  **({} if remask is None else {'remask': remask}))

    def _sample_eager(self, dev, b, h, w, form, temp, sample_steps, noise=None, seed=0, start=None, record=None, target=None,
                      top_k=None, top_p=None, confident=False, steps_b=None, sched=None, remask=None):
        """The reverse process launched kernel by kernel: fresh state buffers, the one step loop.  ``target = (x0, logp, step)``:
        the teacher-forced loop of score() -- logp / step are the caller's zeroed outputs, and of the noise only u is drawn."""
        x_t = torch.empty((b, 1, h, w), dtype=torch.int64, device=dev)
        unmasked = torch.empty((b, 1, h, w), dtype=torch.bool, device=dev)
        self._fill_start(x_t, unmasked, start)
        if sched is not None:
            sched = (sched[0].to(dev), sched[1].to(dev))            # (the host-built tables of sample_confident(schedule=, ...))
        if remask is not None:
            remask = (remask.to(dev), self._commit_conf_start(unmasked))
        if noise is None and self.noise_source == 'host':
            # u and q from torch's global CPU generator in the reference's order: rand_like(x_t.float()) (:116), then
            # multinomial's one-draw fast path (:138); the denoiser call between them there draws nothing
            K = self.num_classes
            if target is None:
                noise = lambda t: (torch.rand(b, 1, h, w).to(dev), torch.empty(b * h * w, K).exponential_(1).to(dev))      # noqa: E731
            else:
                noise = lambda t: (torch.rand(b, 1, h, w).to(dev), None)      # noqa: E731
        need = ops.NeedLists(b, int(self.list_radii), dev) if form.lists else None
        self._reverse_steps(x_t, unmasked, form, _Noise(noise, seed), temp, sample_steps, need=need, record=record, target=target,
                            top_k=top_k, **({} if top_p is None else {'top_p': top_p}), **({'confident': True} if confident else {}),
                            **({} if steps_b is None else {'steps_b': steps_b}), **({} if sched is None else {'sched': sched}),
                            **({} if remask is None else {'remask': remask}))
        return x_t

    @staticmethod
    def _commit_conf_start(unmasked):
        """commit_conf of a remasking run from its start state, one capturable launch: +inf where a position is
        unmasked -- a known token, never revisited --, 0 (never read before a reveal writes it) elsewhere; fp32, the shape of
        ``unmasked``."""
        return torch.where(unmasked, math.inf, 0.0)

    def _fill_start(self, x_t, unmasked, start):
        """Start state into the given buffers: all masked, or ``start = (codes, keep)`` through spk_completion_state."""
        if start is None:
            x_t.fill_(int(self.mask_id))
            unmasked.zero_()
        else:
            ops.completion_state(start[0], start[1], self.num_classes, int(self.mask_id), out=(x_t, unmasked))

    def _reverse_steps(self, x_t, unmasked, form, src, temp, sample_steps, act=None, need=None, inp=None, record=None, target=None,
                       top_k=None, top_p=None, confident=False, steps_b=None, sched=None, remask=None):
        """THE reverse-process loop (R/snn_model/vq_diffusion.py:113-140): steps t = sample_steps .. 1 on ``x_t`` / ``unmasked``
        in place, in launch form ``form`` with the noise of ``src`` (_Noise); eager call and captured graph both run it.
        ``act``: the pair spk_select_active writes (None: the first step allocates it); ``need``: the NeedLists of ``form.lists``;
        ``inp``: dense form without the fused tail -- [B,2,h,w] buffer of the denoiser input, built once and then written by
        every spk_psample_step (one launch less per step; None: every step builds its own); ``record``: see sample();
        ``target = (x0, logp, step)``: teacher-forced (score()) -- the token update of every step is spk_pscore_step, which writes
        the given token x0 where spk_psample_step writes a sampled one and leaves its log-probability in logp, t in step (never a
        fused-tail form: ``form.tail`` / ``form.tail_act`` are off there); ``top_k``: int32 device tensor [B] -- handed to every token
        update of sample_top_k() and to nothing else (None: the calls carry no such keyword); ``top_p``: fp32 device tensor [B] of
        sample_top_p(), handed on in the same way (then always with ``top_k``); ``confident``: sample_confident() -- the token update of
        every step is the confidence-ordered one (spk_den_step_tail_conf, or spk_psample_step_conf after the denoiser; always the
        dense form, always with ``top_k`` and ``top_p``, never with ``target``); ``steps_b``: int32 device tensor [B], the per-image
        step counts of sample_confident() (``sample_steps`` is then their maximum S, ``form`` the elimination form
        without lists or tails) -- every step runs on the list spk_select_pending writes: the denoiser by slot, then
        spk_psample_step_conf_listed, which shifts image i's counters to those of its own run of min(steps_b[i], S) steps;
        ``sched = (w int32 [B, S + 1], a fp32 [B, S + 1])`` on the loop's device: a scheduled sample_confident() (then
        ``confident``, S = ``sample_steps``) -- every token update is the ``_sched`` sibling of the one it would be, with the two
        tables, and an injected u is handed on as the Gumbel uniform; ``remask = (r int32 [B, S + 1], commit_conf fp32 [B,1,h,w])`` on
        the loop's device (then with ``sched``): every token update is the ``_remask`` sibling, commit_conf holds +inf
        at the start state's unmasked positions and is updated in place."""
        dn = self._denoise_fn
        trunc = {} if top_k is None else {'top_k': top_k}
        if top_p is not None:
            trunc['top_p'] = top_p
        if confident:
            trunc['confident'] = True
        if sched is not None:
            trunc['sched'] = sched + (sample_steps,)
        if remask is not None:
            remask = remask + (int(self.mask_id),)
            trunc['remask'] = remask
        b, _, h, w = x_t.shape
        K = self.num_classes
        seed, state = src.seed, src.state
        pre1 = None
        for t in reversed(range(1, sample_steps + 1)):
            u, q = (None, None) if src.draw is None else src.draw(t)
            off = self._step_offset(sample_steps - t, b, h, w, K)
            if steps_b is not None:
                act = ops.select_pending(unmasked, t, steps_b, out=act)
            elif form.skip:
                act = ops.select_active(unmasked, t, u, seed, off, philox_state=state, out=act, K=K)
                if form.lists:
                    ops.select_needed(unmasked, t, act, need, u, seed, off, philox_state=state, K=K)
            elif inp is not None and t == sample_steps:
                ops.den_build_input(x_t, t, out=inp)
            with ops.active_set(*(act if form.skip else (None, None)), need=need):
                if form.tail or form.tail_act:
                    # conv6 on the counts + the token update as ONE launch -- dense: with the next step's first layer (pre1);
                    # elimination: per active slot, without it (that layer belongs to the next step's active set)
                    pre1, logits = dn.sample_step(x_t, unmasked, t, temp, u, q, seed, off, philox_state=state, pre1=pre1,
                                                  want_next=form.tail and t > 1, want_logits=record is not None, **trunc)
                else:
                    logits = dn.logits_from_tokens(x_t, t, inp=inp)          # denoiser + reset_net (:128-129)
                    if steps_b is not None and remask is not None:
                        ops.psample_step_conf_listed_remask(logits, x_t, unmasked, t, temp, steps_b, sample_steps, self.STEP_STRIDE,
                                                            sched[0], *remask, noise_a=sched[1], u=u, q=q, seed=seed, offset=off,
                                                            philox_state=state, top_k=top_k, top_p=top_p)
                    elif remask is not None:
                        ops.psample_step_conf_remask(logits, x_t, unmasked, t, temp, sched[0], sample_steps, *remask, noise_a=sched[1],
                                                     u=u, q=q, seed=seed, offset=off, philox_state=state,
                                                     next_input=inp if t > 1 else None, top_k=top_k, top_p=top_p)
                    elif steps_b is not None and sched is not None:
                        ops.psample_step_conf_listed_sched(logits, x_t, unmasked, t, temp, steps_b, sample_steps, self.STEP_STRIDE,
                                                           sched[0], sched[1], u, q, seed, off, philox_state=state, top_k=top_k,
                                                           top_p=top_p)
                    elif steps_b is not None:
                        ops.psample_step_conf_listed(logits, x_t, unmasked, t, temp, steps_b, sample_steps, self.STEP_STRIDE, u, q,
                                                     seed, off, philox_state=state, top_k=top_k, top_p=top_p)
                    elif sched is not None:
                        ops.psample_step_conf_sched(logits, x_t, unmasked, t, temp, sched[0], sample_steps, sched[1], u, q, seed, off,
                                                    philox_state=state, next_input=inp if t > 1 else None, top_k=top_k, top_p=top_p)
                    elif confident:
                        ops.psample_step_conf(logits, x_t, unmasked, t, temp, u, q, seed, off, philox_state=state,
                                              next_input=inp if t > 1 else None, top_k=top_k, top_p=top_p)
                    elif target is None:
                        ops.psample_step(logits, x_t, unmasked, t, temp, u, q, seed, off, philox_state=state,
                                         next_input=inp if t > 1 else None, **trunc)
                    else:
                        ops.pscore_step(logits, target[0], x_t, unmasked, t, temp, target[1], target[2], u, seed, off,
                                        philox_state=state, next_input=inp if t > 1 else None)
            if record is not None:
                record.append((t, x_t.clone(), unmasked.clone(), logits.clone()))

    def _start_state_args(self, x_init, known, what='x_init', call='sample()', alone=False):
        """Argument checks of ``sample(x_init=, known=)``, before anything is drawn or launched: None for the unconditional call,
        else (codes int64 [B,h,w], keep uint8 [B,h,w]) contiguous on the device.  ``alone`` (score(): ``what`` = 'x_0' is the
        tokens to score and ``known`` optional): x alone is a call too and gives (codes, None)."""
        if x_init is None and known is None and not alone:
            return None
        if (x_init is None or known is None) and not (alone and x_init is not None):
            raise ValueError(f'spkdiff: {call} takes {what} and known together (both or neither)' if not alone else
                             f'spkdiff: {call} takes the tokens {what} to score')
        given = ((what, x_init),) if known is None else ((what, x_init), ('known', known))
        if not all(isinstance(t, torch.Tensor) for _, t in given):
            raise TypeError(f'{" and ".join(n for n, _ in given)} must be torch.Tensors, got {" and ".join(str(type(t)) for _, t in given)}')
        if known is not None and x_init.shape != known.shape:
            raise ValueError(f'spkdiff: {what} {tuple(x_init.shape)} and known {tuple(known.shape)} must have the same shape')
        h, w = self.shape
        if not ((x_init.dim() == 3 and tuple(x_init.shape[1:]) == (h, w)) or
                (x_init.dim() == 4 and tuple(x_init.shape[1:]) == (1, h, w))) or x_init.shape[0] < 1:
            raise ValueError(f'spkdiff: {what} {tuple(x_init.shape)} must be [B,1,{h},{w}] or [B,{h},{w}] (the sampler\'s shape)')
        if x_init.is_floating_point() or x_init.is_complex() or x_init.dtype == torch.bool:
            raise NotImplementedError(f'spkdiff: {what} must be an integer tensor, got {x_init.dtype}')
        if known is not None and known.dtype not in (torch.bool, torch.uint8):
            raise NotImplementedError(f'spkdiff: known must be bool or uint8, got {known.dtype}')
        for name, t in given:
            if not t.is_cuda:
                raise RuntimeError(f"spkdiff: {name} is on '{t.device}'. The HIP kernels are the implementation; "
                                   "there is no CPU path (move the module / tensors to a ROCm device).")
        B = int(x_init.shape[0])
        codes = x_init.reshape(B, h, w).to(torch.int64).contiguous()
        if known is None:
            return codes, None
        keep = known.reshape(B, h, w).contiguous()
        return codes, (keep.view(torch.uint8) if keep.dtype == torch.bool else keep)

    def _list_ok(self, h, w, b=None):
        return bool(self.list_positions) and (h, w) == (7, 7) and (b is None or b >= int(self.list_min_batch))

    def _form(self, b, h, w, recording=False):
        """THE decision of the launch form (SampleForm) for a batch of ``b`` on an h x w latent: the eager call, the captured
        graph, its cache key and ``form_for`` read it.  Every kernel family takes the device-side image count, so
        ``skip_untouched`` holds at any shape -- but not under ``record=``: a record holds the logits of EVERY image at every
        step, and the elimination forms compute them per slot of the active list, for the touched images only."""
        skip = bool(self.skip_untouched) and not recording
        fused = (not skip or bool(self.step_tail_in_elimination)) and self._denoise_fn.tail_fusable(h, w)
        return SampleForm(skip=skip, lists=skip and self._list_ok(h, w, b), tail=fused and not skip, tail_act=fused and skip)

    def form_for(self, b, h, w, sample_steps=None):
        """Name of the launch form ``sample()`` takes for a batch of ``b`` on an h x w latent (same tokens in every form)."""
        form = self._form(b, h, w)
        if not form.skip:
            return 'dense_step_tail' if form.tail else 'dense'
        return 'elimination_lists' if form.lists else 'elimination'

    STEP_STRIDE = 1 << 40        # 'global' layout: counters of one reverse step (images * h*w * K of them must fit)

    def set_shard(self, first: int, count: int = None):
        """This sampler generates images [first, first + count) of a larger job ('global' noise layout): the draws of an
        image are those the whole job would make for it.  ``count`` (optional) also sets ``n_samples``."""
        self.global_first = int(first)
        self._shard_set = True
        if count is not None:
            self.n_samples = int(count)
        return self

    def _step_offset(self, step_index, b, h, w, K):
        """Philox counter offset of reverse step number ``step_index`` (0 = the first step taken) for this sampler's shard."""
        if self.noise_layout == 'global':
            if (int(self.global_first) + b) * h * w * K > self.STEP_STRIDE:
                raise ValueError('spkdiff: global noise layout holds 2^40 counters per reverse step')
            return step_index * self.STEP_STRIDE + int(self.global_first) * h * w * K
        if self.noise_layout != 'rank':
            raise ValueError("noise_layout must be 'global' or 'rank'")
        return step_index * (b * h * w * K)

    @contextlib.contextmanager
    def _one_key(self):
        """Context: ONE noise key for every sample() / score() call inside -- the calls of a job that runs as several shards of one
        sampler (spkdiff.evaluate.temperature_sweep).  The key is an ordinary draw, made here (one draw from torch's CPU generator,
        broadcast under ``_philox_key``'s rule: call ``set_shard`` first); the calls inside draw nothing."""
        if self._pinned_key is not None:
            raise RuntimeError('spkdiff: _one_key() does not nest')
        self._pinned_key = self._philox_key()
        try:
            yield self._pinned_key
        finally:
            self._pinned_key = None

    def _philox_key(self):
        if self._pinned_key is not None:
            return self._pinned_key
        draw = int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64))
        if self.noise_layout == 'global':
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                if not self._shard_set:
                    if not self._warned_unsharded:
                        import warnings
                        warnings.warn("spkdiff: sample() inside a process group without set_shard(): no key broadcast, the rank "
                                      "is folded into the key (per-rank images).  Call set_shard(first, count) on every rank "
                                      "(spkdiff.dist.sample_images_sharded(..., sampler=ab) does) for one split-independent job.")
                        self._warned_unsharded = True
                    return (draw ^ ((int(dist.get_rank()) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF)) & 0x7FFFFFFFFFFFFFFF
                if self.sync_key:
                    dev = next(self._denoise_fn.parameters()).device if dist.get_backend() == 'nccl' else 'cpu'
                    k = torch.tensor([draw], dtype=torch.int64, device=dev)
                    dist.broadcast(k, 0)
                    draw = int(k.item())
            return draw & 0x7FFFFFFFFFFFFFFF
        return (draw ^ ((int(self.philox_stream) * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF)) & 0x7FFFFFFFFFFFFFFF

    def invalidate(self):
        """Drop captured graphs and every derived weight form of the denoiser (see spkdiff.fused.invalidate_derived)."""
        self._graphs.clear()
        invalidate_derived(self._denoise_fn)

    def _check_weights(self, dn):
        """Content checksum of the denoiser's floating-point tensors against the one seen by the previous call: a change
        that left every (data_ptr, _version) pair alone -- ``p.data.copy_(...)``, an optimizer step replayed from a graph
        -- drops the derived forms and the captured graphs here."""
        if not self.verify_weights:
            return
        ts = [t for t in list(dn.parameters()) + list(dn.buffers()) if t.is_floating_point() and t.is_cuda]
        ws = self._wsum
        if ws is None or ws[0].key != ops.TensorChecksum.key_of(ts):
            # (another set of tensors -- e.g. the training path re-laid the weights out channels-last: a new address -- is a
            #  change by itself: whatever was derived from the old ones is dropped)
            if ws is not None:
                self.invalidate()
            ws = self._wsum = [ops.TensorChecksum(ts), None]
        v = ws[0].value()
        if ws[1] is not None and ws[1] != v:
            self.invalidate()
        ws[1] = v

    def _graph_key(self, dev, b, h, w, temp, sample_steps, form, conditional, score=False, top_k=None, top_p=None, confident=False,
                   per_image_steps=False, scheduled=False, remask=False):
        # (the two step-tail switches beside the form they feed: the key changes wherever a switch does, also where the form does not)
        dn = self._denoise_fn
        weights = tuple((p.data_ptr(), p._version) for p in list(dn.parameters()) + list(dn.buffers())) + derived_epoch(dn)
        first = int(self.global_first)
        if isinstance(temp, torch.Tensor):
            # per-image temperatures are a graph input: one graph for every vector -- and for every shard of a job that runs as
            # several calls (temperature_sweep): such a graph takes the shard's counter base as an input too (_sample_graphed)
            temp, first = 'per-image', 'any-shard'
        return (str(dev), b, h, w, self.num_classes, temp, sample_steps, int(self.mask_id), form, int(self.list_radii),
                bool(dn.use_step_tail), bool(self.step_tail_in_elimination), self.noise_layout, first, weights,
                conditional) + (('score',) if score else ()) + (('top-k',) if top_k is not None else ()) + \
            (('top-p',) if top_p is not None else ()) + (('confident',) if confident else ()) + \
            (('per-image-steps',) if per_image_steps else ()) + \
            (('scheduled',) if scheduled else ()) + \
            (('remask',) if remask else ())                         # (sample_steps is then S, the vector's maximum; the tables are inputs)

    def _graph_body(self, g, form, temp, sample_steps):
        """What a sampler graph captures: the start state, then the step loop on the graph's buffers, noise from its state
        (a score graph: its logp / step outputs zeroed first -- the loop writes them at the revealed positions only)."""
        self._fill_start(g.x_t, g.unmasked, g.start_in)
        if g.remask is not None:
            g.commit_conf = self._commit_conf_start(g.unmasked)     # (allocated inside the capture: the graph's own buffer)
        if g.target is not None:
            g.target[1].zero_()
            g.target[2].zero_()
        self._reverse_steps(g.x_t, g.unmasked, form, _Noise(state=g.state), temp if g.temps is None else g.temps, sample_steps,
                            act=g.act, need=g.need, inp=g.inp, target=g.target, top_k=g.topk,
                            **({} if g.topp is None else {'top_p': g.topp}), **({'confident': True} if g.confident else {}),
                            **({} if g.steps is None else {'steps_b': g.steps}), **({} if g.sched is None else {'sched': g.sched}),
                            **({} if g.remask is None else {'remask': (g.remask, g.commit_conf)}))

    def _sample_graphed(self, dev, b, h, w, form, temp, sample_steps, seed, start=None, target=None, top_k=None, top_p=None,
                        confident=False, steps_b=None, sched=None, remask=None):
        """Capture-once / replay-many form of ``_sample_eager``; same kernels, same results for the same seed.
        ``start = (codes, keep)``: the conditional form -- the start state is a graph INPUT (two static buffers filled before
        each replay; spk_completion_state is the first node in place of the two fills) and the graph has a key of its own.
        A per-image ``temp`` (device tensor [B]) is an input in the same way: the key carries a marker in place of the value and the
        vector is copied into the graph's ``temps`` buffer before each replay.  Such a graph is captured at ``global_first = 0`` and
        takes the shard's counter base ``global_first * h * w * K`` through the second word of ``state`` (the kernels add it to
        every step's offset: the same counters), so the calls of a sharded job share it; scalar calls keep the shard in the key.
        ``target = (x0, logp, step)``: a score graph (again a key of its own) -- x0 is one more input (with ``start`` it IS the
        codes input), logp / step receive the graph's outputs.  ``top_k`` (int32 device tensor [B]; ``temp`` is then a vector too):
        a truncating graph -- a marker in the key, the vector copied into the graph's ``topk`` buffer before each replay.
        ``top_p`` (fp32 device tensor [B]; then with ``top_k``): a nucleus graph -- one more marker, one more input (``topp``).
        ``confident``: the graph of sample_confident() (a nucleus graph whose token updates are the confidence-ordered ones): one more
        marker in the key, no further input.  ``steps_b`` (int32 device tensor [B]; then ``confident``, ``sample_steps`` = its maximum):
        a per-image-steps graph -- one more marker, one more input (``steps``): one graph serves every vector with
        the same maximum.  ``sched`` (the two device tables [B, S + 1] of a scheduled sample_confident()): one
        more marker, two more inputs of fixed shape -- one graph serves every schedule and every noise scale; they come as the
        host tensors they were built as and are copied straight into the graph's buffers.  ``remask`` (the host table [B, S + 1] of
        sample_confident(remask=); then with ``sched``): one more marker, one more input; commit_conf is a buffer of
        the graph that every replay re-initialises from the start state."""
        dn = self._denoise_fn
        key = self._graph_key(dev, b, h, w, temp, sample_steps, form, start is not None, target is not None, top_k=top_k, top_p=top_p,
                              **({'confident': True} if confident else {}),
                              **({} if steps_b is None else {'per_image_steps': True}),
                              **({} if sched is None else {'scheduled': True}),
                              **({} if remask is None else {'remask': True}))
        g = self._graphs.get(key)
        if g is None:
            if len(self._graphs) >= 2:                              # at most two live graphs per sampler (e.g. dense and
                self._graphs.clear()                                #  elimination forms): their buffers are not small
            g = _SamplerGraph(dev, b, h, w, form, int(self.list_radii), start is not None, target is not None,
                              per_image_temp=isinstance(temp, torch.Tensor), top_k=top_k is not None,
                              top_p=top_p is not None, **({'confident': True} if confident else {}),
                              **({} if steps_b is None else {'per_image_steps': True}),
                              **({} if sched is None else {'sched_steps': sample_steps}),
                              **({} if remask is None else {'remask': True}))
            # warm-up on a side stream (weight packing, BN terms, allocator pools, this graph's own flag workspaces), then capture
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side), ops.flag_scope(g.flag_ws):
                dn.logits_from_tokens(torch.full((b, 1, h, w), int(self.mask_id), dtype=torch.int64, device=dev), 1)
            torch.cuda.current_stream(dev).wait_stream(side)
            g.graph = torch.cuda.CUDAGraph()
            self._capturing = True
            first = self.global_first
            if g.temps is not None:
                self.global_first = 0                               # (the shard's base is the graph's input)
            try:
                with torch.cuda.graph(g.graph, capture_error_mode="thread_local"), ops.flag_scope(g.flag_ws):
                    self._graph_body(g, form, temp, sample_steps)
            finally:
                self.global_first = first
            self._capturing = False
            g.derived = derived_refs(dn)
            self._graphs[key] = g
        # (step 0's offset is the shard's counter base, range-checked as every step's is)
        base = 0 if g.temps is None else self._step_offset(0, b, h, w, self.num_classes)
        g.state.copy_(torch.tensor([seed, base], dtype=torch.int64), non_blocking=False)
        if g.temps is not None:
            g.temps.copy_(temp)
        if g.topk is not None:
            g.topk.copy_(top_k)
        if g.topp is not None:
            g.topp.copy_(top_p)
        if g.steps is not None:
            g.steps.copy_(steps_b)
        if g.sched is not None:
            g.sched[0].copy_(sched[0])
            g.sched[1].copy_(sched[1])
        if g.remask is not None:
            g.remask.copy_(remask)
        if start is not None:
            g.start_in[0].copy_(start[0])
            g.start_in[1].copy_(start[1])
        if target is not None:
            g.target[0].copy_(target[0])
            g.graph.replay()
            target[1].copy_(g.target[1])
            target[2].copy_(g.target[2])
            return g.x_t
        g.graph.replay()
        return g.x_t.clone()


class DummyModel(nn.Module):
    """Spiking convolutional denoiser ("SDID"); R/snn_model/vq_diffusion.py:150-208."""

    def __init__(self, n_channel: int, num_embeddings, n_steps: int = 16) -> None:
        super(DummyModel, self).__init__()
        self.num_embeddings = num_embeddings
        self.n_steps = n_steps

        def block(cin, cout):
            return FusedSequential(
                layer.Conv2d(in_channels=cin, out_channels=cout, kernel_size=3, stride=1, padding=1),
                layer.BatchNorm2d(cout),
                neuron.LIFNode(surrogate_function=surrogate.ATan()))

        self.conv1 = block(n_channel * 2, 64)
        self.conv2 = block(64, 128)
        self.conv3 = block(128, 256)
        self.conv4 = block(256, 512)
        self.conv5 = block(512, 256)
        self.conv6 = FusedSequential(
            layer.Conv2d(256 + 64, num_embeddings, 3, 1, 1),
        )

    def _fused_ok(self):
        return all(c._fusable(c._blocks()) for c in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5,
                                                     self.conv6)) and self.n_steps <= ops.MAX_T

    # 'mfma-fp6x6': conv2..conv5 on the block-scaled fp6/fp4 MFMA (six exact radix-32 digit planes), conv6 time-collapsed
    # on int8 spike counts; 'mfma-i8x4': conv2..conv6 on the int8 MFMA (four exact base-256 digit planes); 'direct-f64':
    # fp64-accumulating direct kernels.  All return correctly rounded pre-activations of (fixed-point) exact dot products.
    # Request: 'auto' (fastest supported), 'fp6', 'i8', 'direct'.
    conv_impl_request = 'auto'
    # conv6 + mean over T evaluated as ONE convolution of the per-neuron spike counts (exact linearity; the sum over T
    # is rounded once instead of T times: logits agree with the per-step form to ~1 ulp).  False = per-step form.
    collapse_conv6 = True

    _latent_hw = (7, 7)        # latent size of the last call (7x7 MNIST-shaped, 8x8 CIFAR-shaped)

    def _impl_base(self, h, w):
        """Kernel family used for conv2..conv6 on an h x w latent.  conv2..conv5 never see ``num_embeddings``; the fp6 families'
        logits layer runs on the spike counts with its output channels zero-padded to a multiple of 16 inside the packed weights
        (round 6), so EVERY --codebook_size the reference accepts (R/main.py:58) stays on the matrix cores.  Only the int8 family's
        per-step logits kernel (``collapse_conv6 = False`` or request 'i8') still needs a multiple of 16 and otherwise leaves the
        call to the fp64 direct kernels."""
        req = self.conv_impl_request
        if req == 'direct':
            return 'direct-f64'
        if (req in ('auto', 'fp6') and self.collapse_conv6 and
                ops.den_fp6_supported(128, 64, 3, 1, 1, self.n_steps, h, w)):
            return 'mfma-fp6x6'
        if self.conv6[0].out_channels % 16 != 0:
            return 'direct-f64'
        return 'mfma-i8x4' if ops.den_mfma_supported(128, 64, 3, 1, 1, self.n_steps, h, w) else 'direct-f64'

    # the sampler's calls (fresh LIF state, nothing written back) take the second-generation fp6 kernel where it applies
    # (7x7 latents): the same spikes from the four leading digits + certified decisions + exact recomputation of the few neurons
    # near the threshold (csrc/den_mfma_fp6v2.hip).  False = always the first-generation kernel.
    use_fp6v2 = True
    _last_stateful = False

    def impl_for(self, h, w, stateful=False):
        """Kernel family used for conv2..conv5 on an h x w latent (see _impl_base); stateless calls on 7x7 latents refine
        'mfma-fp6x6' to 'mfma-fp6v2'."""
        base = self._impl_base(h, w)
        if (base == 'mfma-fp6x6' and self.use_fp6v2 and not stateful and
                ops.den_fp6v2_supported(128, 64, 3, 1, 1, self.n_steps, h, w)):
            return 'mfma-fp6v2'
        return base

    @property
    def conv_impl(self):
        return self.impl_for(*self._latent_hw, stateful=self._last_stateful)

    def _trunk(self, inp_b2hw, stateful, record=None, pre1=None):
        """conv1 .. conv5 on the input map [B,2,h,w] (``pre1 = (spikes, counts)``: the first layer's output is already there --
        the previous reverse step's tail launch produced it).  Returns (x5, cnt5, x1, cnt1, which, impl, collapse)."""
        T = self.n_steps
        # spikes travel in the records each kernel family stages per K chunk (ops.LAYOUTS): S32 for fp6v2, C4 for the first fp6
        # kernel, CPTC of 32 u8 channels for the int8 and the direct kernels
        hw = (int(inp_b2hw.shape[-2]), int(inp_b2hw.shape[-1])) if pre1 is None else (int(pre1[0].shape[2]), int(pre1[0].shape[3]))
        self._latent_hw = hw
        self._last_stateful = bool(stateful)
        which = self.conv_impl
        impl = 'direct' if which == 'direct-f64' else 'auto'
        collapse = which != 'direct-f64' and self.collapse_conv6
        chunk = {'mfma-fp6v2': ops.S32, 'mfma-fp6x6': ops.C4}.get(which, ops.cptc(32)).chunk
        if pre1 is None:
            with ops.timed('den.conv1'):
                r1 = self.conv1.run(inp_b2hw, IN_TINV, final='ptc', T=T, stateful=stateful, chunk_out=chunk,
                                    want_counts=collapse)
            x1, cnt1 = r1['ptc'], r1['cnt']
        else:
            x1, cnt1 = pre1
        x = x1
        outs = [x1]
        cnt5 = None
        # (inside a position-list scope of the sampler: conv5 feeds the 3x3 logits convolution -> radius 1, conv4 radius 2, ...)
        for name, blk, radius in (('den.conv2', self.conv2, 4), ('den.conv3', self.conv3, 3), ('den.conv4', self.conv4, 2),
                                  ('den.conv5', self.conv5, 1)):
            with ops.timed(name):
                r = blk.run(x, IN_PTC, final='ptc', stateful=stateful, chunk_out=chunk, impl=impl,
                            want_counts=collapse and blk is self.conv5,
                            need_radius=radius if which == 'mfma-fp6v2' and collapse else None)
            x, cnt5 = r['ptc'], r['cnt']
            outs.append(x)
        if record is not None:
            record.extend(outs)
        return x, cnt5, x1, cnt1, which, impl, collapse

    def _conv6_params(self):
        conv = self.conv6[0]
        from spkdiff.fused import conv_params
        return conv, conv_params(conv).get_i8(conv, pad_cout=True)

    def _run(self, inp_b2hw, stateful, record=None):
        T = self.n_steps
        x, cnt5, x1, cnt1, which, impl, collapse = self._trunk(inp_b2hw, stateful, record)
        with ops.timed('den.conv6'):
            if collapse and cnt5 is not None and cnt1 is not None:
                # conv6 is linear and followed by the mean over T: convolve the spike COUNTS once instead of T frames
                conv, packed = self._conv6_params()
                return ops.den_conv3x3_counts(cnt5, packed, conv.out_channels, T, cnt1=cnt1)
            return self.conv6.run(x, IN_PTC, final='mean', in1=x1, impl=impl)['f32']

    # The dense sampler's step: the tail of a reverse step -- conv6 on the spike counts, the token update and the NEXT step's
    # first layer -- is ONE launch per image (csrc/step_tail.hip) instead of three launches and a logits round trip through
    # memory.  False = conv6, spk_psample_step and conv1 as separate launches (same tokens).
    use_step_tail = True

    def tail_fusable(self, h, w):
        """Can ``sample_step`` take the fused tail launch on an h x w latent?  (the reference's architecture on the certified
        fp6 kernel family: up to 512 classes (any --codebook_size, R/main.py:58), 256 + 64 channels into conv6, T = 16, 7x7 or 8x8)"""
        return (self.use_step_tail and self._fused_ok() and not self.training and not has_hooks(self) and self.collapse_conv6
                and self.n_steps == 16 and (h, w) in ((7, 7), (8, 8)) and 1 <= self.conv6[0].out_channels <= ops.STEP_TAIL_MAX_K
                and self.conv6[0].in_channels == 320 and self.conv5[0].out_channels == 256 and self.conv1[0].out_channels == 64
                and self.conv1[0].in_channels == 2 and self.impl_for(h, w, stateful=False) == 'mfma-fp6v2')

    @torch.no_grad()
    def sample_step(self, x_t, unmasked, t, temp, u=None, q=None, seed=0, offset=0, philox_state=None, pre1=None,
                    want_next=True, want_logits=False, top_k=None, top_p=None, confident=False, sched=None, remask=None):
        """One DENSE reverse step of the sampler on this denoiser (R/snn_model/vq_diffusion.py:113-140 with the call of
        :128-129 inside): x_t / unmasked are updated in place from the logits of ``self(x_t, t)`` (fresh LIF state, nothing
        written back).  ``pre1``: the first layer's (spikes, counts) for this step as returned by the previous call;
        ``want_next``: also evaluate it for step t - 1; ``temp``: a number or a per-image fp32 device tensor; ``top_k``: int32 device tensor, one k per image (top-k truncation); ``top_p``: fp32 device tensor, one p per image (nucleus truncation); ``confident``: the tail launch is the confidence-ordered one (spk_den_step_tail_conf); ``sched = (w, a, S)``: with ``confident``, its sibling under a reveal schedule and selection noise (spk_den_step_tail_conf_sched; ``u`` is then the Gumbel uniform); ``remask = (r, commit_conf, mask_id)``: with ``sched``, its sibling with remasking (spk_den_step_tail_conf_remask).  Returns (pre1 for the next step or None, logits or None)."""
        functional.reset_net(self)
        inp = None if pre1 is not None else ops.den_build_input(x_t, int(t))
        x, cnt5, x1, cnt1, which, impl, collapse = self._trunk(inp, False, pre1=pre1)
        conv6, packed6 = self._conv6_params()
        conv1, bn1 = self.conv1[0], self.conv1[1]
        nxt = None
        if want_next:
            a1, b1 = bn1.affine_terms()
            nxt = (conv1._spk_params.get(conv1), None if conv1.bias is None else conv1.bias.detach(), a1, b1)
        trunc = {} if top_k is None else {'top_k': top_k}
        if top_p is not None:
            trunc['top_p'] = top_p
        with ops.timed('den.tail'):
            if confident and sched is not None and remask is not None:
                return ops.den_step_tail_conf_remask(cnt5, cnt1, packed6, x_t, unmasked, int(t), temp, sched[0], sched[2], *remask,
                                                     T=self.n_steps, K=conv6.out_channels, noise_a=sched[1], u=u, q=q, seed=seed,
                                                     offset=offset, philox_state=philox_state, conv1=nxt, want_logits=want_logits,
                                                     **trunc)
            if confident and sched is not None:
                return ops.den_step_tail_conf_sched(cnt5, cnt1, packed6, x_t, unmasked, int(t), temp, sched[0], sched[2],
                                                    T=self.n_steps, K=conv6.out_channels, noise_a=sched[1], u=u, q=q, seed=seed,
                                                    offset=offset, philox_state=philox_state, conv1=nxt, want_logits=want_logits,
                                                    **trunc)
            if confident:
                return ops.den_step_tail_conf(cnt5, cnt1, packed6, x_t, unmasked, int(t), temp, T=self.n_steps,
                                              K=conv6.out_channels, u=u, q=q, seed=seed, offset=offset, philox_state=philox_state,
                                              conv1=nxt, want_logits=want_logits, **trunc)
            return ops.den_step_tail(cnt5, cnt1, packed6, x_t, unmasked, int(t), temp, T=self.n_steps,
                                     K=conv6.out_channels, u=u, q=q, seed=seed, offset=offset, philox_state=philox_state,
                                     conv1=nxt, want_logits=want_logits, **trunc)

    def _run_train(self, x, t):
        """train() mode (R/snn_model/vq_diffusion.py:189-208 with batch-statistics BN and surrogate-gradient LIF): the
        spike-input convolutions run the exact MFMA forward and the native backward (``ops.SpikeConvTrainFunction``; conv6 +
        the time mean: ``ops.SpikeConvMeanTrainFunction``), conv1 the library operator, each block tail is the native fused
        BN+LIF operator (``FusedSequential.train_forward``).  Membrane state follows the module semantics (kept until
        reset_net)."""
        T = self.n_steps
        inp = ops.den_build_input(x.detach(), t)                      # [B,2,h,w]: token ids and step as floats
        h = inp.unsqueeze(0).repeat(T, 1, 1, 1, 1)
        nbt = []                                                      # the five BatchNorm step counters: ONE launch at the end
        for blk in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5):
            object.__setattr__(blk, '_nbt_sink', nbt)
        preps = self._train_weight_prep(x)
        try:
            # (want_c4: the block tail also leaves its spikes in the packed format the next layer's exact forward reads)
            x1 = (self.conv1.train_forward(h, want_c4=preps is not None)
                  if preps is not None and self.conv1._trainable_fused(self.conv1._blocks(), h) else self.conv1(h))
            x5 = x1
            for i, blk in enumerate((self.conv2, self.conv3, self.conv4, self.conv5)):
                # conv2..conv5 see spikes: exact MFMA forward and native backward where the shape fits
                x5 = (blk.train_forward(x5, binary_input=True, prep=None if preps is None else preps[i],
                                        want_c4=preps is not None and i < 3)
                      if blk._trainable_fused(blk._blocks(), x5) else blk(x5))
        finally:
            for blk in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5):
                object.__setattr__(blk, '_nbt_sink', None)
        if nbt:
            torch._foreach_add_(nbt, 1)
        # (the fused block tails hand over channels-last spikes: the operator concatenates the 4-D views so that the layout
        #  survives, and its backward hands the two halves of the gradient on as views)
        cat = ops.CatChannelsFunction.apply(x5, x1)
        c6 = self.conv6
        blocks6 = c6._blocks()
        if c6._trainable_fused(blocks6, cat) and c6.exact_conv_fits(blocks6, cat):
            # conv6 + the time mean as ONE autograd operator: same forward operations, the backward convolves the output
            # gradient once with the spike counts (1/T of the per-step backward)
            conv = blocks6[0][0]
            return ops.SpikeConvMeanTrainFunction.apply(cat, conv.weight, conv.bias, None if preps is None else preps[4])
        x6 = c6.train_forward(cat, binary_input=True) if c6._trainable_fused(blocks6, cat) else c6(cat)
        return torch.sum(x6, dim=0) / T

    # False: every layer packs its own weights inside its forward / backward (20 small launches per iteration more)
    train_weight_prep = True

    def _train_weight_prep(self, x):
        """The weights of conv2..conv6 in the formats this iteration's forward (fp6 digit planes) and backward (two fp16 terms)
        read them in, made by two launches for all five layers (ops.train_weight_prep) -- or None when the model is not in the
        shape that path takes (single Conv-BN-LIF blocks on 7x7 / 8x8 maps, T = 16, channels-last parameters)."""
        if not self.train_weight_prep or self.n_steps != 16 or not x.is_cuda:
            return None
        T, B, H, W = self.n_steps, int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        layers = []
        for i, blk in enumerate((self.conv2, self.conv3, self.conv4, self.conv5, self.conv6)):
            blocks = blk._blocks()
            if blocks is None or len(blocks) != 1:
                return None
            conv = blocks[0][0]
            w = conv.weight
            keep_channels_last(w)
            if not (w.requires_grad and conv.training and exact_spike_conv(conv, T, H, W)):
                return None
            last = i == 4
            n_dg = B if last else (T * B if ops.conv3x3_dgrad_supported(conv.out_channels, conv.in_channels, H, W, T * B) else 0)
            if last and not (conv.out_channels % 16 == 0 and conv.in_channels % 32 == 0 and (H, W) in ((7, 7), (8, 8))):
                n_dg = 0
            layers.append((w, conv.bias, n_dg, (H, W)))
        return ops.train_weight_prep(layers)

    def invalidate(self):
        """Rebuild packed weights / BN terms on the next call (needed after writes through ``.data``)."""
        invalidate_derived(self)

    def train(self, mode: bool = True):
        if mode != self.training:
            invalidate_derived(self)
        return super().train(mode)

    def forward(self, x, t) -> torch.Tensor:
        # x: b,c,h,w (token ids as floats); t: b
        if self.training and torch.is_grad_enabled():
            return self._run_train(x, t)
        if self.training:
            raise NotImplementedError('spkdiff: DummyModel in train() mode runs the differentiable training graph and '
                                      'needs autograd enabled; call .eval() for inference')
        if not self._fused_ok():
            raise RuntimeError('spkdiff: DummyModel needs functional.set_step_mode(net, "m") and .eval()')
        if has_hooks(self):
            return self._run_modules(x, t)
        return self._run(ops.den_build_input(x, t), stateful=True)

    def _run_modules(self, x, t):
        """The reference's forward (R/snn_model/vq_diffusion.py:189-208) module by module -- each child a HIP kernel, fp32
        [T,B,C,H,W] tensors in between -- so that forward hooks registered on the children fire."""
        T = self.n_steps
        h = ops.den_build_input(x, t).unsqueeze(0).repeat(T, 1, 1, 1, 1)
        x1 = self.conv1(h)
        x5 = self.conv5(self.conv4(self.conv3(self.conv2(x1))))
        x6 = self.conv6(torch.cat((x5, x1), dim=2))
        return torch.sum(x6, dim=0) / T

    @torch.no_grad()
    def logits_from_tokens(self, x_t, t: int, record=None, inp=None):
        """Sampler fast path: ``self(x_t.float(), full((b,), t))`` followed by ``functional.reset_net(self)``
        (R/snn_model/vq_diffusion.py:128-129) -- every LIF starts from and returns to the reset state, so no
        membrane tensors are read or written."""
        if not self._fused_ok() or self.training:
            raise RuntimeError('spkdiff: DummyModel needs functional.set_step_mode(net, "m") and .eval()')
        functional.reset_net(self)
        # inp: the input map [B,2,h,w] already on the device (the previous spk_psample_step wrote it): no build launch
        return self._run(inp if inp is not None else ops.den_build_input(x_t, int(t)), stateful=False, record=record)
