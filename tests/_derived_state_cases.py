"""Case table of tests/test_gpu_derived_state.py and tests/test_derived_state_host.py (CPU only: every tensor made here is a host
tensor): SUBJECTS x ROUTES.

The inference kernels read FORMS DERIVED from the parameters -- packed weights (``ConvParams.forms``), folded BatchNorm terms
(``BatchNorm2d._affine_cache``), the per-token spike-pattern table (``_spikegen_tab``), the read-out's coefficient sums
(``ops._COEF_SUMS``), captured graphs -- each kept while ``(data_ptr, _version[, device])`` of its sources stays equal.  A stale form
faults nowhere: it is a plausible image of OLD weights, and a test that builds its model fresh never sees it.  A SUBJECT is a model
with the calls that read its forms; a ROUTE is one way of writing the parameters, with WHO owes the invalidation under the contract
of ``spkdiff.fused.invalidate_derived`` ("automatic": the caller does nothing; "caller": the caller calls ``invalidate_derived``).
The device test calls a subject, applies a route, calls again and compares with a fresh model loaded from the written one's
``state_dict()``: same kernels, no history, so equality is exact.

The write helpers below take a module on any device; the allocator recipe of the R8 routes (free the old storage, take the
replacement at its address) needs a device and lives in the device test."""
import copy

import torch
import torch.nn as nn

T = 16
SCALE = 1.5              # factor of every weight write
SHIFT = 0.05             # summand of every running_mean write
TRAIN_IMAGES = 8         # batch of the VQ-VAE training routes (the size tests/test_gpu_conv_train.py trains at)
TRAIN_TOKENS = 16        # batch of the denoiser's training routes (the size the sampler's training tests train at)

# route -> (the write, who invalidates).  R4 and R8 come in the lettered forms below; the table in DESIGN.md has one row per route.
ROUTES = {
    "R1": ("in-place write under no_grad: p.mul_ on every '...0.weight', running_mean.add_ on every BatchNorm", "automatic"),
    "R2": ("train(), two eager AdamW steps (one fused=True, one foreach=True), eval()", "automatic"),
    "R3": ("two replays of the captured training step (GraphedVQVAETrainStep / GraphedTrainStep), eval()", "automatic"),
    "R4a": ("load_state_dict of changed values, copied into the parameters", "automatic"),
    "R4b": ("load_state_dict of changed values with assign=True", "automatic"),
    "R5": ("p.data.mul_ / running_mean.data.add_, then invalidate_derived(model)", "caller"),
    "R6": ("train(), p.data.mul_ / running_mean.data.add_, eval(), nothing else", "automatic"),
    "R7a": ("statistics only: train(), three forwards with autograd on shifted inputs, no optimizer, eval()", "automatic"),
    "R7b": ("statistics only, toggling the BatchNorm children alone: bn.train(), three forwards, bn.eval()", "automatic"),
    "R8a": ("storage replaced: p.data = scaled copy, allocated at the freed address where the allocator obliges", "automatic"),
    "R8b": ("storage replaced: module.double(), scale, module.float()", "automatic"),
    "R8c": ("storage replaced: p.data.mul_ then keep_channels_last, on every weight it moves", "automatic"),
    "R8d": ("storage replaced: module.cpu(), scale, module.to(device)", "automatic"),
}
R8 = ("R8a", "R8b", "R8c", "R8d")
_ALL = ("R1", "R2", "R3", "R4a", "R4b", "R5", "R6")

# subject -> (what it is, the calls whose outputs are compared, its routes).  A call is "<attribute path on the model>" or
# "<module>:<function>" for the ops the module path reaches; the host test resolves every one.
SUBJECTS = {
    "vqvae_fused": ("SNN_VQVAE(1, 16, 128), B = 4, 28x28: eval model(x_seq, x) -> (e, x_recon, idx)",
                    ("forward",), _ALL + ("R7a",) + R8),
    "vqvae_entry": ("the same model: encode_images; decode_tokens with SPIKEGEN_BY_TOKEN True and False",
                    ("encode_images", "decode_tokens"), _ALL + R8),
    "vqvae_module_path": ("the same model with a forward hook on one child of each container: children run one by one",
                          ("forward", "spkdiff.ops:conv2d", "spkdiff.ops:conv_transpose2d",
                           "spikingjelly.activation_based.layer:BatchNorm2d.affine_terms"), _ALL + R8),
    "vqvae_cifar": ("SNN_VQVAE(3, 16, 256), B = 3, 32x32: vqvae_entry's calls on the other kernel kinds",
                    ("encode_images", "decode_tokens"), ("R1", "R5") + R8),
    "denoiser_direct": ("DummyModel, MNIST config, B = 4, 7x7, K = 128: logits_from_tokens(x, t) and eval den(x, t), called directly",
                        ("logits_from_tokens", "forward"), _ALL + ("R7a",) + R8),
    "plain_sequential": ("nn.Sequential(layer.Conv2d(32, 64, 3, 1, 1), layer.BatchNorm2d(64), neuron.LIFNode()) in multi-step mode on "
                         "[16, 4, 32, 7, 7], and a lone layer.BatchNorm2d(64) on [16, 4, 64, 7, 7]",
                         ("seq.forward", "bn.forward"), ("R1", "R2", "R4a", "R4b", "R5", "R6", "R7b") + R8),
}
READOUT = ("readout_coef", "ops.readout_collapsed on [4, 14, 14, 32] with two coefficient tensors of 16 entries and different sums",
           ("spkdiff.ops:readout_collapsed",))

PAIRS = tuple((s, r) for s, (_, _, routes) in SUBJECTS.items() for r in routes)


def owner(route):
    return ROUTES[route][1]


# ---------------------------------------------------------------------------------------------------------------- inputs
def cifar_config():
    from spkdiff import synth
    return synth.PathConfig(in_dim=3, img=32, num_embeddings=256)


def images(n, seed, cfg=None):
    """[n, C, H, W] in [-0.5, 0.5): stroke images (MNIST shape) or uniform noise (CIFAR shape)."""
    from spkdiff import synth
    if cfg is None or cfg.in_dim == 1:
        return synth.stroke_images(n, seed) - 0.5
    return torch.rand(n, cfg.in_dim, cfg.img, cfg.img, generator=torch.Generator().manual_seed(seed)) - 0.5


def tokens(n, L, K, seed=0):
    """int64 [n, L, L]: every code of the book at least once where n * L * L >= K."""
    return ((torch.arange(n * L * L) * 7 + seed) % K).reshape(n, L, L)


def denoiser_tokens(n, seed, K=128, L=7):
    """int64 [n, 1, L, L] with a third of the positions masked (id K)."""
    g = torch.Generator().manual_seed(9100 + seed)
    x = torch.randint(0, K, (n, 1, L, L), generator=g)
    x[torch.rand(n, 1, L, L, generator=g) < 0.33] = K
    return x


def plain_inputs():
    """(spikes [16, 4, 32, 7, 7] at rate 0.2 for the sequential, fp32 [16, 4, 64, 7, 7] for the lone BatchNorm)."""
    g = torch.Generator().manual_seed(9200)
    return (torch.rand(T, 4, 32, 7, 7, generator=g) < 0.2).float(), torch.randn(T, 4, 64, 7, 7, generator=g)


def plain_state(vqvae_sd):
    """state_dict of the plain_sequential subject (keys 'seq.0.*', 'seq.1.*', 'bn.*') from the synthetic VQ-VAE checkpoint: its
    second encoder layer has this convolution's weight shape [64, 32, 3, 3] and a BatchNorm of 64 channels."""
    sd = {}
    for k, v in vqvae_sd.items():
        if k.startswith("encoder.snn_convs.3."):
            sd["seq.0." + k.rsplit(".", 1)[1]] = v.clone()
        elif k.startswith("encoder.snn_convs.4."):
            sd["seq.1." + k.rsplit(".", 1)[1]] = v.clone()
            sd["bn." + k.rsplit(".", 1)[1]] = v.clone()
    return sd


def readout_inputs(vqvae_sd):
    """(x [4, 14, 14, 32] time-collapsed spikes, weight [32, 1, 3, 3], bias [1], coef_a [16], coef_b [16]); the bias is not zero
    (the coefficient sum multiplies it) and the two sums differ."""
    g = torch.Generator().manual_seed(9300)
    coef_a = torch.pow(0.8, torch.arange(T - 1, -1, -1).float())
    coef_b = torch.pow(0.5, torch.arange(T).float())
    x = ((torch.rand(T, 4, 14, 14, 32, generator=g) < 0.2).float() * coef_a.view(T, 1, 1, 1, 1)).sum(0)
    return x, vqvae_sd["decoder.snn_convs.6.weight"].clone(), vqvae_sd["decoder.snn_convs.6.bias"].clone(), coef_a, coef_b


# ---------------------------------------------------------------------------------------------------------------- writes
def written_weights(model):
    """[(name, parameter)] every route scales: the first convolution of every container ('...0.weight'); of a lone BatchNorm, its
    'weight'."""
    return [(n, p) for n, p in model.named_parameters() if n.endswith("0.weight") or n == "weight" or n == "bn.weight"]


def written_stats(model):
    """[(name, buffer)] every route shifts: the running mean of every BatchNorm."""
    return [(n, b) for n, b in model.named_buffers() if n.endswith("running_mean")]


def write_in_place(model):
    """R1: the writes torch's version counters see."""
    with torch.no_grad():
        for _, p in written_weights(model):
            p.mul_(SCALE)
        for _, b in written_stats(model):
            b.add_(SHIFT)


def write_through_data(model):
    """R5, R6: the same writes through ``.data``: no version counter moves."""
    for _, p in written_weights(model):
        p.data.mul_(SCALE)
    for _, b in written_stats(model):
        b.data.add_(SHIFT)


def changed_state(model, scale=SCALE, shift=SHIFT):
    """R4: a deep copy of ``model.state_dict()`` with the routes' writes applied (tensors stay on the model's device)."""
    sd = copy.deepcopy(model.state_dict())
    for k in sd:
        if k.endswith("0.weight") or k in ("weight", "bn.weight"):
            sd[k] = sd[k] * scale
        elif k.endswith("running_mean"):
            sd[k] = sd[k] + shift
    return sd


def moved_by_channels_last(model):
    """[(name, parameter)] R8c writes: the 4-D weights ``keep_channels_last`` gives new storage (a weight with one input channel or
    a 1x1 kernel already counts as channels-last: nothing would be replaced, and the scale alone is route R5's write)."""
    return [(n, p) for n, p in model.named_parameters()
            if p.dim() == 4 and not p.is_contiguous(memory_format=torch.channels_last)]


def batchnorms(model):
    from spikingjelly.activation_based import layer
    return [m for m in model.modules() if isinstance(m, layer.BatchNorm2d)]


def resolve(call, model=None):
    """The callable a subject's call names (the host test: every one exists)."""
    if ":" in call:
        import importlib
        mod, path = call.split(":")
        obj = importlib.import_module(mod)
    else:
        obj, path = model, call
    for part in path.split("."):
        obj = obj[part] if isinstance(obj, (nn.ModuleDict, nn.Sequential)) and not hasattr(obj, part) else getattr(obj, part)
    return obj
