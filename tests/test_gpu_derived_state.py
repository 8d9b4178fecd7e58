"""Every derived weight form against a fresh model after each kind of write (tests/_derived_state_cases.py: SUBJECTS x ROUTES).

One pattern per (subject, route): build the model and call it, so that every form the call reads is cached (the denoiser, and
every subject on the captured-step route, also captures and replays a graph first, so that ``derived_refs`` and the epoch path
are live); apply the route; call again on the same inputs (``got``); build a new model of the same class, ``load_state_dict`` a
deep copy of the written model's ``state_dict()``, eval, call (``want``).  ``got`` must EQUAL ``want`` in every output -- the
reference is the same kernels without history, so there is no tolerance and no excluded set -- and at least one output must
differ from the call before the write: a route that changed nothing visible cannot pass.

The R8 routes replace a tensor's storage while the parameter object keeps its ``_version``; R8a frees the old storage first and
takes the replacement at its address where the allocator hands it back (several allocations, the misses held).  Each R8 case
records whether an address was reused, and whether the old storage was still held by a cache entry (the entries hold an alias of
their sources: then the address CANNOT be handed out again, which is the point of holding it).  The PARITY_REPORT line carries
per subject: pairs run, stale outputs, R8 cases with a reused address, R8 tensors held."""
import copy

import pytest
import torch
import torch.nn as nn

import _derived_state_cases as cases
from parity_report import record as parity

pytestmark = pytest.mark.gpu

TRIES = 64               # allocations tried for the old address before a replacement settles for another one
STATS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def states():
    """The synthetic checkpoints, made once and never written (every model loads a copy)."""
    from spkdiff import synth
    vq = synth.synth_vqvae_state(synth.MNIST)
    return {"mnist": vq, "cifar": synth.synth_vqvae_state(cases.cifar_config()),
            "denoiser": synth.synth_denoiser_state(synth.MNIST), "plain": cases.plain_state(vq)}


def _count(subject, **add):
    st = STATS.setdefault(subject, {"pairs": 0, "stale_outputs": 0, "r8_cases": 0, "r8_cases_with_reused_address": 0,
                                    "r8_tensors_held_by_an_entry": 0})
    for k, v in add.items():
        st[k] = st.get(k, 0) + int(v)
    parity("derived_state_" + subject, **st)


# ---------------------------------------------------------------------------------------------------------------- subjects
class _VQVAE:
    """vqvae_fused / vqvae_entry / vqvae_module_path / vqvae_cifar: one model class, four ways of calling it."""

    def __init__(self, name, states, dev):
        from spkdiff import synth
        self.name, self.dev = name, dev
        self.cfg = cases.cifar_config() if name == "vqvae_cifar" else synth.MNIST
        self.sd = states["cifar" if name == "vqvae_cifar" else "mnist"]
        B = 3 if name == "vqvae_cifar" else 4
        self.x = cases.images(B, 31, self.cfg).to(dev)
        self.tok = cases.tokens(B, self.cfg.latent, self.cfg.num_embeddings).to(dev)
        self.train_x = [cases.images(cases.TRAIN_IMAGES, 40 + i, self.cfg).to(dev) for i in range(3)]
        self.keep = []

    def build(self, state=None):
        from snn_model.vae_model import SNN_VQVAE, functional
        m = SNN_VQVAE(self.cfg.in_dim, self.cfg.latent_dim, self.cfg.num_embeddings, 0.08)
        functional.set_step_mode(net=m, step_mode='m')
        m.load_state_dict(self.sd if state is None else state)
        m = m.to(self.dev).eval()
        if self.name == "vqvae_module_path":      # a hook on one child of each container: all three run child by child
            for lif in (m.encoder.snn_convs[2], m.vq_layer.poisson[2], m.decoder.snn_convs[2]):
                lif.register_forward_hook(lambda mod, inp, out: None)
        return m

    def call(self, m):
        from snn_model import vae_model
        if self.name in ("vqvae_fused", "vqvae_module_path"):
            with torch.no_grad():
                e, xr, idx = m(self.x.unsqueeze(0).repeat(cases.T, 1, 1, 1, 1), self.x)
            vae_model.functional.reset_net(m)
            return {"e": e, "x_recon": xr, "idx": idx}
        out = {"idx": m.encode_images(self.x)}
        keep = vae_model.SPIKEGEN_BY_TOKEN
        try:
            for by_token in (True, False):
                vae_model.SPIKEGEN_BY_TOKEN = by_token
                f, u8 = m.decode_tokens(self.tok)
                out["pred_table" if by_token else "pred_generator"] = f
                out["u8_table" if by_token else "u8_generator"] = u8
        finally:
            vae_model.SPIKEGEN_BY_TOKEN = keep
        return out

    def live_graph(self, m):
        """Capture and replay decode_tokens: its launches bake the addresses of the derived tensors, and ``derived_refs`` is what
        a graph owner keeps alive past an invalidation."""
        from spkdiff import ops
        from spkdiff.fused import derived_refs
        m.decode_tokens(self.tok)
        store = {}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), ops.flag_scope(store):
            m.decode_tokens(self.tok)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g), ops.flag_scope(store):
            out = m.decode_tokens(self.tok)
        refs = derived_refs(m)
        g.replay()
        torch.cuda.synchronize()
        self.keep += [g, store, out, refs]

    def loss(self, m, i):
        x = self.train_x[i % 3]
        a, b, _ = m(x.unsqueeze(0).repeat(cases.T, 1, 1, 1, 1), x)
        return a + b

    def stat_forward(self, m, i):
        x = self.train_x[i % 3] + 0.1 * (i + 1)
        m(x.unsqueeze(0).repeat(cases.T, 1, 1, 1, 1), x)

    def graphed_step(self, m):
        from spkdiff.train import GraphedVQVAETrainStep
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.001, fused=True, capturable=True)
        step = GraphedVQVAETrainStep(m, opt, self.train_x[0], cases.T, warmup=3)
        self.keep += [step, opt]
        return lambda i: step(self.train_x[(i + 1) % 3])

    lr = 1e-3

    def reset(self, m):
        from snn_model.vae_model import functional
        functional.reset_net(m)


class _Denoiser:
    def __init__(self, name, states, dev):
        self.name, self.dev, self.sd = name, dev, states["denoiser"]
        self.x = cases.denoiser_tokens(4, 0).to(dev)
        self.t = torch.full((4,), 5, dtype=torch.int64, device=dev)
        self.train_x = [cases.denoiser_tokens(cases.TRAIN_TOKENS, 10 + i).clamp(max=127).float().to(dev) for i in range(3)]
        self.keep = []

    def build(self, state=None):
        from snn_model.vq_diffusion import DummyModel, functional
        d = DummyModel(1, 128)
        functional.set_step_mode(net=d, step_mode='m')
        d.load_state_dict(self.sd if state is None else state)
        return d.to(self.dev).eval()

    def call(self, m):
        from snn_model.vq_diffusion import functional
        a = m.logits_from_tokens(self.x, 5)
        with torch.no_grad():
            b = m(self.x.float(), self.t)
        functional.reset_net(m)
        return {"logits_from_tokens": a, "logits_forward": b}

    def _sampler(self, m):
        from snn_model.vq_diffusion import AbsorbingDiffusion
        ab = AbsorbingDiffusion(m, mask_id=128)
        ab.n_samples = 4
        return ab

    def live_graph(self, m):
        """The sampler's captured reverse process of this denoiser, replayed once: the graph entry holds ``derived_refs``."""
        ab = self._sampler(m)
        torch.manual_seed(5)
        ab.sample(temp=1.0, sample_steps=3)
        ab.sample(temp=1.0, sample_steps=3)
        assert ab._graphs, "the sampler captured a graph"
        self.ab = ab
        self.keep.append(ab)

    def loss(self, m, i):
        return self.ab.train_iter(self.train_x[i % 3])['loss']

    def stat_forward(self, m, i):
        m(self.train_x[i % 3], torch.full((cases.TRAIN_TOKENS,), 10 * (i + 1), dtype=torch.int64, device=self.dev))

    def graphed_step(self, m):
        from spkdiff.train import GraphedTrainStep
        opt = torch.optim.AdamW(m.parameters(), lr=self.lr, capturable=True)
        step = GraphedTrainStep(self.ab, opt, self.train_x[0])
        self.keep += [step, opt]
        return lambda i: step(self.train_x[(i + 1) % 3])

    lr = 5e-3

    def reset(self, m):
        from snn_model.vq_diffusion import functional
        functional.reset_net(m)


class _Plain:
    """A plain nn.Sequential of the drop-in layers (no FusedSequential: nothing invalidates for it) and a lone BatchNorm2d."""

    def __init__(self, name, states, dev):
        self.name, self.dev, self.sd = name, dev, states["plain"]
        x, xb = cases.plain_inputs()
        self.x, self.xb = x.to(dev), xb.to(dev)
        self.keep = []

    def build(self, state=None):
        from spikingjelly.activation_based import functional, layer, neuron, surrogate
        m = nn.ModuleDict({
            "seq": nn.Sequential(layer.Conv2d(32, 64, 3, 1, 1), layer.BatchNorm2d(64),
                                 neuron.LIFNode(surrogate_function=surrogate.ATan())),      # (ATan: the surrogate the training kernel has)
            "bn": layer.BatchNorm2d(64)})
        functional.set_step_mode(net=m, step_mode='m')
        m.load_state_dict(self.sd if state is None else state)
        return m.to(self.dev).eval()

    def call(self, m):
        with torch.no_grad():
            out = {"spikes": m["seq"](self.x), "bn": m["bn"](self.xb)}
        self.reset(m)
        return out

    def loss(self, m, i):
        return m["seq"](self.x).mean() + m["bn"](self.xb + 0.1 * i).square().mean()

    def stat_forward(self, m, i):
        m["seq"](self.x + 0.1 * (i + 1))
        m["bn"](self.xb + 0.1 * (i + 1))

    lr = 1e-3

    def reset(self, m):
        from spikingjelly.activation_based import functional
        functional.reset_net(m)


def _subject(name, states, dev):
    return {"denoiser_direct": _Denoiser, "plain_sequential": _Plain}.get(name, _VQVAE)(name, states, dev)


# ---------------------------------------------------------------------------------------------------------------- routes
def _take_old_address(t, values):
    """R8a: ``t.data = <values>`` with the replacement allocated AFTER the old storage lost its last reference, at the same size on
    the same stream, until the allocator hands the old address back (misses held meanwhile).  Returns (address reused, old storage
    still held by somebody -- a cache entry: nothing else refers to a parameter's storage here)."""
    dev, old = t.device, t.data_ptr()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    t.data = torch.empty(0, dtype=t.dtype, device=dev)
    held = torch.cuda.memory_allocated(dev) >= before
    misses, new = [], None
    for _ in range(TRIES):
        new = torch.empty(values.shape, dtype=values.dtype, device=dev)
        if new.data_ptr() == old:
            break
        misses.append(new)
    new.copy_(values)
    t.data = new
    del misses
    return t.data_ptr() == old, held


def _apply(sub, model, route):
    """Apply ``route`` to ``model``; returns (R8: any tracked address reused, tensors held, {name: reused})."""
    from spkdiff import fused
    tracked = cases.written_weights(model) + cases.written_stats(model)
    reused, held = {}, 0
    if route == "R1":
        cases.write_in_place(model)
    elif route == "R2":
        model.train()
        for i, kw in enumerate(({"fused": True}, {"foreach": True})):
            opt = torch.optim.AdamW(model.parameters(), lr=sub.lr, weight_decay=0.001, **kw)
            opt.zero_grad()
            sub.loss(model, i).backward()
            opt.step()
            sub.reset(model)
        model.eval()
    elif route == "R3":
        # The capture's eager warm-up iterations move every version counter and the training path re-lays the weights out, so forms
        # cached BEFORE the capture would be rebuilt whoever invalidates.  The forms are therefore cached once more from the
        # captured step's starting weights (an eval call between capture and replay): from there on the replays are the only
        # writes, no key moves, and only the step's own invalidate_derived and the mode changes can keep the next call fresh.
        model.train()
        step = sub.graphed_step(model)
        model.eval()
        sub.call(model)
        model.train()
        for i in range(2):
            step(i)
        model.eval()
        sub.reset(model)
    elif route == "R4a":
        model.load_state_dict(cases.changed_state(model))
    elif route == "R4b":
        model.load_state_dict(cases.changed_state(model), assign=True)
    elif route == "R5":
        cases.write_through_data(model)
        fused.invalidate_derived(model)
    elif route == "R6":
        model.train()
        cases.write_through_data(model)
        model.eval()
    elif route in ("R7a", "R7b"):
        toggled = [model] if route == "R7a" else cases.batchnorms(model)
        for m in toggled:
            m.train()
        with torch.enable_grad():
            for i in range(3):
                sub.stat_forward(model, i)
                sub.reset(model)
        for m in toggled:
            m.eval()
    elif route == "R8a":
        for name, t in tracked:
            values = (t.data * cases.SCALE if t.dim() > 1 or name.endswith("weight") else t.data + cases.SHIFT).cpu()
            reused[name], h = _take_old_address(t, values)
            held += h
    elif route in ("R8b", "R8d"):
        old = {name: t.data_ptr() for name, t in tracked}
        model.double() if route == "R8b" else model.cpu()
        cases.write_through_data(model)                   # (no version counter moves: the replacement alone is the route's signal)
        model.float() if route == "R8b" else model.to(sub.dev)
        now = dict(model.named_parameters())
        now.update(dict(model.named_buffers()))
        reused = {name: now[name].data_ptr() == ptr for name, ptr in old.items()}
    elif route == "R8c":
        moved = cases.moved_by_channels_last(model)
        assert moved, "the route replaces something"
        old = {name: p.data_ptr() for name, p in moved}
        for _, p in moved:
            p.data.mul_(cases.SCALE)
            fused.keep_channels_last(p)
        reused = {name: p.data_ptr() == old[name] for name, p in moved}
    else:
        raise KeyError(route)
    return reused, held


@pytest.mark.parametrize("subject,route", cases.PAIRS, ids=[f"{s}-{r}" for s, r in cases.PAIRS])
def test_derived_forms_follow_the_write(dev, states, subject, route):
    sub = _subject(subject, states, dev)
    model = sub.build()
    before = sub.call(model)
    if route == "R3" or subject == "denoiser_direct":
        sub.live_graph(model)
    reused, held = _apply(sub, model, route)
    got = sub.call(model)
    fresh = sub.build(copy.deepcopy(model.state_dict()))
    want = sub.call(fresh)
    sub.reset(model)
    sub.reset(fresh)
    stale = [k for k in want if not torch.equal(got[k], want[k])]
    moved = [k for k in want if not torch.equal(got[k], before[k])]
    _count(subject, pairs=1, stale_outputs=len(stale))
    if route in cases.R8:
        _count(subject, r8_cases=1, r8_cases_with_reused_address=any(reused.values()), r8_tensors_held_by_an_entry=held)
        _count(subject, **{route + "_conv_weight_reused": any(v for k, v in reused.items() if k.endswith("weight")),
                           route + "_bn_statistic_reused": any(v for k, v in reused.items() if k.endswith("running_mean"))})
        print(f"{subject}-{route}: reused {sorted(k for k, v in reused.items() if v)} of {len(reused)}, held {held}")
    assert set(got) == set(want) == set(before)
    assert not stale, f"{subject} after {route} ({cases.owner(route)}): stale {stale}"
    assert moved, f"{subject}: {route} changed no output; the pair would pass with every form stale"


def test_readout_coefficient_sum_follows_the_tensor_not_the_address(dev, states):
    """ops.readout_collapsed keeps sum(coef) per (data_ptr, _version, numel), process-wide: a second coefficient tensor of the same
    length at the address of a freed one must get ITS sum (the bias is multiplied by it)."""
    from spkdiff import ops
    x, w, b, coef_a, coef_b = (t.to(dev) if i < 3 else t for i, t in enumerate(cases.readout_inputs(states["mnist"])))
    assert float(coef_a.sum()) != float(coef_b.sum()) and float(b.abs().max()) > 0

    def on_device(values):
        t = torch.empty(values.shape, dtype=values.dtype, device=dev)
        t.copy_(values)                                       # (one in-place write each: equal version counters)
        return t

    def call(coef):
        return ops.readout_collapsed(x, w, b, coef, apply_tanh=True, want_u8=True)

    ca = on_device(coef_a)
    first = call(ca)
    old, ver = ca.data_ptr(), ca._version
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated(dev)
    del ca
    held = torch.cuda.memory_allocated(dev) >= allocated      # (nothing was freed: the entry of the first call holds the tensor)
    misses, reused = [], False
    for _ in range(TRIES):
        cb = on_device(coef_b)
        if cb.data_ptr() == old:
            reused = True
            break
        misses.append(cb)
    del misses
    assert cb._version == ver
    got = call(cb)
    ops._COEF_SUMS.clear()
    want = call(cb)
    stale = [k for k in want if not torch.equal(got[k], want[k])]
    parity("derived_state_readout_coef", pairs=1, stale_outputs=len(stale), address_reused=int(reused),
           freed_tensor_held_by_the_entry=int(held))
    assert not stale, f"readout_collapsed used the freed tensor's coefficient sum (address reused: {reused})"
    assert not torch.equal(got["f32"], first["f32"]), "the two coefficient sums give different read-outs"
