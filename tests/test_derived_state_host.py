"""Host side of tests/test_gpu_derived_state.py: the facts about torch's version counters that decide which writes are SILENT for a
``(data_ptr, _version)`` cache key (a torch upgrade that changes one of them shows here, not as a stale image), what
``invalidate_derived`` / ``derived_refs`` do on models with placeholder cache entries, that a cache entry keeps its sources' storage
alive, and that the case table names calls that exist and an owner for every route."""
import torch
import torch.nn as nn

import _derived_state_cases as cases


def _conv_bn():
    from spikingjelly.activation_based import layer
    return layer.Conv2d(4, 8, 3, 1, 1), layer.BatchNorm2d(8)


# ---------------------------------------------------------------------------------------------------------------- torch facts
def test_writes_through_data_leave_the_version_alone():
    conv, bn = _conv_bn()
    for t in (conv.weight, bn.running_mean):
        v, ptr = t._version, t.data_ptr()
        t.data.mul_(1.5)
        t.data.add_(0.05)
        t.data.copy_(torch.ones_like(t))
        assert t._version == v and t.data_ptr() == ptr


def test_replacing_the_storage_keeps_the_parameters_version():
    from spkdiff.fused import keep_channels_last
    conv, bn = _conv_bn()
    m = nn.Sequential(conv, bn)
    w, v = conv.weight, conv.weight._version
    ptr = w.data_ptr()
    w.data = w.data.clone() * 1.5
    assert conv.weight is w and w._version == v and w.data_ptr() != ptr
    ptr = w.data_ptr()
    m.double()
    m.float()
    assert conv.weight is w and w._version == v and w.dtype == torch.float32 and w.data_ptr() != ptr
    ptr = w.data_ptr()
    keep_channels_last(w)
    assert conv.weight is w and w._version == v and w.data_ptr() != ptr
    assert w.is_contiguous(memory_format=torch.channels_last)
    ptr = w.data_ptr()
    keep_channels_last(w)                                           # already channels-last: nothing is replaced
    assert w.data_ptr() == ptr
    one_in, one_by_one = nn.Conv2d(1, 8, 3).weight, nn.Conv2d(8, 8, 1).weight
    for p in (one_in, one_by_one):                                  # ... and these count as channels-last from the start
        assert (p.is_contiguous(memory_format=torch.channels_last) and
                not any(p is q for _, q in cases.moved_by_channels_last(nn.ParameterList([p]))))


def test_train_mode_batchnorm_moves_the_statistics_but_not_their_version():
    bn = nn.BatchNorm2d(8).train()
    vm, vv = bn.running_mean._version, bn.running_var._version
    mean = bn.running_mean.clone()
    bn(torch.randn(4, 8, 5, 5) + 1.0)
    assert not torch.equal(bn.running_mean, mean)
    assert (bn.running_mean._version, bn.running_var._version) == (vm, vv)


def test_in_place_writes_optimizer_steps_and_copying_loads_move_the_version():
    conv, bn = _conv_bn()
    m = nn.Sequential(conv, bn)
    w = conv.weight
    v = w._version
    with torch.no_grad():
        w.mul_(1.5)
    assert w._version > v
    for kw in ({"foreach": True}, {"foreach": False}):
        v = w._version
        opt = torch.optim.AdamW(m.parameters(), lr=1e-3, **kw)
        nn.functional.conv2d(torch.randn(2, 4, 5, 5), w, conv.bias).sum().backward()
        opt.step()
        assert w._version > v
    v, vm = w._version, bn.running_mean._version
    m.load_state_dict({k: t.clone() for k, t in m.state_dict().items()})
    assert conv.weight is w and w._version > v and bn.running_mean._version > vm


# ---------------------------------------------------------------------------------------------------------------- the entries
def _vqvae():
    from snn_model.vae_model import SNN_VQVAE
    return SNN_VQVAE(1, 16, 128, 0.08)


def test_invalidate_derived_empties_every_cache_and_bumps_every_epoch():
    from spikingjelly.activation_based import layer
    from spkdiff import fused
    m = _vqvae()
    convs = [c for c in m.modules() if fused._is_conv(c)]
    bns = cases.batchnorms(m)
    assert len(convs) == 7 and len(bns) == 6
    packed = [object() for _ in convs]
    for c, pk in zip(convs, packed):
        assert fused.conv_params(c)._form('fp32', c, lambda pk=pk: pk) is pk
        assert fused.conv_params(c)._form('fp32', c, lambda: None) is pk             # kept while the key is equal
    terms = [(torch.zeros(1), torch.ones(1)) for _ in bns]
    for bn, ab in zip(bns, terms):
        bn._affine_cache = ("key", ab, ())
    object.__setattr__(m.vq_layer, '_graphs', {"key": "graph"})
    buf = torch.empty(4, dtype=torch.int16)
    object.__setattr__(m.vq_layer.poisson, '_spikegen_tab', {("cpu", 128, 16): [buf, "key", "stream", ("aliases",)]})
    refs = fused.derived_refs(m)
    flat = [x for r in refs for x in r]
    assert all(any(x is pk for x in flat) for pk in packed), "derived_refs lists every packed form"
    assert all(any(r is bn._affine_cache for r in refs) for bn in bns), "derived_refs lists every BatchNorm entry"
    epoch = fused.derived_epoch(m)
    assert len(epoch) == len(list(m.modules()))
    fused.invalidate_derived(m)
    assert all(not c._spk_params.forms for c in convs)
    assert all(bn._affine_cache is None for bn in bns)
    assert m.vq_layer._graphs == {}
    assert m.vq_layer.poisson._spikegen_tab == {("cpu", 128, 16): [buf, None, None, None]}
    assert m.vq_layer.poisson._spikegen_tab[("cpu", 128, 16)][0] is buf, "the table's buffer stays (a captured graph may address it)"
    assert all(b == a + 1 for a, b in zip(epoch, fused.derived_epoch(m)))
    assert any(x is packed[0] for r in refs for x in r), "what derived_refs returned outlives the invalidation"
    assert isinstance(bns[0], layer.BatchNorm2d)


def test_train_and_eval_transitions_invalidate_also_for_a_lone_batchnorm():
    """A train-mode forward moves the running statistics under an equal key: the mode change itself drops the folded terms -- for a
    FusedSequential, and for a layer.BatchNorm2d toggled on its own or inside a plain nn.Sequential."""
    from spkdiff import fused
    conv, bn = _conv_bn()
    seq = nn.Sequential(conv, bn).eval()
    for toggle in (lambda: (bn.train(), bn.eval()), lambda: (seq.train(), seq.eval())):
        bn._affine_cache = ("key", (torch.zeros(1), torch.ones(1)), ())
        e = fused.derived_epoch(bn)
        bn.eval()                                                   # no change of mode: kept
        assert bn._affine_cache is not None and fused.derived_epoch(bn) == e
        toggle()
        assert bn._affine_cache is None and fused.derived_epoch(bn)[0] > e[0]
    m = _vqvae().eval()
    for b in cases.batchnorms(m):
        b._affine_cache = ("key", (torch.zeros(1), torch.ones(1)), ())
    m.train()
    assert all(b._affine_cache is None for b in cases.batchnorms(m))


def test_a_cache_entry_keeps_the_storage_of_its_sources():
    """The entry's aliases share the parameters' storage and survive ``p.data = new``: the old block cannot be handed to the
    replacement while the entry lives, so an equal (data_ptr, _version) names the same storage."""
    from spkdiff import fused
    conv, _ = _conv_bn()
    pr = fused.conv_params(conv)
    pr._form('fp32', conv, lambda: "packed")
    key, _, held = pr.forms['fp32']
    old = conv.weight.data_ptr()
    assert held[0].data_ptr() == old and held[1].data_ptr() == conv.bias.data_ptr()
    assert held[0]._version == conv.weight._version and not held[0].requires_grad
    conv.weight.data = conv.weight.data.clone() * 1.5
    assert held[0].data_ptr() == old and conv.weight.data_ptr() != old
    assert fused.ConvParams.version(conv) != key[:2]
    assert pr._form('fp32', conv, lambda: "repacked") == "repacked"
    assert pr.forms['fp32'][2][0].data_ptr() == conv.weight.data_ptr()


# ---------------------------------------------------------------------------------------------------------------- the table
def test_every_subject_names_calls_that_exist_and_every_route_an_owner():
    from snn_model.vq_diffusion import DummyModel
    from spikingjelly.activation_based import layer, neuron
    models = {"denoiser_direct": DummyModel(1, 128),
              "plain_sequential": nn.ModuleDict({"seq": nn.Sequential(layer.Conv2d(32, 64, 3, 1, 1), layer.BatchNorm2d(64),
                                                                      neuron.LIFNode()), "bn": layer.BatchNorm2d(64)})}
    for name, (what, calls, routes) in cases.SUBJECTS.items():
        model = models.get(name) or _vqvae()
        assert what and calls and routes
        for call in calls:
            assert callable(cases.resolve(call, model)), (name, call)
        assert set(routes) <= set(cases.ROUTES), name
        assert cases.written_weights(model) and cases.written_stats(model), name
    assert callable(cases.resolve(cases.READOUT[2][0]))
    for route, (write, who) in cases.ROUTES.items():
        assert write and who in ("automatic", "caller"), route
    assert cases.owner("R5") == "caller" and all(cases.owner(r) == "automatic" for r in cases.ROUTES if r != "R5")
    assert set(cases.SUBJECTS["vqvae_cifar"][2]) == {"R1", "R5"} | set(cases.R8)
    assert {s for s, r in cases.PAIRS if r == "R7a"} == {"vqvae_fused", "denoiser_direct"}
    assert {s for s, r in cases.PAIRS if r == "R7b"} == {"plain_sequential"}
    assert {s for s, r in cases.PAIRS if r == "R3"} == set(cases.SUBJECTS) - {"vqvae_cifar", "plain_sequential"}
    assert len(set(cases.PAIRS)) == len(cases.PAIRS)


def test_the_writes_reach_what_they_name_and_the_inputs_are_what_the_table_says():
    from spkdiff import synth
    m = _vqvae()
    names = [n for n, _ in cases.written_weights(m)]
    assert names == ["encoder.snn_convs.0.weight", "vq_layer.poisson.0.weight", "decoder.snn_convs.0.weight"]
    assert len(cases.written_stats(m)) == 6
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    sd1 = cases.changed_state(m)
    assert all(torch.equal(m.state_dict()[k], sd0[k]) for k in sd0), "changed_state leaves the model alone"
    cases.write_in_place(m)
    assert all(torch.equal(m.state_dict()[k], sd1[k]) for k in sd0)
    assert not torch.equal(sd1["decoder.snn_convs.0.weight"], sd0["decoder.snn_convs.0.weight"])
    assert not torch.equal(sd1["encoder.snn_convs.4.running_mean"], sd0["encoder.snn_convs.4.running_mean"])
    moved = [n for n, _ in cases.moved_by_channels_last(m)]
    assert "decoder.snn_convs.0.weight" in moved and "encoder.snn_convs.0.weight" not in moved
    x, xb = cases.plain_inputs()
    assert x.shape == (16, 4, 32, 7, 7) and xb.shape == (16, 4, 64, 7, 7) and set(x.unique().tolist()) == {0.0, 1.0}
    tok = cases.denoiser_tokens(4, 0)
    assert tok.shape == (4, 1, 7, 7) and int(tok.max()) == 128 and int(tok.min()) >= 0
    assert cases.tokens(3, 8, 256).shape == (3, 8, 8) and int(cases.tokens(3, 8, 256).max()) < 256
    assert cases.images(4, 31).shape == (4, 1, 28, 28) and cases.images(3, 31, cases.cifar_config()).shape == (3, 3, 32, 32)
    assert cases.cifar_config().num_embeddings == 256 and synth.MNIST.num_embeddings == 128
