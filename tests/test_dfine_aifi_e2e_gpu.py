"""dfine.bind_all end to end: transformers' DFineForObjectDetection at 2 x 256 x 256, random init, every stage that has kernels bound.
The memory assembly is judged alone by calling the bound DFineModel with inputs_embeds and encoder_outputs, which skips backbone and
hybrid encoder (inputs_embeds only has to be a tensor on the device: DFineModel.forward reads its .device and, with encoder_outputs
given, nothing else): nothing downstream of a convolution is compared for bit equality.  Skips cleanly where `transformers` (or its
D-FINE model) is not importable."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

LEVELS = [(8, 52), (4, 26), (2, 13)]   # the generated valid_mask has 16 zeros: 0.5 / 52 < 0.01


@pytest.fixture(scope="module")
def models(cuda_device):
    try:
        from transformers import DFineConfig, DFineForObjectDetection
    except Exception as ex:
        pytest.skip(f"transformers D-FINE not importable here: {ex}")
    from defectdetection_viaobjectdetection_amd import dfine
    torch.manual_seed(0)
    config = DFineConfig(dropout=0.0, activation_dropout=0.0, attention_dropout=0.0)
    try:
        cpu_model = DFineForObjectDetection(config)
    except ImportError as ex:  # a backbone dependency that is absent on the box; anything else is a failure
        pytest.skip(f"DFineForObjectDetection(DFineConfig()) cannot be built here: {ex}")
    with torch.no_grad():   # D-FINE starts every LQE head's last layer at 0, which would send a zero gradient into the heads
        for head in cpu_model.model.decoder.lqe_layers:
            head.reg_conf.layers[-1].weight.normal_(0.0, 0.1)
    model = cpu_model.to(cuda_device)
    x = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(1)).to(cuda_device)
    labels = [{"class_labels": torch.tensor([1, 0], device=cuda_device),   # DFineConfig() has two labels
               "boxes": torch.tensor([[0.5, 0.5, 0.2, 0.3], [0.3, 0.6, 0.1, 0.1]], device=cuda_device)},
              {"class_labels": torch.tensor([0], device=cuda_device), "boxes": torch.tensor([[0.4, 0.4, 0.3, 0.3]], device=cuda_device)}]
    return dfine, config, model, x, labels


def test_bind_all_training_step_takes_the_kernel_paths(models):
    dfine, config, model, x, labels = models

    def step(m):
        m.train().zero_grad(set_to_none=True)
        torch.manual_seed(3)
        loss = m(pixel_values=x, labels=labels).loss
        assert torch.isfinite(loss)
        loss.backward()
        return {n for n, p in m.named_parameters() if p.grad is not None}

    want = step(copy.deepcopy(model))
    twin = copy.deepcopy(model)
    bound = dfine.bind_all(twin)
    assert bound is twin and list(bound.state_dict()) == list(model.state_dict())
    before = {name: dict(getattr(dfine, name)) for name in ("aifi_calls", "layout_calls", "model_calls", "decoder_calls")}
    got = step(bound)
    for name, was in before.items():
        now = getattr(dfine, name)
        assert now["kernel"] > was["kernel"], (name, was, now)
    assert dfine.aifi_calls["torch"] == before["aifi_calls"]["torch"] and dfine.layout_calls["torch"] == before["layout_calls"]["torch"]
    assert want and want <= got, sorted(want - got)


@pytest.mark.parametrize("assembly", [True, False], ids=["assembly", "torch-assembly"])
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_memory_assembly_alone(models, cuda_device, assembly, mode):
    """enc_output's input is valid_mask * cat(levels) and the decoder's encoder_hidden_states the cat, bit for bit"""
    dfine, config, model, x, labels = models
    bound = dfine.bind_model(copy.deepcopy(model), assembly=assembly).train(mode == "train")
    D = config.d_model
    maps = [torch.randn(2, config.encoder_hidden_dim, h, w, generator=torch.Generator().manual_seed(40 + i)).to(cuda_device)
            for i, (h, w) in enumerate(LEVELS)]
    seen = {}
    hooks = [bound.model.enc_output.register_forward_pre_hook(lambda m, a: seen.__setitem__("memory", a[0].detach())),
             bound.model.decoder.register_forward_pre_hook(
                 lambda m, a, kw: seen.__setitem__("hidden", kw["encoder_hidden_states"].detach()), with_kwargs=True)]
    before = dict(dfine.layout_calls)
    try:
        with torch.no_grad():
            bound.model(inputs_embeds=maps[0], encoder_outputs=(maps,))
            sources = [bound.model.decoder_input_proj[i](m) for i, m in enumerate(maps)]
    finally:
        for h in hooks:
            h.remove()
    assert dfine.layout_calls["kernel"] == before["kernel"] + (1 if assembly else 0)
    cat = torch.cat([s.flatten(2).transpose(1, 2) for s in sources], 1)
    valid_mask = bound.model.generate_anchors(tuple(LEVELS), device=cuda_device, dtype=torch.float32)[1]
    assert int((~valid_mask).sum()) == 16
    assert seen["hidden"].shape == (2, 546, D)
    # DFineConfig() has hidden_size == decoder_in_channels[-1]: decoder_input_proj is nn.Identity, no convolution enters
    assert all(isinstance(p, torch.nn.Identity) for p in bound.model.decoder_input_proj)
    assert torch.equal(seen["hidden"], cat)
    assert torch.equal(seen["memory"], valid_mask.to(cat.dtype) * cat)
    assert bool((seen["memory"][:, ~valid_mask.reshape(-1)] == 0).all())


def test_all_ones_mask_is_found_once_and_memory_is_the_tokens(models, cuda_device):
    """widths below 51 give a valid_mask of ones: memory is source_flatten itself and the instance caches the finding"""
    dfine, config, model, x, labels = models
    bound = dfine.bind_model(copy.deepcopy(model)).eval()
    maps = [torch.randn(1, config.encoder_hidden_dim, h, w, generator=torch.Generator().manual_seed(50 + i)).to(cuda_device)
            for i, (h, w) in enumerate([(24, 24), (12, 12), (6, 6)])]   # 756 tokens: more than the 300 queries
    seen = {}
    hooks = [bound.model.enc_output.register_forward_pre_hook(lambda m, a: seen.__setitem__("memory", a[0])),
             bound.model.decoder.register_forward_pre_hook(lambda m, a, kw: seen.__setitem__("hidden", kw["encoder_hidden_states"]),
                                                           with_kwargs=True)]
    try:
        with torch.no_grad():
            bound.model(inputs_embeds=maps[0], encoder_outputs=(maps,))
            first = bound.model._m355_valid_mask_ones
            bound.model(inputs_embeds=maps[0], encoder_outputs=(maps,))
    finally:
        for h in hooks:
            h.remove()
    assert first[2] is True and bound.model._m355_valid_mask_ones is first
    assert seen["memory"] is seen["hidden"]
