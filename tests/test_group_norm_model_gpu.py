"""The GroupNorm Mask R-CNN on the device, with the reference's weights and batch (tests/golden/whole_model_mask_rcnn_gn.npz), in
the layouts `nchw`, `backbone` and `all`.  Run with `-m gpu`."""
import pytest
import torch

import cpu_shim
from test_whole_model_parity import GRAD_TOL, TOL, _build, _grad_spread, _loss_and_grads

pytestmark = pytest.mark.gpu

NAME = "mask_rcnn_gn"


def _device_runs(monkeypatch, ref_sd, il, targets, ref_losses, cpu_grads, switch):
    """-> {layout: grads}, {layout: (channels-last? of every _C.group_norm_forward input, (layer, dim, channels-last?) of every
    GroupNorm layer's input)}"""
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(_C, "GROUP_NORM", switch)
    _, model, _, _, _, _ = _build(NAME, "cuda")
    model.load_state_dict(ref_sd, strict=True)
    model.to("cuda").train()
    seen = []
    forward = _C.group_norm_forward

    def spy(x, *a, **k):
        seen.append(_C.is_channels_last(x))
        return forward(x, *a, **k)
    monkeypatch.setattr(_C, "group_norm_forward", spy)
    # which 4-d GroupNorm inputs each region of the model sees: hooks on the layers themselves
    from maskrcnn_benchmark.layers import GroupNorm
    met = []
    hooks = [m.register_forward_pre_hook(lambda mod, args, n=n: met.append((n, args[0].dim(), _C.is_channels_last(args[0]))))
             for n, m in model.named_modules() if isinstance(m, GroupNorm)]
    for n, m in model.named_modules():
        if isinstance(m, GroupNorm):       # `fused` bypasses forward hooks: record there too
            def fused(x, relu=False, residual=None, _m=m, _n=n, _f=m.fused):
                met.append((_n, x.dim(), _C.is_channels_last(x)))
                return _f(x, relu=relu, residual=residual)
            m.fused = fused
    runs, calls = {}, {}
    for layout in ("nchw", "backbone", "all"):
        if layout != "nchw":
            model.set_channels_last(True, heads=(layout == "all"))
        del seen[:], met[:]
        losses, grads = _loss_and_grads(model, il, targets, "cuda")
        torch.cuda.synchronize()
        for k, ref in ref_losses.items():
            assert abs(losses[k] - ref) <= TOL * max(1.0, abs(ref)), (switch, layout, k, losses[k], ref)
        assert set(grads) == set(cpu_grads), (switch, layout, sorted(set(grads) ^ set(cpu_grads))[:10])
        runs[layout] = grads
        calls[layout] = (list(seen), list(met))
    for h in hooks:
        h.remove()
    return runs, calls


def _worst(runs, cpu_grads):
    worst = (0.0, None, None)
    for layout, grads in runs.items():
        spread = _grad_spread(grads, cpu_grads)
        n = max(spread, key=spread.get)
        if spread[n] > worst[0]:
            worst = (spread[n], layout, n)
    return worst


def test_gn_layouts_losses_kernels_and_gradients(monkeypatch):
    """Every loss within TOL of the reference's fixture in every layout; the same parameters carry a gradient as on the CPU;
    under `backbone` every 4-d GroupNorm of the body and FPN goes through _C.group_norm_forward with a channels-last input,
    under `all` the box head's xconvs and the mask head as well, under `nchw` none; per-parameter gradient spread against the
    CPU run within GRAD_TOL — or, if the DETOPS_GROUP_NORM=torch run of the same model itself exceeds GRAD_TOL (the constant
    was observed on models without GroupNorm), within 4 x that run's worst spread.
    Observed on an MI355X: worst spread 1.16 with the HIP path and 1.16 with the switch on `torch` (both
    `roi_heads.box.feature_extractor.xconvs.1.weight`: a sum of gradients that cancels to fp32 noise at random init, on ATen's
    path as well), so the bound in force is 4 x 1.16 = 4.63 (profiles/group_norm_tests.txt)."""
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    monkeypatch.setattr(torch.backends.cuda.matmul, "allow_tf32", False)
    _, model, ref_sd, il, targets, ref_losses = _build(NAME, "cpu")
    model.load_state_dict(ref_sd, strict=True)
    model.train()
    with cpu_shim.install("oracle"):
        cpu_losses, cpu_grads = _loss_and_grads(model, il, targets, "cpu")
    for k, ref in ref_losses.items():
        assert abs(cpu_losses[k] - ref) <= TOL * max(1.0, abs(ref)), ("cpu", k, cpu_losses[k], ref)

    torch_runs, torch_calls = _device_runs(monkeypatch, ref_sd, il, targets, ref_losses, cpu_grads, "torch")
    assert all(not seen for seen, _ in torch_calls.values()), "the switch keeps every layer on F.group_norm"
    fused_runs, calls = _device_runs(monkeypatch, ref_sd, il, targets, ref_losses, cpu_grads, "fused")

    def four_d(met, prefix):
        return [cl for n, dim, cl in met if n.startswith(prefix) and dim == 4]

    seen, met = calls["nchw"]
    assert seen == [] and not any(cl for _, _, cl in met)
    seen, met = calls["backbone"]
    body = four_d(met, "backbone.")
    assert len(body) >= 53 + 8 and all(body), "every GroupNorm of the body and the FPN meets a channels-last input"
    assert seen and all(seen) and len(seen) == len(body)
    assert not any(four_d(met, "roi_heads."))
    seen, met = calls["all"]
    body, box, mask = four_d(met, "backbone."), four_d(met, "roi_heads.box.feature_extractor.xconvs"), four_d(met, "roi_heads.mask.")
    assert all(body) and len(box) == 4 and all(box) and len(mask) == 2 and all(mask), (len(box), len(mask))
    assert all(seen) and len(seen) == len(body) + len(box) + len(mask)

    fused_worst, torch_worst = _worst(fused_runs, cpu_grads), _worst(torch_runs, cpu_grads)
    bound = GRAD_TOL if torch_worst[0] <= GRAD_TOL else 4 * torch_worst[0]
    print("\ngradient spread against the CPU run: fused %.3g (%s, %s), torch %.3g (%s, %s), bound %.3g"
          % (fused_worst + torch_worst + (bound,)))
    assert fused_worst[0] <= bound, (fused_worst, torch_worst, bound)
