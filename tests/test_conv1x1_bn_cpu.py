"""The Python side of the fused 1x1 convolution + FrozenBN path without a GPU: the routing predicate case by case, the
autograd Function's backward wiring against the module's existing two-launch path (over the host emulation of the FrozenBN
kernels, the fused forward replaced by its definition), the Bottleneck's fall-back, and the ABI table's new symbols."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cpu_shim
from torch_refs import launches

CL = torch.channels_last


class _Lib(object):
    """stands in for the library: records the `_supported` queries and answers `answer`"""

    def __init__(self, answer):
        self.answer, self.queries = answer, []

    def detops_conv1x1_frozen_bn_act_supported(self, *args):
        self.queries.append(args)
        return self.answer


@pytest.fixture
def device_predicate(monkeypatch):
    """`_C.conv1x1_bn_config` as it decides for device tensors, asked about CPU tensors"""
    from maskrcnn_benchmark import _C
    stub = _Lib(2)
    monkeypatch.setattr(_C, "lib", stub)
    monkeypatch.setattr(_C, "on_device", lambda t: True)
    monkeypatch.setattr(_C, "_on_device", lambda t: _C._NOSPAN)
    monkeypatch.setattr(_C, "_CONV1X1_BN_ROUTE", {})
    return _C, stub


def test_routing_predicate_case_by_case(device_predicate):
    _C, stub = device_predicate
    x = torch.randn(2, 8, 5, 7).contiguous(memory_format=CL)
    w = torch.randn(16, 8, 1, 1)
    r = torch.randn(2, 16, 3, 4).contiguous(memory_format=CL)
    assert _C.conv1x1_bn_config(x, w, 2, r, 0) == 2
    assert stub.queries == [(2, 8, 5, 7, 16, 2, 1, 0)]
    assert _C.conv1x1_bn_config(x, w, 2, r, 0) == 2 and len(stub.queries) == 1          # answered from the cache
    assert _C.conv1x1_bn_config(x, w.contiguous(memory_format=CL), 1, None, 1) == 2
    assert stub.queries[-1] == (2, 8, 5, 7, 16, 1, 0, 1)
    n = len(stub.queries)
    misaligned = torch.randn(2 * 8 * 5 * 7 + 1)[1:].view(2, 5, 7, 8).permute(0, 3, 1, 2)
    assert misaligned.is_contiguous(memory_format=CL) and misaligned.data_ptr() % 16 != 0
    for what, xi, wi in (("NCHW", x.contiguous(), w), ("bf16", x.bfloat16(), w.bfloat16()), ("fp64", x.double(), w.double()),
                         ("3x3 filter", x, torch.randn(16, 8, 3, 3)), ("grouped weight", x, torch.randn(16, 4, 1, 1)),
                         ("empty batch", x[:0], w), ("3-d input", x[0], w), ("misaligned", misaligned, w),
                         ("transposed weight", x, torch.randn(8, 16, 1, 1).transpose(0, 1))):
        assert _C.conv1x1_bn_config(xi, wi, 1, None, 0) == 0, what
    torch.set_autocast_enabled(True)            # (the device's autocast flag: `torch.autocast("cuda")` needs a device)
    try:
        assert _C.conv1x1_bn_config(x, w, 1, None, 0) == 0
    finally:
        torch.set_autocast_enabled(False)
    assert len(stub.queries) == n                                   # the library is not even asked
    stub.answer = 0
    assert _C.conv1x1_bn_config(x, w, 1, None, 2) == 0              # the library's own refusal (shape, routing table)


def test_a_library_without_the_entry_point_serves_nothing(monkeypatch):
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(_C, "lib", object())
    monkeypatch.setattr(_C, "on_device", lambda t: True)
    monkeypatch.setattr(_C, "_CONV1X1_BN_ROUTE", {})
    x = torch.randn(2, 8, 5, 7).contiguous(memory_format=CL)
    assert _C.conv1x1_bn_config(x, torch.randn(16, 8, 1, 1), 1, None, 0) == 0
    assert _C.conv1x1_bn_config(torch.randn(2, 8, 5, 7), torch.randn(16, 8, 1, 1), 1) == 0


def test_only_plain_bias_free_1x1_modules_qualify():
    from maskrcnn_benchmark.layers import Conv2d
    from maskrcnn_benchmark.layers.batch_norm import _plain_conv1x1
    assert _plain_conv1x1(Conv2d(8, 16, 1, bias=False)) and _plain_conv1x1(torch.nn.Conv2d(8, 16, 1, stride=2, bias=False))
    for bad in (Conv2d(8, 16, 1), Conv2d(8, 16, 3, bias=False), Conv2d(8, 16, 1, padding=1, bias=False),
                Conv2d(8, 16, 1, groups=2, bias=False), Conv2d(8, 16, 1, stride=(1, 2), bias=False),
                Conv2d(8, 16, (1, 3), bias=False), torch.nn.Linear(8, 16)):
        assert not _plain_conv1x1(bad), bad


def _bn(C, seed):
    from maskrcnn_benchmark.layers import FrozenBatchNorm2d
    g = torch.Generator().manual_seed(seed)
    bn = FrozenBatchNorm2d(C)
    bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
    bn.bias.copy_(torch.randn(C, generator=g))
    bn.running_mean.copy_(torch.randn(C, generator=g))
    bn.running_var.copy_(torch.rand(C, generator=g) + 0.2)
    return bn


@pytest.mark.parametrize("stride,relu,res,need", [
    (1, True, True, "all"), (1, True, True, "weight"), (1, True, True, "input"), (1, True, True, "residual only"),
    (1, True, False, "all"), (1, True, False, "weight"), (2, False, False, "all"), (2, False, False, "input"),
    (1, False, True, "all"), (1, False, True, "residual only")])
def test_function_on_cpu_tensors_equals_the_modules_existing_path(stride, relu, res, need, monkeypatch):
    """`bn.conv1x1_fused(conv, x, ...)` through the Function — its forward replaced by the definition of the fused launch
    (convolution, then the emulated FrozenBN kernel), its backward the product's — against `bn.fused(conv(x), ...)`:
    output and every requested gradient bit-equal, no gradient where none was requested"""
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.layers import Conv2d
    with cpu_shim.install("emu-lib"):
        monkeypatch.setattr(_C, "conv1x1_bn_config", lambda x, w, s, r=None, config=0: 1)
        seen = []

        def forward(x, w, scale, bias, residual, relu_, stride_, config):
            seen.append((stride_, config, residual is not None))
            return _C.frozen_bn_act_forward(F.conv2d(x, w, None, stride_), scale, bias, residual, relu_)

        monkeypatch.setattr(_C, "conv1x1_bn_forward", forward)
        g = torch.Generator().manual_seed(7)
        conv = Conv2d(8, 16, 1, stride=stride, bias=False)
        conv.weight.requires_grad_(need in ("all", "weight"))
        bn = _bn(16, 3)
        x = torch.randn(2, 8, 5, 7, generator=g).contiguous(memory_format=CL)
        Ho, Wo = (5 - 1) // stride + 1, (7 - 1) // stride + 1
        r = torch.randn(2, 16, Ho, Wo, generator=g).contiguous(memory_format=CL) if res else None
        gy = torch.randn(2, 16, Ho, Wo, generator=g).contiguous(memory_format=CL)

        def run(fused):
            conv.weight.grad = None
            xi = x.clone(memory_format=CL).requires_grad_(need in ("all", "input"))
            ri = r.clone(memory_format=CL).requires_grad_(need in ("all", "residual only")) if res else None
            monkeypatch.setattr(_C, "CONV1X1_BN", 0 if fused else None)
            y = bn.conv1x1_fused(conv, xi, relu=relu, residual=ri)
            y.backward(gy)
            return y.detach(), xi.grad, conv.weight.grad, (ri.grad if res else None)

        got, want = run(True), run(False)
        assert seen == [(stride, 1, res)]
        for a, b, what in zip(got, want, ("y", "grad_x", "grad_w", "grad_residual")):
            assert (a is None) == (b is None), what
            if a is not None:
                assert a.shape == b.shape and torch.equal(a, b), what
        assert (got[1] is not None) == (need in ("all", "input")) and (got[2] is not None) == (need in ("all", "weight"))


def test_bottleneck_without_the_kernel_takes_the_two_launch_path():
    """over the host emulation (which leaves csrc/conv1x1_bn*.hip out) the switch changes nothing: the same launches, the
    same values"""
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.modeling.backbone.resnet import BottleneckWithFixedBatchNorm
    with cpu_shim.install("emu-lib"):
        torch.manual_seed(1)
        block = BottleneckWithFixedBatchNorm(8, 4, 16, stride=2)
        x = torch.randn(2, 8, 6, 10).contiguous(memory_format=CL)
        prev = _C.CONV1X1_BN
        try:
            _C.CONV1X1_BN = 0
            with launches() as calls:
                y = block(x)
            assert calls == {"frozen_bn_fwd": 4}, calls
            _C.CONV1X1_BN = None
            assert torch.equal(block(x), y)
        finally:
            _C.CONV1X1_BN = prev


def test_abi_table_binds_the_new_symbols():
    from maskrcnn_benchmark import _abi, _lib
    sup = _abi.SIGNATURES["detops_conv1x1_frozen_bn_act_supported"]
    fwd = _abi.SIGNATURES["detops_conv1x1_frozen_bn_act_forward_nhwc_f32"]
    assert sup == (ctypes.c_int, [ctypes.c_int] * 8)
    assert fwd == (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_int] * 8 + [ctypes.c_void_p])
    for name, (res, args) in (("detops_conv1x1_frozen_bn_act_supported", sup), ("detops_conv1x1_frozen_bn_act_forward_nhwc_f32", fwd)):
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # argument checks that need no device: nothing is launched for a null pointer or an unserved shape
    assert _lib.lib.detops_conv1x1_frozen_bn_act_forward_nhwc_f32(None, None, None, None, None, None, 2, 8, 5, 7, 16, 1, 1, 1, None) == -1
    buf = np.zeros(64, dtype=np.float32)
    p = buf.ctypes.data - buf.ctypes.data % 16 + 16
    for shape in ((2, 6, 5, 7, 16, 1), (2, 8, 5, 7, 18, 1), (2, 8, 5, 7, 16, 3), (2, 8, 5, 7, 16, 0)):
        assert _lib.lib.detops_conv1x1_frozen_bn_act_forward_nhwc_f32(p, p, p, p, None, p, *shape, 1, 1, None) == -3, shape
        assert _lib.lib.detops_conv1x1_frozen_bn_act_supported(*shape, 0, 1) == 0, shape
    assert _lib.lib.detops_conv1x1_frozen_bn_act_forward_nhwc_f32(p, p, p, p, p, p, 2, 8, 5, 7, 16, 2, 1, 1, None) == -3   # stride 2 + residual
    assert _lib.lib.detops_conv1x1_frozen_bn_act_forward_nhwc_f32(p + 4, p, p, p, None, p, 2, 8, 5, 7, 16, 1, 1, 1, None) == -3
