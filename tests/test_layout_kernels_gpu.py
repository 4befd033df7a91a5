"""Device tests of the kernels the channels-last headline step spends its elementwise time in — the FPN top-down step
(csrc/fpn_topdown.hip) and the fused FrozenBN (+ residual) (+ ReLU) (csrc/frozen_bn.hip), both layouts, fp32 / fp16 / bf16 —
against plain CPU torch on the same dtype-rounded inputs: bit-equal where the kernel's arithmetic is one multiply / add chain
and one rounding, within a derived bound of the fp64 adjoint where it sums.  Shapes are the headline step's (2 images of
1333 x 800 padded to 1344 x 800) plus the edges of every vector-width, grid and alignment branch.  Run with `-m gpu`."""
import pytest
import torch
import torch.nn.functional as F

import torch_refs

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
U32 = 2.0 ** -24          # fp32 unit roundoff


def _C():
    from maskrcnn_benchmark import _C as C
    return C


class _EntrySpy(object):
    """stands in for `_C.lib` and records which library entry points were called"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name.startswith("detops_"):
            self.calls.append(name)
        return getattr(self._lib, name)


@pytest.fixture
def entries(monkeypatch):
    C = _C()
    spy = _EntrySpy(C.lib)
    monkeypatch.setattr(C, "lib", spy)
    return spy.calls


def _randn(shape, dtype, seed, scale=1.0):
    """dtype-rounded normal values made on the device; returned on the device (NCHW-contiguous) and on the host"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    d = (torch.randn(shape, generator=g, device=DEV) * scale).to(dtype)
    return d, d.cpu()


def _misaligned(t, fmt):
    """a copy of `t` in memory format `fmt` whose storage starts one element past an aligned allocation (vector width 1)"""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(N, H, W, C).permute(0, 3, 1, 2) if fmt == CL else buf[1:].view(N, C, H, W)
    v.copy_(t)
    assert v.storage_offset() == 1 and v.is_contiguous(memory_format=fmt)
    return v


def _ulp(v, dtype):
    """one unit in the last place of `dtype` at the magnitude of `v` (fp64 tensor)"""
    fi = torch.finfo(dtype)
    a = v.abs().clamp(min=fi.tiny)
    return fi.eps * torch.exp2(torch.floor(torch.log2(a)))


# ============================================================================ FPN top-down: lateral + nearest_upsample(top)
def _adjoint64(g, h, w):
    """grad of F.interpolate(t, size=g.shape[-2:], mode="nearest") w.r.t. t, in float64 on the host"""
    t = torch.zeros(g.shape[0], g.shape[1], h, w, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(t, size=tuple(g.shape[-2:]), mode="nearest")
    return torch.autograd.grad(up, t, g.double())[0]


def _topdown_check(entries, N, C, H, W, h, w, dtype, fmt, seed, misaligned=False):
    C_ = _C()
    lat_d, lat = _randn((N, C, H, W), dtype, seed)
    top_d, top = _randn((N, C, h, w), dtype, seed + 1)
    g_d, g = _randn((N, C, H, W), dtype, seed + 2)
    place = (lambda t: _misaligned(t, fmt)) if misaligned else (lambda t: t.contiguous(memory_format=fmt))
    lat_d, top_d, g_d = place(lat_d), place(top_d), place(g_d)
    nhwc = C_.is_channels_last(lat_d)
    assert nhwc == (fmt == CL and C > 1 and H * W > 1)

    del entries[:]
    a, b = lat_d.detach().requires_grad_(), top_d.detach().requires_grad_()
    out = C_.fpn_topdown(a, b)
    glat, gtop = torch.autograd.grad(out, (a, b), g_d)
    gtop2 = torch.autograd.grad(C_.fpn_topdown(a, b), b, g_d)[0]
    torch.cuda.synchronize()
    sfx = "_nhwc" if nhwc else ""
    assert "detops_fpn_topdown_forward" + sfx in entries and "detops_fpn_topdown_backward" + sfx in entries, entries

    # forward: one fp32 add, one rounding — bit-equal; output in the lateral's memory format
    want = (lat.float() + F.interpolate(top.float(), size=(H, W), mode="nearest")).to(dtype)
    assert out.dtype == dtype and C_.is_channels_last(out) == nhwc
    assert torch.equal(out.cpu(), want)
    if dtype == torch.float32:
        assert torch.equal(out, lat_d + F.interpolate(top_d, size=(H, W), mode="nearest"))

    # backward: grad_lateral is g; grad_top is a block sum of at most k terms in fp32 -> k * eps32 * sum |terms|
    assert torch.equal(glat, g_d)
    assert C_.is_channels_last(gtop) == nhwc or gtop.is_contiguous()
    ref = _adjoint64(g, h, w)
    k = float(_adjoint64(torch.ones(1, 1, H, W), h, w).max())
    assert k <= -(-H // h) * -(-W // w)
    bound = k * U32 * _adjoint64(g.abs(), h, w)
    if dtype != torch.float32:
        bound = bound + _ulp(ref, dtype)
    err = (gtop.cpu().double() - ref).abs()
    assert bool((err <= bound).all()), "grad_top: max err %g, worst err/bound %g" % (float(err.max()), float((err / bound.clamp(min=1e-300)).max()))
    # the forward's and the backward's index rules are adjoint: <fwd(0, t), g> = <t, bwd(g)> in fp64, up to the backward's rounding
    lhs = (F.interpolate(top.double(), size=(H, W), mode="nearest") * g.double()).sum()
    rhs = (top.double() * gtop.cpu().double()).sum()
    assert abs(float(lhs - rhs)) <= float((top.double().abs() * bound).sum()) + 1e-300
    # deterministic
    assert torch.equal(gtop, gtop2)
    return out, gtop


LEVELS = [((50, 84), (25, 42)), ((100, 168), (50, 84)), ((200, 336), (100, 168))]     # P4 <- P5, P3 <- P4, P2 <- P3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("level", LEVELS, ids=["P4", "P3", "P2"])
def test_fpn_topdown_model_levels(entries, level, fmt, dtype):
    """the three top-down steps of the headline FPN at C = 256, N = 2"""
    (H, W), (h, w) = level
    _topdown_check(entries, 2, 256, H, W, h, w, dtype, fmt, seed=H + 7)


EDGES = [(2, 25, 42, 13, 21), (2, 7, 9, 3, 4), (2, 1, 9, 1, 4), (2, 7, 1, 3, 1), (2, 5, 6, 1, 1), (2, 6, 6, 6, 6),
         (1, 9, 12, 5, 6), (2, 3, 4, 7, 9)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("C", [256, 12, 6, 3])
@pytest.mark.parametrize("shape", EDGES, ids=lambda s: "N%d_%dx%d_from_%dx%d" % s)
def test_fpn_topdown_any_ratio_and_every_vector_width(entries, shape, C, fmt, dtype):
    """the header's claim "any size ratio": non-2x ratios, H or W = 1, h = w = 1, H == h, one image, a coarser "lateral";
    C = 256 / 12 / 6 / 3 select vector widths 8 (half) or 4 (fp32), 4, 2, 1 in the channels-last kernels"""
    N, H, W, h, w = shape
    _topdown_check(entries, N, C, H, W, h, w, dtype, fmt, seed=C * 31 + H * W + h)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fpn_topdown_one_channel_takes_the_nchw_kernels(entries, dtype):
    """C = 1: a channels-last tensor is also NCHW-contiguous, so the NCHW kernels serve it"""
    t = torch.zeros(2, 1, 10, 12, device=DEV).contiguous(memory_format=CL)
    assert not _C().is_channels_last(t)
    _topdown_check(entries, 2, 1, 10, 12, 5, 6, dtype, CL, seed=3)
    assert not any(e.endswith("_nhwc") for e in entries), entries


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("C,H,W,h,w", [(256, 50, 84, 25, 42), (12, 25, 42, 13, 21)])
def test_fpn_topdown_misaligned_views_equal_the_aligned_run(entries, C, H, W, h, w, fmt, dtype):
    """views one element past an aligned allocation drop the kernels to vector width 1: the same bits as the aligned run"""
    o1, g1 = _topdown_check(entries, 2, C, H, W, h, w, dtype, fmt, seed=101)
    o2, g2 = _topdown_check(entries, 2, C, H, W, h, w, dtype, fmt, seed=101, misaligned=True)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)


# ============================================================================ FrozenBN (+ residual) (+ ReLU), channels-last
def _frozen_bn_check(entries, shape, dtype, relu, res, seed, fmt=CL, misaligned=False):
    """_C.frozen_bn_act_{forward,backward} against the fp32 CPU composition with the same scale / bias: bit-equal"""
    C_ = _C()
    N, C, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    scale_d = torch.randn(C, generator=g, device=DEV) * 0.7
    bias_d = torch.randn(C, generator=g, device=DEV)
    scale, bias = scale_d.cpu().reshape(1, -1, 1, 1), bias_d.cpu().reshape(1, -1, 1, 1)
    x_d, x = _randn(shape, dtype, seed + 1, scale=2.0)
    r_d, r = _randn(shape, dtype, seed + 2) if res else (None, None)
    gy_d, gy = _randn(shape, dtype, seed + 3)
    place = (lambda t: _misaligned(t, fmt)) if misaligned else (lambda t: t.contiguous(memory_format=fmt))
    x_d, gy_d = place(x_d), place(gy_d)
    r_d = place(r_d) if res else None
    nhwc = fmt == CL
    assert C_.is_channels_last(x_d) == nhwc

    del entries[:]
    y_d = C_.frozen_bn_act_forward(x_d, scale_d, bias_d, r_d, relu)
    gx_d, gr_d = C_.frozen_bn_act_backward(gy_d, y_d if relu else None, scale_d, relu, res)
    torch.cuda.synchronize()
    sfx = "_nhwc" if nhwc else ""
    assert entries == ["detops_frozen_bn_act_forward" + sfx, "detops_frozen_bn_act_backward" + sfx], entries
    assert C_.is_channels_last(y_d) == nhwc and C_.is_channels_last(gx_d) == nhwc
    assert (gr_d is not None) == res and (not res or C_.is_channels_last(gr_d) == nhwc)

    t = x.float() * scale + bias
    if res:
        t = t + r.float()
    want = (torch.relu(t) if relu else t).to(dtype)
    y = y_d.cpu()
    assert torch.equal(y, want), "forward: %d of %d differ" % (int((y != want).sum()), y.numel())
    m = torch.ops.aten.threshold_backward(gy.float(), want.float(), 0) if relu else gy.float()
    gx = gx_d.cpu()
    assert torch.equal(gx, (m * scale).to(dtype)), "grad_x: %d differ" % int((gx != (m * scale).to(dtype)).sum())
    if res:
        assert torch.equal(gr_d.cpu(), m.to(dtype))
    return y_d, gx_d, gr_d


RELU_RES = [(False, False), (True, False), (True, True), (False, True)]
BACKBONE = [(2, 64, 400, 672), (2, 256, 200, 336), (2, 512, 100, 168), (2, 1024, 50, 84), (2, 2048, 25, 42),
            (2, 64, 200, 336), (2, 128, 100, 168), (2, 256, 50, 84), (2, 512, 25, 42)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu,res", RELU_RES)
@pytest.mark.parametrize("shape", BACKBONE, ids=lambda s: "%d@%dx%d" % s[1:])
def test_frozen_bn_channels_last_backbone_shapes(entries, shape, relu, res, dtype):
    """every FrozenBN of the headline backbone on channels-last activations (stage outputs and bottleneck-internal widths):
    grid branches "per_block % C == 0" (C <= per_block) and "C % per_block == 0" (C = 2048: fp32 V = 4 and half V = 8)"""
    _frozen_bn_check(entries, shape, dtype, relu, res, seed=shape[1] + shape[2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu,res", RELU_RES)
@pytest.mark.parametrize("shape", [(2, 96, 50, 84), (2, 3, 40, 61), (2, 12, 7, 9), (2, 6, 5, 5), (1, 2048, 3, 1)],
                         ids=lambda s: "%d@%dx%d" % s[1:])
def test_frozen_bn_channels_last_window_rederived_per_vector(entries, shape, relu, res, dtype):
    """channel counts with no period between the grid stride and C (96; 3 at V = 1; 12 and 6 at V = 4 / 2): the channel
    window is re-derived per vector; and a C = 2048 tensor smaller than one channel period"""
    _frozen_bn_check(entries, shape, dtype, relu, res, seed=shape[1] * 3 + shape[3])


def test_frozen_bn_channels_last_block_cap(entries):
    """fp32, more than 16384 * 2048 vectors: the grid is capped at 16384 blocks (a whole number of channel periods), so
    every thread walks more vectors than the uncapped grid would give it (~0.55 GB per tensor)"""
    shape = (1, 2048, 260, 256)
    assert shape[0] * shape[1] * shape[2] * shape[3] // 4 > 16384 * 2048
    _frozen_bn_check(entries, shape, torch.float32, True, False, seed=5)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu,res", [(True, True), (False, False)])
@pytest.mark.parametrize("fmt", [torch.contiguous_format, CL], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", [(2, 64, 50, 84), (2, 96, 13, 21)], ids=lambda s: "%d@%dx%d" % s[1:])
def test_frozen_bn_misaligned_views_equal_the_aligned_run(entries, shape, fmt, relu, res, dtype):
    """a view one element past an aligned allocation: vector width 1, the same bits as the aligned run"""
    a = _frozen_bn_check(entries, shape, dtype, relu, res, seed=77, fmt=fmt)
    b = _frozen_bn_check(entries, shape, dtype, relu, res, seed=77, fmt=fmt, misaligned=True)
    for p, q in zip(a, b):
        assert (p is None and q is None) or torch.equal(p, q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_bn_module_fused_channels_last(dtype):
    """FrozenBatchNorm2d.fused through autograd on a channels-last bottleneck tail: bit-equal to the composition with the
    module's folded constants, gradients channels-last"""
    from maskrcnn_benchmark.layers import FrozenBatchNorm2d
    C_ = _C()
    torch.manual_seed(9)
    C = 256
    bn = FrozenBatchNorm2d(C)
    bn.weight.copy_(torch.rand(C) + 0.5); bn.bias.copy_(torch.randn(C))
    bn.running_mean.copy_(torch.randn(C)); bn.running_var.copy_(torch.rand(C) + 0.3)
    bn = bn.to(DEV)
    scale, bias = (t.cpu().reshape(1, -1, 1, 1) for t in bn.folded())
    x_d, x = _randn((2, C, 50, 84), dtype, 1)
    r_d, r = _randn((2, C, 50, 84), dtype, 2)
    g_d, g = _randn((2, C, 50, 84), dtype, 3)
    xi, ri = x_d.contiguous(memory_format=CL).requires_grad_(), r_d.contiguous(memory_format=CL).requires_grad_()
    y = bn.fused(xi, relu=True, residual=ri)
    y.backward(g_d.contiguous(memory_format=CL))
    want = torch.relu(x.float() * scale + bias + r.float()).to(dtype)
    assert C_.is_channels_last(y) and C_.is_channels_last(xi.grad) and C_.is_channels_last(ri.grad)
    assert torch.equal(y.detach().cpu(), want)
    m = torch.ops.aten.threshold_backward(g.float(), want.float(), 0)
    assert torch.equal(xi.grad.cpu(), (m * scale).to(dtype))
    assert torch.equal(ri.grad.cpu(), m.to(dtype))


# ============================================================================ non-finite values through the fused ReLU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channels_last", [False, True], ids=["nchw", "nhwc"])
def test_fused_relu_keeps_nan_like_torch_relu(dtype, channels_last):
    """FrozenBN (both layouts) and bias_act on NaN / +-inf / -0.0 / inf + (-inf): forward = torch.relu, backward =
    aten.threshold_backward, bias gradient = the fp64 column sum of the masked gradient (tests/torch_refs.py)"""
    torch_refs.check_fused_relu_non_finite(DEV, dtype, channels_last)
