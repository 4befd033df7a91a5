"""The fused 1x1 convolution + FrozenBN (+ residual) (+ ReLU) launch (csrc/conv1x1_bn.hip) on the device: bit-exact cases
against an fp64 computation and against the two-launch path it replaces (forward and the Function's gradients), random
floats against fp64, the fall-backs, and a backbone block fused against unfused.

The shapes (N = 2) are the smallest at which each code path of the kernels can go wrong:
  C 64 -> K 256, 5 x 7, residual       70 rows: the M tail of a 64-row tile
  C 256 -> K 64, 9 x 11                K below the 128-wide N tile
  C 256 -> K 512, 9 x 11, stride 2     odd input, 5 x 6 output, no ReLU: the projection shortcut
  C 2048 -> K 512, 3 x 4               long K loop, one partial tile
  C 512 -> K 2048, 3 x 4, residual     long K loop, one partial tile
each under both tile configurations, selected explicitly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from torch_refs import launches

pytestmark = pytest.mark.gpu

CL = torch.channels_last
# C, K, H, W, stride, relu, residual
CASES = [(64, 256, 5, 7, 1, True, True), (256, 64, 9, 11, 1, True, False), (256, 512, 9, 11, 2, False, False),
         (2048, 512, 3, 4, 1, True, False), (512, 2048, 3, 4, 1, True, True)]
CONFIGS = [1, 2]
N = 2


def _dev():
    return torch.device("cuda:0")


def _exact_inputs(C, K, H, W, stride, res, seed):
    """integers small enough that every fp32 sum is exact in any order; pre-activations are half-integers (never 0)"""
    rng = np.random.RandomState(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))  # noqa: E731
    x = t(rng.randint(-2, 3, (N, C, H, W))).contiguous(memory_format=CL)
    w = t(rng.randint(-1, 2, (K, C, 1, 1)))
    scale = t(rng.randint(1, 3, (K,)))
    bias = t(rng.randint(-3, 4, (K,)) + 0.5)
    r = t(rng.randint(-4, 5, (N, K, Ho, Wo))).contiguous(memory_format=CL) if res else None
    gy = t(rng.randint(-2, 3, (N, K, Ho, Wo))).contiguous(memory_format=CL)
    return x, w, scale, bias, r, gy


def _random_inputs(C, K, H, W, stride, res, seed):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = torch.randn(N, C, H, W, generator=g).contiguous(memory_format=CL)
    w = torch.randn(K, C, 1, 1, generator=g) * (2.0 / C) ** 0.5
    scale = torch.rand(K, generator=g) + 0.5
    bias = torch.randn(K, generator=g)
    r = torch.randn(N, K, Ho, Wo, generator=g).contiguous(memory_format=CL) if res else None
    return x, w, scale, bias, r


def _fp64(x, w, scale, bias, r, relu, stride):
    y = torch.einsum("nchw,kc->nkhw", x[:, :, ::stride, ::stride].double(), w[:, :, 0, 0].double())
    y = y * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)
    if r is not None:
        y = y + r.double()
    return y.relu() if relu else y


def _fused(x, w, scale, bias, r, relu, stride, config):
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.layers.batch_norm import _Conv1x1FrozenBNAct
    assert _C.conv1x1_bn_config(x, w, stride, r, config) == config
    return _Conv1x1FrozenBNAct.apply(x, w, scale, bias, r, relu, stride, config)


def _pair(x, w, scale, bias, r, relu, stride):
    from maskrcnn_benchmark.layers.batch_norm import _FrozenBNAct
    return _FrozenBNAct.apply(F.conv2d(x, w, None, stride), scale, bias, r, relu)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "C%d-K%d-%dx%d-s%d" % c[:5])
def test_exact_cases_are_bit_equal_to_fp64_and_to_the_two_launch_path(case, config):
    """forward bit-equal to fp64 and to conv2d + frozen_bn_act_forward; grad_x, grad_w and grad_residual of the Function
    bit-equal to those of the two-launch composition"""
    from maskrcnn_benchmark import _C
    C, K, H, W, stride, relu, res = case
    x, w, scale, bias, r, gy = _exact_inputs(C, K, H, W, stride, res, seed=C + K + config)
    want = _fp64(x, w, scale, bias, r, relu, stride)
    assert not bool((_fp64(x, w, scale, bias, r, False, stride) == 0).any())      # the ReLU mask cannot depend on rounding
    d = _dev()
    out = {}
    for name, fn in (("fused", lambda *a: _fused(*a, config)), ("pair", _pair)):
        xi, wi = x.to(d).requires_grad_(), w.to(d).requires_grad_()
        ri = r.to(d).requires_grad_() if res else None
        with launches() as calls:
            y = fn(xi, wi, scale.to(d), bias.to(d), ri, relu, stride)
        assert calls.get("conv1x1_bn_fwd", 0) == (name == "fused") and calls.get("frozen_bn_fwd", 0) == (name == "pair"), calls
        y.backward(gy.to(d))
        out[name] = (y.detach(), xi.grad, wi.grad, ri.grad if res else None)
    y, gx, gw, gr = out["fused"]
    assert _C.is_channels_last(y) and y.shape == want.shape
    assert torch.equal(y.cpu().double(), want)
    for got, ref, what in zip(out["fused"], out["pair"], ("y", "grad_x", "grad_w", "grad_residual")):
        if ref is None:
            assert got is None
        else:
            assert got.shape == ref.shape and torch.equal(got, ref), what


@pytest.mark.parametrize("config", CONFIGS)
def test_residual_view_and_frozen_input(config):
    """a residual that is a non-contiguous channels-last view (its gradient arrives in the view), and a frozen input:
    no gradient requested for x and w (nothing of the convolution is saved), then none requested at all"""
    from maskrcnn_benchmark.layers.batch_norm import _Conv1x1FrozenBNAct
    C, K, H, W, stride, relu, res = CASES[0]
    x, w, scale, bias, r, gy = _exact_inputs(C, K, H, W, stride, True, seed=5)
    d = _dev()
    big = torch.zeros(N, K, H, W + 3).contiguous(memory_format=CL)
    big[..., 1:W + 1] = r
    big = big.to(d).requires_grad_()
    view = big[..., 1:W + 1]
    assert not view.is_contiguous(memory_format=CL)
    xd, wd = x.to(d), w.to(d)
    y = _fused(xd, wd, scale.to(d), bias.to(d), view, relu, stride, config)
    assert torch.equal(y.detach().cpu().double(), _fp64(x, w, scale, bias, r, relu, stride))
    assert not y.grad_fn.conv_grads and len(y.grad_fn.saved_tensors) == 2
    y.backward(gy.to(d))
    want = torch.where(y.detach() > 0, gy.to(d), torch.zeros((), device=d))
    assert torch.equal(big.grad[..., 1:W + 1], want) and not bool(big.grad[..., 0].any()) and not bool(big.grad[..., W + 1:].any())
    y2 = _Conv1x1FrozenBNAct.apply(xd, wd, scale.to(d), bias.to(d), view.detach(), relu, stride, config)
    assert not y2.requires_grad and torch.equal(y2, y.detach())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "C%d-K%d-%dx%d-s%d" % c[:5])
def test_random_floats_forward_error_stays_within_the_fp32_summation_bound(case):
    """The fused result and the two-launch result each against fp64, elementwise against the a-priori bound of an fp32
    evaluation in ANY summation order: C products, C - 1 additions, the scale product, the bias and residual additions are
    at most C + 3 roundings of relative size u = 2^-24, each of a partial result no larger than
    M = sum_c |x_c w_c| * |scale| + |bias| + |residual|, so |error| <= (C + 4) u M (one rounding of slack for the
    second-order terms).  A reduced-precision matrix mode (xf32 / bf16 inputs: 2^-11 / 2^-8 per product) exceeds it by
    one to two orders of magnitude at every shape here.
    Why not twice the existing path's measured error: at these shapes MIOpen does not run the kernel family it runs at
    the backbone's sizes, and its result sits at the output's rounding floor — 9.8e-07 at C = 256 -> K = 64, one ulp of
    the largest |y|, where the 64 x 128 tile's in-order sum over 256 channels measures 3.8e-06.  Twice one ulp is less
    than any in-order fp32 sum of 256 terms can promise, so that bound would test MIOpen's choice of solver, not this
    kernel.  Both measured errors are printed (profiles/conv1x1_bn_opbench.txt keeps them)."""
    C, K, H, W, stride, relu, res = case
    x, w, scale, bias, r = _random_inputs(C, K, H, W, stride, res, seed=C * 7 + K)
    want = _fp64(x, w, scale, bias, r, relu, stride)
    mag = torch.einsum("nchw,kc->nkhw", x[:, :, ::stride, ::stride].double().abs(), w[:, :, 0, 0].double().abs())
    mag = mag * scale.double().view(1, -1, 1, 1) + bias.double().abs().view(1, -1, 1, 1) + (r.double().abs() if res else 0.0)
    bound = (C + 4) * 2.0 ** -24 * mag
    d = _dev()
    args = (x.to(d), w.to(d), scale.to(d), bias.to(d), r.to(d) if res else None, relu, stride)
    diff_pair = (_pair(*args).cpu().double() - want).abs()
    assert bool((diff_pair <= bound).all())                       # the bound is one the existing path meets as well
    for config in CONFIGS:
        diff = (_fused(*args, config).cpu().double() - want).abs()
        print("\nconv1x1_bn random floats C=%d K=%d %dx%d s=%d config=%d: fused max err %.3e, two-launch max err %.3e, "
              "largest err / bound %.3f (two-launch %.3f)" % (C, K, H, W, stride, config, float(diff.max()), float(diff_pair.max()),
                                                              float((diff / bound).max()), float((diff_pair / bound).max())))
        assert bool((diff <= bound).all()), (config, float(diff.max()), float((diff / bound).max()))


@pytest.mark.parametrize("config", CONFIGS)
def test_the_fused_launch_is_capturable_in_a_hip_graph(config):
    """the call puts nothing on the stream but its kernel launch: captured once (after an eager call, as the graphed training
    step warms up), replayed on new input values, bit-equal to the eager call"""
    from maskrcnn_benchmark import _C
    C, K, H, W, stride, relu, res = CASES[0]
    d = _dev()
    x, w, scale, bias, r = (t.to(d) for t in _random_inputs(C, K, H, W, stride, True, seed=21))
    x2 = _random_inputs(C, K, H, W, stride, True, seed=22)[0].to(d)
    cfg = _C.conv1x1_bn_config(x, w, stride, r, config)
    assert cfg == config
    _C.conv1x1_bn_forward(x, w, scale, bias, r, relu, stride, cfg)
    torch.cuda.synchronize(d)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = _C.conv1x1_bn_forward(x, w, scale, bias, r, relu, stride, cfg)
    x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize(d)
    assert torch.equal(y, _C.conv1x1_bn_forward(x2, w, scale, bias, r, relu, stride, cfg))


def _bn(C, seed, dev):
    from maskrcnn_benchmark.layers import FrozenBatchNorm2d
    g = torch.Generator().manual_seed(seed)
    bn = FrozenBatchNorm2d(C)
    bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
    bn.bias.copy_(torch.randn(C, generator=g))
    bn.running_mean.copy_(torch.randn(C, generator=g))
    bn.running_var.copy_(torch.rand(C, generator=g) + 0.2)
    return bn.to(dev)


def test_fallbacks_give_todays_result_through_todays_kernels(monkeypatch):
    """NCHW input, bf16, groups 2, C = 6, an empty batch and the switch set to off: exactly `bn.fused(conv(x))`, and the
    call counter shows no conv1x1_bn_fwd (with every served shape forced onto the fused path, so that a fall-back is the
    predicate's decision; the first case is the positive control)"""
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.layers import Conv2d
    from maskrcnn_benchmark.modeling.backbone.resnet import BottleneckWithFixedBatchNorm
    d = _dev()
    monkeypatch.setattr(_C, "CONV1X1_BN", 1)
    g = torch.Generator().manual_seed(11)

    def run(Cin, K, fmt, dtype=torch.float32, groups=1, fused=False):
        conv = Conv2d(Cin, K, 1, bias=False, groups=groups).to(d).to(dtype)
        bn = _bn(K, K, d)
        x = torch.randn(2, Cin, 5, 7, generator=g).to(d).to(dtype).contiguous(memory_format=fmt)
        with launches() as calls:
            y = bn.conv1x1_fused(conv, x, relu=True)
        assert calls.get("conv1x1_bn_fwd", 0) == int(fused) and calls.get("frozen_bn_fwd", 0) == int(not fused), calls
        if not fused:
            assert torch.equal(y, bn.fused(conv(x), relu=True))

    run(8, 16, CL, fused=True)
    run(8, 16, torch.contiguous_format)
    run(8, 16, CL, dtype=torch.bfloat16)
    run(8, 16, CL, groups=2)
    run(6, 16, CL)
    monkeypatch.setattr(_C, "CONV1X1_BN", None)
    run(8, 16, CL)
    monkeypatch.setattr(_C, "CONV1X1_BN", 1)
    block = BottleneckWithFixedBatchNorm(8, 4, 16).to(d)
    with launches() as calls:
        y = block(torch.zeros(0, 8, 5, 7, device=d).contiguous(memory_format=CL))
    assert tuple(y.shape) == (0, 16, 5, 7) and not calls, calls


TOL = 1e-4        # outputs: the whole-model device tests' loss tolerance, relative to max(1, |reference|)
GRAD_TOL = 4e-5   # parameter gradients: their relative Frobenius distance, floored at 1e-3 of the block's largest gradient


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("downsample", [False, True])
def test_bottleneck_fused_equals_unfused_on_the_device(downsample, config, monkeypatch):
    """one Bottleneck with a (strided) projection shortcut and one without, 2 x 64 x 12 x 20: outputs, input gradient
    and parameter gradients of the fused block against the two-launch block"""
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.modeling.backbone.resnet import BottleneckWithFixedBatchNorm
    d = _dev()
    torch.manual_seed(3)
    block = (BottleneckWithFixedBatchNorm(64, 32, 128, stride=2) if downsample else BottleneckWithFixedBatchNorm(64, 16, 64)).to(d)
    for i, m in enumerate(block.modules()):
        if hasattr(m, "running_var"):
            src = _bn(m.weight.numel(), i, d)
            m.load_state_dict(src.state_dict())
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 64, 12, 20, generator=g).to(d).contiguous(memory_format=CL)
    gy = torch.randn(2, 128 if downsample else 64, 6 if downsample else 12, 10 if downsample else 20, generator=g).to(d)

    def run(mode):
        monkeypatch.setattr(_C, "CONV1X1_BN", mode)
        block.zero_grad()
        xi = x.clone(memory_format=CL).requires_grad_()
        with launches() as calls:
            y = block(xi)
        y.backward(gy.contiguous(memory_format=CL))
        return y.detach(), xi.grad, {n: p.grad.clone() for n, p in block.named_parameters()}, calls

    y0, gx0, gp0, calls0 = run(None)
    y1, gx1, gp1, calls1 = run(config)
    n_fused = 3 if downsample else 2
    assert calls0.get("conv1x1_bn_fwd", 0) == 0 and calls0["frozen_bn_fwd"] == n_fused + 1, calls0
    assert calls1.get("conv1x1_bn_fwd", 0) == n_fused and calls1["frozen_bn_fwd"] == 1, calls1
    assert float((y1 - y0).abs().max()) <= TOL * max(1.0, float(y0.abs().max()))
    assert float((gx1 - gx0).norm()) <= GRAD_TOL * float(gx0.norm())
    assert set(gp0) == set(gp1) and len(gp0) == (4 if downsample else 3)
    gmax = max(float(v.norm()) for v in gp0.values())
    for n in gp0:
        assert float((gp1[n] - gp0[n]).norm()) <= GRAD_TOL * max(float(gp0[n].norm()), 1e-3 * gmax), n
