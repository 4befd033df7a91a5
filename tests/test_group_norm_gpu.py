"""Device tests of channels-last GroupNorm (+ residual) (+ ReLU) (csrc/group_norm.hip) against fp64 on the host, computed from
the same dtype-rounded values the device made.  Run with `-m gpu`.

Bounds (u = 2^-24; mu, sigma the group's fp64 mean and standard deviation, r = 1 / sqrt(sigma^2 + eps)):
  statistics  |mean - mu| <= 16 u (|mu| + sigma),  |rstd / r - 1| <= 16 u (1 + |mu| / sigma) — linear in |mu| / sigma, which a
              sum-of-squares variance is not; checked on zero-mean data and on data shifted to mean 100 (std 1) and -300 (std 2)
  output      against fp64 evaluated with the kernel's own mean / rstd: 4 u (|x||a| + |mean||a| + |beta|), a = rstd * gamma,
              + |residual| u with a residual, + one ulp of the storage dtype for fp16 / bf16; ReLU clamps the fp64 value
  backward    against fp64 autograd of group_norm (+ residual) with the upstream gradient masked by the DEVICE's y > 0; per
              tensor, max-norm relative to the tensor's largest magnitude, at most 8 x the error ATen's own fp32 CPU backward
              (contiguous NCHW) makes against the same fp64 result — only the order of the sums differs — and for fp16 / bf16
              at least one ulp of the storage dtype.  The observed ratios are printed.
  Observed maxima on an MI355X (profiles/group_norm_tests.txt): mean 0.14 and rstd 0.17 of their bounds, output 0.93 of its bound;
  backward error over ATen's: grad_x 1.8 (fp32), grad_gamma 3.8, grad_beta 4.0.  ATen is the outlier in two bf16 cases
  (2 x 64 x 13 x 9, no ReLU): its fp32 sum for grad_beta is exact against fp64 there, the kernel's order carries one fp32 rounding
  (1.3e-8); they pass on the half-precision floor, which applies to every tensor of a half-precision case."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import torch_refs

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
U = 2.0 ** -24
EPS = 1e-5
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3

# (N, C, G, H, W).  Routing: the sample kernel serves HW * max(lanes per group, 4) <= 4096 (csrc/group_norm.hip::gn_geometry);
# with 2 channels per group that is HW <= 1024: 32 x 32 = 1024 rows sit on one side, 25 x 41 = 1025 on the other.
SHAPES = [
    (2, 64, 32, 13, 9),        # 2 channels per group, odd plane
    (3, 32, 32, 5, 7),         # 1 channel per group
    (2, 8, 1, 6, 5),           # G = 1
    (5, 256, 32, 7, 7),        # whole samples per workgroup
    (3, 256, 32, 14, 14),      # 200 KB sample in fp32
    (2, 2048, 32, 3, 5),       # 64 channels per group
    (2, 64, 32, 100, 168),     # many workgroups per sample
    (2, 64, 32, 32, 32),       # last plane of the sample kernel
    (2, 64, 32, 25, 41),       # first plane of the split regime
    (2, 6, 3, 4, 5),           # 6 channels: vectors of 2
]
FLAGS = list(itertools.product([False, True], [False, True]))      # (relu, residual)


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


def _cl(shape, dtype, seed, mean=0.0, std=1.0, offset=0):
    """dtype-rounded normal values made on the device as a channels-last [N, C, H, W] tensor whose storage starts `offset`
    elements into its allocation; -> (device tensor, host copy)"""
    N, C, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    v = (torch.randn((N, H, W, C), generator=g, device=DEV) * std + mean).to(dtype)
    buf = torch.empty(v.numel() + offset, dtype=dtype, device=DEV)
    d = buf[offset:].view(N, H, W, C).permute(0, 3, 1, 2)
    d.copy_(v.permute(0, 3, 1, 2))
    assert d.storage_offset() == offset and (d.numel() == 0 or d.is_contiguous(memory_format=CL))
    return d, d.cpu()


def _affine(C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    gamma = torch.randn(C, generator=g, device=DEV) + 1.0
    beta = torch.randn(C, generator=g, device=DEV)
    return gamma, beta


def _groups64(t, G):
    """host [N, C, H, W] -> fp64 [N, G, D * H * W]"""
    N, C = t.shape[:2]
    return t.double().reshape(N, G, -1)


def _check_statistics(x, mean, rstd, G):
    xg = _groups64(x, G)
    mu, var = xg.mean(2), xg.var(2, unbiased=False)
    sd = var.sqrt()
    r = 1.0 / (var + EPS).sqrt()
    m_ratio = ((mean.double().cpu() - mu).abs() / (16 * U * (mu.abs() + sd))).max().item()
    r_ratio = ((rstd.double().cpu() / r - 1).abs() / (16 * U * (1 + mu.abs() / sd))).max().item()
    print("  statistics: mean error / bound %.3f, rstd error / bound %.3f" % (m_ratio, r_ratio))
    assert m_ratio <= 1.0 and r_ratio <= 1.0, (m_ratio, r_ratio)


def _check_output(x, res, gamma, beta, y, mean, rstd, G, relu, dtype):
    N, C, H, W = x.shape
    D = C // G
    m = mean.double().cpu().view(N, G, 1).expand(N, G, D).reshape(N, C, 1, 1)
    a = (rstd.double().cpu().view(N, G, 1).expand(N, G, D).reshape(N, C) * gamma.double().cpu().view(1, C)).view(N, C, 1, 1)
    b = beta.double().cpu().view(1, C, 1, 1)
    ref = (x.double() - m) * a + b
    bound = 4 * U * (x.double().abs() * a.abs() + m.abs() * a.abs() + b.abs())
    if res is not None:
        ref = ref + res.double()
        bound = bound + res.double().abs() * U
    if relu:
        ref = ref.clamp(min=0)
    if dtype != torch.float32:
        fi = torch.finfo(dtype)
        bound = bound + fi.eps * torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=fi.tiny))))
    ratio = ((y.double().cpu() - ref).abs() / bound.clamp(min=1e-300)).max().item()
    print("  output: error / bound %.3f" % ratio)
    assert ratio <= 1.0, ratio


def _host_backward(x, res, gamma, beta, gy_masked, G, dtype64):
    """gradients of group_norm(x) [+ res] on the host in `dtype64` (fp64: the reference; fp32: ATen's own error), NCHW"""
    xx = x.to(dtype64).contiguous().requires_grad_(True)
    ga = gamma.cpu().to(dtype64).requires_grad_(True)
    be = beta.cpu().to(dtype64).requires_grad_(True)
    out = F.group_norm(xx, G, ga, be, EPS)
    rr = None
    if res is not None:
        rr = res.to(dtype64).contiguous().requires_grad_(True)
        out = out + rr
    out.backward(gy_masked.to(dtype64).contiguous())
    return {"grad_x": xx.grad, "grad_residual": None if rr is None else rr.grad, "grad_gamma": ga.grad, "grad_beta": be.grad}


def _rel(a, ref):
    return ((a.double() - ref.double()).abs().max() / ref.double().abs().max().clamp(min=1e-300)).item()


def _run(shape, dtype, relu, with_res, seed, mean=0.0, std=1.0, offset=0, backward=True):
    """forward (+ backward) through the wrappers, every check of the module docstring, both runs bit-equal"""
    C_ = _C()
    N, C, G, H, W = shape
    x_d, x = _cl((N, C, H, W), dtype, seed, mean, std, offset)
    res_d, res = _cl((N, C, H, W), dtype, seed + 1, 0.0, 1.0, offset) if with_res else (None, None)
    gamma, beta = _affine(C, seed + 2)
    assert C_.group_norm_supported(x_d, G)
    y, mu, rs = C_.group_norm_forward(x_d, G, gamma, beta, EPS, res_d, relu)
    y2, mu2, rs2 = C_.group_norm_forward(x_d, G, gamma, beta, EPS, res_d, relu)
    assert y.dtype == dtype and y.shape == x_d.shape and y.is_contiguous(memory_format=CL)
    assert mu.dtype == torch.float32 and tuple(mu.shape) == (N, G) and tuple(rs.shape) == (N, G)
    assert torch.equal(y, y2) and torch.equal(mu, mu2) and torch.equal(rs, rs2), "forward is deterministic"
    _check_statistics(x, mu, rs, G)
    _check_output(x, res, gamma, beta, y, mu, rs, G, relu, dtype)
    if not backward:
        return
    gy_d, gy = _cl((N, C, H, W), dtype, seed + 3, 0.0, 1.0, offset)
    got = C_.group_norm_backward(gy_d, x_d, y, G, gamma, mu, rs, relu, with_res, True, True)
    again = C_.group_norm_backward(gy_d, x_d, y, G, gamma, mu, rs, relu, with_res, True, True)
    frozen = C_.group_norm_backward(gy_d, x_d, y, G, gamma, mu, rs, relu, with_res, False, False)
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(a, b), "backward is deterministic"
    assert frozen[2] is None and frozen[3] is None and torch.equal(frozen[0], got[0])
    assert (got[1] is None) == (not with_res) and (frozen[1] is None or torch.equal(frozen[1], got[1]))
    assert got[0].dtype == dtype and got[0].is_contiguous(memory_format=CL) and got[2].dtype == torch.float32
    masked = gy.double() * (y.cpu() > 0).double() if relu else gy.double()
    ref = _host_backward(x, res, gamma, beta, masked, G, torch.float64)
    aten = _host_backward(x, res, gamma, beta, masked, G, torch.float32)
    floor = 0.0 if dtype == torch.float32 else torch.finfo(dtype).eps
    dev = dict(zip(("grad_x", "grad_residual", "grad_gamma", "grad_beta"), got))
    for name, r in ref.items():
        if r is None:
            continue
        mine, theirs = _rel(dev[name].cpu(), r), _rel(aten[name], r)
        allowed = max(8 * theirs, floor)
        print("  %s: error %.3g, ATen fp32 %.3g, ratio %s, allowed %.3g"
              % (name, mine, theirs, ("%.2f" % (mine / theirs)) if theirs > 0 else "-", allowed))
        assert mine <= allowed, (name, mine, theirs, allowed)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("relu,res", FLAGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_against_fp64(shape, relu, res, dtype):
    _run(shape, dtype, relu, res, seed=sum(shape))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("relu,res", FLAGS)
def test_storage_offset_of_one_element_takes_vector_width_one(relu, res, dtype):
    _run((2, 64, 32, 13, 9), dtype, relu, res, seed=5, offset=1)


@pytest.mark.parametrize("mean,std", [(100.0, 1.0), (-300.0, 2.0)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_statistics_of_shifted_data_stay_linear_in_mean_over_sigma(shape, mean, std):
    """what a sum-of-squares variance fails by 8 x and more (its error is quadratic in |mu| / sigma)"""
    _run(shape, torch.float32, False, False, seed=7, mean=mean, std=std, backward=False)


@pytest.mark.parametrize("shape", [(2, 64, 32, 32, 32), (2, 64, 32, 25, 41)], ids=["sample", "split"])
def test_shifted_backward_on_each_side_of_the_routing_threshold(shape):
    _run(shape, torch.float32, True, True, seed=9, mean=100.0, std=1.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_fused_relu_follows_torch_relu_on_a_non_finite_residual(dtype):
    """The GroupNorm analogue of torch_refs.check_fused_relu_non_finite: NaN, +-inf and -0.0 arrive through the RESIDUAL only
    (its patterns there), so the group statistics stay finite.  Forward: torch.relu — y is NaN exactly where the residual is,
    +inf under a +inf residual, 0 under a -inf one.  Backward: the gate is aten.threshold_backward(gy, y, 0), which PASSES the
    gradient where y is NaN (as F.group_norm + relu does under DETOPS_GROUP_NORM=torch): grad_residual equals it exactly, and
    grad_x / grad_gamma / grad_beta meet the module's backward rule against fp64 fed the same masked gradient."""
    C_ = _C()
    N, C, G, H, W = 2, 8, 2, 4, 6
    inf, nan = float("inf"), float("nan")
    x_d, x = _cl((N, C, H, W), dtype, 21)
    res = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(22))
    res[:, :, 1, :4] = torch.tensor([-inf, inf, nan, inf])
    res[:, :, 2, :2] = torch.tensor([-0.0, -inf])
    res = res.to(dtype)
    res_d = res.to(DEV).contiguous(memory_format=CL)
    gamma, beta = _affine(C, 23)
    y_d, mu, rs = C_.group_norm_forward(x_d, G, gamma, beta, EPS, res_d, True)
    y = y_d.cpu()
    _check_statistics(x, mu, rs, G)
    assert torch.equal(y.isnan(), res.isnan()) and int(y.isnan().sum()) == N * C
    assert bool((y[res == inf] == inf).all()) and bool((y[res == -inf] == 0).all()) and not bool(torch.isinf(y[res.isfinite()]).any())
    gy_d, gy = _cl((N, C, H, W), dtype, 24)
    got = dict(zip(("grad_x", "grad_residual", "grad_gamma", "grad_beta"),
                   C_.group_norm_backward(gy_d, x_d, y_d, G, gamma, mu, rs, True, True, True, True)))
    want = torch.ops.aten.threshold_backward(gy.float(), y.float(), 0)
    assert bool((want[y.isnan()] == gy.float()[y.isnan()]).all()) and bool((want[y == 0] == 0).all())
    torch_refs._exact(got["grad_residual"].cpu(), want.to(dtype), "group_norm grad_residual")
    masked = want.double()
    ref = _host_backward(x, res, gamma, beta, masked, G, torch.float64)
    aten = _host_backward(x, res, gamma, beta, masked, G, torch.float32)
    floor = 0.0 if dtype == torch.float32 else torch.finfo(dtype).eps
    for name in ("grad_x", "grad_gamma", "grad_beta"):
        mine, theirs = _rel(got[name].cpu(), ref[name]), _rel(aten[name], ref[name])
        allowed = max(8 * theirs, floor)
        print("  %s: error %.3g, ATen fp32 %.3g, allowed %.3g" % (name, mine, theirs, allowed))
        assert mine <= allowed, (name, mine, theirs, allowed)


def test_host_rule_equals_the_library_rule():
    C_ = _C()
    for C in list(range(1, 70)) + [96, 128, 256, 512, 768, 1024, 2048, 4096]:
        for G in (1, 2, 3, 4, 6, 8, 16, 32, 64, C):
            assert bool(C_.lib.detops_group_norm_supported(C, G)) == bool(C_.group_norm_serves(C, G)), (C, G)
    for C in (64, 128, 256, 512, 1024, 2048):
        assert C_.group_norm_serves(C, 32)


def _module(C, G, seed):
    from maskrcnn_benchmark.layers import GroupNorm
    gn = GroupNorm(G, C).to(DEV)
    gamma, beta = _affine(C, seed)
    with torch.no_grad():
        gn.weight.copy_(gamma)
        gn.bias.copy_(beta)
    return gn


def test_served_input_calls_only_group_norm_entries_and_autograd_agrees(entries):
    gn = _module(64, 32, 1)
    x_d, x = _cl((2, 64, 13, 9), torch.float32, 2)
    res_d, res = _cl((2, 64, 13, 9), torch.float32, 3)
    x_d.requires_grad_(True)
    res_d.requires_grad_(True)
    y = gn.fused(x_d, relu=True, residual=res_d)
    gy_d, gy = _cl((2, 64, 13, 9), torch.float32, 4)
    y.backward(gy_d)
    assert entries and all(n.startswith("detops_group_norm_") for n in entries), entries
    assert "detops_group_norm_forward_nhwc" in entries and "detops_group_norm_backward_nhwc" in entries
    assert y.is_contiguous(memory_format=CL)
    masked = gy.double() * (y.detach().cpu() > 0).double()
    ref = _host_backward(x, res, gn.weight.detach(), gn.bias.detach(), masked, 32, torch.float64)
    assert _rel(x_d.grad.cpu(), ref["grad_x"]) < 1e-5 and _rel(gn.weight.grad.cpu(), ref["grad_gamma"]) < 1e-5
    assert _rel(gn.bias.grad.cpu(), ref["grad_beta"]) < 1e-5 and torch.equal(res_d.grad.cpu().double(), ref["grad_residual"])
    # frozen parameters: no parameter gradient is asked for
    gn2 = _module(64, 32, 1)
    for p in gn2.parameters():
        p.requires_grad = False
    x2 = x_d.detach().clone().requires_grad_(True)
    gn2.fused(x2, relu=True, residual=res_d.detach()).backward(gy_d)
    assert gn2.weight.grad is None and gn2.bias.grad is None and torch.equal(x2.grad, x_d.grad)
    assert torch.equal(gn(x_d.detach()), gn.fused(x_d.detach()))


@pytest.mark.parametrize("case", ["nchw", "2d", "unserved", "switch", "empty"])
def test_everything_else_calls_f_group_norm_and_no_entry(entries, monkeypatch, case):
    C_ = _C()
    C, G, shape = 64, 32, (2, 64, 13, 9)
    if case == "unserved":
        C, G, shape = 12, 2, (2, 12, 4, 5)           # 6 channels per group
    if case == "empty":
        shape = (0, 64, 8, 8)
    gn = _module(C, G, 1)
    if case == "2d":
        g = torch.Generator(device=DEV).manual_seed(2)
        x = torch.randn((6, 64), generator=g, device=DEV)
        res = torch.randn((6, 64), generator=g, device=DEV)
    else:
        x, _ = _cl(shape, torch.float32, 2)
        res, _ = _cl(shape, torch.float32, 3)
        if case == "nchw":
            x, res = x.contiguous(), res.contiguous()
    if case == "switch":
        monkeypatch.setattr(C_, "GROUP_NORM", "torch")
    assert not gn.serves(x)
    ref = F.group_norm(x, G, gn.weight, gn.bias, gn.eps)
    with torch.no_grad():
        assert torch.equal(gn(x), ref)
        assert torch.equal(gn.fused(x, True, res), torch.relu(ref + res))
        assert gn.fused(x, True, res).shape == x.shape
    assert entries == [], entries


def test_bad_arguments_return_their_codes_and_write_nothing():
    C_ = _C()
    lib, ptr = C_.lib, C_.ptr
    N, C, G, H, W = 2, 64, 32, 13, 9
    x_d, _ = _cl((N, C, H, W), torch.float32, 1)
    gamma, beta = _affine(C, 2)
    nbytes = int(lib.detops_group_norm_workspace_bytes(N, H * W, C, G))
    big = (2, 64, 32, 25, 41)                                       # split regime: the forward uses its workspace
    big_bytes = int(lib.detops_group_norm_workspace_bytes(big[0], big[3] * big[4], big[1], big[2]))
    assert nbytes > 0 and big_bytes > 0
    assert lib.detops_group_norm_workspace_bytes(N, H * W, 12, 2) == 0
    ws = torch.empty(max(nbytes, big_bytes), dtype=torch.uint8, device=DEV)
    sentinel = 7.0
    y = torch.full_like(x_d, sentinel)
    mean = torch.full((N, G), sentinel, device=DEV)
    rstd = torch.full((N, G), sentinel, device=DEV)
    st = C_.stream_of(x_d)

    def fwd(xp, c, g, n=N, hw=H * W, wb=nbytes):
        return lib.detops_group_norm_forward_nhwc(xp, ptr(gamma), ptr(beta), None, ptr(y), ptr(mean), ptr(rstd), 0, n, hw, c, g,
                                                  EPS, 0, ptr(ws), wb, st)

    def bwd(gyp, c, g, n=N, hw=H * W, wb=nbytes):
        return lib.detops_group_norm_backward_nhwc(gyp, ptr(x_d), None, ptr(gamma), ptr(mean), ptr(rstd), ptr(y), None, None, None, 0,
                                                   n, hw, c, g, 0, ptr(ws), wb, st)

    assert fwd(None, C, G) == EINVAL and bwd(None, C, G) == EINVAL
    assert fwd(ptr(x_d), C, 24) == EUNSUPPORTED and bwd(ptr(x_d), C, 24) == EUNSUPPORTED       # C % G != 0
    assert fwd(ptr(x_d), 12, 2) == EUNSUPPORTED                                                 # 6 channels per group
    assert fwd(ptr(x_d), C, G, wb=nbytes - 1) == EWORKSPACE and bwd(ptr(x_d), C, G, wb=nbytes - 1) == EWORKSPACE
    assert fwd(ptr(x_d), C, G, n=big[0], hw=big[3] * big[4], wb=big_bytes - 1) == EWORKSPACE
    assert fwd(ptr(x_d), C, G, n=-1) == EINVAL
    assert fwd(ptr(x_d), C, G, n=0) == 0 and fwd(ptr(x_d), C, G, hw=0) == 0 and bwd(ptr(x_d), C, G, n=0) == 0
    torch.cuda.synchronize()
    for t in (y, mean, rstd):
        assert bool((t == sentinel).all()), "nothing was written"
