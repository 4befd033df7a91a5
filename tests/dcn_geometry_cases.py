"""Deformable convolution at the geometries that only the emulation used to run: the K-step widths, deformable groups and
ragged tiles of the fused MFMA forward, the channels-last (NHWC) pipeline away from 3x3 / stride 1 / C == Cout, the
transposed-sampling input gradient, the overflow list, and rectangular kernels / strides / paddings / dilations through
every entry point.  The case table, the input generator and the check bodies live here, parameterised by device:
tests/test_dcn_geometry_gpu.py runs them on the MI355X, tests/test_dcn_geometry_emu.py on CPU tensors through the host
emulation of the same sources (tests/cpu_shim.py, backend "emu-lib"), which proves the cases and the oracle without a GPU.

EXACT-ARITHMETIC INPUTS.  `exact_inputs` draws every operand so that every product and every partial sum of the operator is
exactly representable:

    input x, upstream gradient   integers in [-2, 2]            weights                integers in {-1, 0, 1}
    bias                         integer + 0.5, |bias| <= 3.5   modulation mask        {0.5, 1}
    offsets                      multiples of 0.25 in [-3, 3]; about 5 % replaced by multiples of 0.25 in [-8, 8]
                                 (taps partly and wholly outside the map)

Bilinear weights are then multiples of 1/16, interpolated and modulated column values multiples of 1/32 of magnitude <= 2
(7 significant bits: exact in fp16, bf16 and any reduced-precision GEMM input mode), and all sums stay far below 2^24 of
those units.  The result therefore does not depend on summation order, tile shape, atomics or GEMM solver: in fp32 the
oracle's output IS the answer bit for bit, and a half-precision output is one round-to-nearest-even of that exact value,
`torch.from_numpy(oracle_result).to(dtype)`.  Comparisons are `torch.equal`.  Where half-precision results are not
reproducible (gradients: a pile-up beyond the index's 8 slots is added by per-add-rounded atomics) the project's 2e-2 of the
tensor's largest reference magnitude applies, and one random-float case per path (`synth.dcn_inputs`: general sampling
positions, heavy offset tail) keeps the project's 1e-4 (fp32) / 2e-2 (half) of each tensor's scale.

Every check asserts with the launch counter (`torch_refs.launches`) that the kernel it is about ran: a silent fall-back to
another path does not pass.
"""
import collections

import numpy as np
import torch

import oracle
from torch_refs import launches

Case = collections.namedtuple("Case", "name B C H W Cout kh kw pad stride dil dg")


def _c(name, B, C, H, W, Cout, k, pad, stride, dil, dg=1):
    pair = lambda v: tuple(v) if isinstance(v, tuple) else (v, v)  # noqa: E731
    kh, kw = pair(k)
    return Case(name, B, C, H, W, Cout, kh, kw, pair(pad), pair(stride), pair(dil), dg)


# ---- fused MFMA forward (half precision; BKC = channels of one tap per K-step, picked from (C / dg) % 128 and % 64)
FUSED_CASES = [
    _c("bkc32-ragged", 2, 32, 9, 11, 40, 3, 1, 1, 1),            # BKC = 32 (NP = 1); one ragged Cout tile; 198 pixels: ragged pixel tile
    _c("bkc32-dg2-s2d2", 1, 64, 12, 10, 130, 3, 2, 2, 2, 2),     # BKC = 32, two deformable groups; 2nd Cout tile has 2 rows; stride, dilation
    _c("bkc64", 1, 64, 7, 9, 32, 3, 1, 1, 1),                    # BKC = 64 (NP = 2)
    _c("bkc64-3steps", 1, 192, 6, 7, 64, 3, 1, 1, 1),            # BKC = 64, three steps per tap (192 % 128 != 0)
    _c("bkc128-dg2", 1, 256, 6, 7, 136, 3, 1, 1, 1, 2),          # BKC = 128, two groups; ragged second Cout tile
    _c("rect-1x3", 2, 64, 9, 11, 64, (1, 3), (0, 1), (1, 2), (1, 2)),
    _c("rect-3x1-dg2", 2, 64, 10, 13, 40, (3, 1), (2, 0), (2, 1), (2, 1), 2),
]
# the auto rule (dcn_fused_preferred) picks the fused kernel without any switch: 520 workgroups >= 2 x 256, Cout <= 256
FUSED_AUTO = _c("auto-res2", 2, 64, 130, 128, 64, 3, 1, 1, 1)

# ---- channels-last pipeline (deformable_group == 1; sub = lanes per pixel, nv = 16-byte vectors per lane)
NHWC_S2D2 = _c("s2d2", 1, 128, 12, 10, 64, 3, 2, 2, 2)           # fp32: sub = 32, C != Cout, stride and dilation
NHWC_K1 = _c("k1", 2, 64, 7, 8, 256, 1, 0, 1, 1)                 # k = 1, sub = 16
NHWC_NV4 = _c("nv4", 1, 1024, 5, 6, 64, 3, 1, 1, 1)              # nv = 4: all four register vectors of kMaxNv
NHWC_RECT_1X3 = _c("rect-1x3", 2, 64, 9, 11, 128, (1, 3), (0, 1), (1, 2), (1, 2))
NHWC_RECT_3X1 = _c("rect-3x1", 1, 128, 10, 13, 64, (3, 1), (2, 0), (2, 1), (2, 1))
NHWC_FP32_CASES = [NHWC_S2D2, NHWC_K1, NHWC_NV4, NHWC_RECT_1X3, NHWC_RECT_3X1]
# half precision: a channel count serves the pipeline from 128 on (128 / 8 = 16 vectors).  Cout = 64 of NHWC_S2D2 is
# therefore OUTSIDE the plan in half (64 / 8 = 8): that shape runs the reference-layout kernels, which is asserted;
# NHWC_S2D2_HALF is the same geometry with the smallest Cout the half plan serves (sub = 16).  Its integer column gradient
# stays <= 2 * 128 = 256: every integer up to 256 is a bf16 number.
NHWC_S2D2_HALF = _c("s2d2-cout128", 1, 128, 12, 10, 128, 3, 2, 2, 2)
NHWC_NV4_HALF = _c("nv4-half", 1, 2048, 5, 6, 128, 3, 1, 1, 1)   # nv = 4 in half (fp16 only)

# ---- reference-layout kernels (C = 8: outside both plans), rectangular
REF_RECT_CASES = [_c("ref-3x1", 2, 8, 10, 13, 6, (3, 1), (2, 0), (2, 1), (2, 1), 2),
                  _c("ref-1x3", 2, 8, 10, 13, 6, (1, 3), (0, 2), (1, 2), (1, 2), 2)]

HALF_TOL, FP32_TOL = 2e-2, 1e-4       # the project's tolerances, relative to each tensor's largest reference magnitude


def out_hw(c):
    return ((c.H + 2 * c.pad[0] - (c.dil[0] * (c.kh - 1) + 1)) // c.stride[0] + 1,
            (c.W + 2 * c.pad[1] - (c.dil[1] * (c.kw - 1) + 1)) // c.stride[1] + 1)


def is_square(c):
    return c.kh == c.kw and c.pad[0] == c.pad[1] and c.stride[0] == c.stride[1] and c.dil[0] == c.dil[1]


# (case, modulated) through the layers: the v2 layer takes scalar geometry, so rectangular v2 runs through the reference-named
# entry points only (check_nhwc_reference_names)
NHWC_FP32_LAYER_RUNS = [(c, m) for c in NHWC_FP32_CASES for m in (False, True) if is_square(c) or not m]


def run_id(v):
    return v.name if isinstance(v, Case) else ("v2" if v else "v1")


# ---------------------------------------------------------------------------------------------- inputs and references
def exact_inputs(c, seed=0):
    """-> dict of fp32 arrays x, off, mask, wgt, bias, go (see the module docstring); v1 uses x, off, wgt, go only"""
    rng = np.random.RandomState(1000 + seed)
    Ho, Wo = out_hw(c)
    K = c.kh * c.kw
    quarter = lambda lo, hi, shape: rng.randint(4 * lo, 4 * hi + 1, shape) / 4.0  # noqa: E731
    off = quarter(-3, 3, (c.B, c.dg * 2 * K, Ho, Wo))
    tail = rng.rand(*off.shape) < 0.05
    off[tail] = quarter(-8, 8, int(tail.sum()))
    f = np.float32
    return dict(x=rng.randint(-2, 3, (c.B, c.C, c.H, c.W)).astype(f), off=off.astype(f),
                mask=rng.choice([0.5, 1.0], (c.B, c.dg * K, Ho, Wo)).astype(f),
                wgt=rng.randint(-1, 2, (c.Cout, c.C, c.kh, c.kw)).astype(f),
                bias=(rng.randint(-4, 4, (c.Cout,)) + 0.5).astype(f),
                go=rng.randint(-2, 3, (c.B, c.Cout, Ho, Wo)).astype(f))


def float_inputs(c, dtype, seed=0):
    """ordinary random floats (synth.dcn_inputs: heavy offset tail) for a square case, rounded to `dtype` so that the oracle
    sees the values the kernels see"""
    import synth
    assert is_square(c)
    Ho, Wo = out_hw(c)
    x, off, mask, wgt = synth.dcn_inputs(c.B, c.C, c.H, c.W, c.Cout, c.kh, c.dg, True, seed=50 + seed)
    rng = np.random.RandomState(60 + seed)
    d = dict(x=x, off=off[:, :, :Ho, :Wo], mask=mask[:, :, :Ho, :Wo], wgt=wgt, bias=rng.randn(c.Cout).astype(np.float32),
             go=rng.randn(c.B, c.Cout, Ho, Wo).astype(np.float32))
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype).float().numpy() for k, v in d.items()}


class Problem(object):
    """inputs of one case + the oracle's forward and backward results, computed once and shared (read-only)"""

    def __init__(self, c, modulated, inputs):
        self.case, self.modulated = c, modulated
        self.inp = dict(inputs)
        if not modulated:
            self.inp["mask"] = self.inp["bias"] = None
        for a in self.inp.values():
            if a is not None:
                a.setflags(write=False)
        self._fwd = self._bwd = None

    def _args(self):
        i = self.inp
        return i["x"], i["off"], i["mask"], i["wgt"]

    def _geo(self):
        c = self.case
        return c.pad, c.stride, c.dil, 1, c.dg

    @property
    def forward(self):
        if self._fwd is None:
            self._fwd = oracle.deform_conv_forward(*self._args(), self.inp["bias"], *self._geo())
            self._fwd.setflags(write=False)
        return self._fwd

    @property
    def backward(self):
        """dict input, offset, mask, weight, bias (None where the form has none)"""
        if self._bwd is None:
            r = oracle.deform_conv_backward(*self._args(), self.inp["go"], self.modulated, *self._geo())
            for a in r:
                if a is not None:
                    a.setflags(write=False)
            self._bwd = dict(zip(("input", "offset", "mask", "weight", "bias"), r))
        return self._bwd


_PROBLEMS = {}


def problem(c, modulated, kind="exact", dtype=torch.float32, seed=0):
    """the shared Problem of (case, v1 / v2, "exact" | "float" inputs)"""
    key = (c, modulated, kind, dtype if kind == "float" else None, seed)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = Problem(c, modulated, exact_inputs(c, seed) if kind == "exact" else float_inputs(c, dtype, seed))
    return _PROBLEMS[key]


def pileup_problem(c, landing):
    """the construction of test_emu_deformable_channels_last_input_gradient_with_overflowing_pixels on exact inputs: every
    sampling point of every tap lands on the one dyadic point `landing`, so its 4 neighbouring pixels each receive Ho * Wo
    contributions per tap against the 8 slots of the inverted index (v2: mask in {0.5, 1})"""
    key = (c, "pileup", landing)
    if key not in _PROBLEMS:
        assert is_square(c) and c.stride == (1, 1) and c.dil == (1, 1) and c.dg == 1
        inp = exact_inputs(c, seed=7)
        Ho, Wo = out_hw(c)
        hh, ww = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
        off = np.zeros_like(inp["off"])
        for i in range(c.kh):
            for j in range(c.kw):
                off[:, 2 * (i * c.kw + j)] = landing[0] - (hh - c.pad[0] + i)      # sampling row = ho - pad + i + off_h
                off[:, 2 * (i * c.kw + j) + 1] = landing[1] - (ww - c.pad[1] + j)
        inp["off"] = off
        _PROBLEMS[key] = Problem(c, True, inp)
        rin = _PROBLEMS[key].backward["input"]
        assert np.count_nonzero(np.abs(rin).sum(1)) == 4 * c.B
    return _PROBLEMS[key]


# ---------------------------------------------------------------------------------------------- helpers
def set_tuning(device, key, value):
    """a tuning switch of the library: `_C`'s wrappers read some switches from the device library (`_lib.tuning_get`) and the
    kernels' dispatch reads them in the library that is called — under the emulation both must agree"""
    from maskrcnn_benchmark import _lib
    _lib.tuning_set(key, value)
    if torch.device(device).type == "cpu":
        import emu
        emu.tuning_set(key, value)


def _dcn(calls):
    return {k: v for k, v in calls.items() if k.startswith("dcn_")}


def _tensors(p, device, dtype, fmt=torch.contiguous_format, grad=False):
    """-> dict of tensors of the problem's inputs on `device` in `dtype` (4-d ones in memory format `fmt`)"""
    out = {}
    for k, a in p.inp.items():
        if a is None:
            out[k] = None
            continue
        t = torch.from_numpy(np.array(a)).to(device=device, dtype=dtype)      # (a copy: the shared arrays are read-only)
        if t.dim() == 4:
            t = t.contiguous(memory_format=fmt)
        out[k] = t.requires_grad_() if grad and k != "go" else t
    return out


def _rounded(a, dtype):
    return torch.from_numpy(np.array(a)).to(dtype)


def _bit_equal(got, want, dtype, what):
    got, want = got.detach().cpu().contiguous(), _rounded(want, dtype)
    assert got.dtype == dtype and got.shape == want.shape, (what, got.dtype, tuple(got.shape), tuple(want.shape))
    if not torch.equal(got, want):
        d = (got.double() - want.double()).abs()
        raise AssertionError("%s: %d of %d elements differ, largest difference %g (largest reference magnitude %g)"
                             % (what, int((d > 0).sum()) + int(torch.isnan(d).sum()), d.numel(), float(d.nan_to_num(nan=np.inf).max()),
                                float(want.double().abs().max())))


def _near(got, want, tol, what):
    err = float(np.abs(got.detach().float().cpu().numpy() - want).max())      # NaN (a buffer not overwritten) fails the comparison
    print("%s: largest error %.3g, bound %.3g" % (what, err, tol * float(np.abs(want).max())))
    assert err <= tol * float(np.abs(want).max()), (what, err, float(np.abs(want).max()))


def _forward(p, t, keep=None):
    """the forward of `p` on the tensors `t`: v1 through the layer (which takes per-axis tuples); v2 through the layer where
    the geometry is square (its API is scalar), else through `_C.modulated_deform_conv_forward` (H-before-W)"""
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.layers import deform_conv, modulated_deform_conv
    c = p.case
    if not p.modulated:
        return deform_conv(t["x"], t["off"], t["wgt"], c.stride, c.pad, c.dil, 1, c.dg)
    if is_square(c):
        return modulated_deform_conv(t["x"], t["off"], t["mask"], t["wgt"], t["bias"], c.stride[0], c.pad[0], c.dil[0], 1, c.dg)
    x = t["x"].detach()
    e = x.new_empty(0)
    out = x.new_empty((c.B, c.Cout) + out_hw(c))
    _C.modulated_deform_conv_forward(x, t["wgt"].detach(), t["bias"].detach(), e, t["off"].detach(), t["mask"].detach(), out, e,
                                     c.kh, c.kw, c.stride[0], c.stride[1], c.pad[0], c.pad[1], c.dil[0], c.dil[1], 1, c.dg, True,
                                     keep=keep)
    return out


# ---------------------------------------------------------------------------------------------- fused MFMA forward
def check_fused_forward(device, c, dtype, modulated, kind="exact", force=True):
    """`dcn_fused_fwd_kernel` (tuning dcn_fused = 1, or the auto rule with force=False) in fp16 / bf16, v1 (no mask, no bias)
    or v2 (mask and bias): the launch counter shows the fused kernel and no im2col; on exact inputs the output is bit-equal
    to the rounded oracle, and so is im2col + GEMM (dcn_fused = 2) on the same inputs; on random floats both are within 2e-2
    of the output scale."""
    p = problem(c, modulated, kind, dtype)
    t = _tensors(p, device, dtype)
    set_tuning(device, "dcn_fused", 1 if force else 0)
    with launches() as calls:
        y = _forward(p, t)
    assert _dcn(calls) == {"dcn_fused_fwd": 1}, calls
    if kind == "exact":
        _bit_equal(y, p.forward, dtype, "fused forward %s" % c.name)
    else:
        _near(y, p.forward, HALF_TOL, "fused forward %s" % c.name)
    set_tuning(device, "dcn_fused", 2)
    with launches() as calls:
        y0 = _forward(p, t)
    assert "dcn_fused_fwd" not in calls and (calls.get("dcn_im2col", 0) or calls.get("dcn_im2col_nhwc", 0)), calls
    if kind == "exact":
        _bit_equal(y0, p.forward, dtype, "im2col + GEMM forward %s" % c.name)
    else:
        _near(y0, p.forward, HALF_TOL, "im2col + GEMM forward %s" % c.name)


# ---------------------------------------------------------------------------------------------- channels-last pipeline
def _compare_gradients(p, got, dtype, exact, what):
    for name, g in got.items():
        want = p.backward[name]
        if want is None:
            assert g is None, (what, name)
            continue
        assert g is not None and g.dtype == dtype, (what, name)
        if exact:
            _bit_equal(g, want, dtype, "%s %s gradient" % (what, name))
        else:
            _near(g, want, HALF_TOL if dtype != torch.float32 else FP32_TOL, "%s %s gradient" % (what, name))


def check_nhwc_layer(device, c, dtype, modulated, channels_last=False, input_grad="col2im", kind="exact", in_plan=True):
    """deform_conv / modulated_deform_conv (layers/dcn) forward + backward on a shape of the channels-last plan, NCHW or
    everything channels-last, with the input gradient as the col2im gather or (`_C.DCN_INPUT_GRAD = "transposed"`, set by the
    caller) the transposed sampling + GEMM.  Launches: those of torch_refs.check_dcn_layer_in_plan — one im2col (the column
    matrix is kept for the backward pass), the coordinate kernel, the input-gradient kernel, and two layout transposes for
    NCHW tensors.  Exact inputs: fp32 output and every gradient bit-equal to the oracle; half output bit-equal to the rounded
    oracle, half gradients within 2e-2 of each tensor's largest reference magnitude (a pile-up beyond 8 slots goes through
    per-add-rounded atomics).  Random floats: 1e-4 (fp32) / 2e-2 (half).  v2 carries a bias: it is added inside the forward
    GEMM, so a half output is still ONE rounding of sum + bias.
    `in_plan=False`: the shape is outside the plan in this dtype — the reference-layout kernels must serve it (same values)."""
    from maskrcnn_benchmark import _C
    assert _C.DCN_INPUT_GRAD == input_grad
    p = problem(c, modulated, kind, dtype)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    t = _tensors(p, device, dtype, fmt, grad=True)
    half = dtype != torch.float32
    with launches() as calls:
        y = _forward(p, t)
        y.backward(t["go"])
    if in_plan:
        want = {"dcn_im2col_nhwc": 1, "dcn_coord_nhwc": 1, "dcn_transposed_sample" if input_grad == "transposed" else "dcn_col2im_nhwc": 1}
        if not channels_last:
            want["dcn_to_nhwc"] = 2
        assert _C.is_channels_last(y) == channels_last and _C.is_channels_last(t["x"].grad) == channels_last
    else:
        want = {"dcn_im2col": 2, "dcn_col2im_coord": 1, "dcn_col2im": 1}
    assert _dcn(calls) == want, calls
    what = "%s %s%s" % (c.name, "v2" if modulated else "v1", " channels-last" if channels_last else "")
    if kind == "exact":
        _bit_equal(y, p.forward, dtype, what + " output")
    else:
        _near(y, p.forward, HALF_TOL if half else FP32_TOL, what + " output")
    got = dict(input=t["x"].grad, offset=t["off"].grad, weight=t["wgt"].grad,
               mask=t["mask"].grad if modulated else None, bias=t["bias"].grad if modulated else None)
    _compare_gradients(p, got, dtype, kind == "exact" and not half, what)


def check_nhwc_reference_names(device, c, modulated):
    """the reference-named entry points of `_C` on a rectangular shape of the channels-last plan, fp32, exact inputs — v1:
    deform_conv_forward, deform_conv_backward_input, deform_conv_backward_parameters (scale 0.5), which take W-before-H
    arguments; v2: modulated_deform_conv_forward / _backward, H-before-W — with the reference's ownership rules as in
    torch_refs.check_dcn_reference_names_in_plan: gradInput / gradWeight / grad_bias are accumulated into (pre-filled with
    ones), gradOffset / grad_mask overwritten in full (pre-filled with NaN).  Everything bit-equal to the oracle; a swapped
    H / W pair changes the output shape or the values."""
    from maskrcnn_benchmark import _C
    p = problem(c, modulated)
    t = _tensors(p, device, torch.float32)
    x, off, w, go = t["x"], t["off"], t["wgt"], t["go"]
    e = x.new_empty(0)
    out = torch.full((c.B, c.Cout) + out_hw(c), float("nan"), device=device)
    gi, gw, gb = torch.ones_like(x), torch.ones_like(w), torch.ones(c.Cout, device=device)
    goff, gm = torch.full_like(off, float("nan")), None
    v1 = (c.kw, c.kh, c.stride[1], c.stride[0], c.pad[1], c.pad[0], c.dil[1], c.dil[0], 1, c.dg)
    v2 = (c.kh, c.kw, c.stride[0], c.stride[1], c.pad[0], c.pad[1], c.dil[0], c.dil[1], 1, c.dg)
    with launches() as fwd_calls:
        if modulated:
            _C.modulated_deform_conv_forward(x, w, t["bias"], e, off, t["mask"], out, e, *v2, True)
        else:
            assert _C.deform_conv_forward(x, w, off, out, e, e, *v1, c.B) == 1
    assert _dcn(fwd_calls) == {"dcn_to_nhwc": 1, "dcn_im2col_nhwc": 1}, fwd_calls
    with launches() as calls:
        if modulated:
            gm = torch.full_like(t["mask"], float("nan"))
            _C.modulated_deform_conv_backward(x, w, t["bias"], e, off, t["mask"], e, gi, gw, gb, goff, gm, go, *v2, True)
        else:
            assert _C.deform_conv_backward_input(x, off, go, gi, goff, w, e, *v1, c.B) == 1
            assert _C.deform_conv_backward_parameters(x, off, go, gw, e, e, *v1, 0.5, c.B) == 1
    # v1 asks in two calls, each of which transposes the input and the output gradient again
    assert _dcn(calls) == {"dcn_to_nhwc": 2 if modulated else 4, "dcn_coord_nhwc": 1, "dcn_col2im_nhwc": 1, "dcn_im2col_nhwc": 1}, calls
    what = "%s %s" % (c.name, "v2" if modulated else "v1")
    one, f32 = np.float32(1.0), torch.float32
    r = p.backward
    _bit_equal(out, p.forward, f32, what + " output")
    _bit_equal(gi, one + r["input"], f32, what + " gradInput")
    _bit_equal(goff, r["offset"], f32, what + " gradOffset")
    _bit_equal(gw, one + np.float32(1.0 if modulated else 0.5) * r["weight"], f32, what + " gradWeight")
    if modulated:
        _bit_equal(gm, r["mask"], f32, what + " grad_mask")
        _bit_equal(gb, one + r["bias"], f32, what + " grad_bias")


def check_overflow(device, c, dtype, landing, input_grad):
    """the overflow list behind both forms of the input gradient (col2im_nhwc_overflow_kernel / sampleT_overflow_kernel:
    hardware atomics, packed pairs in half), v2 layer on `pileup_problem`.  fp32: the input gradient is bit-equal to the
    oracle (atomic adds of exactly representable partial sums are order-free); half: within 2e-2 of its largest reference
    magnitude."""
    from maskrcnn_benchmark import _C
    assert _C.DCN_INPUT_GRAD == input_grad
    p = pileup_problem(c, landing)
    t = _tensors(p, device, dtype, grad=True)
    t["bias"] = None
    with launches() as calls:
        y = _forward(p, t)
        y.backward(t["go"])
    kern = "dcn_transposed_sample" if input_grad == "transposed" else "dcn_col2im_nhwc"
    assert _dcn(calls) == {"dcn_im2col_nhwc": 1, "dcn_coord_nhwc": 1, kern: 1, "dcn_to_nhwc": 2}, calls
    what = "pile-up %s %s" % (c.name, input_grad)
    if dtype == torch.float32:
        _bit_equal(t["x"].grad, p.backward["input"], dtype, what + " input gradient")
    else:
        _near(t["x"].grad, p.backward["input"], HALF_TOL, what + " input gradient")


# ---------------------------------------------------------------------------------------------- reference-layout kernels
def check_ref_layout_rect(device, c, col2im, ell_build):
    """rectangular geometry outside both plans (C = 8, two deformable groups), fp32, exact inputs, with the col2im kernel
    forced (tuning dcn_col2im = 1 gather | 2 scatter | 3 fixed-width index; dcn_ell_build 0 tile-owner | 1 scatter build):
    the v1 layer (tuples) forward + backward, v2 through `_C.modulated_deform_conv_forward` / `_backward` (the v2 layer's API
    is scalar), and `_C.deformable_im2col` / `deformable_col2im` / `deformable_col2im_coord` on their own — all bit-equal to
    the oracle."""
    from maskrcnn_benchmark import _C
    set_tuning(device, "dcn_col2im", col2im)
    set_tuning(device, "dcn_ell_build", ell_build)
    f32 = torch.float32
    # v1 through the layer
    p = problem(c, False)
    t = _tensors(p, device, f32, grad=True)
    with launches() as calls:
        y = _forward(p, t)
        y.backward(t["go"])
    assert _dcn(calls) == {"dcn_im2col": 2, "dcn_col2im_coord": 1, "dcn_col2im": 1}, calls
    _bit_equal(y, p.forward, f32, c.name + " v1 output")
    _compare_gradients(p, dict(input=t["x"].grad, offset=t["off"].grad, weight=t["wgt"].grad), f32, True, c.name + " v1")
    # v2 through the reference-named entry points (H-before-W)
    p = problem(c, True)
    t = _tensors(p, device, f32)
    x, off, m, w, go = t["x"], t["off"], t["mask"], t["wgt"], t["go"]
    e = x.new_empty(0)
    with launches() as calls:
        out = _forward(p, t)
        gi, gw, gb = torch.zeros_like(x), torch.zeros_like(w), torch.zeros(c.Cout, device=device)
        goff, gm = torch.full_like(off, float("nan")), torch.full_like(m, float("nan"))
        _C.modulated_deform_conv_backward(x, w, t["bias"], e, off, m, e, gi, gw, gb, goff, gm, go, c.kh, c.kw, c.stride[0], c.stride[1],
                                          c.pad[0], c.pad[1], c.dil[0], c.dil[1], 1, c.dg, True)
    assert _dcn(calls) == {"dcn_im2col": 2, "dcn_col2im_coord": 1, "dcn_col2im": 1}, calls
    _bit_equal(out, p.forward, f32, c.name + " v2 output")
    _compare_gradients(p, dict(input=gi, offset=goff, mask=gm, weight=gw, bias=gb), f32, True, c.name + " v2")
    # the three kernels on their own
    i = p.inp
    geo = (c.kh, c.kw, c.pad[0], c.pad[1], c.stride[0], c.stride[1], c.dil[0], c.dil[1], c.dg)
    ogeo = dict(kh=c.kh, kw=c.kw, pad=c.pad, stride=c.stride, dil=c.dil, dg=c.dg)
    ref_col = oracle.deformable_im2col(i["x"], i["off"], i["mask"], **ogeo)
    _bit_equal(_C.deformable_im2col(x, off, m, *geo), ref_col, f32, c.name + " im2col")
    gcol = np.random.RandomState(9).randint(-2, 3, ref_col.shape).astype(np.float32)
    tg = torch.from_numpy(gcol).to(device)
    gim = torch.ones_like(x)                                   # accumulated into
    _C.deformable_col2im(tg, off, m, gim, *geo)
    _bit_equal(gim, np.float32(1.0) + oracle.deformable_col2im(gcol, i["off"], i["mask"], *i["x"].shape, **ogeo), f32, c.name + " col2im")
    goff, gm = torch.full_like(off, float("nan")), torch.full_like(m, float("nan"))    # overwritten in full
    _C.deformable_col2im_coord(tg, x, off, m, goff, gm, *geo)
    rgoff, rgm = oracle.deformable_col2im_coord(gcol, i["x"], i["off"], i["mask"], **ogeo)
    _bit_equal(goff, rgoff, f32, c.name + " col2im_coord offset")
    _bit_equal(gm, rgm, f32, c.name + " col2im_coord mask")


# ---------------------------------------------------------------------------------------------- 16-bit atomics (scatter, overflow list)
# An odd plane (35 elements: channel planes start on both halves of a dword), two deformable groups.  HALF_ATOMIC_TALL is the
# same map three tiles high (plane of 147): col2im_tile_kernel's LDS window of the first 8-row tile ends at input row 13, so
# taps of output row 7 displaced by 6 rows land in the map but outside the window and take that kernel's DIRECT global
# atomics; at 5 x 7 the window covers the whole map and every add reaches the 16-bit atomic through the window's flush.
HALF_ATOMIC = _c("half-atomic-5x7", 1, 4, 5, 7, 4, 3, 1, 1, 1, 2)
HALF_ATOMIC_TALL = _c("half-atomic-21x7", 1, 4, 21, 7, 4, 3, 1, 1, 1, 2)
HALF_ATOMIC_PILE = 10                 # sampling points of one tap steered onto one pixel (against the index's 8 slots)
HALF_ATOMIC_BOUND = 32.0              # 256 quanta of 1/8: every partial sum below it is a bf16 (and fp16) number


def _half_atomic_draw(c, seed):
    """offsets in multiples of 1/2 (bilinear weights in multiples of 1/4), mask in {0.5, 1}, integer column gradient in
    [-2, 2]: every product is a multiple of 1/8.  Most offsets stay within the scatter's 4-pixel halo; one output row of
    group 1 is displaced by 6 (along the axis on which part of it stays inside the map); about 4 % of the pairs point
    outside the map; HALF_ATOMIC_PILE points of the centre tap of group 0 are steered exactly onto pixel (2, 3), where
    each has weight 1."""
    rng = np.random.RandomState(seed)
    Ho, Wo = out_hw(c)
    K = c.kh * c.kw
    off = rng.randint(-8, 9, (c.B, c.dg, K, 2, Ho, Wo)) / 2.0
    far = rng.rand(c.B, c.dg, K, 1, Ho, Wo) < 0.04
    off = np.where(far, off + 12.0, off)
    if c.H > 8:
        off[:, 1, :, 0, 7, :] = 6.0                              # output row 7, 6 rows down: input rows 12 .. 14 of the tall map
    else:
        off[:, 1, :, 1, 2, :] = 6.0                              # output row 2, 6 columns right: columns 5 and 6, the rest outside
    tap = (c.kh // 2) * c.kw + c.kw // 2
    for n in range(HALF_ATOMIC_PILE):
        ho, wo = divmod(n * 3 % (Ho * Wo), Wo)
        off[0, 0, tap, 0, ho, wo] = 2 - ho                       # centre tap, pad 1, stride 1: samples (ho + off_h, wo + off_w)
        off[0, 0, tap, 1, ho, wo] = 3 - wo
    f = np.float32
    return dict(off=off.reshape(c.B, c.dg * 2 * K, Ho, Wo).astype(f),
                mask=rng.choice([0.5, 1.0], (c.B, c.dg * K, Ho, Wo)).astype(f),
                gcol=rng.randint(-2, 3, (c.C * K, c.B * Ho * Wo)).astype(f))


def half_atomic_problem(c):
    """-> (inputs, oracle's fp32 result of 1 + col2im).  The result is bit-equal in any summation order and with every add
    rounded to fp16 / bf16 only if every partial sum is exactly representable, so the seed is chosen HERE, on the oracle alone,
    such that 1 + col2im(|gcol|) stays below HALF_ATOMIC_BOUND for every element — a condition on the inputs, not a
    tolerance — and (5 x 7) such that the pile-up is there: the centre tap's weights on pixel (2, 3) of group 0 sum to more
    than 8 and no weight exceeds 1, so more than 8 sampling points of that (pixel, tap) contribute."""
    key = (c, "half-atomic")
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    ogeo = dict(kh=c.kh, kw=c.kw, pad=c.pad, stride=c.stride, dil=c.dil, dg=c.dg)
    shape = (c.B, c.C, c.H, c.W)
    K = c.kh * c.kw
    for seed in range(200):
        d = _half_atomic_draw(c, 4000 + seed)
        worst = 1.0 + oracle.deformable_col2im(np.abs(d["gcol"]), d["off"], d["mask"], *shape, **ogeo)
        if float(worst.max()) < HALF_ATOMIC_BOUND:
            break
    assert float(worst.max()) < HALF_ATOMIC_BOUND and float(worst.min()) >= 1.0, (c.name, float(worst.max()))
    onehot = np.zeros_like(d["gcol"])
    onehot[(c.kh // 2) * c.kw + c.kw // 2] = 1.0                   # channel 0 (group 0), centre tap
    hits = oracle.deformable_col2im(onehot, d["off"], None, *shape, **ogeo)
    assert float(hits[0, 0, 2, 3]) > 8.0, (c.name, float(hits[0, 0, 2, 3]))
    want = np.float32(1.0) + oracle.deformable_col2im(d["gcol"], d["off"], d["mask"], *shape, **ogeo)
    for a in list(d.values()) + [want]:
        a.setflags(write=False)
    _PROBLEMS[key] = (d, want)
    return _PROBLEMS[key]


def check_half_atomic_col2im(device, c, dtype, col2im, ell_build=0):
    """`_C.deformable_col2im` (v2) in fp16 / bf16 on `half_atomic_problem`, accumulated into a map pre-filled with 1, with the
    kernel forced: dcn_col2im = 2, the scatter (col2im_tile_kernel: 16-bit compare-and-swap adds from the window's flush and,
    on the tall map, from the direct branch); dcn_col2im = 3, the fixed-width index, whose (pixel, tap) with more than 8
    contributions goes through col2im_ell_overflow_kernel's 16-bit adds, under both index builds.  Bit-equal to the oracle's
    fp32 result cast to the storage type."""
    from maskrcnn_benchmark import _C
    d, want = half_atomic_problem(c)
    set_tuning(device, "dcn_col2im", col2im)
    set_tuning(device, "dcn_ell_build", ell_build)
    t = {k: torch.from_numpy(np.array(a)).to(device=device, dtype=dtype) for k, a in d.items()}
    gim = torch.ones((c.B, c.C, c.H, c.W), device=device, dtype=dtype)
    with launches() as calls:
        _C.deformable_col2im(t["gcol"], t["off"], t["mask"], gim, c.kh, c.kw, c.pad[0], c.pad[1], c.stride[0], c.stride[1],
                             c.dil[0], c.dil[1], c.dg)
    assert _dcn(calls) == {"dcn_col2im": 1}, calls
    _bit_equal(gim, want, dtype, "%s col2im (dcn_col2im = %d, dcn_ell_build = %d)" % (c.name, col2im, ell_build))


# ---------------------------------------------------------------------------------------------- layout transposition, ragged tiles
def check_to_nhwc_tails(device, dtype):
    """`_C._to_nhwc` (nchw_to_nhwc_kernel) on [2, 33, 5, 13]: one channel past a 32-channel block, one pixel past a 64-pixel
    block (H * W = 65) — a copy: equal to the permuted input exactly.  (The same tile copy inside dcn_fused_prep_kernel is
    held bit-equal at ragged pixel tiles by FUSED_CASES: 9 x 11 = 99 pixels and 7 x 9 = 63; its channel count is always a
    multiple of 32.)"""
    from maskrcnn_benchmark import _C
    x = torch.from_numpy(np.random.RandomState(11).randint(-1000, 1000, (2, 33, 5, 13)).astype(np.float32)).to(device=device, dtype=dtype)
    with launches() as calls:
        y = _C._to_nhwc(x)
    assert _dcn(calls) == {"dcn_to_nhwc": 1}, calls
    assert y.shape == (2, 65, 33) and y.dtype == dtype
    assert torch.equal(y.cpu(), x.permute(0, 2, 3, 1).reshape(2, 65, 33).cpu())
