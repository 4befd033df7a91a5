"""Edge cases of csrc/roi_pool.hip, csrc/deform_pool.hip and csrc/f64_ops.hip — shared by tests/test_pool_edges_emu.py (host
emulation: proves the oracle against independent references first) and tests/test_pool_edges_gpu.py (the device).

A plain module: no tests, no fixtures.  Three parts:

  * case builders (numpy only, seeded, cached: treat what they return as read-only), one family per operator.  Every builder
    asserts that its inputs really reach the branch it is named after, in the float arithmetic of the kernel where a
    comparison decides it, so a case cannot silently stop proving anything;
  * `*_expected`: the oracle's answer for a case, computed once per process;
  * `check_*`: one case through an `Ops` — the product's `maskrcnn_benchmark._C` wrappers (and, where a flag is not reachable
    from `_C`, the C ABI underneath them) on tensors of one device.  Under `cpu_shim.install("emu-lib")` that is the host
    emulation of the same HIP sources with CPU tensors; on "cuda" it is the device library.  The assertions are the same.

Every shape is the smallest that reaches its branch.  Constants of the kernels the shapes depend on: roi_pool.hip kBlock =
256 ROIs per owner round, kMaxBinsAxis = 64, kOwnerMaxLds = 144 KiB (192 x 192 floats), channel chunks of 16 at these sizes;
deform_pool.hip kMaxSamples = 2048, 1024 bins per table, kMaxPart = 1024 offset cells in LDS, kWin = 4."""
import functools
import importlib.util
import os
import zlib

import numpy as np

import oracle

FLT_MAX = np.float32(np.finfo(np.float32).max)
EINVAL, EUNSUPPORTED = -1, -3          # include/detops.h


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    """same dtype, shape and bit pattern: +0.0 differs from -0.0, a NaN equals the same NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


# ====================================================================================================== ROIPool, fp32
ROI_POOL_CASES = ("ties", "windows", "non_finite", "no_table", "owner_rounds", "plane_1x1", "plane_100x168", "plane_192x192",
                  "plane_192x193")
# planes run with roi_bwd_impl = 1: the form that must serve them (kOwnerMaxLds = 144 KiB = 192 x 192 floats)
PLANE_FORM = {"plane_1x1": "owner", "plane_100x168": "owner", "plane_192x192": "owner", "plane_192x193": "scatter"}


def pool_windows(rois, scale, PH, PW, H, W):
    """the integer windows of ROIPool in float32, as the operator defines them -> (hs, he [K, PH], ws, we [K, PW])"""
    f32 = np.float32
    r = rois[:, 1:].astype(f32) * f32(scale)
    r = (np.sign(r) * np.floor(np.abs(r) + f32(0.5))).astype(np.int64)          # roundf: half away from zero
    x1, y1, x2, y2 = r.T
    rw, rh = np.maximum(x2 - x1 + 1, 1), np.maximum(y2 - y1 + 1, 1)
    bh, bw = rh.astype(f32) / f32(PH), rw.astype(f32) / f32(PW)
    ph, pw = np.arange(PH, dtype=f32), np.arange(PW, dtype=f32)
    hs = np.clip(np.floor(ph[None] * bh[:, None]).astype(np.int64) + y1[:, None], 0, H)
    he = np.clip(np.ceil((ph[None] + 1) * bh[:, None]).astype(np.int64) + y1[:, None], 0, H)
    ws = np.clip(np.floor(pw[None] * bw[:, None]).astype(np.int64) + x1[:, None], 0, W)
    we = np.clip(np.ceil((pw[None] + 1) * bw[:, None]).astype(np.int64) + x1[:, None], 0, W)
    return hs, he, ws, we


def _random_rois(rng, K, N, H, W, scale, spill=2.0):
    """image-space ROIs over an H x W map at `scale`, some spilling over the border by up to `spill` map pixels"""
    x1 = rng.uniform(-spill, W - 1, K)
    y1 = rng.uniform(-spill, H - 1, K)
    x2 = x1 + rng.uniform(0, W * 0.8, K)
    y2 = y1 + rng.uniform(0, H * 0.8, K)
    b = rng.randint(0, N, K)
    return np.stack([b, x1 / scale, y1 / scale, x2 / scale, y2 / scale], 1).astype(np.float32)


def _tie_fraction(x, rois, scale, PH, PW):
    """fraction of the non-empty (ROI, channel, bin) windows whose maximum occurs more than once"""
    N, C, H, W = x.shape
    hs, he, ws, we = pool_windows(rois, scale, PH, PW, H, W)
    tied = total = 0
    for k in range(rois.shape[0]):
        b = int(rois[k, 0])
        for ph in range(PH):
            for pw in range(PW):
                win = x[b, :, hs[k, ph]:he[k, ph], ws[k, pw]:we[k, pw]].reshape(C, -1)
                if win.shape[1] == 0:
                    continue
                total += C
                tied += int(((win == win.max(1, keepdims=True)).sum(1) > 1).sum())
    return tied / max(total, 1)


@functools.lru_cache(maxsize=None)
def roi_pool_case(name):
    """-> dict(x [N, C, H, W], rois [K, 5], scale, pools ((PH, PW), ...), desc)"""
    rng = np.random.RandomState(_seed("roi_pool/" + name))
    if name == "ties":
        N, C, H, W, K, scale = 2, 20, 13, 17, 40, 0.5
        x = np.maximum(np.round(rng.randn(N, C, H, W) * 1.5), 0).astype(np.float32)      # a ReLU feature map: half zeros
        rois = _random_rois(rng, K, N, H, W, scale)
        pools = ((7, 7), (3, 5))
        assert (x == 0).mean() >= 0.4
        for PH, PW in pools:
            assert _tie_fraction(x, rois, scale, PH, PW) >= 0.25
        desc = "integer ReLU map, tied maxima in most windows; C = 20: one full and one ragged channel chunk of 16"
    elif name == "windows":
        N, C, H, W, scale = 1, 2, 6, 8, 0.5
        x = rng.randn(N, C, H, W).astype(np.float32)
        rois = np.array([[0, -20, -20, -10, -10],      # wholly left of / above the map
                         [0, 40, 40, 50, 50],          # wholly right of / below
                         [0, 10, 4, 4, 8],             # x2 < x1: width clamps to 1
                         [0, -8, -8, 40, 40],          # larger than the map
                         [0, 6, 4, 6, 4],              # one pixel pooled 7 x 7: 49 bins share pixel (2, 3)
                         [0, 3, 5, 9, 7],              # coord * scale = 1.5, 2.5, 4.5, 3.5 -> 2, 3, 5, 4
                         [0, -1, -1, 5, 5]],           # -0.5 -> -1 (half away from zero), 2.5 -> 3
                        np.float32)
        pools = ((7, 7),)
        half = rois[5:, 1:] * np.float32(scale)
        assert (np.abs(half - np.trunc(half)) == 0.5).all() and (half == -0.5).any()
        desc = "one ROI per window kind: outside, inverted, oversized, one pixel under 49 bins, half-integer corners"
    elif name == "non_finite":
        N, C, H, W, scale = 1, 3, 6, 8, 1.0
        x = rng.randn(N, C, H, W).astype(np.float32)
        x[0, 0] = -np.inf                              # every window of channel 0 holds only -inf
        x[0, 1, ::2, ::2] = np.nan                     # every 2 x 2 or larger window of channel 1: NaN first, finite values too
        x[0, 2, 1::2, 1::2] = np.nan
        x[0, 2, 2, 2] = x[0, 2, 4, 6] = np.inf
        rois = np.array([[0, 0, 0, 7, 5], [0, 0, 0, 3, 3], [0, 2, 2, 7, 5], [0, 2, 2, 2, 2]], np.float32)
        pools = ((2, 2), (1, 1))
        desc = "a plane of -inf, windows that start with a NaN, +inf among NaNs"
    elif name == "no_table":
        N, C, H, W, scale = 1, 3, 9, 11, 1.0
        x = rng.randn(N, C, H, W).astype(np.float32)
        rois = _random_rois(rng, 5, N, H, W, scale)
        pools = ((65, 2), (3, 70))
        desc = "PH or PW above kMaxBinsAxis = 64: windows computed per element, no LDS table"
    elif name == "owner_rounds":
        N, C, H, W, scale = 3, 4, 7, 9, 1.0
        x = rng.randn(N, C, H, W).astype(np.float32)
        rois = _random_rois(rng, 513, N, H, W, scale)
        rois[:, 0] = rng.permutation(np.repeat([0, 2], [256, 257]))      # image 1 has no ROI; indices unsorted
        pools = ((2, 2),)
        assert (np.bincount(rois[:, 0].astype(int), minlength=3) == [256, 0, 257]).all() and (np.diff(rois[:, 0]) < 0).any()
        desc = "K = 513 > 2 x kBlock: three rounds of the owner kernel's ROI list; an image without ROIs"
    elif name.startswith("plane_"):
        H, W = (int(v) for v in name[len("plane_"):].split("x"))
        N, C, scale = 1, 2, 1.0
        x = rng.randn(N, C, H, W).astype(np.float32)
        rois = _random_rois(rng, 32, N, H, W, scale)
        pools = ((7, 7),)
        desc = "%d bytes per plane against kOwnerMaxLds = %d" % (4 * H * W, 144 * 1024)
    else:
        raise KeyError(name)
    return _ro(dict(x=x, rois=rois, scale=scale, pools=pools, desc=desc))


@functools.lru_cache(maxsize=None)
def roi_pool_expected(name):
    """per pool size: dict(out, amax, g, gin) from the oracle; g holds integers in [-4, 4], so every partial sum of the
    backward is exact in fp32 in any order"""
    c = roi_pool_case(name)
    rng = np.random.RandomState(_seed("roi_pool_grad/" + name))
    res = []
    for PH, PW in c["pools"]:
        out, amax = oracle.roi_pool_forward(c["x"], c["rois"], c["scale"], PH, PW)
        g = rng.randint(-4, 5, out.shape).astype(np.float32)
        gin = oracle.roi_pool_backward(g, c["rois"], amax, *c["x"].shape)
        res.append(_ro(dict(out=out, amax=amax, g=g, gin=gin)))
    return tuple(res)


def roi_pool_case_properties(name):
    """what a case must show in its expected result, whoever computed it"""
    c, exp = roi_pool_case(name), roi_pool_expected(name)
    x = c["x"]
    for (PH, PW), e in zip(c["pools"], exp):
        out, amax, gin = e["out"], e["amax"], e["gin"]
        empty = amax == -1
        if name == "windows":
            assert empty[:2].all() and not bits(out[:2]).any()                       # outside: -1 and +0.0
            assert empty[3].any() and not empty[3].all()                             # oversized: some bins beyond the map
            assert (amax[4] == 2 * x.shape[3] + 3).all()                             # 49 bins on pixel (2, 3) ...
            assert np.array_equal(gin[0, :, 2, 3] - _others(e, x, 4)[:, 2, 3], e["g"][4].sum((1, 2)))   # ... 49 gradients summed
            hs, he, ws, we = pool_windows(c["rois"], c["scale"], PH, PW, *x.shape[2:])
            assert (ws[5, 0], hs[5, 0], we[5, -1], he[5, -1]) == (2, 3, 6, 5) and (ws[6, 0], hs[6, 0], we[6, -1], he[6, -1]) == (0, 0, 4, 4)
        if name == "non_finite":
            assert same_bits(out[:, 0], np.full_like(out[:, 0], -FLT_MAX)) and empty[:, 0].all()
            sel = x[0].reshape(3, -1)
            for ch in (1, 2):
                assert not np.isnan(out[:, ch]).any()
                picked = np.take_along_axis(sel[ch][None], np.maximum(amax[:, ch].reshape(1, -1), 0), 1)
                assert not np.isnan(picked[0][amax[:, ch].reshape(-1) >= 0]).any()
            assert np.isposinf(out[0, 2]).any() and np.isposinf(out[2, 2]).any()
            assert (amax[3, 1] == -1).all() and same_bits(out[3, 1], np.full_like(out[3, 1], -FLT_MAX))   # a window of one NaN
        if name == "owner_rounds":
            assert not bits(gin[1]).any() and gin[0].any() and gin[2].any()


def _others(e, x, k):
    """the oracle's input gradient of every ROI but `k` (image 0)"""
    g = e["g"].copy()
    g[k] = 0
    return oracle.roi_pool_backward(g, roi_pool_case("windows")["rois"], e["amax"], *x.shape)[0]


def roi_pool_base(name, shape):
    """integer-valued content of grad_in for the accumulating call"""
    return np.random.RandomState(_seed("roi_pool_base/" + name)).randint(-8, 9, shape).astype(np.float32)


# ====================================================================================================== deformable PS-ROI pooling
#   name: no_trans, classes, D (output_dim), G (group_size), P, part, S, scale, map (H, W), ROI kind
PSROI_CASES = {
    "big_part": (False, 1, 2, 1, 23, 23, 1, 0.5, (12, 20), "generic"),      # 2 part^2 = 1058 > kMaxPart: global offset atomics
    "many_bins": (False, 1, 1, 1, 33, 3, 1, 0.5, (12, 20), "generic"),      # P P = 1089 > 1024: direct path, samples <= 2048
    "wide_bins": (False, 2, 4, 2, 3, 3, 4, 1.0, (12, 20), "whole"),         # sample spacing > 1 px: private-window fallback
    "sub_pixel": (True, 1, 4, 2, 7, 7, 4, 1.0, (12, 20), "small"),          # a bin's samples inside one pixel
    "g_above_p": (False, 1, 2, 7, 3, 1, 2, 0.5, (12, 20), "generic"),       # gh / gw clamp, part_size = 1
    "cec_1": (False, 4, 4, 1, 4, 8, 2, 0.5, (12, 20), "generic"),           # output_dim == num_classes, part > P
    "thin_h1": (False, 1, 2, 1, 4, 4, 2, 0.5, (1, 20), "generic"),          # H == 1: dy stays 0
    "thin_w1": (False, 1, 2, 1, 4, 4, 2, 0.5, (12, 1), "generic"),          # W == 1: dx stays 0
    "on_centre": (True, 1, 1, 1, 4, 4, 1, 0.5, (12, 20), "centre"),         # samples on pixel centres and on -0.5 / W - 0.5
    "on_centre_zero_offsets": (False, 1, 1, 1, 4, 4, 1, 0.5, (12, 20), "centre"),   # same samples, offset gradient taken there
}
PSROI_K, PSROI_N, TRANS_STD = 24, 3, 0.1
OUTSIDE = 1000.0          # map pixels: the ROI wholly outside


def psroi_cfg(name):
    """the operator's trailing arguments (no_trans, spatial_scale, output_dim, group_size, pooled, part, spp, trans_std)"""
    no_trans, ncls, D, G, P, part, S, scale, _, _ = PSROI_CASES[name]
    return (no_trans, scale, D, G, P, part, S, 0.0 if no_trans else TRANS_STD)


def lattice_f32(roi, scale, P, S, size_axis):
    """sampling coordinates of one axis without offsets, in the float arithmetic of deform_pool.hip make_lattice /
    make_sample: axis 0 -> w over (pw, iw), axis 1 -> h over (ph, ih); [P, S] float32"""
    f32, f64 = np.float32, np.float64
    lo, hi = (roi[1], roi[3]) if size_axis == 0 else (roi[2], roi[4])
    rnd = lambda v: f32(np.sign(v) * np.floor(np.abs(f32(v)) + f32(0.5)))  # noqa: E731
    start = f32(f64(rnd(lo) * f32(scale)) - 0.5)
    end = f32(f64(f32(f64(rnd(hi)) + 1.0) * f32(scale)) - 0.5)
    size = f32(max(f64(end - start), 0.1))
    bin_ = size / f32(P)
    sub = bin_ / f32(S)
    first = np.arange(P, dtype=f32) * bin_ + start
    return (first[:, None] + np.arange(S, dtype=f32)[None, :] * sub).astype(f32)


@functools.lru_cache(maxsize=None)
def psroi_case(name):
    """-> dict(data [N, D G G + 1, H, W], rois [K, 5], trans [K, 2 classes, part, part] or None, outside (ROI index), desc).
    The last input plane belongs to no output channel: its gradient stays zero."""
    no_trans, ncls, D, G, P, part, S, scale, (H, W), kind = PSROI_CASES[name]
    rng = np.random.RandomState(_seed("psroi/" + name))
    K, N = PSROI_K, PSROI_N
    data = rng.randn(N, D * G * G + 1, H, W).astype(np.float32)
    if kind == "generic":
        rois = _random_rois(rng, K, N, H, W, scale)
        rois[:, 3:] += 1.0 / scale
    elif kind == "whole":                                                   # the whole map, give or take a pixel
        j = rng.randint(-1, 2, (K, 4))
        rois = np.concatenate([np.zeros((K, 1)), j + [0, 0, W - 1, H - 1]], 1).astype(np.float32)
    elif kind == "small":                                                   # 2 or 3 map pixels a side
        x1, y1 = rng.randint(0, W - 3, K), rng.randint(0, H - 3, K)
        rois = np.stack([np.zeros(K), x1, y1, x1 + rng.randint(1, 3, K), y1 + rng.randint(1, 3, K)], 1).astype(np.float32)
    else:                                                                   # "centre": bins of exactly 1 or 2 map pixels at scale 0.5
        xs = [(1, 8), (0, 7), (34, 41), (5, 20), (35, 42)]                  # start 0 | -0.5 | 16.5 (last sample W - 0.5) | 2, bins of 2 | 17 (last sample beyond)
        ys = [(1, 8), (0, 7), (18, 25), (3, 10), (19, 26)]                  # start 0 | -0.5 | 8.5 (last sample H - 0.5) | 1 | 9 (last sample beyond)
        rois = np.array([[0, x[0], y[0], x[1], y[1]] for y in ys for x in xs][:K], np.float32)
    rois[:, 0] = rng.randint(0, N, K)
    rois[:N, 0] = np.arange(N)[::-1]                                        # every image is used; indices unsorted
    outside = K - 1
    rois[outside, 1:] = np.array([OUTSIDE, OUTSIDE, OUTSIDE + 6, OUTSIDE + 4]) / scale
    if no_trans:
        trans = None
    elif name == "on_centre_zero_offsets":
        trans = np.zeros((K, 2 * ncls, part, part), np.float32)
    else:
        trans = (rng.randn(K, 2 * ncls, part, part) * 1.5).astype(np.float32)

    # the branch each case is named after (constants of deform_pool.hip)
    table = P * P * S * S <= 2048 and P * P <= 1024
    lds_offsets = 2 * part * part <= 1024
    if name == "big_part":
        assert table and not lds_offsets
    elif name == "many_bins":
        assert not table and P * P > 1024 and P * P * S * S <= 2048
    else:
        assert table and lds_offsets
    width = np.array([float(lattice_f32(r, scale, P, S, 0)[0, 1] - lattice_f32(r, scale, P, S, 0)[0, 0]) if S > 1 else 0.0
                      for r in rois[:outside]])
    if name == "wide_bins":
        assert (width > 1.0).all() and (width * (S - 1) > 4).all()         # a bin's samples span more than kWin = 4 pixels
    if name == "sub_pixel":
        assert (width * S < 0.5).all()
    if name == "g_above_p":
        assert G > P and part == 1
    if name == "cec_1":
        assert D == ncls and part > P
    if kind == "centre":
        w = np.concatenate([lattice_f32(r, scale, P, S, 0).ravel() for r in rois[:outside]])
        h = np.concatenate([lattice_f32(r, scale, P, S, 1).ravel() for r in rois[:outside]])
        for v, size in ((w, W), (h, H)):
            inside = (v >= -0.5) & (v <= size - 0.5)
            assert ((v == np.floor(v)) & inside).sum() > 20                 # dist == 0: ceil == floor
            assert (v == -0.5).any() and (v == size - 0.5).any() and (~inside).any()
    return _ro(dict(data=data, rois=rois, trans=trans, outside=outside, desc=name))


@functools.lru_cache(maxsize=None)
def psroi_expected(name):
    """dict(out, cnt, g, gin, gtr) from the oracle; gradients accumulated in fp64 (acc64)"""
    c, cfg = psroi_case(name), psroi_cfg(name)
    out, cnt = oracle.deform_psroi_pool_forward(c["data"], c["rois"], c["trans"], *cfg)
    g = np.random.RandomState(_seed("psroi_grad/" + name)).randn(*out.shape).astype(np.float32)
    gin, gtr = oracle.deform_psroi_pool_backward(g, c["data"], c["rois"], c["trans"], cnt, *cfg, acc64=True)
    e = dict(out=out, cnt=cnt, g=g, gin=gin, gtr=gtr)
    o = c["outside"]
    S = cfg[6]
    assert not cnt[o].any() and not bits(out[o]).any() and (cnt[:o] == S * S).any()
    assert not gin[:, -1].any() and (gtr is None or not gtr[o].any())
    return _ro(e)


# ====================================================================================================== ROIAlign, fp64
ALIGN64_CFGS = ((3, 2, 0), (1, 1, 0), (1, 1, 1), (2, 3, 2))          # (PH, PW, sampling_ratio); 0: adaptive grid


@functools.lru_cache(maxsize=None)
def align64_case():
    """-> dict(x [2, 3, 9, 11] float64, rois [K, 5] float64, scale): ROIs partly and wholly outside, narrower than a pixel,
    and with samples exactly on the inclusive limits -1 and `size` (PH = PW = 1, one sample per bin)"""
    rng = np.random.RandomState(_seed("align64"))
    N, C, H, W, scale = 2, 3, 9, 11, 0.5
    x = rng.randn(N, C, H, W)
    rois = _random_rois(rng, 6, N, H, W, scale, spill=4.0).astype(np.float64)
    rois = np.concatenate([rois, np.array([[0, -9, -7, 5, 6],              # partly outside, top left
                                           [1, 15, 11, 30, 25],            # partly outside, bottom right
                                           [0, 100, 100, 120, 120],        # wholly outside
                                           [1, -50, -50, -30, -30],
                                           [1, 6.4, 8.2, 7.2, 8.6],        # 0.4 x 0.2 map pixels
                                           [0, 18, 14, 26, 22],            # centre (22, 18) * 0.5 = (W, H): a sample on `size`
                                           [1, -6, -6, 2, 2]])])           # centre -2 * 0.5 = -1: a sample on -1
    # the two limit ROIs under (1, 1, 1): one sample at start + bin / 2
    for r, want in ((rois[-2], (W, H)), (rois[-1], (-1.0, -1.0))):
        cx, cy = r[1] * scale + (r[3] - r[1]) * scale / 2, r[2] * scale + (r[4] - r[2]) * scale / 2
        assert (cx, cy) == want
    return _ro(dict(x=x, rois=rois, scale=scale))


@functools.lru_cache(maxsize=None)
def align_containment_case():
    """-> dict(x [2, 2, 8, 8] float64 with row 0 and column 0 of every plane +inf, clean (those pixels 0), rois, scale, cfgs).
    Every ROI reaches past the far edge, so some samples lie beyond `size` and count for nothing; the samples in range stay
    at coordinates >= 1 and so read neither row 0 nor column 0."""
    rng = np.random.RandomState(_seed("align_containment"))
    N, C, H, W, scale = 2, 2, 8, 8, 1.0
    clean = rng.randn(N, C, H, W)
    clean[:, :, 0, :] = 0
    clean[:, :, :, 0] = 0
    x = clean.copy()
    x[:, :, 0, :] = np.inf
    x[:, :, :, 0] = np.inf
    rois = np.array([[0, 2, 2, 14, 14], [1, 1.25, 3.5, 12, 9.75], [1, 5, 1, 21, 13], [0, 3, 6.5, 9, 30]], np.float64)
    cfgs = ((2, 2, 2), (3, 2, 0), (1, 1, 3), (7, 7, 2))      # the last: the fixed-grid fast path of the fp32 forward
    for PH, PW, sr in cfgs:
        beyond = 0
        for r in rois:
            for start, end, P, size in ((r[1], r[3], PW, W), (r[2], r[4], PH, H)):
                s, length = start * scale, max((end - start) * scale, 1.0)
                grid = sr if sr > 0 else int(np.ceil(length / P))
                c = s + (np.arange(P * grid) + 0.5) * (length / P / grid)
                assert (c >= 1.0).all()
                beyond += int((c > size).sum())
        assert beyond > 0
    return _ro(dict(x=x, clean=clean, rois=rois, scale=scale, cfgs=cfgs))


# ====================================================================================================== focal loss, fp64
def _focal_formula():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden_focal_formula.py")
    spec = importlib.util.spec_from_file_location("make_golden_focal_formula", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


FOCAL_CASES = tuple((C, gamma) for C in (1, 7) for gamma in (0.0, 2.0))
FOCAL_ALPHA = 0.25


@functools.lru_cache(maxsize=None)
def focal_case(C, gamma):
    """logits in {-100, -20, 0, 20, 100} in every column against targets -1 (ignored), 0 (background), 1 and C; the fp64
    formula of tests/golden/make_golden_focal_formula.py is the reference -> dict(logits, targets, d, loss, grad)"""
    vals = np.array([-100.0, -20.0, 0.0, 20.0, 100.0])
    tg = np.array([-1, 0, 1, C], np.int32)
    R = len(vals) * len(tg)
    logits = np.stack([np.roll(vals, j)[np.arange(R) % 5] for j in range(C)], 1)
    targets = np.repeat(tg, 5).astype(np.int32)
    d = np.random.RandomState(_seed("focal")).rand(R, C) + 0.5
    f = _focal_formula()
    return _ro(dict(logits=logits, targets=targets, d=d, loss=f.forward(logits, targets, gamma, FOCAL_ALPHA),
                    grad=f.backward(logits, targets, d, gamma, FOCAL_ALPHA)))


# ====================================================================================================== NMS, fp64
def nms_greedy(boxes, scores, thr, dtype=np.float64):
    """greedy NMS from its definition in `dtype` arithmetic: by descending score (ties: lower index first), a box is dropped
    when its IoU (the +1 pixel convention) with a kept box is >= thr -> ascending kept indices"""
    b = np.asarray(boxes).astype(dtype)
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    kept = []
    for i in np.argsort(-np.asarray(scores, np.float64), kind="stable"):
        for j in kept:
            w = max(dtype(0), min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]) + 1)
            h = max(dtype(0), min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]) + 1)
            if w * h / (area[i] + area[j] - w * h) >= dtype(np.float32(thr)):
                break
        else:
            kept.append(int(i))
    return np.sort(np.asarray(kept, np.int64))


NMS64_CASES = ("chain_1", "chain_2", "chain_63", "chain_64", "chain_65", "chain_129", "iou_equals_threshold",
               "iou_below_threshold", "equal_scores", "below_fp32_resolution")


@functools.lru_cache(maxsize=None)
def nms64_case(name):
    """-> dict(boxes [n, 4] float64, scores [n] float64, thr, keep)"""
    if name.startswith("chain_"):
        # box 0 alone; boxes 1.. each overlap the next with IoU = 40 / 160 = 0.25 = thr exactly and the one after not at all:
        # 1, 3, 5, ... are kept, 63 suppresses 64 and 127 suppresses 128 across a 64-bit word of the mask
        n, thr = int(name[6:]), 0.25
        i = np.arange(n, dtype=np.float64)
        boxes = np.stack([i * 6, np.zeros(n), i * 6 + 9, np.full(n, 9.0)], 1)
        boxes[0] = [-100, -100, -91, -91]
        scores = 1.0 - i / 256
        keep = nms_greedy(boxes, scores, thr)
        assert np.array_equal(keep, np.array([0] + list(range(1, n, 2)), np.int64))
    elif name in ("iou_equals_threshold", "iou_below_threshold"):
        boxes = np.array([[0, 0, 9, 9], [0, 0, 9, 4]], np.float64)         # 50 / 100: dyadic, IoU = 0.5 exactly
        scores = np.array([0.9, 0.8])
        thr = 0.5 if name == "iou_equals_threshold" else 0.5000001
        keep = nms_greedy(boxes, scores, thr)
        assert list(keep) == ([0] if name == "iou_equals_threshold" else [0, 1])
    elif name == "equal_scores":
        boxes = np.array([[0, 0, 10, 10]] * 3 + [[50, 50, 60, 60]] * 2 + [[0, 0, 10, 10]], np.float64)
        scores = np.full(6, 0.5)
        thr = 0.5
        keep = nms_greedy(boxes, scores, thr)
        assert list(keep) == [0, 3]
    elif name == "below_fp32_resolution":
        # pairs at offset 2^26 (fp32 spacing 8) shifted by 0.5: IoU = 76.5 / 85.5 = 0.895 in double, identical boxes in float
        T, thr = float(2 ** 26), 0.95
        boxes = np.array([[T, 0, T + 8, 8], [T + 0.5, 0, T + 8.5, 8], [T, 64, T + 8, 72], [T, 64.5, T + 8, 72.5],
                          [T + 64, 0, T + 72, 8], [T + 64, 0, T + 72, 8]], np.float64)
        scores = np.linspace(0.9, 0.4, 6)
        keep = nms_greedy(boxes, scores, thr)
        assert list(keep) == [0, 1, 2, 3, 4]
        assert np.array_equal(boxes.astype(np.float32)[0], boxes.astype(np.float32)[1])
        assert list(nms_greedy(boxes, scores, thr, np.float32)) == [0, 2, 3, 4]      # fp32 cannot tell the first pair apart
    else:
        raise KeyError(name)
    return _ro(dict(boxes=boxes, scores=scores, thr=thr, keep=keep))


# ====================================================================================================== the code under test
class Ops(object):
    """numpy in, numpy out, through `maskrcnn_benchmark._C` on tensors of `device` (and `_C.lib`, the C ABI, where a flag
    has no `_C` spelling).  Outputs the library must write in full are pre-filled with NaN / -7."""

    def __init__(self, device):
        import torch
        from maskrcnn_benchmark import _C
        self.torch, self.C, self.device = torch, _C, device

    def t(self, a, dtype=None):
        if a is None:
            return None
        t = self.torch.from_numpy(np.array(a, order="C"))        # a copy: the cached cases are read-only
        return (t if dtype is None else t.to(dtype)).to(self.device)

    @staticmethod
    def n(t):
        return t.detach().cpu().numpy()

    def tune(self, key, value):
        rc = self.C.lib.detops_tuning_set(key.encode(), int(value))
        assert rc == 0, (key, rc)

    # ---- ROIPool
    def roi_pool_forward(self, x, rois, scale, PH, PW):
        out, amax = self.C.roi_pool_forward(self.t(x), self.t(rois), scale, PH, PW)
        return self.n(out), self.n(amax)

    def roi_pool_backward(self, g, rois, amax, shape, PH, PW, impl=0):
        self.tune("roi_bwd_impl", impl)
        try:
            return self.n(self.C.roi_pool_backward(self.t(g), None, self.t(rois), self.t(amax), 0.0, PH, PW, *shape))
        finally:
            self.tune("roi_bwd_impl", 0)

    def roi_pool_backward_into(self, g, rois, amax, base, impl):
        """detops_roi_pool_backward_f32 with zero_grad_in = 0 onto a copy of `base`"""
        C = self.C
        tg, tr, ta, gin = self.t(g), self.t(rois), self.t(amax), self.t(base.copy())
        K, _, PH, PW = g.shape
        self.tune("roi_bwd_impl", impl)
        try:
            rc = C.lib.detops_roi_pool_backward_f32(C.ptr(tg), C.ptr(tr), C.ptr(ta), C.ptr(gin), *base.shape, K, PH, PW, 0,
                                                    C.stream_of(tg))
        finally:
            self.tune("roi_bwd_impl", 0)
        assert rc == 0, rc
        return self.n(gin)

    # ---- deformable PS-ROI pooling
    def psroi_forward(self, c, cfg):
        D, P = cfg[2], cfg[4]
        K = c["rois"].shape[0]
        out = self.t(np.full((K, D, P, P), np.nan, np.float32))
        cnt = self.t(np.full((K, D, P, P), np.nan, np.float32))
        trans = self.t(np.zeros(0, np.float32) if c["trans"] is None else c["trans"])
        self.C.deform_psroi_pooling_forward(self.t(c["data"]), self.t(c["rois"]), trans, out, cnt, *cfg)
        return self.n(out), self.n(cnt)

    def psroi_backward(self, g, c, cnt, cfg):
        """through `_C`: accumulates into zeroed gradients, as the reference's entry point does"""
        trans = self.t(np.zeros(0, np.float32) if c["trans"] is None else c["trans"])
        gin = self.t(np.zeros_like(c["data"]))
        gtr = self.torch.zeros_like(trans)
        self.C.deform_psroi_pooling_backward(self.t(g), self.t(c["data"]), self.t(c["rois"]), trans, self.t(cnt), gin, gtr, *cfg)
        return self.n(gin), (None if c["trans"] is None else self.n(gtr))

    def psroi_raw(self, c, cfg, ct, g=None, cnt=None, fill=7.0, zero_grads=0, bases=None):
        """the two C entry points themselves -> (rc, first result, second result); results start as `fill` (forward: out,
        top_count; backward, given `g`: data_grad, trans_grad from `bases` or `fill`)"""
        C = self.C
        no_trans, scale, D, G, P, part, S, std = cfg
        data, rois, trans = self.t(c["data"]), self.t(c["rois"]), self.t(c["trans"])
        N, Cc, H, W = c["data"].shape
        K = c["rois"].shape[0]
        tail = (N, Cc, H, W, K, ct, int(no_trans), float(scale), D, G, P, part, S, float(std))
        if g is None:
            a = self.t(np.full((K, D, P, P), fill, np.float32))
            b = self.t(np.full((K, D, P, P), fill, np.float32))
            rc = C.lib.detops_deform_psroi_pool_forward_f32(C.ptr(data), C.ptr(rois), C.ptr(trans), C.ptr(a), C.ptr(b), *tail,
                                                            C.stream_of(data))
        else:
            a = self.t(np.full(c["data"].shape, fill, np.float32) if bases is None else bases[0].copy())
            tshape = (K, max(ct, 2), part, part)
            b = self.t(np.full(tshape, fill, np.float32) if bases is None else bases[1].copy())
            tg, tc = self.t(g), self.t(cnt)
            rc = C.lib.detops_deform_psroi_pool_backward_f32(C.ptr(tg), C.ptr(data), C.ptr(rois), C.ptr(trans), C.ptr(tc), C.ptr(a),
                                                             C.ptr(b), *tail, int(zero_grads), C.stream_of(data))
        return rc, self.n(a), self.n(b)


# ====================================================================================================== checks
def _close(a, b, rtol, atol):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def check_roi_pool(ops, name):
    """forward and argmax bit-equal to the oracle; backward on integer gradients bit-equal to it as the default, the owner
    (roi_bwd_impl = 1) and the scatter form (3)"""
    c = roi_pool_case(name)
    for (PH, PW), e in zip(c["pools"], roi_pool_expected(name)):
        out, amax = ops.roi_pool_forward(c["x"], c["rois"], c["scale"], PH, PW)
        assert amax.dtype == np.int32 and np.array_equal(amax, e["amax"]), (name, PH, PW, np.argwhere(amax != e["amax"])[:5])
        assert same_bits(out, e["out"]), (name, PH, PW, np.argwhere(bits(out) != bits(e["out"]))[:5])
        for impl in (0, 1, 3):
            gin = ops.roi_pool_backward(e["g"], c["rois"], amax, c["x"].shape, PH, PW, impl)
            assert same_bits(gin, e["gin"]), (name, PH, PW, impl, np.argwhere(bits(gin) != bits(e["gin"]))[:5])


def check_roi_pool_accumulate(ops, name="owner_rounds"):
    """zero_grad_in = 0 (C ABI): owner and scatter form add onto what grad_in holds"""
    c = roi_pool_case(name)
    base = roi_pool_base(name, c["x"].shape)
    for e in roi_pool_expected(name):
        want = base + e["gin"]
        for impl in (1, 3):
            got = ops.roi_pool_backward_into(e["g"], c["rois"], e["amax"], base, impl)
            assert same_bits(got, want), (name, impl, np.argwhere(bits(got) != bits(want))[:5])


def roi_pool_form(ops, name):
    """which backward form serves the case under roi_bwd_impl = 1, told from the result alone: accumulating onto a plane of
    -0.0, the owner form writes every pixel (-0.0 + 0.0 = +0.0) while the scatter form leaves the pixels no bin points at
    untouched (-0.0) -> "owner" | "scatter" | None (every pixel is some bin's argmax)"""
    c = roi_pool_case(name)
    e = roi_pool_expected(name)[0]
    N, C, H, W = c["x"].shape
    touched = np.zeros((N, C, H * W), bool)
    for k in range(c["rois"].shape[0]):
        for ch in range(C):
            a = e["amax"][k, ch].ravel()
            touched[int(c["rois"][k, 0]), ch, a[a >= 0]] = True
    untouched = ~touched.reshape(N, C, H, W)
    got = ops.roi_pool_backward_into(e["g"], c["rois"], e["amax"], np.full(c["x"].shape, -0.0, np.float32), 1)
    assert np.array_equal(got, e["gin"])                     # values; the sign of zero is the observation
    if not untouched.any():
        return None
    neg = np.signbit(got[untouched])
    assert neg.all() or not neg.any(), name
    return "scatter" if neg.all() else "owner"


def check_roi_pool_form(ops, name):
    form = roi_pool_form(ops, name)
    if name == "plane_1x1":
        assert form in (None, "owner")                       # its one pixel may be some bin's argmax: nothing to observe
    else:
        assert form == PLANE_FORM[name], (name, form)


def check_psroi(ops, name):
    c, cfg, e = psroi_case(name), psroi_cfg(name), psroi_expected(name)
    o = c["outside"]
    out, cnt = ops.psroi_forward(c, cfg)
    assert same_bits(cnt, e["cnt"]), (name, np.argwhere(cnt != e["cnt"])[:5])
    _close(out, e["out"], 1e-4, 1e-5)
    assert not bits(out[o]).any()                            # the ROI outside the map: count 0, +0.0 ...
    gin, gtr = ops.psroi_backward(e["g"], c, cnt, cfg)
    _close(gin, e["gin"], 1e-4, 1e-4)
    assert not gin[:, -1].any()                              # the plane no output channel reads
    if cfg[0]:
        assert gtr is None
    else:
        _close(gtr, e["gtr"], 1e-3, 1e-3 * max(1.0, float(np.abs(e["gtr"]).max())))
        assert not gtr[o].any()                              # ... and no gradient
        assert np.abs(e["gtr"]).max() > 1e-3                 # the comparison is not against nothing


def check_psroi_accumulate(ops, name="cec_1"):
    """zero_grads = 0 (C ABI): both gradients are added onto non-zero content"""
    c, cfg, e = psroi_case(name), psroi_cfg(name), psroi_expected(name)
    rng = np.random.RandomState(_seed("psroi_base"))
    bases = (rng.randn(*c["data"].shape).astype(np.float32), rng.randn(*c["trans"].shape).astype(np.float32))
    rc, gin, gtr = ops.psroi_raw(c, cfg, c["trans"].shape[1], g=e["g"], cnt=e["cnt"], zero_grads=0, bases=bases)
    assert rc == 0
    _close(gin, bases[0].astype(np.float64) + e["gin"], 1e-4, 1e-4)
    _close(gtr, bases[1].astype(np.float64) + e["gtr"], 1e-3, 1e-3 * max(1.0, float(np.abs(e["gtr"]).max())))
    # zero_grads = 1 on the same content: overwritten
    rc, gin, gtr = ops.psroi_raw(c, cfg, c["trans"].shape[1], g=e["g"], cnt=e["cnt"], zero_grads=1, bases=bases)
    assert rc == 0
    _close(gin, e["gin"], 1e-4, 1e-4)
    _close(gtr, e["gtr"], 1e-3, 1e-3 * max(1.0, float(np.abs(e["gtr"]).max())))


def check_psroi_refusals(ops):
    """the two configurations the library refuses, forward and backward: the code, and nothing written"""
    c = psroi_case("cec_1")                                  # 5 input planes, trans [K, 8, 8, 8]
    K = c["rois"].shape[0]
    g = np.ones((K, 3, 4, 4), np.float32)
    #                     no_trans scale D  G  P  part S  std   channels_trans
    for cfg, ct, want in (((False, 0.5, 3, 1, 4, 8, 2, 0.1), 4, EUNSUPPORTED),       # output_dim % num_classes = 3 % 2
                          ((False, 0.5, 3, 2, 4, 8, 2, 0.1), 6, EINVAL)):            # output_dim G G = 12 > C = 5
        rc, out, cnt = ops.psroi_raw(c, cfg, ct)
        assert rc == want and (out == 7.0).all() and (cnt == 7.0).all(), (cfg, rc)
        rc, gin, gtr = ops.psroi_raw(c, cfg, ct, g=g, cnt=np.ones_like(g))
        assert rc == want and (gin == 7.0).all() and (gtr == 7.0).all(), (cfg, rc)


# ---- fp64 operators
def align64_reference(x, rois, scale, PH, PW, sr, g=None):
    """roi_align_torch in fp64 on the host -> (out, input gradient for `g` or None)"""
    import torch
    from torch_refs import roi_align_torch
    xt = torch.tensor(x).requires_grad_(g is not None)
    out = roi_align_torch(xt, torch.tensor(rois), scale, PH, PW, sr)
    if g is None:
        return out.detach().numpy(), None
    out.backward(torch.tensor(g))
    return out.detach().numpy(), xt.grad.numpy()


@functools.lru_cache(maxsize=None)
def align64_expected(cfg):
    c = align64_case()
    PH, PW, sr = cfg
    g = np.random.RandomState(_seed("align64_grad")).randn(c["rois"].shape[0], c["x"].shape[1], PH, PW)
    out, gin = align64_reference(c["x"], c["rois"], c["scale"], PH, PW, sr, g)
    if cfg == (1, 1, 1):
        assert out[-2].any() and out[-1].any()               # the samples on `size` and on -1 count
    assert not out[8].any() and not out[9].any()             # wholly outside
    return _ro(dict(out=out, g=g, gin=gin))


def check_align64(ops, cfg):
    c, e = align64_case(), align64_expected(cfg)
    PH, PW, sr = cfg
    C = ops.C
    x, r = ops.t(c["x"]), ops.t(c["rois"])
    out = C.roi_align_forward(x, r, c["scale"], PH, PW, sr)
    assert out.dtype == ops.torch.float64
    _close(ops.n(out), e["out"], 1e-12, 1e-12)
    gin = C.roi_align_backward(ops.t(e["g"]), r, c["scale"], PH, PW, *c["x"].shape, sr)
    _close(ops.n(gin), e["gin"], 1e-9, 1e-11)


def check_align_containment_f64(ops):
    c = align_containment_case()
    C = ops.C
    r = ops.t(c["rois"])
    for PH, PW, sr in c["cfgs"]:
        dirty = ops.n(C.roi_align_forward(ops.t(c["x"]), r, c["scale"], PH, PW, sr))
        clean = ops.n(C.roi_align_forward(ops.t(c["clean"]), r, c["scale"], PH, PW, sr))
        assert np.isfinite(dirty).all(), ((PH, PW, sr), "non-finite outputs: %d of %d" % ((~np.isfinite(dirty)).sum(), dirty.size))
        assert same_bits(dirty, clean), (PH, PW, sr)
        _close(clean, align64_reference(c["clean"], c["rois"], c["scale"], PH, PW, sr)[0], 1e-12, 1e-12)


def check_align_containment_f32(ops):
    """the same case through the fp32 forward: the default kernels, the generic gather kernel (roi_fwd_impl = 1) and the
    channels-last entry point"""
    c = align_containment_case()
    C, torch = ops.C, ops.torch
    r = ops.t(c["rois"], torch.float32)
    x, clean = ops.t(c["x"], torch.float32), ops.t(c["clean"], torch.float32)
    for PH, PW, sr in c["cfgs"]:
        want = oracle.roi_align_forward(c["clean"].astype(np.float32), c["rois"].astype(np.float32), c["scale"], PH, PW, sr)
        for impl in (0, 1):
            ops.tune("roi_fwd_impl", impl)
            try:
                dirty, ok = ops.n(C.roi_align_forward(x, r, c["scale"], PH, PW, sr)), ops.n(C.roi_align_forward(clean, r, c["scale"], PH, PW, sr))
            finally:
                ops.tune("roi_fwd_impl", 0)
            assert np.isfinite(dirty).all() and same_bits(dirty, ok), (PH, PW, sr, impl)
            assert np.abs(ok - want).max() <= 1e-4
        xl, cl = (t.contiguous(memory_format=torch.channels_last) for t in (x, clean))
        assert C.is_channels_last(xl)
        dirty = ops.n(C.roi_align_fpn_forward([xl], r, [c["scale"]], PH, PW, sr, 4, 4)[0])
        ok = ops.n(C.roi_align_fpn_forward([cl], r, [c["scale"]], PH, PW, sr, 4, 4)[0])
        assert np.isfinite(dirty).all() and same_bits(dirty, ok), (PH, PW, sr, "channels-last")
        assert np.abs(ok - want).max() <= 1e-4


def check_roi_pool_f64(ops, name):
    """the fp32 cases as double: values and argmax of the fp32 oracle exactly (the inputs are fp32 numbers, and ROI corners
    times the power-of-two scale are exact in both types)"""
    c = roi_pool_case(name)
    C = ops.C
    for (PH, PW), e in zip(c["pools"], roi_pool_expected(name)):
        out, amax = C.roi_pool_forward(ops.t(c["x"].astype(np.float64)), ops.t(c["rois"].astype(np.float64)), c["scale"], PH, PW)
        out, amax = ops.n(out), ops.n(amax)
        assert out.dtype == np.float64 and np.array_equal(amax, e["amax"]), (name, PH, PW)
        assert same_bits(out, e["out"].astype(np.float64)), (name, PH, PW, out[bits(out) != bits(e["out"].astype(np.float64))][:5])


def check_roi_pool_f64_below_flt_max(ops):
    """a window of -1e300: below the -FLT_MAX the reference starts its maximum at for every T -> (-FLT_MAX, -1)"""
    x = np.full((1, 1, 4, 5), -1e300)
    rois = np.array([[0, 0, 0, 4, 3], [0, 1, 1, 2, 2]], np.float64)
    out, amax = ops.C.roi_pool_forward(ops.t(x), ops.t(rois), 1.0, 2, 2)
    out, amax = ops.n(out), ops.n(amax)
    assert (amax == -1).all(), amax.ravel()
    assert same_bits(out, np.full(out.shape, np.float64(-FLT_MAX))), out.ravel()


def check_focal_f64(ops, C, gamma):
    c = focal_case(C, gamma)
    lg, tg = ops.t(c["logits"]), ops.t(c["targets"])
    f = ops.n(ops.C.sigmoid_focalloss_forward(lg, tg, C, gamma, FOCAL_ALPHA))
    b = ops.n(ops.C.sigmoid_focalloss_backward(lg, tg, ops.t(c["d"]), C, gamma, FOCAL_ALPHA))
    assert f.dtype == np.float64 and b.dtype == np.float64
    ign = c["targets"] < 0
    assert ign.any() and not f[ign].any() and not b[ign].any()          # exactly +-0.0, never NaN
    _close(f, c["loss"], 1e-4, 1e-6)
    _close(b, c["grad"], 1e-4, 1e-6)
    assert np.isfinite(f).all() and np.isfinite(b).all()


def nms_host_f64(boxes, scores, thr):
    """detops_nms_cpu_f64: the library's host branch (always the product library: it runs on the CPU)"""
    import ctypes
    from maskrcnn_benchmark import _lib
    b, s = np.ascontiguousarray(boxes, np.float64), np.ascontiguousarray(scores, np.float64)
    n = b.shape[0]
    keep, num = np.full((n,), -1, np.int64), np.zeros((1,), np.int32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = _lib.lib.detops_nms_cpu_f64(p(b), p(s), n, float(thr), p(keep), p(num))
    assert rc == 0, rc
    return keep[:int(num[0])].copy()


def check_nms64(ops, name):
    c = nms64_case(name)
    keep = ops.C.nms(ops.t(c["boxes"]), ops.t(c["scores"]), c["thr"])
    assert keep.dtype == ops.torch.int64
    keep = ops.n(keep)
    assert np.array_equal(keep, c["keep"]), (name, keep, c["keep"])
    assert np.array_equal(keep, nms_host_f64(c["boxes"], c["scores"], c["thr"])), name
