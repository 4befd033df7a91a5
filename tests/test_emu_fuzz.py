"""Randomised small-shape sweeps of the emulated HIP kernels against the oracle (CPU only).  Shapes,
ROI geometry, bin counts, sampling ratios and channel counts are drawn per case from a seeded
generator, so every run covers the same 60-odd configurations — odd sizes, ROIs outside the map,
degenerate ROIs, maps smaller than a tile, channel counts that are not multiples of any chunk."""
import numpy as np
import pytest

import emu
import fuzz_cases
import oracle

SEEDS = fuzz_cases.SEEDS


def _case(family, seed):
    """the shared case of (family, seed); the seeds whose drawn geometry has no output pixel skip"""
    c = fuzz_cases.FAMILIES[family](seed)
    if c is None:
        pytest.skip("empty output")
    return c


@pytest.mark.parametrize("seed", range(SEEDS["roi_align"]))
def test_emu_fuzz_roi_align(seed):
    c = _case("roi_align", seed)
    N, C, H, W, K, ph, pw, sr, scale = (c[k] for k in ("N", "C", "H", "W", "K", "ph", "pw", "sr", "scale"))
    x, rois, g = c["x"], c["rois"], c["g"]
    out = emu.roi_align_forward(x, rois, scale, ph, pw, sr)
    assert np.array_equal(out, oracle.roi_align_forward(x, rois, scale, ph, pw, sr)), "forward must be bit-equal"
    ref = oracle.roi_align_backward(g, rois, scale, ph, pw, N, C, H, W, sr, acc64=True)
    tol = 2e-5 * max(1.0, np.abs(ref).max())
    impls = [("scan", 2), ("atomic", 3)] + ([("ring", 1), ("acc", 4)] if (ph, pw) in ((7, 7), (14, 14)) else [])
    for name, impl in impls:
        emu.tuning_set("roi_bwd_impl", impl)
        if impl == 1:
            emu.tuning_set("roi_bwd_seg", 8 + seed % 3)        # split whatever is crowded
        if impl == 4:
            emu.tuning_set("roi_bwd_groups", [0, 1, 3][seed % 3])   # auto / one group (direct store) / three partial maps
        emu.stats(reset=True)
        got = emu.roi_align_backward(g, rois, scale, ph, pw, N, C, H, W, sr)
        assert np.abs(got - ref).max() <= tol, name
        if impl == 4:   # maps beyond 32 x 32 (or beyond the LDS budget) fall through to the scan kernel
            if H > 32 or W > 32:
                assert emu.stats().get("bwda.units", 0) == 0, (H, W)
            elif ph == 7:
                assert emu.stats().get("bwda.units", 0) > 0, (H, W)
            emu.tuning_set("roi_bwd_groups", 0)
    if seed % 3 == 0:
        emu.tuning_set("roi_bwd_impl", 2)
        emu.tuning_set("roi_bwd_groups", 5)
        got = emu.roi_align_backward(g, rois, scale, ph, pw, N, C, H, W, sr)
        assert np.abs(got - ref).max() <= tol, "ROI-list split"


@pytest.mark.parametrize("seed", range(SEEDS["nms"]))
def test_emu_fuzz_nms(seed):
    c = _case("nms", seed)
    boxes, scores, thr = c["boxes"], c["scores"], c["thr"]
    assert np.array_equal(emu.nms(boxes, scores, thr), oracle.nms(boxes, scores, thr))


@pytest.mark.parametrize("seed", range(SEEDS["deformable"]))
def test_emu_fuzz_deformable(seed):
    c = _case("deformable", seed)
    B, dg, C, H, W, k, stride, pad, dil = (c[n] for n in ("B", "dg", "C", "H", "W", "k", "stride", "pad", "dil"))
    x, off, mask, gcol = c["x"], c["off"], c["mask"], c["gcol"]
    geo = dict(kh=k, kw=k, pad=(pad, pad), stride=(stride, stride), dil=(dil, dil), dg=dg)
    ref_col = oracle.deformable_im2col(x, off, mask, **geo)
    np.testing.assert_allclose(emu.deformable_im2col(x, off, mask, **geo), ref_col, rtol=1e-5, atol=1e-5)
    assert gcol.shape == ref_col.shape
    ref = oracle.deformable_col2im(gcol, off, mask, B, C, H, W, **geo)
    tol = dict(rtol=1e-4, atol=2e-5 * max(1.0, np.abs(ref).max()))
    np.testing.assert_allclose(emu.deformable_col2im(gcol, off, mask, B, C, H, W, gather=True, **geo), ref, **tol)
    np.testing.assert_allclose(emu.deformable_col2im(gcol, off, mask, B, C, H, W, gather=False, **geo), ref, **tol)
    goff, gmask = emu.deformable_col2im_coord(gcol, x, off, mask, **geo)
    roff, rmask = oracle.deformable_col2im_coord(gcol, x, off, mask, **geo)
    np.testing.assert_allclose(goff, roff, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(roff).max()))
    if mask is not None:
        np.testing.assert_allclose(gmask, rmask, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(rmask).max()))


@pytest.mark.parametrize("seed", range(SEEDS["nms_batched"]))
def test_emu_fuzz_nms_batched_single_launch(seed):
    """ragged segment sets through the ONE-launch path (sort, mask tiles and scan as workgroup roles of one kernel) and
    through the three launches: random segment counts and lengths over every scan width, integer boxes (exact IoU ties),
    score ties, empty segments"""
    c = _case("nms_batched", seed)
    sizes, boxes, scores, offs, thr, max_n = (c[k] for k in ("sizes", "boxes", "scores", "offs", "thr", "max_n"))
    segs = fuzz_cases.segments(c)
    for fused in (0, 2):
        emu.tuning_set("nms_fused", fused)
        keep, num = emu.nms_batched(boxes, scores, offs, max_n, thr)
        km, num2 = emu.nms_batched(boxes, scores, offs, max_n, thr, mask=True)
        assert np.array_equal(num, num2)
        for i, (b, s) in enumerate(segs):
            ref = oracle.nms(b, s, thr) if len(s) else np.zeros(0, np.int64)
            assert num[i] == len(ref), (fused, i, sizes[i])
            assert np.array_equal(keep[offs[i]:offs[i] + num[i]], ref), (fused, i, sizes[i])
            want = np.zeros(len(s), np.uint8)
            want[ref] = 1
            assert np.array_equal(km[offs[i]:offs[i + 1]], want)


@pytest.mark.parametrize("seed", range(SEEDS["roi_align_fpn"]))
def test_emu_fuzz_roi_align_fpn_fused(seed):
    """the multi-level launches the pooler uses (level mapping on the device, LDS-DMA forward, ring backward with split
    hit lists) on random pyramids: odd map sizes, 2-4 levels, ROIs of every scale incl. degenerate ones"""
    c = _case("roi_align_fpn", seed)
    L, shapes, scales, feats, rois, ph, g = (c[k] for k in ("L", "shapes", "scales", "feats", "rois", "ph", "g"))
    out, lv = emu.roi_align_fpn_forward(feats, rois, scales, ph, ph, 2, 2, 2 + L - 1)
    ref_lv = oracle.fpn_level(rois, 2, 2 + L - 1, 224.0, 4.0, 1e-6)
    assert np.array_equal(lv, ref_lv)
    for l in range(L):
        sel = np.nonzero(lv == l)[0]
        if sel.size:
            assert np.array_equal(out[sel], oracle.roi_align_forward(feats[l], rois[sel], scales[l], ph, ph, 2)), l
    emu.tuning_set("roi_bwd_seg", 4 + seed % 5)
    gins = emu.roi_align_fpn_backward(g, rois, lv, shapes, scales, ph, ph, 2)
    again = emu.roi_align_fpn_backward(g, rois, lv, shapes, scales, ph, ph, 2)
    for l in range(L):
        sel = np.nonzero(lv == l)[0]
        ref = oracle.roi_align_backward(g[sel], rois[sel], scales[l], ph, ph, *shapes[l], 2, acc64=True) if sel.size \
            else np.zeros(shapes[l], np.float32)
        assert np.abs(gins[l] - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), l
        assert np.array_equal(gins[l], again[l]), "bit-reproducible"


@pytest.mark.parametrize("seed", range(SEEDS["deformable_channels_last"]))
def test_emu_fuzz_deformable_channels_last(seed):
    """the channels-last pipeline (NHWC im2col, in-wave coordinate-gradient reduction, transposed sampling + GEMMs) on
    random geometries against the oracle's reference-layout arithmetic"""
    c = _case("deformable_channels_last", seed)
    k, stride, pad, dil = (c[n] for n in ("k", "stride", "pad", "dil"))
    x, off, mask, wgt, go = (c[n] for n in ("x", "off", "mask", "wgt", "go"))
    geo = ((pad, pad), (stride, stride), (dil, dil))
    out, gin, goff, gmask, gw = emu.deformable_nhwc(x, off, mask, wgt, go, k, k, *geo)
    ref_out = oracle.deform_conv_forward(x, off, mask, wgt, None, *geo, 1, 1)
    np.testing.assert_allclose(out, ref_out, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(ref_out).max()))
    rin, roff, rmask, rw, _ = oracle.deform_conv_backward(x, off, mask, wgt, go, False, *geo, 1, 1)
    tol = lambda r: dict(rtol=1e-4, atol=2e-4 * max(1.0, np.abs(r).max()))  # noqa: E731
    np.testing.assert_allclose(gin, rin, **tol(rin))
    np.testing.assert_allclose(goff, roff, **tol(roff))
    np.testing.assert_allclose(gw, rw, **tol(rw))
    if mask is not None:
        np.testing.assert_allclose(gmask, rmask, **tol(rmask))


@pytest.mark.parametrize("seed", range(SEEDS["focal"]))
def test_emu_fuzz_focal(seed):
    """the focal-loss kernels on the shared shapes: forward, forward with the two-stage sum, elementwise and scalar backward
    against the oracle at the project's focal bound (rtol 1e-4, atol 1e-6; the sum within 1e-4 of the fp64 sum of the
    oracle's losses, which are non-negative).  Host arrays are 16-byte aligned: class counts that are multiples of 4 take the
    float4 kernels here, the others the scalar kernels, and seeds 12 / 13 stride a second time.  The emulation takes no
    pointer offset (`offset_floats` is the device test's)."""
    c = _case("focal", seed)
    logits, targets, gamma, alpha = c["logits"], c["targets"], c["gamma"], c["alpha"]
    ref = oracle.sigmoid_focal_loss_forward(logits, targets, gamma, alpha)
    tol = dict(rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(emu.focal_forward(logits, targets, gamma, alpha), ref, **tol)
    out, total = emu.focal_forward(logits, targets, gamma, alpha, with_sum=True)
    np.testing.assert_allclose(out, ref, **tol)
    ref_sum = float(ref.astype(np.float64).sum())
    assert abs(total - ref_sum) <= 1e-4 * abs(ref_sum), (total, ref_sum)
    dref = oracle.sigmoid_focal_loss_backward(logits, targets, c["d_losses"], gamma, alpha)
    np.testing.assert_allclose(emu.focal_backward(logits, targets, c["d_losses"], gamma, alpha), dref, **tol)
    sref = oracle.sigmoid_focal_loss_backward(logits, targets, np.full_like(logits, c["d_scalar"]), gamma, alpha)
    np.testing.assert_allclose(emu.focal_backward(logits, targets, c["d_scalar"], gamma, alpha), sref, **tol)


# ------------------------------------------------------------------------------------------ the sweep itself
def test_fuzz_cases_reproduce_the_recorded_digests(golden_dir):
    """tests/golden/fuzz_case_digests.json holds one sha256 per (family, seed) over the case's arrays and parameters
    (fuzz_cases.digest).  The six older families' digests were taken from the draws as they stood inline in this file before
    they moved to tests/fuzz_cases.py, so every case is still the one it was; `focal` is new and recorded from its generator.
    A family yields None for `deformable(0)` and `deformable_channels_last(1)` and for no other seed.  Neither the
    emulation sweep nor the device sweep can be narrowed without this test noticing."""
    import json
    import os
    with open(os.path.join(golden_dir, "fuzz_case_digests.json")) as f:
        want = json.load(f)
    assert set(want) == set(SEEDS) == set(fuzz_cases.FAMILIES)
    for family, n in sorted(SEEDS.items()):
        assert len(want[family]) == n, family
        got = [fuzz_cases.digest(fuzz_cases.FAMILIES[family](seed)) for seed in range(n)]
        assert got == want[family], (family, [s for s in range(n) if got[s] != want[family][s]])
        assert tuple(s for s in range(n) if got[s] is None) == fuzz_cases.EMPTY.get(family, ()), family
    assert fuzz_cases.EMPTY == {"deformable": (0,), "deformable_channels_last": (1,)}


def test_fuzz_sweep_reaches_the_named_branches():
    """the dispatch conditions of the kernels, evaluated on the cases' parameters (no counter exists on the device for these;
    the emulation's `bwda.units` is asserted in test_emu_fuzz_roi_align):
      * focal_loss.hip launch(): float4 kernels iff C % 4 == 0 and 16-byte aligned pointers; grid capped at 2048 workgroups
        of 256 work items — at least three seeds of 0..11 put C % 4 == 0 on a misaligned pointer (scalar kernels), one of
        them with C = 4; C = 4 and C = 8 (one / two float4 groups per row) occur; seed 12 wraps the scalar kernels with
        gamma == 2, seed 13 the float4 kernels with gamma != 2 (the smallest R that does), each by less than one further grid;
      * roi_align_bwd.hip acc_plan(): a 7x7 seed with a map within 32 x 32 (the LDS budget holds for every such map at 7x7:
        the largest, 32 x 32, needs 4 * (4 * 4 * 64 * 4 + 2 * 32 * 8 * 20 + 16 * 1024 + 8 * 64 * 8) + 144 = 139 408 bytes
        <= 150 KB);
      * roi_align_nhwc.hip: the staged block needs 49 bins, a contiguous gradient and C % 4 == 0; 14x14 bins and C = 17
        take the unstaged one, and C = 17 vector width 1;
      * nms.hip: max_n <= 4096 for every batched case (the single launch unless nms_fused == 2), segments on both sides of
        the 1024 and 2048 scan widths."""
    F = fuzz_cases
    focal = [F.focal(s) for s in range(12)]
    scalar_c4 = [c for c in focal if c["C"] % 4 == 0 and c["offset_floats"] == 1]
    assert len(scalar_c4) >= 3 and any(c["C"] == 4 for c in scalar_c4)
    assert {4, 8} <= {c["C"] for c in focal}
    assert all(c["R"] * c["C"] <= F.FOCAL_MAX_ITEMS for c in focal)
    for c in focal:
        assert c["R"] in (1, 2, 37, 255, 257, 1000) and c["C"] in (1, 3, 4, 7, 8, 80, 81)
        assert c["gamma"] in (0.0, 1.0, 2.0, 1.5) and c["alpha"] in (0.25, 0.4, 0.5) and c["offset_floats"] in (0, 1)
        assert c["targets"].min() >= -1 and c["targets"].max() <= c["C"]
        assert list(c["targets"][:4]) == [-1, 0, 1, c["C"]][:c["R"]]
        assert c["logits"][0].min() == -100.0 and (c["C"] == 1 or c["logits"][0].max() == 100.0)
    c12, c13 = F.focal(12), F.focal(13)
    assert (c12["R"], c12["C"], c12["gamma"]) == (6554, 81, 2.0) and (c13["R"], c13["C"], c13["gamma"]) == (26215, 80, 1.5)
    assert F.FOCAL_MAX_ITEMS < c12["R"] * c12["C"] < 2 * F.FOCAL_MAX_ITEMS
    assert F.FOCAL_MAX_ITEMS < c13["R"] * c13["C"] // 4 < 2 * F.FOCAL_MAX_ITEMS and (c13["R"] - 1) * c13["C"] // 4 <= F.FOCAL_MAX_ITEMS
    roi = [F.roi_align(s) for s in range(SEEDS["roi_align"])]
    assert any(c["ph"] == 7 and c["H"] <= 32 and c["W"] <= 32 for c in roi)
    assert {(c["ph"], c["pw"]) for c in roi} == {(7, 7), (14, 14), (1, 1), (2, 5), (5, 2), (3, 3), (9, 4)}
    assert {1, 3, 5, 17, 33} <= {c["C"] for c in roi}
    fpn = [F.roi_align_fpn(s) for s in range(SEEDS["roi_align_fpn"])]
    assert any(c["ph"] == 7 and c["C"] % 4 == 0 for c in fpn) and any(c["ph"] == 14 for c in fpn) and any(c["C"] == 17 for c in fpn)
    assert {c["L"] for c in fpn} == {2, 3, 4}
    nb = [F.nms_batched(s) for s in range(SEEDS["nms_batched"])]
    assert all(c["max_n"] <= 4096 for c in nb)
    sizes = {n for c in nb for n in c["sizes"]}
    assert 0 in sizes and any(n <= 1024 for n in sizes if n) and any(1024 < n <= 2048 for n in sizes) and any(n > 2048 for n in sizes)
