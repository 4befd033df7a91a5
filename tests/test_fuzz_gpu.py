"""The seeded random-shape sweep of tests/fuzz_cases.py on the MI355X — run with `-m gpu`.  The device sibling of
tests/test_emu_fuzz.py: same families, same seeds, the same cases bit for bit (tests/golden/fuzz_case_digests.json).

Everything goes through `maskrcnn_benchmark._C` and `_lib.tuning_set`.  The emulation steps through a wave in program
order on zeroed host memory; what it cannot see is what this file is about: real cross-lane operations, LDS reuse and flags
between workgroups at shapes nobody chose by hand, and UNINITIALISED DEVICE MEMORY.  `_C` takes every output and workspace
from `torch.empty`, and a test process mostly hands out fresh (zero) pages.  So every case runs twice in the same test
(`_clean_then_dirty` of tests/dirty_memory.py): once on the allocator as it is, once after `dirty_allocator()` has left
0xFF bytes — NaN in every float type, -1 in every integer type — in the free blocks that the next allocations are cut from.  Both runs meet the reference;
what the kernels promise to reproduce (bit-exact forwards, NMS, the no-atomics backwards, the two-stage focal sum) is also
equal in bits between the two runs.  A kernel that relies on a zeroed workspace, or leaves an output element unwritten,
fails the second run.  `test_dirty_allocator_positive_control` shows that the helper does what the second runs rely on.

Every tolerance is the one an existing test of the same operator states; each test names it."""
import numpy as np
import pytest
import torch

import fuzz_cases
import oracle
from dirty_memory import _clean_then_dirty, _within, dirty_allocator
from graph_replay import bits_equal, first_difference
from torch_refs import launches

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = fuzz_cases.SEEDS


def _C():
    from maskrcnn_benchmark import _C as C

    return C


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().contiguous().cpu().numpy()


def _tune(key, value):
    from maskrcnn_benchmark import _lib
    _lib.tuning_set(key, value)


def _case(family, seed):
    c = fuzz_cases.FAMILIES[family](seed)
    if c is None:
        pytest.skip("empty output")
    return c


# ------------------------------------------------------------------------------------------ dirty memory
def test_dirty_allocator_positive_control():
    """straight after `dirty_allocator()` a small and a large `torch.empty` read back all-NaN: without this the second run
    of every case below would prove nothing"""
    dirty_allocator()
    small = torch.empty(1000, device=DEV)
    large = torch.empty(4 << 20, device=DEV)
    ints = torch.empty(1000, dtype=torch.int32, device=DEV)      # (all three before any check: a check's temporaries are cut from the same blocks)
    assert bool(torch.isnan(small).all()), "%d of 1000 floats of a small allocation are not NaN" % int((~torch.isnan(small)).sum())
    assert bool(torch.isnan(large).all()), "%d of 4 Mi floats of a large allocation are not NaN" % int((~torch.isnan(large)).sum())
    assert bool((ints == -1).all())


# ------------------------------------------------------------------------------------------ ROIAlign, one map
def _acc_plan_holds(H, W, ph):
    """roi_align_bwd.hip acc_plan(): maps within 32 x 32 whose ring + two T buffers + map + row tables fit 150 KB of LDS (the
    formula of test_roi_align_backward_acc_and_two_call_ring_random_shapes); other shapes fall through to the scan kernel"""
    nring, pad = (4, 8) if ph == 7 else (3, 16)
    lds = 4 * (nring * 4 * (64 if ph == 7 else 256) * 4 + 2 * H * pad * 20 + 16 * ((H * W + 3) & ~3) + 8 * (H + W) * pad) + 144
    return H <= 32 and W <= 32 and lds <= 150 * 1024


@pytest.mark.parametrize("seed", range(SEEDS["roi_align"]))
def test_fuzz_roi_align(seed):
    """single-level ROIAlign: the forward np.array_equal to the oracle (pooled sizes (1,1) (2,5) (5,2) (3,3) (9,4) and channel
    counts 1 3 5 17 33 reach the device here only); the backward under roi_bwd_impl 2 (scan) and 3 (atomic), for 7x7 / 14x14
    also 1 (ring, roi_bwd_seg = 8 + seed % 3) and 4 (acc, roi_bwd_groups 0 / 1 / 3), for seed % 3 == 0 the scan kernel's
    ROI-list split (groups 5).  Bounds: 2e-5 * max(1, |ref|max) against the fp64-accumulated oracle for ring, scan and acc
    (the emulation test's and test_roi_align_backward_acc_and_two_call_ring_random_shapes'), 1e-4 * max(1, |ref|max) for
    the atomic kernel (test_roi_align_backward_cfg1: its order of addition is not fixed).
    Reproducible, hence equal between clean and dirty memory: the forward, and the acc result where the acc plan holds
    (`_acc_plan_holds`; seeds 0 and 5 among the 7x7 ones, 17 at 14x14: the map accumulates in LDS and, for groups 3 — seed
    5 — in partial maps of the workspace, combined in a fixed order).  Scan and atomic add with atomics; the ring kernel
    adds without, but which crowded tiles get their hit list split depends on the order in which the pre-pass's workgroups
    claim the few extra segments, so its summation order is not fixed once more splits are wanted than there are."""
    c = _case("roi_align", seed)
    N, C, H, W, K, ph, pw, sr, scale = (c[k] for k in ("N", "C", "H", "W", "K", "ph", "pw", "sr", "scale"))
    x, rois, g = c["x"], c["rois"], c["g"]
    ref_out = oracle.roi_align_forward(x, rois, scale, ph, pw, sr)
    ref = oracle.roi_align_backward(g, rois, scale, ph, pw, N, C, H, W, sr, acc64=True)
    tol = 2e-5 * max(1.0, np.abs(ref).max())
    tol_atomic = 1e-4 * max(1.0, np.abs(ref).max())
    impls = [("scan", 2), ("atomic", 3)] + ([("ring", 1), ("acc", 4)] if (ph, pw) in ((7, 7), (14, 14)) else [])

    def run():
        keep = {}
        tx, tr, tg = _t(x), _t(rois), _t(g)
        out = _C().roi_align_forward(tx, tr, scale, ph, pw, sr)
        assert np.array_equal(_np(out), ref_out), "forward must be bit-equal"
        keep["forward"] = out
        for name, impl in impls:
            _tune("roi_bwd_impl", impl)
            _tune("roi_bwd_seg", 8 + seed % 3 if impl == 1 else 0)
            _tune("roi_bwd_groups", [0, 1, 3][seed % 3] if impl == 4 else 0)
            got = _C().roi_align_backward(tg, tr, scale, ph, pw, N, C, H, W, sr)
            _within(_np(got), ref, tol_atomic if impl == 3 else tol, name)
            if impl == 4 and _acc_plan_holds(H, W, ph):
                keep[name] = got
        if seed % 3 == 0:
            _tune("roi_bwd_impl", 2)
            _tune("roi_bwd_seg", 0)
            _tune("roi_bwd_groups", 5)
            got = _C().roi_align_backward(tg, tr, scale, ph, pw, N, C, H, W, sr)
            _within(_np(got), ref, tol, "ROI-list split")
        for key in ("roi_bwd_impl", "roi_bwd_seg", "roi_bwd_groups"):
            _tune(key, 0)
        return keep

    _clean_then_dirty(run)


# ------------------------------------------------------------------------------------------ ROIAlign over a pyramid
def _fpn_refs(c):
    L, shapes, scales, feats, rois, ph, g = (c[k] for k in ("L", "shapes", "scales", "feats", "rois", "ph", "g"))
    lv = oracle.fpn_level(rois, 2, 2 + L - 1, 224.0, 4.0, 1e-6)
    sels = [np.nonzero(lv == l)[0] for l in range(L)]
    fwd = [oracle.roi_align_forward(feats[l], rois[s], scales[l], ph, ph, 2) if s.size else None for l, s in enumerate(sels)]
    bwd = [oracle.roi_align_backward(g[s], rois[s], scales[l], ph, ph, *shapes[l], 2, acc64=True) if s.size
           else np.zeros(shapes[l], np.float32) for l, s in enumerate(sels)]
    return lv, sels, fwd, bwd


def _scan_split_adds_with_atomics(shapes, K, bins):
    """roi_align_bwd.hip run_backward_scan(): tiles of 8 x 32 pixels, 16 channels per workgroup unless that leaves fewer
    than 2 * 256 work items (then 4); still fewer, and more than 64 ROIs -> the ROI list is split over min(32, ceil(K / 16))
    groups of workgroups, which add into the zeroed maps with atomics"""
    def items(ct):
        return sum(N * -(-H // 8) * -(-W // 32) * -(-C // ct) for (N, C, H, W) in shapes)
    ct = 4 if (items(16) < 512 or bins > 256) else 16
    return items(ct) < 512 and K > 64


@pytest.mark.parametrize("seed", range(SEEDS["roi_align_fpn"]))
def test_fuzz_roi_align_fpn(seed):
    """random 2-4-level pyramids with odd level sizes through the fused FPN pair (NCHW): the level map equal to
    oracle.fpn_level, the forward bit-equal per level, roi_align_fpn_backward with roi_bwd_seg = 4 + seed % 5 within
    2e-5 * max(1, |ref|max) of the fp64-accumulated oracle per level (the emulation test's bound), an empty level all zero.
    Route of the default dispatch (roi_align_bwd.hip run_backward): several levels rule out the acc kernel; the ring plan
    declines a launch of fewer than 2 * 256 (tile, channel chunk) units — at most 8 x 3 tiles x 2 images x 1 chunk plus the
    smaller levels here — so the scan kernel runs, and splits the ROI list over groups that add with atomics where
    `_scan_split_adds_with_atomics` says so (the seeds with 150 ROIs).  Two runs are asserted bit-equal only on the other
    seeds; with atomics both meet the bound.  `roi_bwd_seg` acts on the ring kernel only, so the same call runs once more
    with roi_bwd_impl = 1 (the ring kernel wherever its plan applies; ring_plan() raises the switch to its minimum, segments of 8 hits).  Both of its runs meet
    the bound; they are not asserted equal: a pyramid this small has 8 extra segments, crowded tiles want more, and which
    tiles the pre-pass grants them to depends on the order its workgroups arrive in (roi_bwd_prep_kernel: "a refused split
    is only slower") — measured on seed 4: 4507 of 17280 elements of level 0 differ in the last bit or two between two
    runs.  `launches()` counts one fused forward and the backward calls."""
    c = _case("roi_align_fpn", seed)
    L, shapes, scales, feats, rois, ph, g, K = (c[k] for k in ("L", "shapes", "scales", "feats", "rois", "ph", "g", "K"))
    ref_lv, sels, ref_fwd, ref_bwd = _fpn_refs(c)
    atomics = _scan_split_adds_with_atomics(shapes, K, ph * ph)

    def run():
        keep = {}
        tf, tr, tg = [_t(f) for f in feats], _t(rois), _t(g)
        with launches() as calls:
            out, lv = _C().roi_align_fpn_forward(tf, tr, scales, ph, ph, 2, 2, 2 + L - 1)
        assert calls == {"roi_align_fpn_fwd": 1}, calls
        assert np.array_equal(_np(lv), ref_lv)
        outn = _np(out)
        for l in range(L):
            if sels[l].size:
                assert np.array_equal(outn[sels[l]], ref_fwd[l]), l
        keep["forward"], keep["levels"] = out, lv
        _tune("roi_bwd_seg", 4 + seed % 5)
        for impl, name, reproducible in ((0, "default", not atomics), (1, "ring", False)):
            _tune("roi_bwd_impl", impl)
            with launches() as calls:
                gins = _C().roi_align_fpn_backward(tg, tr, lv, shapes, scales, ph, ph, 2)
                again = _C().roi_align_fpn_backward(tg, tr, lv, shapes, scales, ph, ph, 2)
            assert calls == {"roi_align_fpn_bwd": 2}, calls
            for l in range(L):
                bound = 2e-5 * max(1.0, np.abs(ref_bwd[l]).max())
                _within(_np(gins[l]), ref_bwd[l], bound, (name, l))
                _within(_np(again[l]), ref_bwd[l], bound, (name, l, "again"))
                if reproducible:
                    assert bits_equal(gins[l], again[l]), (name, l, first_difference(gins[l], again[l]))
                    keep["%s backward, level %d" % (name, l)] = gins[l]
        _tune("roi_bwd_impl", 0)
        _tune("roi_bwd_seg", 0)
        return keep

    _clean_then_dirty(run)


@pytest.mark.parametrize("seed", range(SEEDS["roi_align_fpn"]))
def test_fuzz_roi_align_fpn_channels_last(seed, monkeypatch):
    """the same pyramids and ROIs with the features as channels_last tensors (csrc/roi_align_nhwc.hip; so far tested on
    synth.fpn_shapes() only): the forward with a contiguous and a channels-last pooled tensor bit-equal to the oracle;
    roi_align_fpn_backward(channels_last=True) from a contiguous and from a channels-last gradient, once with
    `_C.NHWC_BACKWARD = "native"` and once with the default (whose ring plan declines these underfilled launches and hands
    them to the native kernel), within 1e-4 * max(1, |want|max) of the fp64-accumulated oracle and bit-equal between two
    runs (test_roi_align_fpn_backward_channels_last_matches_the_oracle_and_is_reproducible: a pixel-owner kernel, no atomics).
    Route (detops_roi_align_fpn_backward_nhwc_f32): the staged block needs a contiguous gradient, 49 bins and
    (C * 49) % 4 == 0 — the even seeds (7x7) with C in 4, 16, 32; 14x14 bins (odd seeds), C = 17 and every channels-last
    gradient take the unstaged one; C = 17 runs at vector width 1 in both directions."""
    C_ = _C()
    c = _case("roi_align_fpn", seed)
    L, shapes, scales, feats, rois, ph, g = (c[k] for k in ("L", "shapes", "scales", "feats", "rois", "ph", "g"))
    ref_lv, sels, ref_fwd, ref_bwd = _fpn_refs(c)
    default_mode = C_.NHWC_BACKWARD

    def run():
        keep = {}
        tf = [_t(f).contiguous(memory_format=torch.channels_last) for f in feats]
        tr, tlv = _t(rois), _t(ref_lv.astype(np.int32))
        for out_cl in (False, True):
            out, lv = C_.roi_align_fpn_forward(tf, tr, scales, ph, ph, 2, 2, 2 + L - 1, out_channels_last=out_cl)
            assert C_.is_channels_last(out) == out_cl
            assert np.array_equal(_np(lv), ref_lv)
            outn = _np(out)
            for l in range(L):
                if sels[l].size:
                    assert np.array_equal(outn[sels[l]], ref_fwd[l]), (out_cl, l)
            keep["forward, channels-last output %s" % out_cl] = out.contiguous()
        for mode in ("native", default_mode):
            monkeypatch.setattr(C_, "NHWC_BACKWARD", mode)
            for g_cl in (False, True):
                tg = _t(g).contiguous(memory_format=torch.channels_last) if g_cl else _t(g)
                a = C_.roi_align_fpn_backward(tg, tr, tlv, shapes, scales, ph, ph, 2, channels_last=True)
                b = C_.roi_align_fpn_backward(tg, tr, tlv, shapes, scales, ph, ph, 2, channels_last=True)
                for l in range(L):
                    what = (mode, g_cl, l)
                    assert tuple(a[l].shape) == tuple(shapes[l]) and (C_.is_channels_last(a[l]) or a[l].is_contiguous()), what
                    assert bits_equal(a[l].contiguous(), b[l].contiguous()), (what, first_difference(a[l].contiguous(), b[l].contiguous()))
                    _within(_np(a[l]), ref_bwd[l], 1e-4 * max(1.0, np.abs(ref_bwd[l]).max()), what)
                    keep["backward %s, channels-last gradient %s, level %d" % (mode, g_cl, l)] = a[l].contiguous()
        monkeypatch.setattr(C_, "NHWC_BACKWARD", default_mode)
        return keep

    _clean_then_dirty(run)


# ------------------------------------------------------------------------------------------ NMS
@pytest.mark.parametrize("seed", range(SEEDS["nms"]))
def test_fuzz_nms(seed):
    """`_C.nms` equal to oracle.nms with the sortedness check on and off (nms_no_presorted 0 / 1): integer boxes with exact
    IoU == threshold ties, score ties, duplicates, thresholds 0 and 1; the keep list and its count come from torch.empty"""
    c = _case("nms", seed)
    boxes, scores, thr = c["boxes"], c["scores"], c["thr"]
    ref = oracle.nms(boxes, scores, thr)

    def run():
        keep = {}
        tb, ts = _t(boxes), _t(scores)
        for no_presorted in (0, 1):
            _tune("nms_no_presorted", no_presorted)
            got = _C().nms(tb, ts, thr)
            assert got.dtype == torch.int64
            assert np.array_equal(_np(got), ref), no_presorted
            keep["keep, nms_no_presorted %d" % no_presorted] = got
        _tune("nms_no_presorted", 0)
        return keep

    _clean_then_dirty(run)


@pytest.mark.parametrize("seed", range(SEEDS["nms_batched"]))
def test_fuzz_nms_batched(seed):
    """ragged segment sets through the single launch (nms_fused 0; 3: without the scan-first roles) and the three launches
    (nms_fused 2): nms_batched and nms_batched_mask per segment against oracle.nms, the two counts equal, empty segments
    give 0, max_n = max(max(sizes), 1).  Route (nms.hip): max_n <= 4096 in every case, so nms_fused != 2 is the single
    launch, whose roles hand over through flags in the workspace — taken from torch.empty, 0xFF-filled in the second run.
    `keep` beyond a segment's count is not written and not compared.  The kernel timer counts the mask entry point."""
    c = _case("nms_batched", seed)
    sizes, boxes, scores, offs, thr, max_n = (c[k] for k in ("sizes", "boxes", "scores", "offs", "thr", "max_n"))
    segs = fuzz_cases.segments(c)
    refs = [oracle.nms(b, s, thr) if len(s) else np.zeros(0, np.int64) for b, s in segs]
    assert max_n <= 4096

    def run():
        out = {}
        tb, ts, to = _t(boxes), _t(scores), _t(offs)
        for fused in (0, 3, 2):
            _tune("nms_fused", fused)
            with launches() as calls:
                keep, num = _C().nms_batched(tb, ts, to, max_n, thr)
                km, num2 = _C().nms_batched_mask(tb, ts, to, max_n, thr)
            assert calls == ({"nms_batched": 1} if sum(sizes) else {}), calls
            keep, num, km = _np(keep), _np(num), _np(km)
            assert np.array_equal(num, _np(num2))
            for i, (b, s) in enumerate(segs):
                assert num[i] == len(refs[i]), (fused, i, sizes[i])
                assert np.array_equal(keep[offs[i]:offs[i] + num[i]], refs[i]), (fused, i, sizes[i])
                want = np.zeros(len(s), bool)
                want[refs[i]] = True
                assert np.array_equal(km[offs[i]:offs[i + 1]], want), (fused, i, sizes[i])
            out["mask, nms_fused %d" % fused] = torch.from_numpy(km)
            out["counts, nms_fused %d" % fused] = torch.from_numpy(num)
        _tune("nms_fused", 0)
        return out

    _clean_then_dirty(run)


# ------------------------------------------------------------------------------------------ deformable convolution
@pytest.mark.parametrize("seed", range(SEEDS["deformable"]))
def test_fuzz_deformable(seed):
    """the reference-layout kernels, called as in test_deformable_kernels_vs_oracle_fp32: deformable_im2col (rtol 1e-5, atol
    1e-5), deformable_col2im under dcn_col2im 1 (inverted-index gather, run twice: bit-equal), 2 (atomic LDS window), 3
    (fixed-width index) and 0 (default), deformable_col2im_coord — rtol 1e-4, atol 1e-4 * max(1, |ref|max), both bounds from
    that test.  col2im accumulates into a zeroed map; the column matrix, the offset / mask gradients (torch.empty here as in
    the layers) and the gather's index workspace are what the dirty run poisons."""
    c = _case("deformable", seed)
    k, stride, pad, dil, dg = (c[n] for n in ("k", "stride", "pad", "dil", "dg"))
    x, off, mask, gcol = c["x"], c["off"], c["mask"], c["gcol"]
    geo = (k, k, pad, pad, stride, stride, dil, dil, dg)
    ogeo = dict(kh=k, kw=k, pad=(pad, pad), stride=(stride, stride), dil=(dil, dil), dg=dg)
    ref_col = oracle.deformable_im2col(x, off, mask, **ogeo)
    assert ref_col.shape == gcol.shape
    ref_gim = oracle.deformable_col2im(gcol, off, mask, *x.shape, **ogeo)
    rgoff, rgmask = oracle.deformable_col2im_coord(gcol, x, off, mask, **ogeo)

    def close(got, ref, what):
        np.testing.assert_allclose(_np(got), ref, rtol=1e-4, atol=1e-4 * max(1.0, np.abs(ref).max()), err_msg=what)

    def run():
        keep = {}
        C_ = _C()
        tx, toff, tg = _t(x), _t(off), _t(gcol)
        tm = None if mask is None else _t(mask)
        col = C_.deformable_im2col(tx, toff, tm, *geo)
        np.testing.assert_allclose(_np(col), ref_col, rtol=1e-5, atol=1e-5)
        for switch in (1, 1, 2, 3, 0):
            _tune("dcn_col2im", switch)
            gim = torch.zeros(*x.shape, device=DEV)
            C_.deformable_col2im(tg, toff, tm, gim, *geo)
            close(gim, ref_gim, "dcn_col2im %d" % switch)
            if switch == 1:
                if "gather" in keep:
                    assert bits_equal(gim, keep["gather"]), "gather col2im must be deterministic: " + first_difference(gim, keep["gather"])
                keep["gather"] = gim
        goff = torch.empty(*off.shape, device=DEV)
        gmask = None if mask is None else torch.empty(*mask.shape, device=DEV)
        C_.deformable_col2im_coord(tg, tx, toff, tm, goff, gmask, *geo)
        close(goff, rgoff, "offset gradient")
        if mask is not None:
            close(gmask, rgmask, "mask gradient")
        return keep

    _clean_then_dirty(run)


@pytest.mark.parametrize("seed", range(SEEDS["deformable_channels_last"]))
@pytest.mark.parametrize("channels_last", [False, True])
def test_fuzz_deformable_channels_last(seed, channels_last):
    """the layers (deform_conv / modulated_deform_conv, the entry points of dcn_geometry_cases.check_nhwc_layer) forward and
    backward on shapes of the channels-last plan, NCHW tensors and everything channels-last: output, input, offset, mask
    and weight gradients against oracle.deform_conv_forward / deform_conv_backward at rtol 1e-4, atol 2e-4 * max(1,
    |ref|max) — the emulation test's bound; check_nhwc_layer's bit-equality holds on its exact-arithmetic inputs only.
    The launch counter shows the plan: one NHWC im2col, the coordinate kernel, the col2im gather, and the two layout
    transposes of NCHW tensors."""
    from maskrcnn_benchmark import _C as C_
    from maskrcnn_benchmark.layers import deform_conv, modulated_deform_conv
    assert C_.DCN_INPUT_GRAD == "col2im"
    c = _case("deformable_channels_last", seed)
    stride, pad, dil = c["stride"], c["pad"], c["dil"]
    x, off, mask, wgt, go = (c[n] for n in ("x", "off", "mask", "wgt", "go"))
    geo = ((pad, pad), (stride, stride), (dil, dil))
    ref_out = oracle.deform_conv_forward(x, off, mask, wgt, None, *geo, 1, 1)
    rin, roff, rmask, rw, _ = oracle.deform_conv_backward(x, off, mask, wgt, go, False, *geo, 1, 1)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    want_calls = {"dcn_im2col_nhwc": 1, "dcn_coord_nhwc": 1, "dcn_col2im_nhwc": 1}
    if not channels_last:
        want_calls["dcn_to_nhwc"] = 2

    def close(got, ref, what):
        np.testing.assert_allclose(_np(got), ref, rtol=1e-4, atol=2e-4 * max(1.0, np.abs(ref).max()), err_msg=what)

    def run():
        t = {n: None if a is None else _t(a).contiguous(memory_format=fmt) for n, a in (("x", x), ("off", off), ("mask", mask), ("wgt", wgt), ("go", go))}
        for n in ("x", "off", "mask", "wgt"):
            if t[n] is not None:
                t[n].requires_grad_()
        with launches() as calls:
            if mask is None:
                y = deform_conv(t["x"], t["off"], t["wgt"], (stride, stride), (pad, pad), (dil, dil), 1, 1)
            else:
                y = modulated_deform_conv(t["x"], t["off"], t["mask"], t["wgt"], None, stride, pad, dil, 1, 1)
            y.backward(t["go"])
        assert {k: v for k, v in calls.items() if k.startswith("dcn_")} == want_calls, calls
        close(y, ref_out, "output")
        close(t["x"].grad, rin, "input gradient")
        close(t["off"].grad, roff, "offset gradient")
        close(t["wgt"].grad, rw, "weight gradient")
        if mask is not None:
            close(t["mask"].grad, rmask, "mask gradient")
        return {}

    _clean_then_dirty(run)


# ------------------------------------------------------------------------------------------ focal loss
def _placed(a, offset_floats):
    """`a` on the device as a contiguous view that starts `offset_floats` floats into a larger buffer: `_C` passes a
    contiguous view's data_ptr() through unchanged, so offset 1 gives the kernels a pointer with data_ptr() % 16 == 4"""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
    v = buf[offset_floats:offset_floats + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * offset_floats
    return v


@pytest.mark.parametrize("seed", range(SEEDS["focal"]))
def test_fuzz_focal(seed):
    """sigmoid_focalloss_forward, _backward, _forward_sum and _backward_scalar against the oracle: elementwise rtol 1e-4, atol
    1e-6 (the project's focal bound), the sum within 1e-4 * |fp64 sum of the oracle's losses| (test_focal_full_size_
    properties_and_module; the losses are non-negative: no cancellation), _forward_sum twice bit-equal (fixed-order
    two-stage reduction, per-workgroup sums in a torch.empty workspace), all outputs finite.
    Three placements: everything aligned; for `offset_floats` = 1 the logits one float into a larger buffer; and, in a
    second pass, the upstream gradient there with aligned logits.  Route (focal_loss.hip launch()): float4 kernels iff
    C % 4 == 0 and logits, output and elementwise upstream gradient are 16-byte aligned, so an offset placement runs the
    scalar kernels at C = 4 (seeds 2, 9), 8 (seed 11) and 80 (seeds 5, 13) where the aligned one runs the float4 kernels
    (one and two float4 groups per row at C = 4 and 8); the offset results agree with the aligned ones within the bound.
    Grids are capped at 2048 x 256 work items: seed 12 (530 874 elements, C = 81) wraps the scalar kernels, seed 13
    (524 300 float4 groups, gamma 1.5) the float4 kernels outside the gamma == 2 instantiation and, offset, the scalar
    ones.  The kernel timer counts the two model entry points."""
    c = _case("focal", seed)
    R, C, gamma, alpha, o = c["R"], c["C"], c["gamma"], c["alpha"], c["offset_floats"]
    logits, targets, d_losses, d_scalar = c["logits"], c["targets"], c["d_losses"], c["d_scalar"]
    ref = oracle.sigmoid_focal_loss_forward(logits, targets, gamma, alpha)
    ref_sum = float(ref.astype(np.float64).sum())
    dref = oracle.sigmoid_focal_loss_backward(logits, targets, d_losses, gamma, alpha)
    sref = oracle.sigmoid_focal_loss_backward(logits, targets, np.full_like(logits, d_scalar), gamma, alpha)
    tol = dict(rtol=1e-4, atol=1e-6)

    def one(tl, td, tt, what):
        C_ = _C()
        with launches() as calls:
            f = C_.sigmoid_focalloss_forward(tl, tt, C, gamma, alpha)
            b = C_.sigmoid_focalloss_backward(tl, tt, td, C, gamma, alpha)
            total = C_.sigmoid_focalloss_forward_sum(tl, tt, C, gamma, alpha)
            total2 = C_.sigmoid_focalloss_forward_sum(tl, tt, C, gamma, alpha)
            s = C_.sigmoid_focalloss_backward_scalar(tl, tt, torch.full((), d_scalar, device=DEV), C, gamma, alpha)
        assert calls == {"focal_fwd_sum": 2, "focal_bwd_scalar": 1}, calls
        np.testing.assert_allclose(_np(f), ref, err_msg=what + " forward", **tol)
        np.testing.assert_allclose(_np(b), dref, err_msg=what + " backward", **tol)
        np.testing.assert_allclose(_np(s), sref, err_msg=what + " scalar backward", **tol)
        assert abs(float(total) - ref_sum) <= 1e-4 * abs(ref_sum), (what, float(total), ref_sum)
        assert bits_equal(total, total2), (what, float(total), float(total2))
        assert all(bool(torch.isfinite(v).all()) for v in (f, b, s, total)), what
        return {what + " forward": f, what + " backward": b, what + " sum": total, what + " scalar backward": s}

    def run():
        tt = _t(targets)
        keep = one(_placed(logits, 0), _placed(d_losses, 0), tt, "aligned")
        if o:
            keep.update(one(_placed(logits, o), _placed(d_losses, 0), tt, "offset logits"))
            keep.update(one(_placed(logits, 0), _placed(d_losses, o), tt, "offset gradient"))
            for name in ("forward", "backward", "scalar backward"):
                for what in ("offset logits ", "offset gradient "):
                    np.testing.assert_allclose(_np(keep[what + name]), _np(keep["aligned " + name]), err_msg=what + name, **tol)
            for what in ("offset logits sum", "offset gradient sum"):
                assert abs(float(keep[what]) - float(keep["aligned sum"])) <= 1e-4 * abs(ref_sum), what
        return keep

    _clean_then_dirty(run)
