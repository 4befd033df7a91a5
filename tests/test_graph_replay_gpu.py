"""Every sync-free HIP operator of the captured training step, replayed from a HIP graph (tests/graph_replay.py): one capture,
then replays whose VALUES steer the kernels onto other data-dependent routes than the capture saw — other survivor counts,
other pyramid levels, other numbers of valid / sampled / positive rows — each replay held against an eager call made after it
and against the reference of the operator's own eager test (the oracle library, tests/target_cases.py, tests/torch_refs.py,
the fp64 torch composites).  Tolerances are "bits" or the constants of those eager tests, imported or quoted.  Run with
`-m gpu`; single-stream captures only."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import synth
import target_cases as tc
import torch_refs
from graph_replay import assert_bits, bits_equal, check_replay, first_difference

DEV = "cuda"
CL = torch.channels_last
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") != "0",
                                 reason="HIP graph replay needs DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 before the HIP runtime starts "
                                        "(tests/conftest.py sets it; profiles/r04a_hip_graph_flags.txt)")]


def _C():
    from maskrcnn_benchmark import _C as C
    return C


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()) if torch.is_tensor(t) else t


def _tensors(sets):
    """value sets as tuples of host tensors (check_replay then hands the same objects to `expect`)"""
    return [tuple(a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)) for a in s) for s in sets]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _exact_nan(got, want, what):
    """the comparison of the layout kernels' eager tests (torch.equal, tests/torch_refs.py `_exact`): same dtype, same NaN
    positions, every other element equal"""
    torch_refs._exact(got.detach().cpu(), want, what)


# ============================================================================ positive controls: the harness must notice
def test_control_a_host_value_baked_before_capture_fails_the_harness():
    """fn multiplies by a Python float it read from the first value set before the capture: the eager call made after each
    replay is wrong in the same way, the reference is not"""
    baked = {}

    def fn(x):
        if "k" not in baked:
            baked["k"] = float(x[0])             # (the first call is the eager one outside the capture)
        return x * baked["k"]

    sets = [(torch.tensor([2.0, 1.0, 3.0]),), (torch.tensor([5.0, 1.0, 3.0]),)]
    with pytest.raises(AssertionError, match="against the reference"):
        check_replay(fn, sets, expect=lambda v: (v[0] * v[0][0],))


def test_control_an_output_not_rewritten_on_replay_fails_the_harness():
    """fn returns a tensor that it fills on its first call only: nothing writes it during a replay"""
    kept = {}

    def fn(x):
        if "out" not in kept:
            kept["out"] = x * 2
        x.add(1)                                 # (captured work, so that the graph is not empty)
        return kept["out"]

    with pytest.raises(AssertionError):
        check_replay(fn, [(torch.tensor([1.0, 2.0]),), (torch.tensor([3.0, 4.0]),)])


def test_control_a_correct_function_passes_the_harness():
    got = check_replay(lambda x, m: (x * 2 + 1, m & (x > 0)), [(torch.tensor([1.0, -2.0]), torch.tensor([True, True])),
                                                              (torch.tensor([-3.0, 4.0]), torch.tensor([False, True]))],
                       expect=lambda v: (v[0] * 2 + 1, v[1] & (v[0] > 0)))
    assert len(got) == 4 and torch.equal(got[1][1].cpu(), torch.tensor([False, True]))


# ============================================================================ segmented NMS
NMS_THR = 0.55


def _nms_value_sets(lengths):
    """V0 random clustered boxes (the generator of test_nms_bit_exact_vs_oracle), V1 every box identical (one survivor per
    segment), V2 pairwise disjoint boxes with descending scores (all survive; presorted shortcut), V3 a dependency chain
    (test_nms_dependency_chains, step 25 at threshold 0.55)"""
    sets = []
    for kind in ("random", "identical", "disjoint", "chain"):
        bs, ss = [], []
        for i, n in enumerate(lengths):
            rng = np.random.RandomState(7 + i)
            if kind == "random":
                b, s = synth.nms_boxes(n, seed=40 + n % 7)
            elif kind == "identical":
                b = np.tile(np.float32([[30 + i, 40, 130 + i, 100]]), (n, 1))
                s = rng.permutation(n).astype(np.float32) / n
            elif kind == "disjoint":
                j = np.arange(n)
                x0, y0 = (j % 128) * 20.0, (j // 128) * 20.0
                b = np.stack([x0, y0, x0 + 10, y0 + 10], 1).astype(np.float32)
                s = np.linspace(1.0, 0.1, n).astype(np.float32)
            else:
                x0 = np.arange(n, dtype=np.float32) * 25
                b = np.stack([x0, np.zeros(n, np.float32), x0 + 99, np.full(n, 49, np.float32)], 1)
                s = np.linspace(1.0, 0.1, n).astype(np.float32)
            bs.append(b)
            ss.append(s)
        sets.append((np.concatenate(bs), np.concatenate(ss)))
    return sets


def _nms_expect(lengths):
    offs = np.cumsum([0] + list(lengths))

    def expect(values):
        boxes, scores = _np(values[0]), _np(values[1])
        keep = np.full(offs[-1], -1, np.int64)
        mask = np.zeros(offs[-1], bool)
        num = np.zeros(len(lengths), np.int32)
        for i in range(len(lengths)):
            ref = oracle.nms(boxes[offs[i]:offs[i + 1]], scores[offs[i]:offs[i + 1]], NMS_THR)
            num[i] = len(ref)
            keep[offs[i]:offs[i] + len(ref)] = ref
            mask[offs[i] + ref] = True
        return keep, num, mask, num
    return expect


def _nms_replay(lengths):
    C = _C()
    max_n = max(lengths)
    offs_np = np.cumsum([0] + list(lengths)).astype(np.int32)
    offs = _t(offs_np)
    seg = _t(np.repeat(np.arange(len(lengths)), lengths).astype(np.int64))
    pos = _t(np.concatenate([np.arange(n) for n in lengths]).astype(np.int64))
    sets = _nms_value_sets(lengths)
    expect = _nms_expect(lengths)
    survivors = [expect(v)[1] for v in sets]
    assert all(survivors[1] == 1) and all(survivors[2] == np.array(lengths))
    assert all(1 < k < n for k, n in zip(survivors[3], lengths) if n >= 64)
    assert len({tuple(s) for s in survivors}) == 4                  # four different survivor counts per segment
    ob, os_ = synth.nms_boxes(100, seed=3)
    ob, os_, oo = _t(ob), _t(os_), _t(np.array([0, 100], np.int32))

    def fn(boxes, scores):
        keep, num = C.nms_batched(boxes, scores, offs, max_n, NMS_THR)
        mask, num2 = C.nms_batched_mask(boxes, scores, offs, max_n, NMS_THR)
        # rows of `keep` past a segment's count are unspecified: -1 there, as in the reference
        keep = torch.where(pos < num.long()[seg], keep, torch.full_like(keep, -1))
        return keep, num, mask, num2

    assert C.nms_repaired_segments(DEV, reset=True) == 0
    check_replay(fn, sets, expect=expect, between=lambda: C.nms_batched(ob, os_, oo, 100, 0.7))
    assert C.nms_repaired_segments(DEV, reset=True) == 0


@pytest.mark.parametrize("fused", [0, 3, 2], ids=["scan_first", "scans_last", "three_launches"])
@pytest.mark.parametrize("lengths", [(1, 65, 200), (2049,)], ids=["S3_max200", "S1_n2049"])
def test_nms_batched_single_launch_and_three_launch_routes(lengths, fused):
    """_C.nms_batched + _C.nms_batched_mask against the oracle, bit for bit.  Routes (csrc/nms.hip run_nms, read from the
    code): max_n = 200 gives nbmax = 4 <= 32 -> nms_fused_kernel<false>, 4 row blocks and 10 mask tiles -> G = 2 tile
    workgroups per segment; n = 2049 gives nbmax = 33 -> nms_fused_kernel<true>.  Tuning nms_fused = 0 lets the host choose
    scan_first, 3 forces the scans behind the tiles, 2 takes the three launches (sort, mask, scan).  A replay presents the same
    token on the same control block: only the word the scan workgroup cleared makes it wait again."""
    from maskrcnn_benchmark import _lib
    _lib.tuning_set("nms_fused", fused)          # (tests/conftest.py resets the switches after every test)
    _nms_replay(lengths)


def test_nms_batched_device_sort_route():
    """S = 2, n = 8193 > kSortLdsMax = 8192: keys are made, sorted by the device-wide sort and gathered in separate launches
    (the `big` branch of run_nms; 8193 > kFusedMaxN, so the three-launch mask and scan follow)"""
    _nms_replay((8193, 8193))


# ============================================================================ ROIAlign over the pyramid
ROI_LEVELS = ((32, 40), (16, 20), (8, 10), (4, 5))                  # strides 4 .. 32 of a 128 x 160 image
ROI_LEVELS_RANKED = ((112, 160), (56, 80), (28, 40), (14, 20))      # ... of a 448 x 640 image
ROI_SCALES = [1.0 / s for s in synth.FPN_STRIDES[:4]]


def _roi_set(kind, K, levels, seed):
    """[K, 5] ROIs (image, x1, y1, x2, y2), not clipped to the image"""
    rng = np.random.RandomState(seed)
    img_h, img_w = levels[0][0] * 4, levels[0][1] * 4
    b = rng.randint(0, 2, K)
    cx, cy = rng.uniform(0, img_w, K), rng.uniform(0, img_h, K)
    if kind == "mixed":
        s = np.exp(rng.uniform(np.log(8.0), np.log(800.0), K))
    elif kind == "tiny":
        s = rng.uniform(4, 30, K)
    elif kind == "huge":
        s = rng.uniform(500, 900, K)
        b[:] = 1
    else:                                        # partly off the map: centres on the image border and beyond
        s = rng.uniform(20, 200, K)
        side = rng.randint(0, 4, K)
        cx = np.where(side == 0, rng.uniform(-0.2, 0.05, K) * img_w, np.where(side == 1, rng.uniform(0.95, 1.2, K) * img_w, cx))
        cy = np.where(side == 2, rng.uniform(-0.2, 0.05, K) * img_h, np.where(side == 3, rng.uniform(0.95, 1.2, K) * img_h, cy))
    ar = rng.uniform(0.5, 2.0, K)
    w, h = s * np.sqrt(ar), s / np.sqrt(ar)
    return np.stack([b, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)


def _roi_value_sets(K, C, ph, levels):
    sets = []
    for i, kind in enumerate(("mixed", "tiny", "huge", "off_map")):
        rng = np.random.RandomState(50 + i)
        feats = [rng.randn(2, C, h, w).astype(np.float32) for h, w in levels]
        sets.append((feats, _roi_set(kind, K, levels, 60 + i), rng.randn(K, C, ph, ph).astype(np.float32)))
    lv = [synth.level_map(s[1]) for s in sets]
    assert len(set(lv[0])) >= 3 and not lv[1].any() and (lv[2] == 3).all() and (sets[2][1][:, 0] == 1).all()
    return sets


def _roi_expect(ph, sr, levels):
    def expect(values):
        feats, rois, g = [_np(v) for v in values[:4]], _np(values[4]), _np(values[5])
        lv = synth.level_map(rois)
        out = np.zeros(g.shape, np.float32)
        grads = []
        for l, (f, s) in enumerate(zip(feats, ROI_SCALES)):
            sel = np.nonzero(lv == l)[0]
            if sel.size:
                out[sel] = oracle.roi_align_forward(f, rois[sel], s, ph, ph, sr)
                grads.append(oracle.roi_align_backward(g[sel], rois[sel], s, ph, ph, *f.shape, sr, acc64=True))
            else:
                grads.append(None)               # no ROI on this level: the gradient map is exactly zero
        return out, lv, grads
    return expect


def _roi_tol(got, want, what):
    """forward and levels in bits; backward within the 1e-4 relative bound of
    test_roi_align_fpn_backward_channels_last_matches_the_oracle_and_is_reproducible"""
    out, lv, grads = want
    assert_bits(got[:2], (out, lv), what + " forward against the oracle")
    for l, (g, r) in enumerate(zip(got[2:], grads)):
        g = _np(g.contiguous())
        if r is None:
            assert not g.any(), "%s: level %d received no ROI and must be exactly zero" % (what, l)
        else:
            assert np.abs(g - r).max() <= 1e-4 * max(1.0, np.abs(r).max()), "%s: gradient of level %d" % (what, l)
    image0 = sum(float(np.abs(_np(g)[0]).sum()) for g in got[2:])
    if (lv == 3).all():
        assert image0 == 0.0, what + ": every ROI is on image 1, image 0 receives nothing"


@pytest.mark.parametrize("layout", ["nchw", "nhwc_auto", "nhwc_native"])
@pytest.mark.parametrize("K,ph", [(40, 7), (415, 7), (40, 14)], ids=["K40_7x7", "K415_7x7", "K40_14x14"])
def test_roi_align_fpn_forward_and_backward(K, ph, layout, monkeypatch):
    """_C.roi_align_fpn_forward + _C.roi_align_fpn_backward (no `prepared=`) over a four-level pyramid, N = 2, C = 32,
    sampling ratio 2, NCHW and channels-last (backward with NHWC_BACKWARD "auto" and "native").  The ROIs of the replays land
    on other levels and images than those of the capture: mixed sizes; all tiny (every ROI on k_min: the other levels' maps
    must come back exactly zero); all larger than the image and on image 1 (k_max; image 0 receives nothing); partly off the
    map.  Routes: K = 40 is below the ranking pre-pass (csrc/roi_align_fwd.hip: order for K >= 384).  The NCHW forward ranks
    only when the maps exceed 2 MiB (launch_fwd_dma: map_pixels * C * 4 > 2 << 20), which the 32 x 40 pyramid (218 KB) does
    not: NCHW K = 415 therefore runs on a 112 x 160 pyramid (3.0 MB), the smallest 4-level pyramid of this family past that
    limit; the workspace query confirms the ranked layout (it grows by the K int32 order).  The backward zeroes its maps and
    builds its hit lists per call; which backward kernel the host picks depends on the shapes only."""
    C_ = _C()
    Cc, sr = 32, 2
    nhwc = layout != "nchw"
    ranked = K == 415 and not nhwc
    levels = ROI_LEVELS_RANKED if ranked else ROI_LEVELS
    if ranked:
        q = C_.lib.detops_roi_align_forward_workspace_bytes
        assert int(q(K, ph, ph, sr)) - int(q(383, ph, ph, sr)) > (K - 383) * (2 * 16 + 5 * 16 * ph * ph)   # records + the order
        assert sum(h * w for h, w in levels) * Cc * 4 > (2 << 20) > sum(h * w for h, w in ROI_LEVELS) * Cc * 4
    if nhwc:
        monkeypatch.setattr(C_, "NHWC_BACKWARD", "native" if layout == "nhwc_native" else "auto")
    shapes = [(2, Cc, h, w) for h, w in levels]
    sets = []
    for feats, rois, g in _roi_value_sets(K, Cc, ph, levels):
        tf = [torch.from_numpy(f) for f in feats]
        if nhwc:
            tf = [f.contiguous(memory_format=CL) for f in tf]
        sets.append(tuple(tf) + (rois, g))
    small = [torch.randn(1, 4, h, w, device=DEV) for h, w in ((8, 10), (4, 5))]
    if nhwc:
        small = [f.contiguous(memory_format=CL) for f in small]
    small_rois = _t(np.float32([[0, 1, 2, 30, 28], [0, 3, 3, 9, 12], [0, -5, 4, 39, 31]]))

    def fn(f0, f1, f2, f3, rois, g):
        out, lv = C_.roi_align_fpn_forward([f0, f1, f2, f3], rois, ROI_SCALES, ph, ph, sr, 2, 5)
        gins = C_.roi_align_fpn_backward(g, rois, lv, shapes, ROI_SCALES, ph, ph, sr, channels_last=nhwc)
        assert all(C_.is_channels_last(t) == nhwc for t in gins)
        return (out, lv) + tuple(gins)

    check_replay(fn, sets, expect=_roi_expect(ph, sr, levels), tol=_roi_tol,
                 between=lambda: C_.roi_align_fpn_forward(small, small_rois, [0.25, 0.125], 3, 3, 2, 2, 3))


# ============================================================================ matcher, samplers, targets
def _matcher_sets(batched):
    c = tc.matcher_inputs("256x1023", batched)
    N, M = c["valid"].shape
    sets = []
    for kind in ("all", "one", "none"):
        valid = np.ones((N, M), bool)
        if kind == "one":
            valid[:] = False
            valid[0, 7], valid[1, 0] = True, True
        elif kind == "none":
            valid[:] = False
        gt = c["gt"].copy()
        gt[~valid] = tc.PAD_GT
        sets.append((gt, valid, c["boxes"]))
    return sets


@pytest.mark.parametrize("thresholds", tc.MATCHER_THRESHOLDS, ids=("rpn_lq", "box_head"))
@pytest.mark.parametrize("batched", (False, True), ids=("shared", "batched"))
def test_match_boxes_with_changing_valid_ground_truth(batched, thresholds):
    """_C.match_boxes at the smallest random case of tests/target_cases.py (M = 256 ground-truth rows, K = 1023 boxes, N = 2)
    against the torch Matcher, bit for bit.  The kernel zeroes its per-gt `best` words before it raises them: the valid mask
    goes from all rows to one row per image to none, so a word left over from the capture would show as a low-quality match."""
    C_ = _C()
    hi, lo, lq = thresholds
    sets = _matcher_sets(batched)
    one = tc.matcher_case("1x1", batched, thresholds)
    og, ov, ob = _t(one["gt"]), _t(one["valid"]), _t(one["boxes"])
    refs = [tc.matcher_reference(g, v, b, hi, lo, lq) for g, v, b in sets]
    assert int((refs[0] >= 0).sum()) > 10 and int((refs[1] >= 0).sum()) > 0 and int((refs[2] >= 0).sum()) == 0
    check_replay(lambda g, v, b: C_.match_boxes(g, v, b, hi, lo, lq), sets,
                 expect=lambda v: tc.matcher_reference(_np(v[0]), _np(v[1]), _np(v[2]), hi, lo, lq),
                 between=lambda: C_.match_boxes(og, ov, ob, hi, lo, lq))


def test_match_labels_replayed():
    """_C.match_labels (1 x 255: one element short of a block) against the numpy restatement, int64 and float32 labels"""
    C_ = _C()
    c = tc.labels_case(1, 255)
    m1 = np.abs(c["matched"]) % c["gt_labels"].shape[1]
    sets = [(c["matched"], c["gt_labels"], c["valid"]),
            (m1, c["gt_labels"][:, ::-1].copy(), np.ones_like(c["valid"])),            # everything matched and valid
            (c["matched"], c["gt_labels"], np.zeros_like(c["valid"]))]                 # nothing valid: all -1
    other = tc.labels_case(2, 128)
    om, ol = _t(other["matched"]), _t(other["gt_labels"])
    for dtype, npdt in ((torch.int64, np.int64), (torch.float32, np.float32)):
        check_replay(lambda m, gl, v: C_.match_labels(m, gl, v, dtype), sets,
                     expect=lambda v: tc.match_labels_reference(_np(v[0]), _np(v[1]), _np(v[2]), npdt),
                     between=lambda: C_.match_labels(om, ol, None, dtype))


def _slots_reference(boxes, matched, gt, gl, valid, idx, slot_valid, obj, weights):
    """the reference of tc.slots_case for other values of the same shapes"""
    N, K = matched.shape
    M = gt.shape[1]
    sel = np.clip(idx, 0, K - 1)
    rows = np.arange(N)[:, None]
    m = matched[rows, sel]
    labels = tc.match_labels_reference(matched, gl, valid, np.int64)[rows, sel]
    labels[~slot_valid] = -1
    reg = tc.encode64(torch.from_numpy(gt[rows, np.clip(m, 0, M - 1)]), torch.from_numpy(boxes[rows, sel]), weights).numpy()
    return boxes[rows, sel], labels, reg, m, obj[rows, sel]


def test_roi_head_targets_replayed():
    """_C.roi_head_targets (N = 1, B = 255 slots) against the restatement: copied boxes, labels, matched rows and
    objectness bit for bit, the encoded regression targets within BOUNDS["roi_head_targets"] of fp64 (test_targets_edges_gpu).
    The slots' validity changes from most to none to all between the replays."""
    from test_targets_edges_gpu import BOUNDS
    C_ = _C()
    c = tc.slots_case(1, 255, True, True)
    w = c["weights"]
    base = (c["boxes"], c["matched"], c["gt"], c["gt_labels"], c["valid"], c["idx"], c["slot_valid"], c["objectness"])
    rng = np.random.RandomState(3)
    sets = [base,
            base[:5] + (rng.randint(0, 300, c["idx"].shape).astype(np.int64), np.zeros_like(c["slot_valid"]), base[7]),
            (base[0][:, ::-1].copy(), base[1], base[2], base[3], np.ones_like(c["valid"]), base[5], np.ones_like(c["slot_valid"]),
             base[7])]
    ref0 = _slots_reference(*[_np(v) for v in sets[0]], w)
    for a, b in zip(ref0, c["ref"]):
        assert np.array_equal(a, b)              # the restatement above IS the one of target_cases
    o = tc.slots_case(2, 128, True, True)
    oa = [_t(o[k]) for k in ("boxes", "matched", "gt", "gt_labels", "valid", "idx", "slot_valid", "objectness")]

    def tol(got, want, what):
        rb, rl, rreg, rm, ro = want
        assert_bits((got[0], got[1], got[3], got[4]), (rb, rl, rm, ro), what)
        err = tc.grad_err(_np(got[2]), rreg)
        assert err <= BOUNDS["roi_head_targets"][1], (what, err)

    check_replay(lambda *a: C_.roi_head_targets(*a, w), sets, expect=lambda v: _slots_reference(*[_np(x) for x in v], w), tol=tol,
                 between=lambda: C_.roi_head_targets(*oa, w))


def test_mask_targets_replayed():
    """_C.mask_targets (5 x 7 masks, nine edge boxes twice, M = 14) against project_masks_on_boxes on the CPU, bit for bit"""
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.loss import project_masks_on_boxes
    C_ = _C()
    c = tc.mask_case(5, 7)
    masks = c["masks"][torch.uint8]
    sets = [(masks, c["index"], c["boxes"]),
            (1 - masks, c["index"][::-1].copy(), c["boxes"] + np.float32(0.5)),
            (torch.zeros_like(masks), c["index"], c["boxes"])]
    o = tc.mask_case(33, 20)
    om, oi, ob = o["masks"][torch.uint8].to(DEV), _t(o["index"]), _t(o["boxes"])
    check_replay(lambda m, i, b: C_.mask_targets(m, i, b, 14), sets,
                 expect=lambda v: project_masks_on_boxes(v[0], v[1], v[2], 14),
                 between=lambda: C_.mask_targets(om, oi, ob, 28))


def test_rpn_decode_at_non_zero_col_and_off():
    """_C.rpn_decode (3 images, A = 3, 7 x 9: every anchor is a candidate, min_size 24 removes many) written at col = 3 /
    off = 5 into NaN-filled results, against RPNPostProcessor._level_candidates on the same device, bit for bit, guard bands
    included.  The image sizes live in a device tensor: they change between the replays and with them the clipped boxes and
    the rows under min_size."""
    C_ = _C()
    c = tc.decode_case("all_candidates_min_size")
    post, col, off = c["post"], c["col"], c["off"]
    anchors = c["anchors"].to(DEV)
    N, A, H, W = c["obj"].shape
    k = min(post.pre_nms_top_n, A * H * W)
    K, R = col + k + 2, off + N * k + 3
    g = torch.Generator().manual_seed(5)
    sizes = [list(c["sizes"]), [(40, 60)] * N, [(H * 32, W * 32)] * N]
    sets = [(c["reg"], c["obj"], torch.tensor(sizes[0], dtype=torch.float32)),
            (torch.randn(c["reg"].shape, generator=g) * 0.3, torch.randn(c["obj"].shape, generator=g), torch.tensor(sizes[1], dtype=torch.float32)),
            (torch.zeros_like(c["reg"]), c["obj"].flip(0), torch.tensor(sizes[2], dtype=torch.float32))]
    nan = float("nan")

    def fn(reg, obj, hw):
        s, idx = obj.permute(0, 2, 3, 1).reshape(N, -1).sigmoid().topk(k, dim=1, sorted=True)
        ob, os_ = torch.full((N, K, 4), nan, device=DEV), torch.full((N, K), nan, device=DEV)
        nb, ns = torch.full((R, 4), nan, device=DEV), torch.full((R,), nan, device=DEV)
        okk = torch.full((R,), 7, dtype=torch.uint8, device=DEV)
        C_.rpn_decode(reg, idx, s, anchors, hw, post.box_coder.weights, post.box_coder.bbox_xform_clip, c["min_size"],
                      ob, os_, col, nb, ns, okk, off)
        return ob, os_, nb, ns, okk

    def expect(v):
        sz = [(int(h), int(w)) for h, w in v[2].tolist()]
        boxes, scores, ok = post._level_candidates(anchors, v[1].to(DEV), v[0].to(DEV), sz)
        ob, os_ = torch.full((N, K, 4), nan, device=DEV), torch.full((N, K), nan, device=DEV)
        nb, ns = torch.full((R, 4), nan, device=DEV), torch.full((R,), nan, device=DEV)
        okk = torch.full((R,), 7, dtype=torch.uint8, device=DEV)
        ob[:, col:col + k], os_[:, col:col + k] = boxes, scores
        flat = ok.reshape(-1)
        far = torch.tensor([-1e6, -1e6, -1e6 + 1, -1e6 + 1], device=DEV)
        nb[off:off + N * k] = torch.where(flat[:, None], boxes.reshape(-1, 4), far)
        ns[off:off + N * k] = torch.where(flat, scores.reshape(-1), scores.new_full((), -1.0))
        okk[off:off + N * k] = flat.to(torch.uint8)
        return ob, os_, nb, ns, okk

    kept = [int(expect(v)[4][off:off + N * k].sum()) for v in sets]
    assert 0 < kept[0] < N * k and len(set(kept)) >= 2, kept
    check_replay(fn, sets, expect=expect)


def test_sample_labels_draws_a_new_stream_on_every_replay():
    """_C.sample_labels (case n255: 255 labels, 8 per image, at most 2 positives) under a GRAPH_SEED word that the captured
    function increments first, as GraphedTrainStep._iteration does.  The word of the graph persists from replay to replay:
    replay i must equal the restatement at word i + 1 (tc.sampler_reference), with more positives than the quota, then
    fewer, then none.  Eager calls count on a word of their own that starts one lower (the eager warm-up call takes one),
    so the eager call after replay i draws the same stream from another address."""
    C_ = _C()
    c = tc.sampler_case("n255")
    lab0 = c["labels"]
    pos = np.nonzero(lab0[0] >= 1)[0]
    assert len(pos) > c["max_pos"]
    lab1, lab2 = lab0.copy(), lab0.copy()
    lab1[0, pos[1:]] = 0                          # one positive: fewer than the quota of 2
    lab2[0, pos] = 0                              # none
    sets = [(lab0,), (lab1,), (lab2,)]
    words = {True: torch.zeros(1, dtype=torch.int64, device=DEV), False: torch.full((1,), -1, dtype=torch.int64, device=DEV)}

    def fn(labels):
        w = words[bool(torch.cuda.is_current_stream_capturing())]
        w.add_(1)
        C_.GRAPH_SEED = w
        try:
            return C_.sample_labels(labels, c["B"], c["max_pos"], with_list=True, seed=c["seed"])
        finally:
            C_.GRAPH_SEED = None

    other = _t(tc.sampler_case("n5")["labels"])
    got = check_replay(fn, sets, between=lambda: C_.sample_labels(other, 4, 4, with_list=True, seed=3))
    order = [0, 1, 2, 0, 0]
    assert int(words[True]) == len(order) and int(words[False]) == len(order)      # (-1, the warm-up call, one call per replay)
    for i, (k, g) in enumerate(zip(order, got)):
        ref = tc.sampler_reference(sets[k][0], c["B"], c["max_pos"], c["seed"], word=i + 1)
        assert_bits(g, ref, "replay %d against the restatement at word %d" % (i, i + 1))
    assert not bits_equal(got[0][2], got[3][2]) and not bits_equal(got[3][2], got[4][2])     # same labels, a new stream


# ============================================================================ losses with their gradients
def _figure(kernel, what, value, grad):
    from test_targets_edges_gpu import BOUNDS
    print("FIGURE %-14s %-40s value %-10s grad %s" % (kernel, what, "-" if value is None else "%.3g" % value, "%.3g" % grad))
    vb, gb = BOUNDS[kernel]
    assert value is None or value <= vb, (kernel, what, "value", value)
    assert grad <= gb, (kernel, what, "grad", grad)


def test_rpn_loss_with_changing_sampled_anchors():
    """_C.rpn_loss forward + backward (eight uneven levels, N = 2, A = 3) against fp64 autograd within BOUNDS["rpn_loss"]
    (test_targets_edges_gpu), and bit-equal to eager.  Value sets: the `eight_levels` case, `nothing_sampled` (both
    losses and every gradient exactly zero) and `negatives_only` (box loss and box gradients exactly zero).  The capture
    bakes the code weights of `eight_levels`; the two other references do not depend on them (no positive row)."""
    C_ = _C()
    cases = [tc.rpn_loss_case(n) for n in ("eight_levels", "nothing_sampled", "negatives_only")]
    L = len(cases[0]["obj"])
    beta, weights = cases[0]["beta"], cases[0]["weights"]
    sets = _tensors([tuple(c["obj"]) + tuple(c["box"]) + (c["anchors"], c["matched"], c["pos"], c["neg"], c["gt"]) for c in cases])
    refs = {id(s[0]): c["ref"] for s, c in zip(sets, cases)}
    one = tc.rpn_loss_case("single_anchor")
    oa = [[_t(t) for t in one["obj"]], [_t(t) for t in one["box"]]] + [_t(one[k]) for k in ("anchors", "matched", "pos", "neg", "gt")]

    def fn(*a):
        obj = [t.detach().requires_grad_() for t in a[:L]]
        box = [t.detach().requires_grad_() for t in a[L:2 * L]]
        lo, lb = C_.rpn_loss(obj, box, *a[2 * L:], beta, weights)
        return (lo, lb) + torch.autograd.grad(tc.RPN_UPSTREAM[0] * lo + tc.RPN_UPSTREAM[1] * lb, obj + box)

    def tol(got, want, what):
        ro, rb, rgo, rgb = want
        lo, lb = float(got[0]), float(got[1])
        grads = [_np(g) for g in got[2:]]
        if ro == 0.0:
            assert lo == 0.0 and lb == 0.0 and all(not g.any() for g in grads), what
            return
        if rb == 0.0:
            assert lb == 0.0 and all(not g.any() for g in grads[L:]), what
        value = tc.rel_err(lo, ro) if rb == 0.0 else max(tc.rel_err(lo, ro), tc.rel_err(lb, rb))
        _figure("rpn_loss", what, value, tc.grad_err(grads, rgo + rgb))

    assert cases[1]["ref"][0] == 0.0 and cases[2]["ref"][1] == 0.0 and cases[0]["ref"][1] != 0.0
    check_replay(fn, sets, expect=lambda v: refs[id(v[0])], tol=tol,
                 between=lambda: C_.rpn_loss(*oa, one["beta"], one["weights"]))


def test_fastrcnn_loss_with_changing_sampled_rows():
    """_C.fastrcnn_loss forward + backward (R = 9, C = 65, beta = 1 / 9) against fp64 autograd within BOUNDS["fastrcnn_loss"],
    and bit-equal to eager: the case's labels, then every row unsampled (-1: losses and gradients exactly zero), then every
    row background (sampled, no positive: box loss and box gradient exactly zero)"""
    C_ = _C()
    R, C, agnostic, beta, scale = tc.FASTRCNN_CASES[3]
    c = tc.fastrcnn_case(R, C, agnostic, beta, scale)
    labels = [c["labels"], np.full_like(c["labels"], -1), np.zeros_like(c["labels"])]
    sets = [(c["logits"], c["box"] if i != 2 else -c["box"], lab, c["targets"]) for i, lab in enumerate(labels)]
    o = tc.fastrcnn_case(*tc.FASTRCNN_CASES[1])
    oa = [_t(o[k]) for k in ("logits", "box", "labels", "targets")]

    def fn(logits, box, lab, targets):
        fl, fb = logits.detach().requires_grad_(), box.detach().requires_grad_()
        lc, lb = C_.fastrcnn_loss(fl, fb, lab, targets, agnostic, beta)
        return (lc, lb) + torch.autograd.grad(tc.HEAD_UPSTREAM[0] * lc + tc.HEAD_UPSTREAM[1] * lb, (fl, fb))

    def tol(got, want, what):
        rc_, rr, rgl, rgb = want
        lc, lb, gl, gb = float(got[0]), float(got[1]), _np(got[2]), _np(got[3])
        if rc_ == 0.0:
            assert lc == 0.0 and lb == 0.0 and not gl.any() and not gb.any(), what
            return
        if rr == 0.0:
            assert lb == 0.0 and not gb.any(), what
        value = tc.rel_err(lc, rc_) if rr == 0.0 else max(tc.rel_err(lc, rc_), tc.rel_err(lb, rr))
        _figure("fastrcnn_loss", what, value, tc.grad_err([gl, gb], [rgl, rgb]))

    expect = lambda v: tc.fastrcnn_reference(_np(v[0]), _np(v[1]), _np(v[2]), _np(v[3]), agnostic, beta, tc.HEAD_UPSTREAM)  # noqa: E731
    assert expect(sets[1])[0] == 0.0 and expect(sets[2])[1] == 0.0 and expect(sets[2])[0] > 0.0
    check_replay(fn, sets, expect=expect, tol=tol, between=lambda: C_.fastrcnn_loss(*oa, tc.FASTRCNN_CASES[1][2], tc.FASTRCNN_CASES[1][3]))


def test_mask_loss_with_and_without_positives():
    """_C.mask_loss forward + backward (P = 5, C = 9, M = 17, logits up to +-160) against fp64 autograd within
    BOUNDS["mask_loss"], and bit-equal to eager: the case's labels, then no positive row (loss and gradient exactly zero)"""
    C_ = _C()
    P, C, M, scale = tc.MASK_LOSS_CASES[3]
    cases = [tc.mask_loss_case(P, C, M, scale), tc.mask_loss_case(P, C, M, scale, no_positives=True)]
    sets = _tensors([(c["logits"], c["labels"], c["targets"]) for c in cases])
    refs = {id(s[1]): c["ref"] for s, c in zip(sets, cases)}
    o = tc.mask_loss_case(*tc.MASK_LOSS_CASES[1])
    oa = [_t(o[k]) for k in ("logits", "labels", "targets")]

    def fn(logits, lab, targets):
        x = logits.detach().requires_grad_()
        loss = C_.mask_loss(x, lab, targets)
        return (loss,) + torch.autograd.grad(tc.MASK_UPSTREAM * loss, (x,))

    def tol(got, want, what):
        rl, rg = want
        if rl == 0.0:
            assert float(got[0]) == 0.0 and not _np(got[1]).any(), what
            return
        _figure("mask_loss", what, tc.rel_err(float(got[0]), rl), tc.grad_err(_np(got[1]), rg))

    assert cases[0]["ref"][0] > 0.0 and cases[1]["ref"][0] == 0.0
    check_replay(fn, sets, expect=lambda v: refs[id(v[1])], tol=tol, between=lambda: C_.mask_loss(*oa))


def test_keypoint_loss_with_changing_valid_rows():
    """_C.keypoint_loss forward + backward (P = 8, K = 17, 56 x 56) against fp64 cross-entropy within the 1e-5 relative of
    test_keypoint_gpu.test_loss_kernel_value_and_gradient (upstream 2.5), and bit-equal to eager: 70 % of the rows valid,
    none (loss and gradient exactly zero), all"""
    from test_keypoint_gpu import _fp64_reference, _loss_inputs
    C_ = _C()
    sets = [_loss_inputs(P=8, seed=s, frac=f) for s, f in ((0, 0.7), (1, 0.0), (2, 1.0))]
    assert int(sets[1][2].sum()) == 0 and bool(sets[2][2].all())
    o = [t.to(DEV) for t in _loss_inputs(P=3, K=5, M=7, seed=4)]

    def fn(logits, heat, valid):
        x = logits.detach().requires_grad_()
        loss = C_.keypoint_loss(x, heat, valid)
        return (loss,) + torch.autograd.grad(loss * 2.5, (x,))

    def tol(got, want, what):
        ref, ref_g = want
        g = got[1].cpu().double()
        if ref == 0.0:
            assert float(got[0]) == 0.0 and bool(torch.all(g == 0)), what
            return
        assert abs(float(got[0]) - ref) <= 1e-5 * abs(ref), what
        assert (g - 2.5 * ref_g).abs().max() <= 1e-5 * (2.5 * ref_g).abs().max(), what

    check_replay(fn, sets, expect=lambda v: _fp64_reference(*v), tol=tol, between=lambda: C_.keypoint_loss(*o))


def test_rpn_head_sparse_with_changing_sampled_anchors(monkeypatch):
    """_C.rpn_head_sparse (the whole RPN head as one autograd node, max_rows = N x 48) + _C.rpn_loss, forward + backward, at
    the reduced shape of test_rpn_sparse_bwd_gpu (N = 2, C = 32, five levels from 40 x 56).  The sampled anchors go from the
    sampler's full quota to a handful to none: the backward rebuilds its row list from the gradients on every replay.
    Criterion of that test: the head outputs and every gradient within GRAD_TOL (relative Frobenius, floored) of fp64
    autograd of the dense composition on the CPU, fed with the loss kernel's gradients on the replayed outputs.  The library
    convolutions of the forward add with atomics, so eager-vs-replay bits are not asked.  rpn_sparse_overflows stays 0."""
    from test_rpn_sparse_bwd_gpu import A, _inputs, _loss_grads
    from test_whole_model_parity import GRAD_TOL, _grad_spread
    C_ = _C()
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    N, C, B = 2, 32, 48
    levels = [(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)]
    L = len(levels)
    p, feats, anchors, gt, matched, pos, neg = _inputs(C, levels, N, B, seed=9)
    names = list(p)
    params = [p[k].to(DEV).requires_grad_() for k in names]
    for t in (params[0], params[2], params[4]):
        assert t.dim() == 4
    few_p, few_n = pos.clone(), neg.clone()
    few_p[:, 3000:], few_n[:, 3000:] = False, False
    masks = [(pos, neg), (few_p, few_n), (torch.zeros_like(pos), torch.zeros_like(neg))]
    counts = [int((a | b).sum()) for a, b in masks]
    assert counts[0] == N * B and 0 < counts[1] < counts[0] and counts[2] == 0, counts
    g = torch.Generator().manual_seed(3)
    sets = [tuple(f if i == 0 else torch.randn(f.shape, generator=g) for f in feats) + (a.cpu(), b.cpu())
            for i, (a, b) in enumerate(masks)]
    sets = [tuple(t.contiguous(memory_format=CL) if t.dim() == 4 else t for t in s) for s in sets]

    def fn(*a):
        xs = [t.detach().requires_grad_() for t in a[:L]]
        obj, box = C_.rpn_head_sparse(xs, *params, N * B)
        lo, lb = C_.rpn_loss(obj, box, anchors, matched, a[L], a[L + 1], gt, 1.0 / 9, (1.0, 1.0, 1.0, 1.0))
        return tuple(obj) + tuple(box) + torch.autograd.grad(1.3 * lo + 0.7 * lb, params + xs)

    def tol(got, want, what):
        xs64, pos_, neg_ = want
        outs = [o.detach() for o in got[:2 * L]]
        grads = [t.double().cpu() for t in _loss_grads(outs, (anchors, gt, matched, pos_.to(DEV), neg_.to(DEV)))]
        pp = {k: v.detach().double().cpu().requires_grad_() for k, v in zip(names, params)}
        xs = [x.clone().requires_grad_() for x in xs64]
        ts = [F.relu(F.conv2d(x, pp["conv.weight"], pp["conv.bias"], padding=1)) for x in xs]
        ref_outs = [F.conv2d(t, pp["cls_logits.weight"], pp["cls_logits.bias"]) for t in ts] + \
                   [F.conv2d(t, pp["bbox_pred.weight"], pp["bbox_pred.bias"]) for t in ts]
        fwd = _grad_spread({str(i): o.double().cpu() for i, o in enumerate(outs)}, {str(i): o.detach() for i, o in enumerate(ref_outs)})
        assert max(fwd.values()) <= GRAD_TOL, (what, "head outputs", fwd)
        torch.autograd.backward(ref_outs, grads)
        ref = {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in pp.items()}
        ref.update({"x%d" % i: (x.grad if x.grad is not None else torch.zeros_like(x)) for i, x in enumerate(xs)})
        mine = dict(zip(names + ["x%d" % i for i in range(L)], [t.double().cpu() for t in got[2 * L:]]))
        if not any(float(g_.abs().max()) for g_ in grads):          # nothing sampled: every gradient is exactly zero
            assert all(not bool(v.any()) for v in mine.values()), what
            return
        spread = _grad_spread(mine, ref)
        print("%s: %s" % (what, {k: "%.3g" % v for k, v in spread.items()}))
        assert max(spread.values()) <= GRAD_TOL, (what, spread)

    C_.rpn_sparse_overflows(reset=True)
    check_replay(fn, sets, expect=lambda v: ([t.double() for t in v[:L]], v[L], v[L + 1]), tol=tol, eager_bits=False)
    assert C_.rpn_sparse_overflows() == 0


# ============================================================================ layout kernels
def _rounded(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _fmt(t, nhwc):
    return t.contiguous(memory_format=CL) if nhwc else t.contiguous()


def _layout_sets(shape, dtype, nhwc, seed, n_tensors):
    """random values; values that make every pre-activation negative (x far below zero, residual below zero); one NaN"""
    rnd = [_rounded(shape, dtype, seed + i, 2.0 if i == 0 else 1.0) for i in range(n_tensors)]
    neg = [(-(t.float().abs()) - (100.0 if i == 0 else 0.0)).to(dtype) for i, t in enumerate(rnd)]
    neg[-1] = rnd[-1]                             # (the last tensor is the upstream gradient)
    nan = [t.clone() for t in rnd]
    nan[0].view(-1)[5] = float("nan")
    return [tuple(_fmt(t, nhwc) for t in s) for s in (rnd, neg, nan)]


LAYOUT_SHAPES = [((2, 64, 5, 7), True), ((2, 12, 9, 3), True), ((2, 12, 5, 7), False), ((2, 64, 9, 3), False)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("shape,nhwc", LAYOUT_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("nhwc" if v else "nchw"))
def test_frozen_bn_forward_and_backward(shape, nhwc, relu, res, dtype):
    """_C.frozen_bn_act_forward + _C.frozen_bn_act_backward, both layouts, with and without residual and ReLU, fp32 and bf16,
    N = 2 at 5 x 7 and 9 x 3: equal to the fp32 CPU composition with one rounding (the reference of
    test_layout_kernels_gpu._frozen_bn_check; NaN kept like torch.relu / aten.threshold_backward), bit-equal to eager.  The second
    value set makes every pre-activation negative: an empty ReLU mask."""
    C_ = _C()
    Cc = shape[1]
    g = torch.Generator().manual_seed(Cc)
    scale, bias = torch.rand(Cc, generator=g) * 0.7 + 0.1, torch.randn(Cc, generator=g)
    sd, bd = scale.to(DEV), bias.to(DEV)
    sets = _layout_sets(shape, dtype, nhwc, 11, 3)
    ox = _fmt(torch.randn(1, 8, 3, 3, device=DEV).to(dtype), nhwc)

    def fn(x, r, gy):
        y = C_.frozen_bn_act_forward(x, sd, bd, r if res else None, relu)
        gx, gr = C_.frozen_bn_act_backward(gy, y if relu else None, sd, relu, res)
        return y, gx, gr

    def expect(v):
        x, r, gy = v
        t = x.float() * scale.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1)
        if res:
            t = t + r.float()
        want = (torch.relu(t) if relu else t).to(dtype)
        m = torch.ops.aten.threshold_backward(gy.float(), want.float(), 0) if relu else gy.float()
        return want, (m * scale.view(1, -1, 1, 1)).to(dtype), (m.to(dtype) if res else None)

    def tol(got, want, what):
        for i, name in enumerate(("y", "grad_x", "grad_residual")):
            assert (got[i] is None) == (want[i] is None)
            if want[i] is not None:
                _exact_nan(got[i], want[i], "%s %s" % (what, name))

    if relu:
        assert not bool(expect(sets[1])[0].any()) and not bool(expect(sets[1])[1].any())
    check_replay(fn, sets, expect=expect, tol=tol,
                 between=lambda: C_.frozen_bn_act_forward(ox, torch.ones(8, device=DEV), torch.zeros(8, device=DEV), None, True))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", [(2, 256, 5, 7), (2, 12, 9, 3)], ids=["C256_fused", "C12_column_sum"])
def test_bias_act_forward_and_backward(shape, relu, dtype, monkeypatch):
    """_C.bias_act through autograd on channels-last activations: C = 256 takes the fused kernels (forward, and the backward
    with its partial-sum workspace), C = 12 the in-place add and `column_sum`; checked with the entry points the calls make.
    Reference of tests/torch_refs.check_fused_relu_non_finite: forward and grad_x equal the fp32 composition, the bias gradient
    is within n * 2^-24 * sum |terms| of the fp64 column sum; everything bit-equal to eager.  With every pre-activation
    negative the ReLU mask is empty and the bias gradient exactly zero."""
    from test_layout_kernels_gpu import _EntrySpy
    C_ = _C()
    spy = _EntrySpy(C_.lib)
    monkeypatch.setattr(C_, "lib", spy)
    Cc = shape[1]
    fused = Cc == 256
    b = torch.randn(Cc, generator=torch.Generator().manual_seed(2))
    bd = b.to(DEV).requires_grad_()
    sets = _layout_sets(shape, dtype, True, 21, 2)
    ox = _fmt(torch.randn(1, 8, 3, 3, device=DEV).to(dtype), True)
    ob = torch.zeros(8, device=DEV)

    def fn(x, gy):
        xd = x.detach().requires_grad_()
        y = C_.bias_act(xd.clone(memory_format=CL), bd, relu)
        return (y,) + torch.autograd.grad(y, (xd, bd), gy)

    def expect(v):
        x, gy = v
        bias_as = b if fused else b.to(dtype).float()       # (the generic path adds the bias in the activation's dtype)
        want = x.float() + bias_as.view(1, -1, 1, 1)
        want = (torch.relu(want) if relu else want).to(dtype)
        m = torch.ops.aten.threshold_backward(gy.float(), want.float(), 0) if relu else gy.float()
        return want, m.to(dtype), m.double()

    def tol(got, want, what):
        _exact_nan(got[0], want[0], what + " y")
        _exact_nan(got[1], want[1], what + " grad_x")
        terms = want[2]
        if bool(terms.isnan().any()):
            return
        colsum, bound = terms.sum((0, 2, 3)), terms[:, 0].numel() * 2.0 ** -24 * terms.abs().sum((0, 2, 3))
        gb = got[2].cpu().double()
        assert bool(((gb - colsum).abs() <= bound).all()), (what, "grad_bias", gb, colsum)

    if relu:
        assert not bool(expect(sets[1])[2].any())
    check_replay(fn, sets, expect=expect, tol=tol, between=lambda: C_.bias_act(ox.clone(memory_format=CL), ob, relu))
    assert ("detops_bias_act_backward_nhwc" in spy.calls) == fused and ("detops_column_sum" in spy.calls) == (not fused), set(spy.calls)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("relu,res", [(False, False), (True, True)])
@pytest.mark.parametrize("shape", [(2, 64, 32, 5, 7), (2, 6, 3, 9, 3), (2, 3, 3, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_group_norm_forward_and_backward(shape, relu, res, dtype):
    """_C.group_norm_forward + _C.group_norm_backward (partial sums through the workspace), one (C, G) per vector width that
    group_norm_serves accepts: C = 64 (vectors of 4 fp32 / 8 bf16), C = 6 (2), C = 3 (1).  gamma and beta are inputs: the second
    value set (beta = -50, gamma = 0.1, residual below zero) makes every pre-activation negative.  Bit-equal to eager (the
    eager test asserts both passes deterministic); on the finite value sets the checks of test_group_norm_gpu._run: statistics,
    output bound, backward within 8 x ATen's own fp32 error of fp64."""
    import test_group_norm_gpu as gn
    C_ = _C()
    N, Cc, G, H, W = shape
    assert C_.group_norm_serves(Cc, G)
    base = _layout_sets((N, Cc, H, W), dtype, True, 31, 3)
    g = torch.Generator().manual_seed(Cc)
    gamma, beta = torch.randn(Cc, generator=g) + 1.0, torch.randn(Cc, generator=g)
    affine = [(gamma, beta), (torch.full((Cc,), 0.1), torch.full((Cc,), -50.0)), (gamma, beta)]
    sets = [s[:2] + a + s[2:] for s, a in zip(base, affine)]
    sets[1] = (base[0][0],) + sets[1][1:]         # ordinary activations; the affine part and the residual make them negative
    ox = _fmt(torch.randn(1, 8, 3, 3, device=DEV).to(dtype), True)

    def fn(x, r, ga, be, gy):
        y, mean, rstd = C_.group_norm_forward(x, G, ga, be, gn.EPS, r if res else None, relu)
        return (y, mean, rstd) + tuple(C_.group_norm_backward(gy, x, y, G, ga, mean, rstd, relu, res, True, True))

    def tol(got, want, what):
        x, r, ga, be, gy = want
        if bool(x.isnan().any()):
            return
        ga, be = ga.clone(), be.clone()          # (the host reference marks the tensors it is given as requiring a gradient)
        y, mean, rstd = got[:3]
        r = r if res else None
        gn._check_statistics(x, mean, rstd, G)
        gn._check_output(x, r, ga, be, y, mean, rstd, G, relu, dtype)
        masked = gy.double() * (y.cpu() > 0).double() if relu else gy.double()
        ref = gn._host_backward(x, r, ga, be, masked, G, torch.float64)
        aten = gn._host_backward(x, r, ga, be, masked, G, torch.float32)
        floor = 0.0 if dtype == torch.float32 else torch.finfo(dtype).eps
        for name, mine in zip(("grad_x", "grad_residual", "grad_gamma", "grad_beta"), got[3:]):
            if ref[name] is None:
                assert mine is None
                continue
            if not bool(ref[name].any()):
                assert not bool(mine.any()), (what, name, "exactly zero")
                continue
            err, theirs = gn._rel(mine.cpu(), ref[name]), gn._rel(aten[name], ref[name])
            assert err <= max(8 * theirs, floor), (what, name, err, theirs)

    if relu:
        y1 = F.group_norm(sets[1][0].float(), G, sets[1][2], sets[1][3], gn.EPS) + sets[1][1].float()
        assert float(y1.max()) < 0
    check_replay(fn, sets, expect=lambda v: v, tol=tol,
                 between=lambda: C_.group_norm_forward(ox, 2, None, None, gn.EPS, None, False))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("C,H,W,h,w", [(12, 5, 7, 3, 4), (64, 9, 3, 5, 2)])
def test_fpn_topdown_forward_and_backward(C, H, W, h, w, nhwc, dtype):
    """_C.fpn_topdown through autograd (lateral 5 x 7 from 3 x 4, 9 x 3 from 5 x 2, N = 2), both layouts, fp32 and bf16: the forward
    equals the fp32 composition with one rounding, grad_lateral is the upstream gradient, grad_top is within the block-sum bound
    of test_layout_kernels_gpu._topdown_check of the fp64 adjoint; everything bit-equal to eager"""
    from test_layout_kernels_gpu import U32, _adjoint64, _ulp
    C_ = _C()
    N = 2
    sets = []
    for i in range(3):
        lat, top, g = _rounded((N, C, H, W), dtype, 40 + i), _rounded((N, C, h, w), dtype, 50 + i), _rounded((N, C, H, W), dtype, 60 + i)
        if i == 1:
            lat, top = (-lat.float().abs() - 100).to(dtype), (-top.float().abs()).to(dtype)
        if i == 2:
            top.view(-1)[3] = float("nan")
        sets.append(tuple(_fmt(t, nhwc) for t in (lat, top, g)))
    oa, ob = _fmt(torch.randn(1, 8, 4, 4, device=DEV).to(dtype), nhwc), _fmt(torch.randn(1, 8, 2, 2, device=DEV).to(dtype), nhwc)

    def fn(lat, top, g):
        a, b = lat.detach().requires_grad_(), top.detach().requires_grad_()
        out = C_.fpn_topdown(a, b)
        return (out,) + torch.autograd.grad(out, (a, b), g)

    def tol(got, want, what):
        lat, top, g = want
        _exact_nan(got[0], (lat.float() + F.interpolate(top.float(), size=(H, W), mode="nearest")).to(dtype), what + " forward")
        assert bits_equal(got[1], g), what + " grad_lateral: " + first_difference(got[1], g)
        ref = _adjoint64(g, h, w)
        k = float(_adjoint64(torch.ones(1, 1, H, W), h, w).max())
        bound = k * U32 * _adjoint64(g.abs(), h, w)
        if dtype != torch.float32:
            bound = bound + _ulp(ref, dtype)
        err = (got[2].cpu().double() - ref).abs()
        assert bool((err <= bound).all()), "%s grad_top: max err %g" % (what, float(err.max()))

    check_replay(fn, sets, expect=lambda v: v, tol=tol, between=lambda: C_.fpn_topdown(oa, ob))


# ============================================================================ focal loss
@pytest.mark.parametrize("C", [80, 7], ids=["C80_vector", "C7_scalar"])
def test_focal_loss_sum_and_scalar_backward(C):
    """_C.sigmoid_focalloss_forward_sum + _C.sigmoid_focalloss_backward_scalar at R = 37: C = 80 takes the float4 kernels
    (csrc/focal_loss.hip launch: C % 4 == 0 and 16-byte aligned pointers), C = 7 the scalar ones.  Targets all background, all
    one class, mixed (ignored rows included), logits up to |x| = 100.  Reference: the oracle,
    within the rtol 1e-4 / atol 1e-6 per element of test_focal_vs_oracle_and_golden (summed over the elements for the sum).  The
    forward is the two-stage fixed-order reduction (test_focal_model_entry_points_vs_oracle_full_size asserts it bit-reproducible)
    and the backward is elementwise: both are compared with eager in bits."""
    C_ = _C()
    R, gamma, alpha = 37, 2.0, 0.25
    sets = []
    for i, kind in enumerate(("background", "one_class", "mixed")):
        rng = np.random.RandomState(70 + i)
        logits = np.clip(rng.randn(R, C) * 40, -100, 100).astype(np.float32)
        logits[0, :4], logits[R - 1, C - 1] = (-100, 100, 0, -0.0), 100
        if kind == "background":
            targets = np.zeros(R, np.int32)
        elif kind == "one_class":
            targets = np.full(R, 3, np.int32)
        else:
            targets = rng.randint(-1, C + 1, R).astype(np.int32)
            targets[:4] = (1, C, -1, 0)
        sets.append((logits, targets))
    one = torch.ones((), device=DEV)
    ol, ot = synth.focal_inputs(50, 12)
    ol, ot = _t(ol), _t(ot)

    def fn(logits, targets):
        return (C_.sigmoid_focalloss_forward_sum(logits, targets, C, gamma, alpha),
                C_.sigmoid_focalloss_backward_scalar(logits, targets, one, C, gamma, alpha))

    def expect(v):
        logits, targets = _np(v[0]), _np(v[1])
        return (oracle.sigmoid_focal_loss_forward(logits, targets, gamma, alpha).astype(np.float64),
                oracle.sigmoid_focal_loss_backward(logits, targets, np.ones_like(logits), gamma, alpha))

    def tol(got, want, what):
        losses, d = want
        assert abs(float(got[0]) - losses.sum()) <= (1e-6 + 1e-4 * np.abs(losses)).sum(), (what, float(got[0]), losses.sum())
        np.testing.assert_allclose(_np(got[1]), d, rtol=1e-4, atol=1e-6, err_msg=what)

    check_replay(fn, sets, expect=expect, tol=tol, between=lambda: C_.sigmoid_focalloss_forward_sum(ol, ot, 12, gamma, alpha))


# ============================================================================ deformable conv
def _dcn_offsets(kind, B, k, H, W, seed):
    """[B, 2 k k, H, W] offsets (dh at 2 tap, dw at 2 tap + 1; 3 x 3, pad 1, stride 1)"""
    rng = np.random.RandomState(seed)
    if kind == "small":
        return (rng.randn(B, 2 * k * k, H, W) * 2.0).astype(np.float32)
    if kind == "off_map":
        return np.full((B, 2 * k * k, H, W), 1000.0, np.float32)
    # every sample of a tap lands on one of two points: a few pixels receive every gradient
    off = np.zeros((B, 2 * k * k, H, W), np.float32)
    ho, wo = np.arange(H, dtype=np.float32)[:, None], np.arange(W, dtype=np.float32)[None, :]
    for i in range(k):
        for j in range(k):
            tap = i * k + j
            th, tw = ((4.25, 5.5), (2.75, 1.25))[tap % 2]
            off[:, 2 * tap] = th - (ho - 1 + i)
            off[:, 2 * tap + 1] = tw - (wo - 1 + j)
    return off


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
def test_deform_conv_layer_forward_and_backward(modulated, dtype):
    """deform_conv / modulated_deform_conv (layers/dcn) forward + backward at torch_refs.DCN_IN_PLAN (B = 2, C = 64, 9 x 11,
    k = 3: the smallest shape the channels-last plan serves; tests/torch_refs.check_dcn_layer_in_plan checks the launches) in
    fp32 and fp16.  Offsets: small and random; all samples off the map (empty index lists: output and every gradient but the
    bias-free weight's are zero); all samples of a tap piled onto one of two points (the unequal tiles of
    test_deformable_index_tile_owner_build_on_device: the inverted index zeroes its counters and fills its overflow list on
    every replay).  Reference: torch_refs.deform_conv_torch in fp64 with autograd on the dtype-rounded inputs; fp32 within
    1e-4 of max(1, |reference|) (check_dcn_layer_in_plan), fp16 within 2e-2 of |reference|
    (test_deform_conv_cfg5_layer4_half_fwd_bwd).  Pile-ups beyond the index's slots are added by atomics, so eager-vs-replay
    bits are not asked."""
    from maskrcnn_benchmark.layers import deform_conv, modulated_deform_conv
    g = torch_refs.DCN_IN_PLAN
    B, Cc, H, W, k = g["B"], g["C"], g["H"], g["W"], g["k"]
    sets = []
    for i, kind in enumerate(("small", "off_map", "piled")):
        x, _, mask, wgt = synth.dcn_inputs(B, Cc, H, W, Cc, k, 1, modulated, seed=80 + i)
        go = np.random.RandomState(90 + i).randn(B, Cc, H, W).astype(np.float32)
        vals = [x, _dcn_offsets(kind, B, k, H, W, 85 + i), wgt * 0.25, go] + ([mask] if modulated else [])
        sets.append(tuple(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype) for a in vals))
    ox, ooff, _, ow = synth.dcn_inputs(1, 8, 5, 6, 8, 3, 1, False, seed=1)
    ox, ooff, ow = _t(ox).to(dtype), _t(ooff).to(dtype), _t(ow).to(dtype)

    def fn(x, off, w, go, mask=None):
        leaves = [t.detach().requires_grad_() for t in ((x, off, w) + ((mask,) if modulated else ()))]
        if modulated:
            y = modulated_deform_conv(leaves[0], leaves[1], leaves[3], leaves[2], None, 1, 1, 1, 1, 1)
        else:
            y = deform_conv(leaves[0], leaves[1], leaves[2], 1, 1, 1, 1, 1)
        return (y,) + torch.autograd.grad(y, leaves, go)

    def expect(v):
        leaves = [t.double().requires_grad_() for t in ((v[0], v[1], v[2]) + ((v[4],) if modulated else ()))]
        y = torch_refs.deform_conv_torch(leaves[0], leaves[1], leaves[3] if modulated else None, leaves[2], None, 1, 1, 1, 1, 1)
        return (y.detach(),) + torch.autograd.grad(y, leaves, v[3].double())

    def tol(got, want, what):
        for name, a, r in zip(("output", "grad_input", "grad_offset", "grad_weight", "grad_mask"), got, want):
            assert a.dtype == dtype
            err, top = float((a.double().cpu() - r).abs().max()), float(r.abs().max())      # NaN (not overwritten) fails
            assert err <= (1e-4 * max(1.0, top) if dtype == torch.float32 else 2e-2 * top), (what, name, err, top)

    off_map = expect(sets[1])
    assert not bool(off_map[0].any()) and not bool(off_map[1].any())
    check_replay(fn, sets, expect=expect, tol=tol, eager_bits=False, between=lambda: deform_conv(ox, ooff, ow, 1, 1, 1, 1, 1))
