"""The edge-shape cases of tests/target_cases.py through the host emulation of csrc/targets.hip and csrc/head_loss.hip.

This is what proves the references before tests/test_targets_edges_gpu.py trusts them on the device: the emulation runs the
same kernel source (workgroups one after another, glibc math), so exact cases must agree exactly and the fp64 references
within 1e-6 (measured: values <= 1.0e-7 relative; gradients and encoded targets <= 3.5e-7 of the largest reference entry,
the RPN loss's residuals under beta being the worst: their gradient d / beta amplifies the target's rounding by 9)."""
import ctypes

import numpy as np
import pytest
import torch

import emu
import target_cases as tc

TOL = 1e-6


# ------------------------------------------------------------------------------------------ matcher
@pytest.mark.parametrize("thresholds", tc.MATCHER_THRESHOLDS, ids=("rpn_lq", "box_head"))
@pytest.mark.parametrize("batched", (False, True), ids=("shared", "batched"))
@pytest.mark.parametrize("shape", tc.MATCHER_SHAPES)
def test_emu_match_boxes_edge_shapes(shape, batched, thresholds):
    c = tc.matcher_case(shape, batched, thresholds)
    ref = c["ref"].numpy()
    if c["random"]:                          # a constant output cannot pass
        assert (ref >= 0).sum() > 10 and (ref == -1).sum() > 10 and (c["lo"] == c["hi"] or (ref == -2).sum() > 10)
    if shape == "invalid_image":
        assert (ref[1] == -1).all()
    out = emu.match_boxes(c["gt"], c["valid"], c["boxes"], c["hi"], c["lo"], c["lq"])      # workspace poisoned with 0xAB
    assert np.array_equal(out, ref), np.argwhere(out != ref)[:5]
    assert np.array_equal(emu.match_boxes(c["gt"], c["valid"], c["boxes"], c["hi"], c["lo"], c["lq"]), out)


# ------------------------------------------------------------------------------------------ sampler
def _check_sampler(got, c):
    for g, r, what in zip(got, c["ref"], ("pos_mask", "neg_mask", "idx", "valid")):
        assert np.array_equal(np.asarray(g), r), (what, np.argwhere(np.asarray(g) != r)[:5])


@pytest.mark.parametrize("name", tc.SAMPLER_CASES)
def test_emu_sample_labels_equals_the_restatement(name):
    c = tc.sampler_case(name)
    _check_sampler(emu.sample_labels(c["labels"], c["B"], c["max_pos"], c["seed"]), c)
    B, val = c["B"], c["ref"][3]
    if name == "no_neg_and_no_pos":
        assert val[0].all() and val[1].sum() == 10 and val[2].all() and c["ref"][0][2].sum() == 0
    if name == "rpn_3_and_900":
        assert c["ref"][0][0].sum() == 3 and c["ref"][1][0].sum() == B - 3 and c["ref"][0][1].sum() == 128


def test_emu_sample_labels_device_seed_word():
    c = tc.sampler_case("n255", word=0x123456789ABCDEF)
    _check_sampler(emu.sample_labels(c["labels"], c["B"], c["max_pos"], c["seed"], seed_dev=c["word"]), c)
    assert not np.array_equal(c["ref"][2], tc.sampler_case("n255")["ref"][2])


# ------------------------------------------------------------------------------------------ mask targets
@pytest.mark.parametrize("H,W", tc.MASK_IMAGES)
def test_emu_mask_targets_edge_boxes(H, W):
    c = tc.mask_case(H, W)
    for M in tc.MASK_SIZES:
        for dt in tc.MASK_DTYPES:
            m = c["masks"][dt]
            if dt in (torch.int64, torch.int16):     # the product wrapper hands every other integer mask over as uint8
                m = m.to(torch.uint8)
            out = emu.mask_targets(m.numpy(), c["index"], c["boxes"], M)
            assert np.array_equal(out, tc.mask_reference(H, W, M, dt).numpy()), (M, dt)
    if H > 1:
        ref = tc.mask_reference(H, W, 14, torch.float32)
        assert 0 < float(ref.mean()) < 1 and not torch.equal(ref[:9], ref[9:])      # mask_index 0 and G - 1 differ


# ------------------------------------------------------------------------------------------ RPN loss
@pytest.mark.parametrize("name", tc.RPN_LOSS_CASES)
def test_emu_rpn_loss_edge_cases(name):
    c = tc.rpn_loss_case(name)
    ro, rb, rgo, rgb = c["ref"]
    lo, lb, gobj, gbox = emu.rpn_loss(c["obj"], c["box"], c["anchors"], c["matched"], c["pos"], c["neg"], c["gt"], c["beta"],
                                      c["weights"], upstream=tc.RPN_UPSTREAM)
    if name == "nothing_sampled":
        assert ro == 0 and rb == 0 and lo == 0.0 and lb == 0.0 and all(not g.any() for g in gobj + gbox)
        return
    if name == "negatives_only":
        assert rb == 0 and lb == 0.0 and all(not g.any() for g in gbox)
    else:
        assert tc.rel_err(lb, rb) <= TOL
    assert tc.rel_err(lo, ro) <= TOL
    assert tc.grad_err(gobj + gbox, rgo + rgb) <= TOL


# ------------------------------------------------------------------------------------------ RPN decode
@pytest.mark.parametrize("name", sorted(tc.DECODE_CASES))
def test_emu_rpn_decode_edge_levels_and_guard_bands(name):
    """glibc expf vs ATen's vectorised exp differ in the last place (the device test asserts bit equality): here the boxes
    agree to that, the guard bands and everything that does not pass through exp exactly"""
    c = tc.decode_case(name)
    post, obj, reg, col, off = c["post"], c["obj"], c["reg"], c["col"], c["off"]
    boxes, scores, ok = post._level_candidates(c["anchors"], obj, reg, c["sizes"])
    N, A, H, W = obj.shape
    k = boxes.shape[1]
    idx = obj.permute(0, 2, 3, 1).reshape(N, -1).sigmoid().topk(k, dim=1, sorted=True)[1].numpy()
    hw = np.asarray(c["sizes"], np.float32)
    K = col + k + 2
    ob = np.full((N, K, 4), np.nan, np.float32)
    os_ = np.full((N, K), np.nan, np.float32)
    nb = np.full((off + N * k + 3, 4), np.nan, np.float32)
    ns = np.full((off + N * k + 3,), np.nan, np.float32)
    okk = np.full((off + N * k + 3,), 7, np.uint8)
    p = lambda a, byte: ctypes.c_void_p(a.ctypes.data + byte)
    sc, an, rg = scores.numpy(), c["anchors"].numpy(), reg.numpy()
    rc = emu.lib().detops_rpn_decode_f32(p(rg, 0), p(idx, 0), p(sc, 0), p(an, 0), p(hw, 0), N, A, H, W, k, 1.0, 1.0, 1.0, 1.0,
                                         float(post.box_coder.bbox_xform_clip), float(c["min_size"]), p(ob, 16 * col), 4 * K,
                                         p(os_, 4 * col), K, p(nb, 16 * off), p(ns, 4 * off), p(okk, off), None)
    assert rc == 0
    # guard bands: untouched outside [col, col + k) and [off, off + N k)
    assert np.isnan(ob[:, :col]).all() and np.isnan(ob[:, col + k:]).all() and np.isnan(os_[:, :col]).all() and np.isnan(os_[:, col + k:]).all()
    for a in (nb, ns):
        assert np.isnan(a[:off]).all() and np.isnan(a[off + N * k:]).all()
    assert (okk[:off] == 7).all() and (okk[off + N * k:] == 7).all()
    b, s = ob[:, col:col + k], os_[:, col:col + k]
    ref = boxes.numpy()
    assert np.array_equal(s, sc) and np.allclose(b, ref, rtol=1e-6, atol=4e-3) and np.mean(b == ref) > 0.9
    got_ok = okk[off:off + N * k].astype(bool)
    sz = np.minimum(ref[..., 2] - ref[..., 0], ref[..., 3] - ref[..., 1]).reshape(-1) + 1
    sure = np.abs(sz - c["min_size"]) > 1e-2
    assert np.array_equal(got_ok[sure], ok.reshape(-1).numpy()[sure])
    far = np.asarray([-1e6, -1e6, -1e6 + 1, -1e6 + 1], np.float32)
    assert np.array_equal(nb[off:off + N * k], np.where(got_ok[:, None], b.reshape(-1, 4), far))
    assert np.array_equal(ns[off:off + N * k], np.where(got_ok, s.reshape(-1), np.float32(-1)))
    if c["min_size"]:
        assert 0 < got_ok.sum() < got_ok.size
    if name == "image_smaller_than_anchors":
        for n, (h, w) in enumerate(c["sizes"]):      # every candidate is cut down to the image
            assert (ref[n, :, 2] <= w - 1).all() and (ref[n, :, 3] <= h - 1).all() and (ref[n, :, 2] == w - 1).any()


# ------------------------------------------------------------------------------------------ labels and slots
@pytest.mark.parametrize("N,K", tc.LABEL_SHAPES)
def test_emu_match_labels_edge_totals(N, K):
    c = tc.labels_case(N, K)
    for dtype in (np.float32, np.int64):
        for gl in (None, c["gt_labels"]):
            for valid in (None, c["valid"]):
                ref = tc.match_labels_reference(c["matched"], gl, valid, dtype)
                out = emu.match_labels(c["matched"], gl, valid, dtype)
                assert out.dtype == ref.dtype and np.array_equal(out, ref), (dtype, gl is None, valid is None)
    assert (c["matched"] >= c["gt_labels"].shape[1]).any()


@pytest.mark.parametrize("with_valid,with_obj", ((True, True), (False, False)))
@pytest.mark.parametrize("N,B", tc.LABEL_SHAPES)
def test_emu_roi_head_targets_edge_totals(N, B, with_valid, with_obj):
    c = tc.slots_case(N, B, with_valid, with_obj)
    rb, rl, rreg, rm, ro = c["ref"]
    ob, ol, oreg, om, oo = emu.roi_head_targets(c["boxes"], c["matched"], c["gt"], c["gt_labels"], c["valid"], c["idx"],
                                                c["slot_valid"], c["objectness"], c["weights"])
    assert np.array_equal(ob, rb) and np.array_equal(ol, rl) and np.array_equal(om, rm)
    assert (oo is None and ro is None) if not with_obj else np.array_equal(oo, ro)
    assert tc.grad_err(oreg, rreg) <= TOL
    assert (rl[~c["slot_valid"]] == -1).all() and (rl > 0).any() and (rl == 0).any() and (rm >= c["gt"].shape[1]).any()


# ------------------------------------------------------------------------------------------ box-head loss
@pytest.mark.parametrize("R,C,agnostic,beta,scale", tc.FASTRCNN_CASES)
def test_emu_fastrcnn_loss_edge_shapes(R, C, agnostic, beta, scale):
    c = tc.fastrcnn_case(R, C, agnostic, beta, scale)
    rc_, rr, rgl, rgb = c["ref"]
    lc, lb, gl, gb = emu.fastrcnn_loss(c["logits"], c["box"], c["labels"], c["targets"], agnostic, beta, upstream=tc.HEAD_UPSTREAM)
    assert tc.rel_err(lc, rc_) <= TOL and tc.rel_err(lb, rr) <= TOL
    assert tc.grad_err(gl, rgl) <= TOL and tc.grad_err(gb, rgb) <= TOL
    assert not gl[(c["labels"] < 0) | (c["labels"] >= C)].any() and not gb[(c["labels"] <= 0) | (c["labels"] >= C)].any()
    # backward through the class loss alone: no box gradient at all
    _, _, gl0, gb0 = emu.fastrcnn_loss(c["logits"], c["box"], c["labels"], c["targets"], agnostic, beta, upstream=(tc.HEAD_UPSTREAM[0], 0.0))
    assert not gb0.any() and np.array_equal(gl0, gl)


def test_emu_fastrcnn_loss_nothing_sampled():
    R, C, agnostic, beta, scale = tc.FASTRCNN_CASES[3]
    c = tc.fastrcnn_case(R, C, agnostic, beta, scale, unsampled=True)
    lc, lb, gl, gb = emu.fastrcnn_loss(c["logits"], c["box"], c["labels"], c["targets"], agnostic, beta, upstream=tc.HEAD_UPSTREAM)
    assert c["ref"][0] == 0 and c["ref"][1] == 0 and lc == 0.0 and lb == 0.0 and not gl.any() and not gb.any()


# ------------------------------------------------------------------------------------------ mask-head loss
@pytest.mark.parametrize("P,C,M,scale", tc.MASK_LOSS_CASES)
def test_emu_mask_loss_edge_shapes(P, C, M, scale):
    c = tc.mask_loss_case(P, C, M, scale)
    rl, rg = c["ref"]
    lo, g = emu.mask_loss(c["logits"], c["labels"], c["targets"], upstream=tc.MASK_UPSTREAM)
    assert tc.rel_err(lo, rl) <= TOL and tc.grad_err(g, rg) <= TOL
    own = np.zeros((P, C), bool)
    fg = (c["labels"] > 0) & (c["labels"] < C)
    own[np.nonzero(fg)[0], c["labels"][fg]] = True
    assert fg.any() and not g[~own].any()            # every plane but the ROI's own: exactly 0
    c0 = tc.mask_loss_case(P, C, M, scale, no_positives=True)
    lo, g = emu.mask_loss(c0["logits"], c0["labels"], c0["targets"], upstream=tc.MASK_UPSTREAM)
    assert c0["ref"][0] == 0 and lo == 0.0 and not g.any()
