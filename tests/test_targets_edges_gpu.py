"""The edge-shape cases of tests/target_cases.py through maskrcnn_benchmark._C on the device: csrc/targets.hip and
csrc/head_loss.hip where small and odd inputs take them — second LDS chunk of ground truth, several workgroups raising one
per-gt word, ballots and wave reductions under partial exec masks, whole-wave early returns, device expf / logf.
tests/test_targets_edges_emu.py holds the same cases against the same references on the host emulation.

Exact where the operation is exact (matcher, sampler, mask targets, labels, copied boxes, RPN decode against the ATen
composition on the same device).  The losses, their gradients and the encoded regression targets are measured against fp64:
values as relative error, arrays as max|g - ref| / max|ref|.

Measured on an MI355X (worst case per kernel over the cases below; each test prints its figures, run with -s):
    kernel               values      gradients / arrays
    rpn_loss             9.89e-08    5.03e-07   (eight levels: d / beta of the residuals under beta, 1 / beta = 9)
    fastrcnn_loss        8.81e-08    1.47e-07
    mask_loss            1.02e-07    1.64e-07
    roi_head_targets     -           1.34e-07   (encoded regression targets)
The host emulation gives 9.9e-08 / 3.5e-07, 8.8e-08 / 1.5e-07, 1.0e-07 / 1.6e-07 and 1.3e-07 on the same cases: device
expf / logf cost nothing measurable here.
Bounds: 8 x the measured figure (margin for other seeds and compiler versions); values no tighter than 4 fp32 ulp
(4.8e-7); all far inside the 1e-5 (values) / 1e-4 (gradients) of tests/test_targets_gpu.py at model size and its 2e-6
for the encoded targets."""
import numpy as np
import pytest
import torch

import target_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"

#          kernel: (bound on values, bound on gradients / arrays)
ULP4 = 4 * 2.0 ** -23
BOUNDS = {"rpn_loss": (max(8 * 9.89e-08, ULP4), 8 * 5.03e-07), "fastrcnn_loss": (max(8 * 8.81e-08, ULP4), 8 * 1.47e-07),
          "mask_loss": (max(8 * 1.02e-07, ULP4), 8 * 1.64e-07), "roi_head_targets": (None, 8 * 1.34e-07)}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _figure(kernel, case, value=None, grad=None):
    """print the measured figures of a case, then hold them against the kernel's bounds"""
    print("FIGURE %-17s %-28s value %-10s grad %s" % (kernel, case, "-" if value is None else "%.3g" % value,
                                                     "-" if grad is None else "%.3g" % grad))
    vb, gb = BOUNDS[kernel]
    assert value is None or value <= vb, (kernel, case, "value", value)
    assert grad is None or grad <= gb, (kernel, case, "grad", grad)


# ------------------------------------------------------------------------------------------ matcher
def _match_raw(c, fill):
    """the library entry point itself, into a sentinel-filled result and a workspace poisoned with `fill`"""
    from maskrcnn_benchmark import _lib
    gt, valid, boxes = _dev(c["gt"]), _dev(c["valid"].astype(np.uint8)), _dev(c["boxes"])
    N, M = gt.shape[:2]
    K = boxes.shape[-2]
    out = torch.full((N, K), -99, dtype=torch.int64, device=DEV)
    nbytes = int(_lib.lib.detops_match_boxes_workspace_bytes(N, M))
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib.detops_match_boxes_f32(gt.data_ptr(), valid.data_ptr(), boxes.data_ptr(), int(boxes.dim() == 3), N, M, K,
                                               c["hi"], c["lo"], int(c["lq"]), out.data_ptr(), ws.data_ptr(), nbytes,
                                               _lib.stream_of(out)), "match_boxes")
    return out.cpu()


@pytest.mark.parametrize("thresholds", tc.MATCHER_THRESHOLDS, ids=("rpn_lq", "box_head"))
@pytest.mark.parametrize("batched", (False, True), ids=("shared", "batched"))
@pytest.mark.parametrize("shape", tc.MATCHER_SHAPES)
def test_match_boxes_edge_shapes(shape, batched, thresholds):
    from maskrcnn_benchmark import _C
    c = tc.matcher_case(shape, batched, thresholds)
    ref = c["ref"]
    if c["random"]:                          # a constant output cannot pass
        assert int((ref >= 0).sum()) > 10 and int((ref == -1).sum()) > 10 and (c["lo"] == c["hi"] or int((ref == -2).sum()) > 10)
    out = _C.match_boxes(_dev(c["gt"]), _dev(c["valid"]), _dev(c["boxes"]), c["hi"], c["lo"], c["lq"]).cpu()
    assert torch.equal(out, ref), (out != ref).nonzero()[:5]
    first, second = _match_raw(c, 0xAB), _match_raw(c, 0x7F)
    assert torch.equal(first, ref) and torch.equal(second, first)


# ------------------------------------------------------------------------------------------ sampler
def _check_sampler(got, c):
    for g, r, what in zip(got, c["ref"], ("pos_mask", "neg_mask", "idx", "valid")):
        g = g.cpu().numpy()
        assert g.dtype == r.dtype and np.array_equal(g, r), (what, np.argwhere(g != r)[:5])


@pytest.mark.parametrize("name", tc.SAMPLER_CASES)
def test_sample_labels_equals_the_restatement(name):
    from maskrcnn_benchmark import _C
    c = tc.sampler_case(name)
    lab = _dev(c["labels"])
    _check_sampler(_C.sample_labels(lab, c["B"], c["max_pos"], with_list=True, seed=c["seed"]), c)
    pos, neg = _C.sample_labels(lab, c["B"], c["max_pos"], seed=c["seed"])                   # without the list: same masks
    assert np.array_equal(pos.cpu().numpy(), c["ref"][0]) and np.array_equal(neg.cpu().numpy(), c["ref"][1])


def test_sample_labels_mixes_the_graph_seed_word(monkeypatch):
    from maskrcnn_benchmark import _C
    word = 0x123456789ABCDEF
    c = tc.sampler_case("n255", word=word)
    monkeypatch.setattr(_C, "GRAPH_SEED", torch.tensor([word], dtype=torch.int64, device=DEV))
    _check_sampler(_C.sample_labels(_dev(c["labels"]), c["B"], c["max_pos"], with_list=True, seed=c["seed"]), c)
    assert not np.array_equal(c["ref"][2], tc.sampler_case("n255")["ref"][2])


# ------------------------------------------------------------------------------------------ mask targets
@pytest.mark.parametrize("H,W", tc.MASK_IMAGES)
def test_mask_targets_edge_boxes(H, W):
    from maskrcnn_benchmark import _C
    c = tc.mask_case(H, W)
    index, boxes = _dev(c["index"]), _dev(c["boxes"])
    for M in tc.MASK_SIZES:
        for dt in tc.MASK_DTYPES:
            out = _C.mask_targets(c["masks"][dt].to(DEV), index, boxes, M).cpu()
            assert torch.equal(out, tc.mask_reference(H, W, M, dt)), (M, dt)


# ------------------------------------------------------------------------------------------ RPN loss
@pytest.mark.parametrize("name", tc.RPN_LOSS_CASES)
def test_rpn_loss_edge_cases(name):
    from maskrcnn_benchmark import _C
    c = tc.rpn_loss_case(name)
    ro, rb, rgo, rgb = c["ref"]
    obj = [_dev(t).requires_grad_() for t in c["obj"]]
    box = [_dev(t).requires_grad_() for t in c["box"]]
    lo, lb = _C.rpn_loss(obj, box, _dev(c["anchors"]), _dev(c["matched"]), _dev(c["pos"]), _dev(c["neg"]), _dev(c["gt"]),
                         c["beta"], c["weights"])
    (tc.RPN_UPSTREAM[0] * lo + tc.RPN_UPSTREAM[1] * lb).backward()
    gobj, gbox = [t.grad.cpu().numpy() for t in obj], [t.grad.cpu().numpy() for t in box]
    lo, lb = lo.item(), lb.item()
    if name == "nothing_sampled":
        assert lo == 0.0 and lb == 0.0 and all(not g.any() for g in gobj + gbox)
        return
    if name == "negatives_only":
        assert lb == 0.0 and all(not g.any() for g in gbox)
        value = tc.rel_err(lo, ro)
    else:
        value = max(tc.rel_err(lo, ro), tc.rel_err(lb, rb))
    _figure("rpn_loss", name, value, tc.grad_err(gobj + gbox, rgo + rgb))


# ------------------------------------------------------------------------------------------ RPN decode
@pytest.mark.parametrize("name", sorted(tc.DECODE_CASES))
def test_rpn_decode_edge_levels_and_guard_bands(name):
    """bit-equal to RPNPostProcessor._level_candidates on the same device, written at non-zero `col` / `off` into NaN-filled
    results: everything outside [col, col + k) and [off, off + N k) stays NaN"""
    from maskrcnn_benchmark import _C
    c = tc.decode_case(name)
    post, col, off = c["post"], c["col"], c["off"]
    anchors, obj, reg = c["anchors"].to(DEV), c["obj"].to(DEV), c["reg"].to(DEV)
    boxes, scores, ok = post._level_candidates(anchors, obj, reg, c["sizes"])
    N, A, H, W = obj.shape
    k = boxes.shape[1]
    assert k == min(post.pre_nms_top_n, A * H * W)
    s, idx = obj.permute(0, 2, 3, 1).reshape(N, -1).sigmoid().topk(k, dim=1, sorted=True)
    assert torch.equal(s, scores)
    K, R = col + k + 2, off + N * k + 3
    ob = torch.full((N, K, 4), float("nan"), device=DEV)
    os_ = torch.full((N, K), float("nan"), device=DEV)
    nb = torch.full((R, 4), float("nan"), device=DEV)
    ns = torch.full((R,), float("nan"), device=DEV)
    okk = torch.full((R,), 7, dtype=torch.uint8, device=DEV)
    hw = torch.tensor([[h, w] for h, w in c["sizes"]], dtype=torch.float32, device=DEV)
    _C.rpn_decode(reg, idx, s, anchors, hw, post.box_coder.weights, post.box_coder.bbox_xform_clip, c["min_size"],
                  ob, os_, col, nb, ns, okk, off)
    assert ob[:, :col].isnan().all() and ob[:, col + k:].isnan().all() and os_[:, :col].isnan().all() and os_[:, col + k:].isnan().all()
    for a in (nb, ns):
        assert a[:off].isnan().all() and a[off + N * k:].isnan().all()
    assert (okk[:off] == 7).all() and (okk[off + N * k:] == 7).all()
    assert torch.equal(ob[:, col:col + k], boxes) and torch.equal(os_[:, col:col + k], scores)
    flat_ok = ok.reshape(-1)
    assert torch.equal(okk[off:off + N * k].bool(), flat_ok)
    far = torch.tensor([-1e6, -1e6, -1e6 + 1, -1e6 + 1], device=DEV)
    assert torch.equal(nb[off:off + N * k], torch.where(flat_ok[:, None], boxes.reshape(-1, 4), far))
    assert torch.equal(ns[off:off + N * k], torch.where(flat_ok, scores.reshape(-1), scores.new_full((), -1.0)))
    if c["min_size"]:
        assert 0 < int(flat_ok.sum()) < flat_ok.numel()


# ------------------------------------------------------------------------------------------ labels and slots
@pytest.mark.parametrize("N,K", tc.LABEL_SHAPES)
def test_match_labels_edge_totals(N, K):
    from maskrcnn_benchmark import _C
    c = tc.labels_case(N, K)
    matched = _dev(c["matched"])
    for dtype, npdt in ((torch.float32, np.float32), (torch.int64, np.int64)):
        for gl in (None, c["gt_labels"]):
            for valid in (None, c["valid"]):
                out = _C.match_labels(matched, _dev(gl), _dev(valid), dtype)
                ref = tc.match_labels_reference(c["matched"], gl, valid, npdt)
                assert out.dtype == dtype and np.array_equal(out.cpu().numpy(), ref), (dtype, gl is None, valid is None)


@pytest.mark.parametrize("with_valid,with_obj", ((True, True), (False, False)))
@pytest.mark.parametrize("N,B", tc.LABEL_SHAPES)
def test_roi_head_targets_edge_totals(N, B, with_valid, with_obj):
    from maskrcnn_benchmark import _C
    c = tc.slots_case(N, B, with_valid, with_obj)
    rb, rl, rreg, rm, ro = c["ref"]
    ob, ol, oreg, om, oo = _C.roi_head_targets(_dev(c["boxes"]), _dev(c["matched"]), _dev(c["gt"]), _dev(c["gt_labels"]),
                                               _dev(c["valid"]), _dev(c["idx"]), _dev(c["slot_valid"]), _dev(c["objectness"]),
                                               c["weights"])
    assert np.array_equal(ob.cpu().numpy(), rb) and np.array_equal(ol.cpu().numpy(), rl) and np.array_equal(om.cpu().numpy(), rm)
    assert (oo is None and ro is None) if not with_obj else np.array_equal(oo.cpu().numpy(), ro)
    _figure("roi_head_targets", "N=%d B=%d valid=%d" % (N, B, with_valid), None, tc.grad_err(oreg.cpu().numpy(), rreg))


# ------------------------------------------------------------------------------------------ box-head loss
def _fastrcnn(c, agnostic, beta):
    from maskrcnn_benchmark import _C
    fl, fb = _dev(c["logits"]).requires_grad_(), _dev(c["box"]).requires_grad_()
    lc, lb = _C.fastrcnn_loss(fl, fb, _dev(c["labels"]), _dev(c["targets"]), agnostic, beta)
    return fl, fb, lc, lb


@pytest.mark.parametrize("R,C,agnostic,beta,scale", tc.FASTRCNN_CASES)
def test_fastrcnn_loss_edge_shapes(R, C, agnostic, beta, scale):
    c = tc.fastrcnn_case(R, C, agnostic, beta, scale)
    rc_, rr, rgl, rgb = c["ref"]
    fl, fb, lc, lb = _fastrcnn(c, agnostic, beta)
    (tc.HEAD_UPSTREAM[0] * lc + tc.HEAD_UPSTREAM[1] * lb).backward()
    gl, gb = fl.grad.cpu().numpy(), fb.grad.cpu().numpy()
    assert not gl[(c["labels"] < 0) | (c["labels"] >= C)].any() and not gb[(c["labels"] <= 0) | (c["labels"] >= C)].any()
    _figure("fastrcnn_loss", "R=%d C=%d agnostic=%d" % (R, C, agnostic), max(tc.rel_err(lc.item(), rc_), tc.rel_err(lb.item(), rr)),
            max(tc.grad_err(gl, rgl), tc.grad_err(gb, rgb)))
    # backward through the class loss alone: no box gradient at all
    fl, fb, lc, lb = _fastrcnn(c, agnostic, beta)
    (tc.HEAD_UPSTREAM[0] * lc).backward()
    assert fb.grad is not None and not bool(fb.grad.any()) and np.array_equal(fl.grad.cpu().numpy(), gl)


def test_fastrcnn_loss_nothing_sampled_and_second_backward():
    R, C, agnostic, beta, scale = tc.FASTRCNN_CASES[3]
    c = tc.fastrcnn_case(R, C, agnostic, beta, scale, unsampled=True)
    fl, fb, lc, lb = _fastrcnn(c, agnostic, beta)
    (tc.HEAD_UPSTREAM[0] * lc + tc.HEAD_UPSTREAM[1] * lb).backward(retain_graph=True)
    assert lc.item() == 0.0 and lb.item() == 0.0 and not bool(fl.grad.any()) and not bool(fb.grad.any())
    with pytest.raises(RuntimeError, match="backward called twice"):    # the stored gradients were scaled in place
        (lc + lb).backward()


# ------------------------------------------------------------------------------------------ mask-head loss
@pytest.mark.parametrize("P,C,M,scale", tc.MASK_LOSS_CASES)
def test_mask_loss_edge_shapes(P, C, M, scale):
    from maskrcnn_benchmark import _C
    c = tc.mask_loss_case(P, C, M, scale)
    rl, rg = c["ref"]
    x = _dev(c["logits"]).requires_grad_()
    loss = _C.mask_loss(x, _dev(c["labels"]), _dev(c["targets"]))
    (tc.MASK_UPSTREAM * loss).backward()
    g = x.grad.cpu().numpy()
    own = np.zeros((P, C), bool)
    fg = (c["labels"] > 0) & (c["labels"] < C)
    own[np.nonzero(fg)[0], c["labels"][fg]] = True
    assert fg.any() and not g[~own].any()            # every plane but the ROI's own: exactly 0
    _figure("mask_loss", "P=%d C=%d M=%d" % (P, C, M), tc.rel_err(loss.item(), rl), tc.grad_err(g, rg))
    c0 = tc.mask_loss_case(P, C, M, scale, no_positives=True)
    x = _dev(c0["logits"]).requires_grad_()
    loss = _C.mask_loss(x, _dev(c0["labels"]), _dev(c0["targets"]))
    loss.backward()
    assert loss.item() == 0.0 and not bool(x.grad.any())
