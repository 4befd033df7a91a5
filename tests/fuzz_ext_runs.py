"""The extension-operator families of tests/fuzz_cases.py: their references and the one way each case is run through
`maskrcnn_benchmark._C` — shared by tests/test_emu_fuzz_ext.py (CPU tensors over the host-emulation library) and
tests/test_fuzz_ext_gpu.py (the MI355X, clean and dirty memory).

A plain module: no tests, no fixtures.  `refs(family, seed)` computes a case's references once per process (read-only);
`RUN[family](case, ref, dev)` makes the calls on device `dev`, asserts every result against the reference and returns the
dict name -> tensor of everything the operator promises to reproduce bit for bit.  Nothing in `refs` calls the code under test.

Bounds.  Exact results (matcher, labels, sampler, copied boxes, RPN decode against the ATen composition on the same device,
the runs, strings, packs, pair counts, fp64 IoUs and matches of the mask chain, the merge of test-time augmentation, the ReLU
select) are compared with array_equal.  Losses, gradients and encoded targets are measured against fp64 as in
tests/test_targets_edges_gpu.py (values: relative error; arrays: max|g - ref| / max|ref|) and held to its BOUNDS — or, where
a drawn case is conditioned worse than that file's hand-picked ones, to 8 x the worst error of the plain fp32 ATen composition
of the same operation over the family's seeds (`bounds_of`: computed from ATen on the CPU, never from the code under test);
the keypoint loss to the 1e-5 of tests/test_keypoint_gpu.py::test_loss_kernel_value_and_gradient; each prints a FIGURE line.
The sparse RPN-head backward is held to GRAD_TOL of tests/test_whole_model_parity.py against fp64 dense autograd, as
test_reduced_shape_equals_fp64_autograd_on_the_cpu holds it.  GroupNorm is held to the analytic bounds of
tests/test_group_norm_gpu.py (its own checkers are called), the bias pass to the criteria of
tests/test_ops_gpu.py::test_bias_act_channels_last_forward_backward_and_bias_gradient: the output within (1e-6 / 2e-3 / 2e-2
per dtype) x max(1, |ref|max), the bias gradient and the column sums within 1e-5 x max(1, largest column sum of magnitudes)
of the fp64 sum of the stored values.  tests/test_fuzz_ext_gpu.py records what an
MI355X measured."""
import functools

import numpy as np
import torch

import bbox_aug_cases
import fuzz_cases
import target_cases as tc
from test_targets_edges_gpu import BOUNDS

KEYPOINT_BOUND = 1e-5                      # tests/test_keypoint_gpu.py::test_loss_kernel_value_and_gradient, value and gradient
KEYPOINT_UPSTREAM = 2.5
BIAS_TOL = {"float32": 1e-6, "float16": 2e-3, "bfloat16": 2e-2}
EPS = 1e-5
assert fuzz_cases.CHAIN_THRESHOLDS == tc.MATCHER_THRESHOLDS


def _C():
    from maskrcnn_benchmark import _C as C
    return C


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().contiguous().cpu().numpy()


FAMILY_OF = {"roi_head_targets": "targets_chain", "fastrcnn_loss": "head_losses", "mask_loss": "head_losses", "rpn_loss": "rpn_loss_decode"}


@functools.lru_cache(maxsize=None)
def aten_worst(kernel):
    """the worst error, over the family's seeds, of the plain fp32 ATen composition of `kernel`'s operation on the CPU against
    the fp64 reference -> (value, gradients / arrays)"""
    family = FAMILY_OF[kernel]
    figures = [refs(family, seed)["aten"][kernel] for seed in range(fuzz_cases.SEEDS[family])]
    return tuple(max(f[i] for f in figures) if figures[0][i] is not None else None for i in (0, 1))


def bounds_of(kernel):
    """BOUNDS of tests/test_targets_edges_gpu.py (8 x what that file's hand-picked cases measured), and where a drawn case
    is conditioned worse than those, 8 x `aten_worst`: never anything the code under test produced"""
    return tuple(None if b is None else max(b, 8 * a) for b, a in zip(BOUNDS[kernel], aten_worst(kernel)))


def figure(kernel, case, value=None, grad=None, bounds=None):
    """print the measured figures of a case, then hold them against the kernel's bounds"""
    print("FIGURE %-17s %-28s value %-10s grad %s" % (kernel, case, "-" if value is None else "%.3g" % value,
                                                     "-" if grad is None else "%.3g" % grad))
    vb, gb = bounds if bounds is not None else bounds_of(kernel)
    assert value is None or value <= vb, (kernel, case, "value", value, vb)
    assert grad is None or grad <= gb, (kernel, case, "grad", grad, gb)


@functools.lru_cache(maxsize=None)
def refs(family, seed):
    return _REFS[family](fuzz_cases.FAMILIES[family](seed))


# ------------------------------------------------------------------------------------------ targets chain
def _chain_refs(c):
    N, M, K = c["N"], c["M"], c["K"]
    matched = tc.matcher_reference(c["gt"], c["gt_valid"], c["boxes"], c["hi"], c["lo"], c["lq"]).numpy()
    labels = tc.match_labels_reference(matched, None if c["rpn_rule"] else c["gt_labels"], c["box_valid"],
                                       np.float32 if c["rpn_rule"] else np.int64)
    pos, neg, idx, val = tc.sampler_reference(labels, c["B"], c["max_pos"], c["sampler_seed"])
    boxes = c["boxes"] if c["batched"] else np.broadcast_to(c["boxes"], (N, K, 4))
    rows = np.arange(N)[:, None]
    m = matched[rows, idx]
    slot_labels = tc.match_labels_reference(matched, c["gt_labels"], c["box_valid"], np.int64)[rows, idx]
    slot_labels[~val] = -1
    slot_gt, slot_box = torch.from_numpy(c["gt"][rows, np.clip(m, 0, M - 1)]), torch.from_numpy(boxes[rows, idx])
    reg = tc.encode64(slot_gt, slot_box, c["weights"]).numpy()
    aten = (None, tc.grad_err(tc.encode64(slot_gt, slot_box, c["weights"], torch.float32).numpy(), reg))
    return dict(aten={"roi_head_targets": aten}, matched=matched, labels=labels, pos=pos, neg=neg, idx=idx, val=val,
                slot_boxes=np.ascontiguousarray(boxes[rows, idx]), slot_labels=slot_labels, reg=reg, slot_matched=m,
                slot_obj=None if c["objectness"] is None else c["objectness"][rows, idx])


def run_targets_chain(c, r, dev):
    """every stage reads the previous stage's device output; all of it is integer logic or copies except the encoded
    regression targets (BOUNDS["roi_head_targets"]); include/detops.h calls each of the four kernels deterministic"""
    C_ = _C()
    N, K = c["N"], c["K"]
    gt, boxes = _t(c["gt"], dev), _t(c["boxes"], dev)
    matched = C_.match_boxes(gt, _t(c["gt_valid"], dev), boxes, c["hi"], c["lo"], c["lq"])
    assert np.array_equal(_np(matched), r["matched"]), np.argwhere(_np(matched) != r["matched"])[:5]
    gl, bv = _t(c["gt_labels"], dev), _t(c["box_valid"], dev)
    labels = C_.match_labels(matched, None if c["rpn_rule"] else gl, bv, torch.float32 if c["rpn_rule"] else torch.int64)
    assert _np(labels).dtype == r["labels"].dtype and np.array_equal(_np(labels), r["labels"])
    pos, neg, idx, val = C_.sample_labels(labels, c["B"], c["max_pos"], with_list=True, seed=c["sampler_seed"])
    for got, name in ((pos, "pos"), (neg, "neg"), (idx, "idx"), (val, "val")):
        assert _np(got).dtype == r[name].dtype and np.array_equal(_np(got), r[name]), (name, np.argwhere(_np(got) != r[name])[:5])
    pos2, neg2 = C_.sample_labels(labels, c["B"], c["max_pos"], seed=c["sampler_seed"])          # without the list: same masks
    assert np.array_equal(_np(pos2), r["pos"]) and np.array_equal(_np(neg2), r["neg"])
    bN = boxes if c["batched"] else boxes.unsqueeze(0).expand(N, K, 4).contiguous()
    ob, ol, oreg, om, oo = C_.roi_head_targets(bN, matched, gt, gl, bv, idx, val, _t(c["objectness"], dev), c["weights"])
    assert np.array_equal(_np(ob), r["slot_boxes"]) and np.array_equal(_np(ol), r["slot_labels"])
    assert np.array_equal(_np(om), r["slot_matched"])
    assert (oo is None) == (r["slot_obj"] is None) and (oo is None or np.array_equal(_np(oo), r["slot_obj"]))
    figure("roi_head_targets", "N=%d M=%d K=%d B=%d" % (N, c["M"], K, c["B"]), None, tc.grad_err(_np(oreg), r["reg"]))
    keep = dict(matched=matched, labels=labels, pos=pos, neg=neg, idx=idx, val=val, slot_boxes=ob, slot_labels=ol,
                regression_targets=oreg, slot_matched=om)
    if oo is not None:
        keep["slot_objectness"] = oo
    return keep


# ------------------------------------------------------------------------------------------ head losses
def _keypoint_reference(logits, heat, valid, upstream):
    """fp64 log-softmax over the plane: mean cross-entropy of the valid rows (0 without one) -> (loss, d/d logits)"""
    P, K, H, W = logits.shape
    x = torch.from_numpy(logits).double().reshape(P * K, H * W).requires_grad_()
    v = torch.from_numpy(valid).reshape(-1)
    ls = torch.log_softmax(x, 1).gather(1, torch.from_numpy(heat).reshape(-1, 1)).squeeze(1)
    loss = -torch.where(v, ls, torch.zeros_like(ls)).sum() / v.sum().clamp(min=1).double()
    (upstream * loss).backward()
    return loss.item(), x.grad.view(P, K, H, W).numpy()


def _loss_refs(c):
    fr_args = (c["fr_logits"], c["fr_box"], c["fr_labels"], c["fr_targets"], c["fr_agnostic"], c["fr_beta"], tc.HEAD_UPSTREAM)
    mk_args = (c["mk_logits"], c["mk_labels"], c["mk_targets"], tc.MASK_UPSTREAM)
    fr, mk = tc.fastrcnn_reference(*fr_args), tc.mask_loss_reference(*mk_args)
    fr32, mk32 = tc.fastrcnn_reference(*fr_args, dtype=torch.float32), tc.mask_loss_reference(*mk_args, dtype=torch.float32)
    aten = {"fastrcnn_loss": (max(tc.rel_err(fr32[0], fr[0]), tc.rel_err(fr32[1], fr[1])),
                              max(tc.grad_err(fr32[2], fr[2]), tc.grad_err(fr32[3], fr[3]))),
            "mask_loss": (tc.rel_err(mk32[0], mk[0]), tc.grad_err(mk32[1], mk[1]))}
    return dict(fr=fr, mk=mk, kp=_keypoint_reference(c["kp_logits"], c["kp_heat"], c["kp_valid"], KEYPOINT_UPSTREAM), aten=aten)


def run_head_losses(c, r, dev):
    """forward and backward through the product's autograd nodes with non-unit upstream gradients.  include/detops.h: the
    three losses reduce in a fixed order without atomics (per-row / per-plane partial sums in the workspace, one finishing
    block), so values and gradients are reproducible bit for bit"""
    C_ = _C()
    keep = {}
    # box head
    R, C = c["fr_R"], c["fr_C"]
    rc_, rr, rgl, rgb = r["fr"]
    fl, fb = _t(c["fr_logits"], dev).requires_grad_(), _t(c["fr_box"], dev).requires_grad_()
    lc, lb = C_.fastrcnn_loss(fl, fb, _t(c["fr_labels"], dev), _t(c["fr_targets"], dev), c["fr_agnostic"], c["fr_beta"])
    (tc.HEAD_UPSTREAM[0] * lc + tc.HEAD_UPSTREAM[1] * lb).backward()
    gl, gb = _np(fl.grad), _np(fb.grad)
    L = c["fr_labels"]
    assert not gl[(L < 0) | (L >= C)].any() and not gb[(L <= 0) | (L >= C)].any()
    if not ((L >= 0) & (L < C)).any():
        assert lc.item() == 0.0 and lb.item() == 0.0 and not gl.any() and not gb.any()
    figure("fastrcnn_loss", "R=%d C=%d agnostic=%d" % (R, C, c["fr_agnostic"]),
           max(tc.rel_err(lc.item(), rc_), tc.rel_err(lb.item(), rr)), max(tc.grad_err(gl, rgl), tc.grad_err(gb, rgb)))
    keep.update(fr_class_loss=lc.detach(), fr_box_loss=lb.detach(), fr_grad_logits=fl.grad, fr_grad_box=fb.grad)
    # mask head
    P, Cm, M = c["mk_P"], c["mk_C"], c["mk_M"]
    rl, rg = r["mk"]
    x = _t(c["mk_logits"], dev).requires_grad_()
    loss = C_.mask_loss(x, _t(c["mk_labels"], dev), _t(c["mk_targets"], dev))
    (tc.MASK_UPSTREAM * loss).backward()
    g = _np(x.grad)
    fg = (c["mk_labels"] > 0) & (c["mk_labels"] < Cm)
    own = np.zeros((P, Cm), bool)
    own[np.nonzero(fg)[0], c["mk_labels"][fg]] = True
    assert not g[~own].any()                   # every plane but the ROI's own: exactly 0
    if not fg.any():
        assert loss.item() == 0.0 and not g.any()
    figure("mask_loss", "P=%d C=%d M=%d" % (P, Cm, M), tc.rel_err(loss.item(), rl), tc.grad_err(g, rg))
    keep.update(mk_loss=loss.detach(), mk_grad=x.grad)
    # keypoint head
    rl, rg = r["kp"]
    d = _t(c["kp_logits"], dev)
    if c["kp_channels_last"]:
        d = d.contiguous(memory_format=torch.channels_last)
    d.requires_grad_()
    loss = C_.keypoint_loss(d, _t(c["kp_heat"], dev), _t(c["kp_valid"], dev))
    (KEYPOINT_UPSTREAM * loss).backward()
    g = _np(d.grad)
    assert not g[~c["kp_valid"]].any()
    if not c["kp_valid"].any():
        assert loss.item() == 0.0
    figure("keypoint_loss", "P=%d K=%d %dx%d cl=%d" % (c["kp_P"], c["kp_K"], c["kp_H"], c["kp_W"], c["kp_channels_last"]),
           tc.rel_err(loss.item(), rl), tc.grad_err(g, rg), bounds=(KEYPOINT_BOUND, KEYPOINT_BOUND))
    keep.update(kp_loss=loss.detach(), kp_grad=d.grad.contiguous())
    return keep


# ------------------------------------------------------------------------------------------ RPN loss and decode
def _rpn_refs(c):
    args = (c["obj"], c["box"], c["anchors"], c["matched"], c["pos"], c["neg"], c["gt"], c["beta"], c["weights"], c["A"])
    ref = tc.rpn_loss_reference(*args)
    r32 = tc.rpn_loss_reference(*args, dtype=torch.float32)
    aten = (max(tc.rel_err(r32[0], ref[0]), tc.rel_err(r32[1], ref[1])), tc.grad_err(r32[2] + r32[3], ref[2] + ref[3]))
    return dict(ref=ref, aten={"rpn_loss": aten})


def run_rpn_loss_decode(c, r, dev):
    """`_C.rpn_loss` forward and backward (upstream tc.RPN_UPSTREAM) against fp64, then one `_C.rpn_decode` per level at
    non-zero `col` / `off` into NaN-filled results, against RPNPostProcessor._level_candidates (the ATen composition) on the
    same device.  On the MI355X the decode is bit-equal to that composition; the host emulation's glibc expf differs from
    ATen's vectorised exp in the last place, so there boxes agree to rtol 1e-6 / atol 4e-3 and the min_size test is compared
    away from its edge (tests/test_targets_edges_emu.py).  csrc/targets.hip sums the loss in a fixed order without atomics."""
    from maskrcnn_benchmark.modeling.box_coder import BoxCoder
    from maskrcnn_benchmark.modeling.rpn.inference import RPNPostProcessor
    C_ = _C()
    exact = torch.device(dev).type != "cpu"
    N, A, L = c["N"], c["A"], c["L"]
    ro, rb, rgo, rgb = r["ref"]
    obj = [_t(t, dev).requires_grad_() for t in c["obj"]]
    box = [_t(t, dev).requires_grad_() for t in c["box"]]
    anchors = _t(c["anchors"], dev)
    lo, lb = C_.rpn_loss(obj, box, anchors, _t(c["matched"], dev), _t(c["pos"], dev), _t(c["neg"], dev), _t(c["gt"], dev),
                         c["beta"], c["weights"])
    (tc.RPN_UPSTREAM[0] * lo + tc.RPN_UPSTREAM[1] * lb).backward()
    gobj, gbox = [_np(t.grad) for t in obj], [_np(t.grad) for t in box]
    if not (c["pos"] | c["neg"]).any():
        assert lo.item() == 0.0 and lb.item() == 0.0 and all(not g.any() for g in gobj + gbox)
    if not c["pos"].any():
        assert lb.item() == 0.0 and all(not g.any() for g in gbox)
    value = max(tc.rel_err(lo.item(), ro), tc.rel_err(lb.item(), rb))
    figure("rpn_loss", "N=%d A=%d L=%d T=%d" % (N, A, L, c["anchors"].shape[0]), value, tc.grad_err(gobj + gbox, rgo + rgb))
    keep = dict(objectness_loss=lo.detach(), box_loss=lb.detach())
    keep.update({"grad_objectness_%d" % l: t.grad for l, t in enumerate(obj)})
    keep.update({"grad_box_%d" % l: t.grad for l, t in enumerate(box)})
    # decode, level by level
    first = 0
    hw = torch.tensor([[h, w] for h, w in c["sizes"]], dtype=torch.float32, device=dev)
    for l, ((H, W), (topn, min_size, col, off)) in enumerate(zip(c["shapes"], c["decode"])):
        lv_anchors = anchors[first:first + A * H * W]
        first += A * H * W
        o = obj[l].detach()
        reg = (box[l].detach() * (c["reg_scale"] / 0.2)).contiguous()
        if c["clip"]:
            reg[0, 2::4] += 6.0              # width deltas past bbox_xform_clip and past the image
        post = RPNPostProcessor(topn, topn, 0.7, min_size, BoxCoder((1.0, 1.0, 1.0, 1.0)))
        boxes, scores, ok = post._level_candidates(lv_anchors, o, reg, c["sizes"])
        k = boxes.shape[1]
        assert k == min(topn, A * H * W)
        s, idx = o.permute(0, 2, 3, 1).reshape(N, -1).sigmoid().topk(k, dim=1, sorted=True)
        assert torch.equal(s, scores)
        K, R = col + k + 2, off + N * k + 3
        ob = torch.full((N, K, 4), float("nan"), device=dev)
        os_ = torch.full((N, K), float("nan"), device=dev)
        nb = torch.full((R, 4), float("nan"), device=dev)
        ns = torch.full((R,), float("nan"), device=dev)
        okk = torch.full((R,), 7, dtype=torch.uint8, device=dev)
        C_.rpn_decode(reg, idx, s, lv_anchors, hw, post.box_coder.weights, post.box_coder.bbox_xform_clip, min_size,
                      ob, os_, col, nb, ns, okk, off)
        assert ob[:, :col].isnan().all() and ob[:, col + k:].isnan().all() and os_[:, :col].isnan().all() and os_[:, col + k:].isnan().all()
        for a in (nb, ns):
            assert a[:off].isnan().all() and a[off + N * k:].isnan().all()
        assert (okk[:off] == 7).all() and (okk[off + N * k:] == 7).all()
        got_b, got_ok = ob[:, col:col + k], okk[off:off + N * k].bool()
        assert torch.equal(os_[:, col:col + k], scores)
        flat_ok = ok.reshape(-1)
        if exact:
            assert torch.equal(got_b, boxes), (l, first_mismatch(got_b, boxes))
            assert torch.equal(got_ok, flat_ok), l
        else:
            assert torch.allclose(got_b, boxes, rtol=1e-6, atol=4e-3), l
            size = torch.minimum(boxes[..., 2] - boxes[..., 0], boxes[..., 3] - boxes[..., 1]).reshape(-1) + 1
            sure = (size - min_size).abs() > 1e-2
            assert torch.equal(got_ok[sure], flat_ok[sure]), l
        far = torch.tensor([-1e6, -1e6, -1e6 + 1, -1e6 + 1], device=dev)
        assert torch.equal(nb[off:off + N * k], torch.where(got_ok[:, None], got_b.reshape(-1, 4), far))
        assert torch.equal(ns[off:off + N * k], torch.where(got_ok, scores.reshape(-1), scores.new_full((), -1.0)))
        keep.update({"decode_boxes_%d" % l: got_b.contiguous(), "decode_ok_%d" % l: okk[off:off + N * k].contiguous()})
    return keep


def first_mismatch(a, b):
    d = (a != b).nonzero()
    if d.numel() == 0:
        return "equal"
    i = tuple(d[0].tolist())
    return "%d differ, first at %s: %r vs %r" % (d.shape[0], i, a[i].item(), b[i].item())


# ------------------------------------------------------------------------------------------ sparse RPN-head backward
def _sparse_refs(c):
    """fp64 autograd of the dense composition on the CPU (tests/test_rpn_sparse_bwd_emu.py::_dense_f64) -> {name: gradient}"""
    import torch.nn.functional as F
    pp = {k: torch.from_numpy(v).double().requires_grad_() for k, v in zip(fuzz_cases.SPARSE_PARAMS, c["params"])}
    xs = [torch.from_numpy(f).double().requires_grad_() for f in c["feats"]]
    ts = [F.relu(F.conv2d(x, pp["conv.weight"], pp["conv.bias"], padding=1)) for x in xs]
    outs = [F.conv2d(t, pp["cls_logits.weight"], pp["cls_logits.bias"]) for t in ts] + \
           [F.conv2d(t, pp["bbox_pred.weight"], pp["bbox_pred.bias"]) for t in ts]
    torch.autograd.backward(outs, [torch.from_numpy(g).double() for g in c["gobj"] + c["gbox"]])
    ref = {k: v.grad for k, v in pp.items()}
    ref.update({"x%d" % i: x.grad for i, x in enumerate(xs)})
    return dict(grads=ref, outs=[o.detach() for o in outs])


def run_rpn_head_sparse(c, r, dev):
    """`_C.rpn_head_sparse` forward, then its backward on the case's incoming gradients, against fp64 dense autograd on the
    CPU at the criterion of test_reduced_shape_equals_fp64_autograd_on_the_cpu (relative Frobenius distance per tensor <=
    GRAD_TOL, floored).  The row list overflows on exactly one seed: grad_w_conv is all NaN, the counter rises by one and every
    other gradient stays finite.  include/detops.h: the backward is deterministic, no atomics on floating-point data — asked
    here of two backwards over ONE saved forward (the forward's convolutions are the library's, whose kernels may add in another order
    from call to call), which is also what is compared between clean and dirty memory where the two forwards agree in bits."""
    from test_whole_model_parity import GRAD_TOL, _grad_spread
    C_ = _C()
    cl = torch.channels_last
    overflow = c["rows"] > c["max_rows"]
    pp = {k: _t(v, dev) for k, v in zip(fuzz_cases.SPARSE_PARAMS, c["params"])}
    pp = {k: (v.contiguous(memory_format=cl) if v.dim() == 4 else v).requires_grad_() for k, v in pp.items()}
    xs = [_t(f, dev).contiguous(memory_format=cl).requires_grad_() for f in c["feats"]]
    grads = [_t(g, dev) for g in c["gobj"] + c["gbox"]]
    C_.rpn_sparse_overflows(reset=True)
    obj, box = C_.rpn_head_sparse(xs, *[pp[k] for k in fuzz_cases.SPARSE_PARAMS], c["max_rows"])
    for o, want in zip(obj + box, r["outs"]):
        assert o.is_contiguous() and torch.allclose(o.detach().cpu().double(), want, rtol=1e-5, atol=1e-5)
    leaves = [pp[k] for k in fuzz_cases.SPARSE_PARAMS] + xs
    names = list(fuzz_cases.SPARSE_PARAMS) + ["x%d" % i for i in range(len(xs))]
    got = dict(zip(names, torch.autograd.grad(obj + box, leaves, grads, retain_graph=True)))
    again = dict(zip(names, torch.autograd.grad(obj + box, leaves, grads)))
    assert C_.rpn_sparse_overflows(reset=True) == (2 if overflow else 0)
    for k in names:
        assert got[k].shape == again[k].shape and torch.equal(got[k].isnan(), again[k].isnan())
        assert torch.equal(got[k].nan_to_num(), again[k].nan_to_num()), "two backwards over one forward: " + k
    if overflow:
        assert bool(got["conv.weight"].isnan().all())
        assert all(bool(torch.isfinite(v).all()) for k, v in got.items() if k != "conv.weight")
    elif c["rows"] == 0:                  # no row at all: exact zeros (the criterion's norm ratio has no denominator)
        assert all(not bool(v.any()) for v in got.values()) and all(not bool(v.any()) for v in r["grads"].values())
    else:
        spread = _grad_spread({k: v.detach().double().cpu() for k, v in got.items()}, r["grads"])
        worst = max(spread, key=spread.get)
        print("FIGURE rpn_head_sparse   C=%d rows=%d max_rows=%d largest spread %.3g (%s)" % (c["C"], c["rows"], c["max_rows"], spread[worst], worst))
        for k, v in spread.items():
            assert v <= GRAD_TOL, (k, v)
    keep = {"forward_%d" % i: o.detach() for i, o in enumerate(obj + box)}
    keep.update({"grad " + k: v.contiguous() for k, v in got.items()})
    return keep


# ------------------------------------------------------------------------------------------ masks: inference and evaluation
def _rle_runs(plane):
    """bool [H, W] -> uncompressed COCO RLE: run lengths in column-major order, starting with a 0-run"""
    f = np.asarray(plane, bool).flatten(order="F").astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], f]))) if f.size else np.zeros(0, np.int64)
    bounds = np.concatenate([[0], edges, [f.size]])
    return [int(v) for v in np.diff(bounds)]


def _pack_plane(plane):
    """bool [H, W] -> (words uint64 [H * ceil(W / 64)]: bit b of word c of a row = pixel 64 c + b, pixel count, extent = first /
    last non-empty row, first / last non-empty word column; (H, -1, ceil(W / 64), -1) for an empty plane)"""
    H, W = plane.shape
    WW = (W + 63) // 64
    padded = np.zeros((H, WW * 64), np.uint8)
    padded[:, :W] = plane != 0
    words = np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(H, WW)
    rows, cols = np.flatnonzero(words.any(1)), np.flatnonzero(words.any(0))
    extent = [int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])] if rows.size else [H, -1, WW, -1]
    return words.reshape(-1), int(padded.sum()), extent


def _voc_iou(d, g):
    """the VOC evaluation's IoU in fp32 (include/detops.h, EVAL_VOC: x2 + 1, y2 + 1, then "+ 1" widths; a union of 0 gives 0)"""
    f, one = np.float32, np.float32(1)
    d, g = [f(v) for v in d], [f(v) for v in g]
    dx2, dy2, gx2, gy2 = d[2] + one, d[3] + one, g[2] + one, g[3] + one
    area_d = ((dx2 - d[0]) + one) * ((dy2 - d[1]) + one)
    area_g = ((gx2 - g[0]) + one) * ((gy2 - g[1]) + one)
    w = max((min(dx2, gx2) - max(d[0], g[0])) + one, f(0))
    h = max((min(dy2, gy2) - max(d[1], g[1])) + one, f(0))
    inter = f(w * h)
    u = f(f(area_d + area_g) - inter)
    return float(f(inter / u)) if u != 0 else 0.0


def _mask_refs(c):
    """the CPU planes of paste_masks_torch and their near-threshold pixels (tests/test_masker_cpu.py::near_planes) per
    detection; the box with a NaN coordinate and windows off the image are all-zero planes (include/detops.h)"""
    import test_masker_cpu as mcpu
    from maskrcnn_benchmark.modeling.roi_heads.mask_head import inference as mi
    dtype = getattr(torch, c["dtype"])
    maps = torch.from_numpy(c["maps"]).to(dtype)
    boxes = torch.from_numpy(c["boxes"])
    planes, near, det_sizes = [], [], []
    k = 0
    for (H, W), n in zip(c["sizes"], c["counts"]):
        for j in range(k, k + n):
            if bool(torch.isnan(boxes[j]).any()):
                planes.append(torch.zeros((H, W), dtype=torch.bool))
                near.append(torch.zeros((H, W), dtype=torch.bool))
            else:
                m, b = maps[j:j + 1].float().unsqueeze(1), boxes[j:j + 1]
                planes.append(mi.paste_masks_torch(m, b, H, W, c["threshold"], c["padding"])[0, 0])
                near.append(mcpu.near_planes(m, b, H, W, c["threshold"], c["padding"])[0])
            det_sizes.append((H, W))
        k += n
    return dict(dtype=dtype, maps=maps, planes=planes, near=near, det_sizes=det_sizes)


def run_mask_chain(c, r, dev):
    """paste_masks -> paste_masks_rle -> rle_strings -> rle_string_decode -> mask_pack_rle, mask_pack of the dense planes,
    mask_pair_counts against the ground-truth planes -> eval_iou (segm, bbox, VOC) -> eval_match, one problem per image.
    The pasted planes equal paste_masks_torch outside its near-threshold pixels (tests/test_masker_gpu.py); every later step
    is exact and is checked against numpy restatements applied to the planes the FIRST step produced: the runs, the strings
    (tests/rle_string_refs.py), the packs (popcounts), the pair counts (brute force), the IoUs (tests/eval_refs.py, fp64) and the
    matching (eval_refs.evaluate_img).  include/detops.h: every one of these writes each output element exactly once in a fixed
    order (integer atomics only for areas and extents)."""
    import eval_refs
    import rle_string_refs
    C_ = _C()
    D, sizes, counts = c["D"], c["sizes"], c["counts"]
    maps, boxes = r["maps"].to(dev), _t(c["boxes"], dev)
    thr, pad = c["threshold"], c["padding"]
    flat, views = C_.paste_masks(maps, boxes, sizes, thr, pad, counts=counts)
    assert flat.dtype == torch.uint8 and (D == 0 or int(flat.max()) <= 1)
    assert [tuple(v.shape) for v in views] == [(n, 1, h, w) for (h, w), n in zip(sizes, counts)]
    got = [p for v in views for p in v[:, 0].cpu()]
    for k, (g, p, n) in enumerate(zip(got, r["planes"], r["near"])):
        assert g.shape == p.shape and torch.equal(g | n, p | n), (
            "detection %d: %d pixels differ outside the near set" % (k, int(((g != p) & ~n).sum())))
    if D >= 2:
        assert not got[1].any()                          # the NaN box
    planes = [g.numpy() for g in got]                    # what every later step is held to
    keep = dict(planes=flat)
    # uncompressed RLE
    runs, run_offset = C_.paste_masks_rle(maps, boxes, sizes, thr, pad, counts=counts)
    want_runs = [_rle_runs(p) for p in planes]
    want_off = np.concatenate([[0], np.cumsum([len(w) for w in want_runs])]).astype(np.int64)
    assert runs.dtype == torch.int32 and np.array_equal(_np(run_offset), want_off)
    assert _np(runs).tolist() == [v for w in want_runs for v in w]
    # strings and back
    data, byte_offset = C_.rle_strings(runs, run_offset)
    want_strings = [rle_string_refs.rle_to_string(w) for w in want_runs]
    assert C_.rle_string_list(data, byte_offset) == want_strings
    assert _np(byte_offset).tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want_strings])]).tolist()
    runs2, run_offset2 = C_.rle_string_decode(data, byte_offset, hw=torch.tensor(r["det_sizes"], dtype=torch.int32).reshape(-1, 2))
    assert torch.equal(runs2.cpu(), runs.cpu()) and torch.equal(run_offset2.cpu(), run_offset.cpu())
    keep.update(runs=runs, run_offset=run_offset, strings=data, byte_offset=byte_offset, runs_decoded=runs2)
    # packs: from the runs and from the dense planes
    packed = [_pack_plane(p) for p in planes]
    want_words = np.concatenate([w for w, _, _ in packed]) if packed else np.zeros(0, np.uint64)
    per = [h * ((w + 63) // 64) for h, w in r["det_sizes"]]
    want_pack = (want_words.view(np.int64), np.concatenate([[0], np.cumsum(per)])[:-1].astype(np.int64),
                 np.asarray(r["det_sizes"], np.int32).reshape(-1, 2), np.asarray([a for _, a, _ in packed], np.int32),
                 np.asarray([e for _, _, e in packed], np.int32).reshape(-1, 4))
    hw_all = torch.tensor(r["det_sizes"], dtype=torch.int32).reshape(-1, 2)
    pack_rle = C_.mask_pack_rle(runs2, run_offset2, hw_all)
    pack_dense = C_.mask_pack([v[:, 0] for v in views])
    for name, pack in (("mask_pack_rle", pack_rle), ("mask_pack", pack_dense)):
        for g, w, part in zip(pack, want_pack, ("words", "word_offset", "hw", "area", "extent")):
            assert _np(g).dtype == w.dtype and np.array_equal(_np(g), w), (name, part)
    keep.update({"pack_rle_%d" % i: t for i, t in enumerate(pack_rle)})
    keep.update({"pack_dense_%d" % i: t for i, t in enumerate(pack_dense)})
    # evaluation: one problem per image, detections in input order (scores descending with the index)
    gt_planes = [_t(g, dev) for g in c["gt_planes"]]
    gt_pack = C_.mask_pack(gt_planes)
    G = [g.shape[0] for g in c["gt_planes"]]
    cs = lambda v: torch.from_numpy(np.concatenate([[0], np.cumsum(v)]).astype(np.int64))  # noqa: E731
    dt_offset, gt_offset = cs(counts).to(torch.int32).to(dev), cs(G).to(torch.int32).to(dev)
    iou_offset = cs([d * g for d, g in zip(counts, G)]).to(dev)
    total = int(iou_offset[-1])
    pick = lambda p: (p[0], p[1], p[2], p[4])  # noqa: E731
    pair = C_.mask_pair_counts(pick(pack_rle), pick(gt_pack), dt_offset, gt_offset, iou_offset, total)
    gts_flat = [g for per_image in c["gt_planes"] for g in per_image]
    crowd = np.concatenate(c["gt_crowd"]) if sum(G) else np.zeros(0, np.uint8)
    gt_boxes = np.concatenate(c["gt_boxes"]) if sum(G) else np.zeros((0, 4), np.float32)
    pairs, d0, g0 = [], 0, 0
    for n, g in zip(counts, G):
        pairs += [(d0 + i, g0 + j) for i in range(n) for j in range(g)]
        d0, g0 = d0 + n, g0 + g
    want_pair = [int((planes[i] & (gts_flat[j] != 0)).sum()) for i, j in pairs]
    assert pair.dtype == torch.int32 and _np(pair).tolist() == want_pair
    keep["pair_counts"] = pair
    tcrowd = _t(crowd, dev)
    iou = C_.eval_iou(C_.EVAL_COCO_SEGM, dt_offset, gt_offset, iou_offset, total, counts=pair, dt_area=pack_rle[3], gt_area=gt_pack[3],
                      gt_crowd=tcrowd)
    want_iou = np.asarray([eval_refs.mask_iou(planes[i], gts_flat[j] != 0, bool(crowd[j])) for i, j in pairs], np.float64)
    assert iou.dtype == torch.float64 and np.array_equal(_np(iou), want_iou)
    keep["iou_segm"] = iou
    dt_boxes = np.nan_to_num(c["boxes"], nan=0.0)
    kw = dict(dt_boxes=_t(dt_boxes, dev), gt_boxes=_t(gt_boxes, dev), gt_crowd=tcrowd)
    got_b = C_.eval_iou(C_.EVAL_COCO_BBOX, dt_offset, gt_offset, iou_offset, total, **kw)
    assert np.array_equal(_np(got_b), np.asarray([eval_refs.bbox_iou(dt_boxes[i], gt_boxes[j], bool(crowd[j])) for i, j in pairs], np.float64))
    got_v = C_.eval_iou(C_.EVAL_VOC, dt_offset, gt_offset, iou_offset, total, **kw)
    assert np.array_equal(_np(got_v), np.asarray([_voc_iou(dt_boxes[i], gt_boxes[j]) for i, j in pairs], np.float64))
    keep.update(iou_bbox=got_b, iou_voc=got_v)
    dt_area, gt_area = pack_rle[3].double(), gt_pack[3].double()
    dtm, dti, gti = C_.eval_match(C_.EVAL_COCO_SEGM, iou, dt_offset, gt_offset, iou_offset, (D, sum(G), max(G + [0])), tcrowd,
                                  eval_refs.IOU_THRS, dt_area=dt_area, gt_area=gt_area, area_rngs=eval_refs.AREA_RNGS)
    dtm, dti, gti = _np(dtm), _np(dti), _np(gti)
    T = len(eval_refs.IOU_THRS)
    d0, g0 = 0, 0
    for n, g in zip(counts, G):
        dts = [{"score": -float(i), "mask": planes[d0 + i]} for i in range(n)]
        gts = [{"mask": gts_flat[g0 + j] != 0, "iscrowd": int(crowd[g0 + j]), "area": float((gts_flat[g0 + j] != 0).sum())} for j in range(g)]
        for a, rng in enumerate(eval_refs.AREA_RNGS):
            e = eval_refs.evaluate_img(dts, gts, "segm", rng, 10 ** 6)
            if e is None:
                continue
            assert np.array_equal(dtm[a][:, d0:d0 + n], np.asarray(e["dt_match"], np.int32).reshape(T, n)), (a, d0)
            assert np.array_equal(dti[a][:, d0:d0 + n] != 0, np.asarray(e["dt_ignore"], bool).reshape(T, n)), (a, d0)
            assert np.array_equal(gti[a][g0:g0 + g] != 0, np.asarray(e["gt_ignore"], bool)), (a, g0)
        d0, g0 = d0 + n, g0 + g
    keep.update(dt_match=torch.from_numpy(dtm), dt_ignore=torch.from_numpy(dti), gt_ignore=torch.from_numpy(gti))
    return keep


# ------------------------------------------------------------------------------------------ test-time augmentation merge
def _aug_refs(c):
    case = bbox_aug_cases.make_case(**c)
    return dict(case=case, ref=bbox_aug_cases.reference(case))


def run_bbox_aug_merge(c, r, dev):
    """count / host read / write through one workspace: bit-equal to the torch formulation (include/detops.h: exact)"""
    case = r["case"]
    want_b, want_s, want_seg, want_longest = r["ref"]
    boxes, scores, seg, longest = _C().bbox_aug_merge(case["boxes"].to(dev), case["scores"].to(dev), case["row_offset"], case["geom"],
                                                      case["ratio"], case["N"], case["T"], bbox_aug_cases.THRESH)
    assert seg.dtype == torch.int32 and seg.cpu().tolist() == want_seg.tolist() and longest == want_longest
    assert boxes.shape == want_b.shape and scores.shape == want_s.shape
    assert torch.equal(bbox_aug_cases.bits(scores), bbox_aug_cases.bits(want_s))
    assert torch.equal(bbox_aug_cases.bits(boxes), bbox_aug_cases.bits(want_b))
    if c["C"] == 1 or c["pass_rate"] == 0.0 or not sum(map(sum, c["rows"])):
        assert boxes.shape[0] == 0 and longest == 0 and not seg.any()
    return dict(boxes=boxes, scores=scores, seg_offsets=seg)


# ------------------------------------------------------------------------------------------ GroupNorm
def _rounded(a, dtype):
    return None if a is None else torch.from_numpy(a).to(dtype)


def _gn_refs(c):
    dtype = getattr(torch, c["dtype"])
    return dict(dtype=dtype, x=_rounded(c["x"], dtype), res=_rounded(c["residual"], dtype), gy=_rounded(c["gy"], dtype))


def _placed_cl(t, offset, dev, channels_last=True):
    """host [N, C, H, W] -> the same values on `dev` as a channels-last tensor whose storage starts `offset` elements into its
    allocation (`channels_last=False`: C == 1 or H == W == 1, where that layout is the NCHW one as well)"""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=dev)
    d = buf[offset:].view(N, H, W, C).permute(0, 3, 1, 2)
    d.copy_(t)
    assert d.storage_offset() == offset and _C().is_channels_last(d) == channels_last
    return d


def run_group_norm(c, r, dev):
    """forward and backward through the wrappers under the checks of tests/test_group_norm_gpu.py (statistics, output against
    fp64 from the kernel's own statistics, backward against fp64 autograd within 8 x ATen's fp32 error or one ulp of a half
    type).  An absent gamma / beta is 1 / 0 in the reference.  include/detops.h: forward and backward are deterministic"""
    import test_group_norm_gpu as gn
    C_ = _C()
    N, C, G, relu, dtype, o = c["N"], c["C"], c["G"], c["relu"], r["dtype"], c["offset"]
    x, res, gy = r["x"], r["res"], r["gy"]
    if C == 1 or c["H"] * c["W"] == 1:
        # such a tensor is NCHW-contiguous as well: `_C.is_channels_last` says no, the layer keeps it on ATen, and the wrapper
        # refuses it rather than guess a layout.  What the sweep can check of this draw is that refusal
        import pytest
        x_d = _placed_cl(x, o, dev, channels_last=False)
        assert not C_.group_norm_supported(x_d, G)
        with pytest.raises(RuntimeError, match="channels-last"):
            C_.group_norm_forward(x_d, G, _t(c["gamma"], dev), _t(c["beta"], dev), EPS, None, relu)
        return {}
    x_d = _placed_cl(x, o, dev)
    res_d = None if res is None else _placed_cl(res, o, dev)
    gamma, beta = _t(c["gamma"], dev), _t(c["beta"], dev)
    gamma1 = gamma if gamma is not None else torch.ones(C, device=dev)
    beta0 = beta if beta is not None else torch.zeros(C, device=dev)
    y, mu, rs = C_.group_norm_forward(x_d, G, gamma, beta, EPS, res_d, relu)
    assert y.dtype == dtype and y.shape == x_d.shape and C_.is_channels_last(y)
    assert mu.dtype == torch.float32 and tuple(mu.shape) == (N, G) and tuple(rs.shape) == (N, G)
    gn._check_statistics(x, mu, rs, G)
    gn._check_output(x, res, gamma1, beta0, y, mu, rs, G, relu, dtype)
    gy_d = _placed_cl(gy, o, dev)
    got = C_.group_norm_backward(gy_d, x_d, y, G, gamma, mu, rs, relu, res is not None, gamma is not None, beta is not None)
    assert (got[1] is None) == (res is None) and (got[2] is None) == (gamma is None) and (got[3] is None) == (beta is None)
    assert got[0].dtype == dtype and C_.is_channels_last(got[0])
    masked = gy.double() * (y.cpu() > 0).double() if relu else gy.double()
    fresh = lambda t: None if t is None else t.detach().cpu().clone()      # noqa: E731  (_host_backward makes leaves of its arguments)
    ref = gn._host_backward(fresh(x), fresh(res), fresh(gamma1), fresh(beta0), masked, G, torch.float64)
    aten = gn._host_backward(fresh(x), fresh(res), fresh(gamma1), fresh(beta0), masked, G, torch.float32)
    floor = 0.0 if dtype == torch.float32 else torch.finfo(dtype).eps
    for name, mine in zip(("grad_x", "grad_residual", "grad_gamma", "grad_beta"), got):
        if mine is None:
            continue
        err, theirs = gn._rel(mine.cpu(), ref[name]), gn._rel(aten[name], ref[name])
        allowed = max(8 * theirs, floor)
        print("  %s: error %.3g, ATen fp32 %.3g, allowed %.3g" % (name, err, theirs, allowed))
        assert err <= allowed, (name, err, theirs, allowed)
    keep = dict(y=y.contiguous(), mean=mu, rstd=rs)
    keep.update({name: t.contiguous() for name, t in zip(("grad_x", "grad_residual", "grad_gamma", "grad_beta"), got) if t is not None})
    return keep


# ------------------------------------------------------------------------------------------ bias (+ ReLU) and column sums
def _bias_refs(c):
    dtype = getattr(torch, c["dtype"])
    return dict(dtype=dtype, x=_rounded(c["x"], dtype), gy=_rounded(c["gy"], dtype), m=_rounded(c["m"], dtype))


def run_bias_act(c, r, dev):
    """`_C.bias_act` forward and backward on a width the fused kernels serve, and `_C.column_sum` of a narrow matrix; the
    select of the backward is exact, the sums are fp32 sums of the stored values in a fixed order (include/detops.h:
    deterministic)"""
    C_ = _C()
    dtype, relu, tol = r["dtype"], c["relu"], BIAS_TOL[c["dtype"]]
    cl = torch.channels_last
    assert bool(C_.lib.detops_bias_act_supported(c["C"])), "the fused kernels serve the widths of BIAS_C"
    xi = r["x"].clone().to(dev).contiguous(memory_format=cl).requires_grad_()      # (a copy: the reference tensors stay as they are)
    bias = _t(c["bias"], dev).requires_grad_()
    one_row = c["rows"] == 1               # [1, C, 1, 1] is NCHW-contiguous as well: not "channels-last" to the product, same bytes
    assert C_.bias_act_supported(xi, bias) == (not one_row)
    y = C_.bias_act(xi, bias, relu)
    assert C_.is_channels_last(y) == (not one_row) and y.dtype == dtype
    y.backward(r["gy"].to(dev).contiguous(memory_format=cl))
    ref = r["x"].double() + torch.from_numpy(c["bias"]).double().view(1, -1, 1, 1)
    ref = ref.relu() if relu else ref
    assert float((y.detach().cpu().double() - ref).abs().max()) <= tol * max(1.0, float(ref.abs().max()))
    g = r["gy"].float() * ((y.detach().cpu().float() > 0).float() if relu else 1.0)
    assert torch.equal(xi.grad.cpu().float(), g)                   # a select: exact in every storage type
    assert bias.grad.dtype == torch.float32
    want = g.double().sum((0, 2, 3))
    print("FIGURE bias_act          C=%d rows=%d %s bias gradient error %.3g" % (c["C"], c["rows"], c["dtype"],
                                                                                float((bias.grad.cpu().double() - want).abs().max())))
    assert float((bias.grad.cpu().double() - want).abs().max()) <= 1e-5 * max(1.0, float(g.abs().double().sum((0, 2, 3)).max()))
    sums = C_.column_sum(r["m"].to(dev))
    want = r["m"].double().sum(0)
    assert sums.dtype == torch.float32 and tuple(sums.shape) == (c["Cs"],)
    print("FIGURE column_sum        C=%d rows=%d %s error %.3g" % (c["Cs"], c["rows"], c["dtype"],
                                                                  float((sums.cpu().double() - want).abs().max())))
    assert float((sums.cpu().double() - want).abs().max()) <= 1e-5 * max(1.0, float(r["m"].double().abs().sum(0).max()))
    return dict(y=y.detach().contiguous(), grad_x=xi.grad.contiguous(), grad_bias=bias.grad, column_sums=sums)


_REFS = {"targets_chain": _chain_refs, "head_losses": _loss_refs, "rpn_loss_decode": _rpn_refs, "rpn_head_sparse": _sparse_refs,
         "mask_chain": _mask_refs, "bbox_aug_merge": _aug_refs, "group_norm": _gn_refs, "bias_act": _bias_refs}
RUN = {"targets_chain": run_targets_chain, "head_losses": run_head_losses, "rpn_loss_decode": run_rpn_loss_decode,
       "rpn_head_sparse": run_rpn_head_sparse, "mask_chain": run_mask_chain, "bbox_aug_merge": run_bbox_aug_merge,
       "group_norm": run_group_norm, "bias_act": run_bias_act}
assert set(RUN) == set(_REFS) == set(fuzz_cases.EXTENSION)
