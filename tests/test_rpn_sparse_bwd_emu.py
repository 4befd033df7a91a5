"""Sparse backward of the RPN head (csrc/targets.hip, `_C.rpn_head_sparse`) WITHOUT a GPU: the product's own wrappers and
autograd function over the host-emulation build of the HIP sources (cpu_shim backend "emu-lib"), against fp64
`torch.autograd` of the plain dense composition (conv2d + bias + ReLU + two 1x1 convolutions).  Criterion: the project's
own (tests/test_whole_model_parity.py): relative Frobenius distance per tensor <= GRAD_TOL, with its floor."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cpu_shim
from maskrcnn_benchmark import _C
from test_whole_model_parity import GRAD_TOL, _grad_spread

C, A, N = 16, 3, 2
LEVELS = [(24, 32), (12, 16), (6, 8), (3, 4), (2, 2)]
PARAMS = ("conv.weight", "conv.bias", "cls_logits.weight", "cls_logits.bias", "bbox_pred.weight", "bbox_pred.bias")


@pytest.fixture(autouse=True)
def _product_wrappers():
    with cpu_shim.install("emu-lib"):
        _C.rpn_sparse_overflows(reset=True)
        yield


def _head(seed=0, weights_channels_last=True):
    g = torch.Generator().manual_seed(seed)
    p = {"conv.weight": torch.randn(C, C, 3, 3, generator=g) * 0.2, "conv.bias": torch.randn(C, generator=g) * 0.1,
         "cls_logits.weight": torch.randn(A, C, 1, 1, generator=g) * 0.3, "cls_logits.bias": torch.randn(A, generator=g) * 0.1,
         "bbox_pred.weight": torch.randn(4 * A, C, 1, 1, generator=g) * 0.3, "bbox_pred.bias": torch.randn(4 * A, generator=g) * 0.1}
    if weights_channels_last:
        p = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in p.items()}
    feats = [torch.randn(N, C, h, w, generator=g).contiguous(memory_format=torch.channels_last) for h, w in LEVELS]
    return p, feats


def _grads_from_entries(entries, seed=1):
    """entries: (level, image, y, x, anchor) -> zero gradients except random values at those anchors"""
    g = torch.Generator().manual_seed(seed)
    gobj = [torch.zeros(N, A, h, w) for h, w in LEVELS]
    gbox = [torch.zeros(N, 4 * A, h, w) for h, w in LEVELS]
    for l, n, y, x, a in entries:
        gobj[l][n, a, y, x] = float(torch.randn((), generator=g)) * 2.5
        gbox[l][n, 4 * a:4 * a + 4, y, x] = torch.randn(4, generator=g) * 0.7
    return gobj, gbox


def _dense_f64(p, feats, gobj, gbox):
    """fp64 autograd of the dense composition -> {name: gradient}"""
    pp = {k: v.double().contiguous().requires_grad_() for k, v in p.items()}
    xs = [f.double().contiguous().requires_grad_() for f in feats]
    outs = []
    for x in xs:
        t = F.relu(F.conv2d(x, pp["conv.weight"], pp["conv.bias"], padding=1))
        outs.append(F.conv2d(t, pp["cls_logits.weight"], pp["cls_logits.bias"]))
    for x in xs:
        t = F.relu(F.conv2d(x, pp["conv.weight"], pp["conv.bias"], padding=1))
        outs.append(F.conv2d(t, pp["bbox_pred.weight"], pp["bbox_pred.bias"]))
    torch.autograd.backward(outs, [g.double() for g in gobj + gbox])
    ref = {k: v.grad for k, v in pp.items()}
    ref.update({"x%d" % i: x.grad for i, x in enumerate(xs)})
    return ref, [o.detach() for o in outs]


def _sparse(p, feats, gobj, gbox, max_rows):
    pp = {k: v.clone(memory_format=torch.preserve_format).requires_grad_() for k, v in p.items()}
    xs = [f.clone(memory_format=torch.preserve_format).requires_grad_() for f in feats]
    obj, box = _C.rpn_head_sparse(xs, *[pp[k] for k in PARAMS], max_rows)
    torch.autograd.backward(obj + box, gobj + gbox)
    got = {k: v.grad for k, v in pp.items()}
    got.update({"x%d" % i: x.grad for i, x in enumerate(xs)})
    return got, pp, xs, [o.detach() for o in obj + box]


def _check(got, ref, what):
    spread = _grad_spread({k: v.double() for k, v in got.items()}, ref)
    worst = max(spread, key=spread.get)
    print("\nsparse RPN-head backward %s: largest spread %.3g (%s)" % (what, spread[worst], worst))
    for k, s in spread.items():
        assert s <= GRAD_TOL, (what, k, s)


CASES = {
    "corner-and-edge": [(0, 0, 0, 0, 0), (0, 1, 23, 31, 2), (0, 0, 0, 5, 1), (1, 0, 7, 0, 0), (4, 1, 1, 1, 2), (3, 0, 2, 3, 1)],
    "two-anchors-of-one-pixel": [(0, 0, 5, 5, 0), (0, 0, 5, 5, 2), (2, 1, 3, 3, 1), (2, 1, 3, 3, 2)],
    "overlapping-footprints": [(0, 0, 10, 10, 1), (0, 0, 10, 11, 0), (0, 0, 11, 10, 2), (0, 0, 12, 12, 0), (1, 1, 3, 3, 0),
                               (1, 1, 4, 4, 1), (1, 1, 3, 5, 2), (4, 0, 0, 0, 0), (4, 0, 1, 1, 1), (4, 0, 0, 1, 0)],
    "levels-without-rows": [(1, 0, 4, 4, 0), (3, 1, 0, 0, 2)],
}


@pytest.mark.parametrize("weights_channels_last", [True, False], ids=["w-nhwc", "w-contiguous"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_sparse_backward_equals_fp64_autograd_of_the_dense_head(case, weights_channels_last):
    p, feats = _head(3, weights_channels_last)
    gobj, gbox = _grads_from_entries(CASES[case])
    ref, ref_out = _dense_f64(p, feats, gobj, gbox)
    got, pp, xs, out = _sparse(p, feats, gobj, gbox, max_rows=64)
    for o, r in zip(out, ref_out):       # the forward is the dense head's
        assert o.is_contiguous() and torch.allclose(o.double(), r, rtol=1e-5, atol=1e-5)
    _check(got, ref, case)
    for k in PARAMS:                     # each gradient in its parameter's memory format
        assert got[k].shape == pp[k].shape and got[k].stride() == pp[k].stride(), (k, got[k].stride(), pp[k].stride())
    for i, x in enumerate(xs):
        assert got["x%d" % i].stride() == x.stride()
    # the feature gradient is EXACTLY zero outside the 3x3 neighbourhoods of the rows
    for l, (h, w) in enumerate(LEVELS):
        near = torch.zeros(N, h, w, dtype=torch.bool)
        for ll, n, y, x, a in CASES[case]:
            if ll == l:
                near[n, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
        gx = got["x%d" % l].permute(0, 2, 3, 1)
        assert not gx[~near].any() and (not near.any() or gx[near].abs().sum() > 0)
    assert _C.rpn_sparse_overflows() == 0


def test_no_row_at_all_gives_exact_zeros():
    p, feats = _head(4)
    gobj, gbox = _grads_from_entries([])
    got, _, _, _ = _sparse(p, feats, gobj, gbox, max_rows=8)
    for k, v in got.items():
        assert v is not None and not v.any(), k
    assert _C.rpn_sparse_overflows() == 0


def _random_entries(k, seed):
    rng = np.random.RandomState(seed)
    seen = set()
    while len(seen) < k:
        l = int(rng.randint(len(LEVELS)))
        h, w = LEVELS[l]
        seen.add((l, int(rng.randint(N)), int(rng.randint(h)), int(rng.randint(w)), int(rng.randint(A))))
    return sorted(seen)


def test_exactly_the_capacity_and_one_row_more():
    p, feats = _head(5)
    entries = _random_entries(40, 11)
    gobj, gbox = _grads_from_entries(entries)
    ref, _ = _dense_f64(p, feats, gobj, gbox)
    got, _, _, _ = _sparse(p, feats, gobj, gbox, max_rows=40)
    _check(got, ref, "rows == capacity")
    assert _C.rpn_sparse_overflows() == 0
    # one row more than the capacity: never silently wrong — the conv-weight gradient is NaN, the counter moved, and every
    # output keeps its shape with finite values elsewhere (nothing written past the capacity)
    got, pp, xs, _ = _sparse(p, feats, gobj, gbox, max_rows=39)
    assert torch.isnan(got["conv.weight"]).all()
    assert _C.rpn_sparse_overflows() == 1
    for k, v in got.items():
        assert k == "conv.weight" or torch.isfinite(v).all(), k
    assert _C.rpn_sparse_overflows(reset=True) == 1 and _C.rpn_sparse_overflows() == 0
    got, _, _, _ = _sparse(p, feats, gobj, gbox, max_rows=41)      # and the next launch with room is right again
    _check(got, ref, "rows == capacity - 1, after an overflow")


# The compaction ranks the rows among the candidates (every anchor of the pyramid) in rounds of 256 candidates, 4 waves, with
# a running base: name -> (levels, anchors per location, images, rows).  255 / 256 / 257 candidates are a round not full,
# full, and a second round of one candidate, on a second level (no candidate at all: test_no_row_at_all_gives_exact_zeros); 255 / 256 / 257 rows
# of the module's pyramid fill every wave of every round and cross a workgroup's 1024 candidates.
COMPACTION_CASES = {
    "candidates-255": ([(15, 17)], 1, 1, 40),
    "candidates-256": ([(16, 16)], 1, 1, 40),
    "candidates-257": ([(15, 17), (1, 2)], 1, 1, 40),
    "rows-255": (LEVELS, A, N, 255),
    "rows-256": (LEVELS, A, N, 256),
    "rows-257": (LEVELS, A, N, 257),
}


def compaction_case(name, monkeypatch):
    """-> (parameters, features, incoming gradients, rows) of a case, this module's pyramid set to the case's; the first and
    the last candidate are rows"""
    import sys
    levels, a, n, rows = COMPACTION_CASES[name]
    me = sys.modules[__name__]
    for k, v in (("LEVELS", levels), ("A", a), ("N", n)):
        monkeypatch.setattr(me, k, v)
    h, w = levels[-1]
    first, last = (0, 0, 0, 0, 0), (len(levels) - 1, n - 1, h - 1, w - 1, a - 1)
    entries = [first] + [e for e in _random_entries(rows, 30 + rows) if e not in (first, last)][:rows - 2] + [last]
    assert len(entries) == rows
    p, feats = _head(9)
    return (p, feats) + tuple(_grads_from_entries(entries)) + (rows,)


@pytest.mark.parametrize("case", sorted(COMPACTION_CASES))
def test_candidates_and_rows_around_one_round_of_the_compaction(case, monkeypatch):
    p, feats, gobj, gbox, rows = compaction_case(case, monkeypatch)
    ref, _ = _dense_f64(p, feats, gobj, gbox)
    got, _, _, _ = _sparse(p, feats, gobj, gbox, max_rows=rows)         # exactly the capacity: one row more would overflow
    _check(got, ref, case)
    assert _C.rpn_sparse_overflows() == 0


def test_relu_mask_follows_bias_act_rule_for_nan_and_zero_activations():
    """m = 0 where t <= 0, 1 otherwise: a dead pixel takes no gradient (not even a NaN one)"""
    p, feats = _head(6)
    p["conv.bias"] = torch.full((C,), -100.0)                       # every hidden activation is clipped to zero
    gobj, gbox = _grads_from_entries(CASES["overlapping-footprints"])
    got, _, _, _ = _sparse(p, feats, gobj, gbox, max_rows=32)
    assert not got["conv.weight"].any() and not got["conv.bias"].any() and not any(got["x%d" % i].any() for i in range(5))
    assert not got["cls_logits.weight"].any() and got["cls_logits.bias"].any() and got["bbox_pred.bias"].any()


def _rpn_module(monkeypatch, mode):
    import maskrcnn_benchmark.modeling.rpn.rpn as rpn
    monkeypatch.setattr(rpn, "_SPARSE_BWD", mode)
    return rpn


@pytest.mark.parametrize("mode", ["0", "1", "force"])
def test_head_module_switch_and_shape_test(mode, monkeypatch):
    """RPNHead.forward(x, sparse_rows): "0" is the dense composition (the sparse entry point is never called), "1" decides by
    the static shape test, "force" takes the sparse path wherever the kernels serve the tensors; upstream gradients are the
    real loss kernel's, scaled by factors other than 1."""
    rpn = _rpn_module(monkeypatch, mode)
    p, feats = _head(7)
    head = rpn.RPNHead(None, C, A)
    head.load_state_dict(p)
    head.to(memory_format=torch.channels_last)
    calls = []
    real = _C.rpn_head_sparse
    monkeypatch.setattr(_C, "rpn_head_sparse", lambda *a, **k: calls.append(a[-1]) or real(*a, **k))
    pixels = N * sum(h * w for h, w in LEVELS)
    rows = 64                                        # 64 * 16 <= 2060 pixels: pays
    assert rows * rpn._SPARSE_PIXELS_PER_ROW <= pixels
    gobj, gbox = _grads_from_entries(_random_entries(50, 5))
    gobj = [g * 2.5 for g in gobj]
    gbox = [g * 0.3 for g in gbox]
    xs = [f.clone(memory_format=torch.preserve_format).requires_grad_() for f in feats]
    obj, box = head(xs, sparse_rows=rows)
    assert calls == ([] if mode == "0" else [rows])
    torch.autograd.backward(list(obj) + list(box), gobj + gbox)
    got = {k: v.grad for k, v in head.named_parameters()}
    got.update({"x%d" % i: x.grad for i, x in enumerate(xs)})
    ref, _ = _dense_f64(p, feats, gobj, gbox)
    _check(got, ref, "module, switch %s" % mode)
    # too many rows for the pyramid: "1" stays dense, "force" does not care; without the promise, or without gradients, dense
    del calls[:]
    head([f.clone(memory_format=torch.preserve_format).requires_grad_() for f in feats], sparse_rows=pixels)
    assert calls == ([pixels] if mode == "force" else [])
    del calls[:]
    head(xs)
    with torch.no_grad():
        head(xs, sparse_rows=rows)
    head([f.contiguous() for f in feats], sparse_rows=rows)          # NCHW features: dense
    assert calls == []


def test_gradients_of_the_real_loss_kernel_with_upstream_scalars():
    """the gradient pattern `_C.rpn_loss` really hands back (sampled anchors only), for 2.5 * objectness + 0.3 * box"""
    p, feats = _head(8)
    T = A * sum(h * w for h, w in LEVELS)
    g = torch.Generator().manual_seed(2)
    obj = [torch.randn(N, A, h, w, generator=g).requires_grad_() for h, w in LEVELS]
    box = [(torch.randn(N, 4 * A, h, w, generator=g) * 0.4).requires_grad_() for h, w in LEVELS]
    anchors = torch.rand(T, 2, generator=g) * 60
    anchors = torch.cat([anchors, anchors + 8 + torch.rand(T, 2, generator=g) * 30], 1)
    gt = torch.tensor([[[5.0, 5.0, 40.0, 50.0], [20.0, 10.0, 70.0, 44.0]]] * N)
    matched = torch.randint(0, 2, (N, T), generator=g)
    pick = torch.rand(N, T, generator=g)
    pos, neg = pick < 0.004, (pick > 0.5) & (pick < 0.504)
    rows = int((pos | neg).sum())
    assert 10 <= rows <= 120
    lo, lb = _C.rpn_loss(obj, box, anchors, matched, pos, neg, gt, 1.0 / 9, (1.0, 1.0, 1.0, 1.0))
    (2.5 * lo + 0.3 * lb).backward()
    gobj, gbox = [t.grad for t in obj], [t.grad for t in box]
    assert sum(int((a != 0).any(1).sum()) for a in gobj) <= rows
    ref, _ = _dense_f64(p, feats, gobj, gbox)
    got, _, _, _ = _sparse(p, feats, gobj, gbox, max_rows=rows)
    _check(got, ref, "real loss gradients, %d rows" % rows)
    assert _C.rpn_sparse_overflows() == 0


def test_tiny_detector_sparse_equals_switch_off(monkeypatch):
    """One training forward / backward of the tiny detector (channels-last pyramid and heads, the real RPNLossComputation)
    with the sparse path forced on, against the switch off: every parameter gradient within GRAD_TOL, no overflow."""
    from maskrcnn_benchmark.data.synthetic import BatchCollator, SyntheticCOCODataset
    from maskrcnn_benchmark.engine.bench_step import load_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    cfg = load_cfg("e2e_mask_rcnn_R_50_FPN_1x.yaml",
                   ["MODEL.DEVICE", "cpu", "MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 100, "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", 150,
                    "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 32, "MODEL.RESNETS.RES2_OUT_CHANNELS", 16,
                    "MODEL.RESNETS.WIDTH_PER_GROUP", 4, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16,
                    "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 32, "MODEL.ROI_MASK_HEAD.CONV_LAYERS", (16, 16),
                    "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 64])
    ds = SyntheticCOCODataset(length=2, height=96, width=128, with_masks=True, min_objects=2, max_objects=4)
    images, targets, _ = BatchCollator(32)([ds[0], ds[1]])
    calls = []
    real = _C.rpn_head_sparse
    monkeypatch.setattr(_C, "rpn_head_sparse", lambda *a, **k: calls.append(a[-1]) or real(*a, **k))

    def run(mode):
        _rpn_module(monkeypatch, mode)
        torch.manual_seed(0)
        model = build_detection_model(cfg).train()
        model.set_channels_last(True, heads=True)
        _C._SAMPLER_CALLS[0] = 0
        torch.manual_seed(1)
        losses = model(images, list(targets))
        sum(losses.values()).backward()
        return ({k: float(v.detach()) for k, v in losses.items()},
                {n: q.grad.detach().double() for n, q in model.named_parameters() if q.grad is not None})

    dense_losses, dense = run("0")
    assert calls == []
    sparse_losses, sparse = run("force")
    assert calls == [2 * 64]
    assert sparse_losses == dense_losses and set(sparse) == set(dense)
    assert any(n.startswith("rpn.head.conv") for n in dense) and any(n.startswith("backbone.") for n in dense)
    spread = _grad_spread(sparse, dense)
    worst = max(spread, key=spread.get)
    print("\ntiny detector, sparse vs switch off: largest spread %.3g (%s)" % (spread[worst], worst))
    for n, s in spread.items():
        assert s <= GRAD_TOL, (n, s)
    assert _C.rpn_sparse_overflows() == 0
