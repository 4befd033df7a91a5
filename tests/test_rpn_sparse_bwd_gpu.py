"""Sparse backward of the RPN head on the device at the headline shapes (N = 2, C = 256, A = 3, P2..P6 of 800 x 1344), with
the gradient pattern of the real sampler + RPN loss kernels: against the dense library path (switch off) on the same
inputs, and — at a reduced shape — against fp64 autograd of the dense composition on the CPU.  Criterion: the project's
own (tests/test_whole_model_parity.py): relative Frobenius distance per tensor <= GRAD_TOL, with its floor."""
import pytest
import torch
import torch.nn.functional as F

from test_whole_model_parity import GRAD_TOL, _grad_spread

pytestmark = pytest.mark.gpu

A = 3
HEADLINE = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]


def _inputs(C, levels, N, batch_per_image, seed, dev="cuda"):
    from maskrcnn_benchmark import _C
    g = torch.Generator().manual_seed(seed)
    T = A * sum(h * w for h, w in levels)
    p = {"conv.weight": torch.randn(C, C, 3, 3, generator=g) * (1.5 / (9 * C) ** 0.5), "conv.bias": torch.randn(C, generator=g) * 0.1,
         "cls_logits.weight": torch.randn(A, C, 1, 1, generator=g) * 0.05, "cls_logits.bias": torch.randn(A, generator=g) * 0.1,
         "bbox_pred.weight": torch.randn(4 * A, C, 1, 1, generator=g) * 0.05, "bbox_pred.bias": torch.randn(4 * A, generator=g) * 0.1}
    feats = [torch.randn(N, C, h, w, generator=g) for h, w in levels]
    anchors = torch.rand(T, 2, generator=g) * 700
    anchors = torch.cat([anchors, anchors + 16 + torch.rand(T, 2, generator=g) * 200], 1)
    gt = torch.tensor([[[50.0, 60.0, 400.0, 500.0], [300.0, 100.0, 700.0, 440.0], [10.0, 10.0, 90.0, 120.0]]] * N)
    matched = torch.randint(0, 3, (N, T), generator=g)
    u = torch.rand(N, T, generator=g)
    labels = torch.where(u < 0.002, 1.0, torch.where(u < 0.7, 0.0, -1.0))     # ~ 540 positives, most of the rest negatives
    pos, neg = _C.sample_labels(labels.to(dev), batch_per_image, batch_per_image // 2, seed=seed)
    return p, feats, anchors.to(dev), gt.to(dev), matched.to(dev), pos, neg


def _forward(mode, p, feats, rows, monkeypatch, dev="cuda"):
    """RPNHead (channels-last) forward with the switch at `mode` -> (head, inputs, outputs); the autograd graph stays alive"""
    import maskrcnn_benchmark.modeling.rpn.rpn as rpn
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(rpn, "_SPARSE_BWD", mode)
    C = p["conv.bias"].numel()
    head = rpn.RPNHead(None, C, A)
    head.load_state_dict(p)
    head.to(dev).to(memory_format=torch.channels_last)
    xs = [f.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_() for f in feats]
    calls = []
    real = _C.rpn_head_sparse
    monkeypatch.setattr(_C, "rpn_head_sparse", lambda *a, **k: calls.append(a[-1]) or real(*a, **k))
    obj, box = head(xs, sparse_rows=rows)
    monkeypatch.setattr(_C, "rpn_head_sparse", real)
    assert calls == ([] if mode == "0" else [rows])
    return head, xs, list(obj) + list(box)


def _loss_grads(outs, loss_args):
    """d (1.3 * objectness loss + 0.7 * box loss) / d (head outputs) from the loss kernel, on detached copies"""
    from maskrcnn_benchmark import _C
    anchors, gt, matched, pos, neg = loss_args
    leaves = [o.detach().clone().requires_grad_() for o in outs]
    L = len(leaves) // 2
    lo, lb = _C.rpn_loss(leaves[:L], leaves[L:], anchors, matched, pos, neg, gt, 1.0 / 9, (1.0, 1.0, 1.0, 1.0))
    (1.3 * lo + 0.7 * lb).backward()
    return [t.grad for t in leaves]


def _backward(head, xs, outs, grads, retain=False):
    names = [k for k, _ in head.named_parameters()] + ["x%d" % i for i in range(len(xs))]
    got = torch.autograd.grad(outs, [v for _, v in head.named_parameters()] + list(xs), grads, retain_graph=retain)
    torch.cuda.synchronize()
    return dict(zip(names, got))


def _run(mode, p, feats, loss_args, rows, monkeypatch):
    head, xs, outs = _forward(mode, p, feats, rows, monkeypatch)
    return _backward(head, xs, outs, _loss_grads(outs, loss_args)), [o.detach() for o in outs]


def test_headline_shapes_sparse_equals_the_dense_library_path(monkeypatch):
    """The library's forward convolutions split their reduction over workgroups and add with atomics (`..._gkgs` kernels), so
    two forwards of the same head differ in the last bits: both paths therefore receive the SAME incoming gradients (the loss
    kernel's, on the dense forward's outputs), and bit-identity is asked of the sparse backward on one saved forward."""
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    N, C, B = 2, 256, 256
    p, feats, anchors, gt, matched, pos, neg = _inputs(C, HEADLINE, N, B, seed=5)
    sampled = (pos | neg)
    print("\nsampled anchors %d, positives %d" % (int(sampled.sum()), int(pos.sum())))
    assert int(sampled.sum()) == N * B and int(pos.sum()) > 50          # the real sampler's masks, full quota
    loss_args = (anchors, gt, matched, pos, neg)
    _C.rpn_sparse_overflows(reset=True)
    head_d, xs_d, out_d = _forward("0", p, feats, N * B, monkeypatch)
    grads = _loss_grads(out_d, loss_args)
    dense = _backward(head_d, xs_d, out_d, grads)
    del head_d, xs_d
    head_s, xs_s, out_s = _forward("1", p, feats, N * B, monkeypatch)   # the static shape test takes the headline shape
    fwd = _grad_spread({str(i): o.detach().double().cpu() for i, o in enumerate(out_s)},
                       {str(i): o.detach().double().cpu() for i, o in enumerate(out_d)})
    print("forward outputs, sparse node vs dense composition: largest spread %.3g" % max(fwd.values()))
    assert max(fwd.values()) <= GRAD_TOL
    sparse = _backward(head_s, xs_s, out_s, grads, retain=True)
    again = _backward(head_s, xs_s, out_s, grads)
    spread = _grad_spread({k: v.double().cpu() for k, v in sparse.items()}, {k: v.double().cpu() for k, v in dense.items()})
    worst = max(spread, key=spread.get)
    print("headline shapes, sparse vs dense library path: %s" % {k: "%.3g" % v for k, v in spread.items()})
    differ = [k for k in sparse if not torch.equal(sparse[k], again[k])]
    print("tensors that differ between two runs of the sparse backward: %s" % differ)
    outside = {}
    first = 0
    for l, (h, w) in enumerate(HEADLINE):
        m = sampled[:, first:first + A * h * w].view(N, h, w, A).any(-1).float().unsqueeze(1)
        first += A * h * w
        near = F.max_pool2d(m, 3, 1, 1) > 0
        gx = sparse["x%d" % l]
        outside[l] = (int((gx * (~near) != 0).sum()), int((gx * near != 0).sum()), int(near.sum()))
    print("dX non-zeros outside / inside the 3x3 neighbourhoods, neighbourhood pixels: %s" % outside)
    print("overflows: %d" % _C.rpn_sparse_overflows())
    for k, s in spread.items():
        assert s <= GRAD_TOL, (k, s, worst)
    assert not differ, "two runs of the sparse path are bit-identical"
    for k in sparse:
        assert sparse[k].shape == dense[k].shape, k
    # dX is exactly zero outside the 3x3 neighbourhoods of the sampled pixels
    for l, (out_nz, in_nz, pixels) in outside.items():
        assert out_nz == 0 and (in_nz > 0 or pixels == 0), (l, out_nz, in_nz, pixels)
    assert _C.rpn_sparse_overflows() == 0


@pytest.mark.parametrize("case", ["candidates-255", "candidates-256", "candidates-257", "rows-255", "rows-256", "rows-257"])
def test_candidates_and_rows_around_one_round_of_the_compaction(case, monkeypatch):
    """the cases of tests/test_rpn_sparse_bwd_emu.py (its helpers, its fp64 reference) on the device"""
    import test_rpn_sparse_bwd_emu as E
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    assert case in E.COMPACTION_CASES
    p, feats, gobj, gbox, rows = E.compaction_case(case, monkeypatch)
    ref, _ = E._dense_f64(p, feats, gobj, gbox)
    _C.rpn_sparse_overflows(reset=True)
    got, _, _, _ = E._sparse({k: v.cuda() for k, v in p.items()}, [f.cuda() for f in feats], [g.cuda() for g in gobj],
                             [g.cuda() for g in gbox], max_rows=rows)
    torch.cuda.synchronize()
    E._check({k: v.cpu() for k, v in got.items()}, ref, case)
    assert _C.rpn_sparse_overflows() == 0


def test_reduced_shape_equals_fp64_autograd_on_the_cpu(monkeypatch):
    from maskrcnn_benchmark import _C
    monkeypatch.setattr(torch.backends.cudnn, "allow_tf32", False)
    N, C, B = 2, 32, 48
    levels = [(40, 56), (20, 28), (10, 14), (5, 7), (3, 4)]
    p, feats, anchors, gt, matched, pos, neg = _inputs(C, levels, N, B, seed=9)
    _C.rpn_sparse_overflows(reset=True)
    got, out = _run("force", p, feats, (anchors, gt, matched, pos, neg), N * B, monkeypatch)
    # the incoming gradients, from the loss kernel on detached copies of the head outputs
    leaves = [o.clone().requires_grad_() for o in out]
    lo, lb = _C.rpn_loss(leaves[:5], leaves[5:], anchors, matched, pos, neg, gt, 1.0 / 9, (1.0, 1.0, 1.0, 1.0))
    (1.3 * lo + 0.7 * lb).backward()
    grads = [t.grad.double().cpu() for t in leaves]
    pp = {k: v.double().requires_grad_() for k, v in p.items()}
    xs = [f.double().requires_grad_() for f in feats]
    ts = [F.relu(F.conv2d(x, pp["conv.weight"], pp["conv.bias"], padding=1)) for x in xs]
    outs = [F.conv2d(t, pp["cls_logits.weight"], pp["cls_logits.bias"]) for t in ts] + \
           [F.conv2d(t, pp["bbox_pred.weight"], pp["bbox_pred.bias"]) for t in ts]
    torch.autograd.backward(outs, grads)
    ref = {k: v.grad for k, v in pp.items()}
    ref.update({"x%d" % i: x.grad for i, x in enumerate(xs)})
    spread = _grad_spread({k: v.double().cpu() for k, v in got.items()}, ref)
    print("\nreduced shape, sparse on the device vs fp64 on the CPU: %s" % {k: "%.3g" % v for k, v in spread.items()})
    for k, s in spread.items():
        assert s <= GRAD_TOL, (k, s)
    assert _C.rpn_sparse_overflows() == 0
