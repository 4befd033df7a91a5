"""Per-operator micro-benchmarks of the HIP detection-head kernels (HIP-event timed on the stream
the kernels are launched on) with the ALGORITHMIC byte counts of SURVEY.md §8(d).

    python tools/opbench.py [--iters 50] [--json out.json] [--only roi_align_fwd,...]

Used by bench.py for the `roofline` object and by the profiling recipes in profiles/README.md.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "maskrcnn-benchmark_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X spec (MI355X_MICROARCH.md); ~6290 GB/s measured copy ceiling


def dev_time_us(fn, iters=50, warmup=5):
    """Average device time of fn() in microseconds, HIP events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / iters


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _entry(name, us, alg_bytes, extra=None):
    e = {"op": name, "us": round(us, 2), "alg_bytes": int(alg_bytes),
         "gbs": round(alg_bytes / us / 1e3, 1), "frac_of_8TBs": round(alg_bytes / us / 1e3 / HBM_PEAK_GBS, 4)}
    if extra:
        e.update(extra)
    return e


def tune(key, value):
    """library tuning / test switch (include/detops.h: detops_tuning_set)"""
    from maskrcnn_benchmark import _lib
    _lib.tuning_set(key, value)



def bench_roi_align(C, iters, which=("fwd", "bwd"), fused_only=False, experimental=False):
    """fused_only: just the FPN-fused launches with the model's shapes (the PMC traffic passes use this,
    so every ROIAlign kernel in their trace is the box-head / mask-head launch bench.py times)."""
    out = []
    # cfg-1 (BASELINE configs[0]) ---------------------------------------------------------
    inp, rois, scale = synth.cfg1_roi_align()
    ti, tr = _t(inp), _t(rois)
    for ph, pw, sr in ([] if fused_only else [(7, 7, 2), (14, 14, 2), (7, 7, 0)]):
        K, Cc = rois.shape[0], inp.shape[1]
        alg = 4 * K * Cc * ph * pw + 4 * inp.size + 20 * K
        if "fwd" in which:
            us = dev_time_us(lambda: C.roi_align_forward(ti, tr, scale, ph, pw, sr), iters)
            out.append(_entry(f"roi_align_fwd cfg1 {ph}x{pw} sr{sr}", us, alg))
        if "bwd" in which:
            g = torch.randn(K, Cc, ph, pw, device="cuda")
            us = dev_time_us(lambda: C.roi_align_backward(g, tr, scale, ph, pw, 1, Cc, 14, 14, sr), iters)
            out.append(_entry(f"roi_align_bwd cfg1 {ph}x{pw} sr{sr} (gather, ROI list split over 32 groups)", us, alg))
            for grp in (1, 16):
                tune("roi_bwd_groups", grp)
                us = dev_time_us(lambda: C.roi_align_backward(g, tr, scale, ph, pw, 1, Cc, 14, 14, sr), max(3, iters // 5))
                out.append(_entry(f"roi_align_bwd cfg1 {ph}x{pw} sr{sr} [groups={grp}]", us, alg))
            tune("roi_bwd_groups", 0)
    # cfg-2 box head: 1024 ROIs over P2..P5, 7x7 sr2; cfg-3 mask head: 256 ROIs, 14x14 sr2 ----
    feats = [torch.randn(2, 256, h, w, device="cuda") for (h, w) in synth.fpn_shapes()[:4]]
    scales = [1.0 / s for s in synth.FPN_STRIDES[:4]]
    shapes = [tuple(f.shape) for f in feats]
    feat_bytes = sum(f.numel() * 4 for f in feats)
    for tag, K, ph in (("box-head 1024x7x7", 1024, 7), ("mask-head 256x14x14", 256, 14)):
        rois = synth.fpn_rois(per_image=K // 2)
        tr = _t(rois)
        alg = 4 * K * 256 * ph * ph + feat_bytes + 20 * K
        lv = synth.level_map(rois)
        per = [(l, _t(rois[lv == l])) for l in range(4)]

        def per_level_fwd():
            for l, r in per:
                C.roi_align_forward(feats[l], r, scales[l], ph, ph, 2)

        if "fwd" in which:
            us = dev_time_us(lambda: C.roi_align_fpn_forward(feats, tr, scales, ph, ph, 2, 2, 5), iters)
            out.append(_entry(f"roi_align_fwd fpn-fused {tag}", us, alg))
            if not fused_only:
                us = dev_time_us(per_level_fwd, iters)
                out.append(_entry(f"roi_align_fwd fpn-per-level(4 launches) {tag}", us, alg))
        if "fwd" in which and not fused_only:
            base = C.roi_align_fpn_forward(feats, tr, scales, ph, ph, 2, 2, 5)[0]
            for label, key, val in (("LDS-DMA, ROIs in caller order (no ranking pre-pass)", "roi_fwd_order", 1),
                                    ("generic gather kernel", "roi_fwd_impl", 1)):
                tune(key, val)
                us = dev_time_us(lambda: C.roi_align_fpn_forward(feats, tr, scales, ph, ph, 2, 2, 5), iters)
                same = bool(torch.equal(base, C.roi_align_fpn_forward(feats, tr, scales, ph, ph, 2, 2, 5)[0]))
                tune(key, 0)
                out.append(_entry(f"roi_align_fwd fpn-fused {tag} [{label}]", us, alg, {"bit_equal_to_default": same}))
        if "bwd" in which:
            g = torch.randn(K, 256, ph, ph, device="cuda")
            tl = _t(lv)
            us = dev_time_us(lambda: C.roi_align_fpn_backward(g, tr, tl, shapes, scales, ph, ph, 2), iters)
            out.append(_entry(f"roi_align_bwd fpn-fused ring pixel-owner (atomic-free, incl. pre-pass + zero-fill) {tag}", us, alg))
            if fused_only:
                continue
            ref_g = C.roi_align_fpn_backward(g, tr, tl, shapes, scales, ph, ph, 2)
            for label, key, val in (("ring, hit lists never split", "roi_bwd_seg", 1 << 20), ("ring, segments of 16 hits", "roi_bwd_seg", 16),
                                    ("scan pixel-owner (no pre-pass)", "roi_bwd_impl", 2), ("atomic scatter", "roi_bwd_impl", 3)):
                tune(key, val)
                us = dev_time_us(lambda: C.roi_align_fpn_backward(g, tr, tl, shapes, scales, ph, ph, 2), max(3, iters // 5))
                got = C.roi_align_fpn_backward(g, tr, tl, shapes, scales, ph, ph, 2)
                tune(key, 0)
                out.append(_entry(f"roi_align_bwd fpn-fused [{label}] {tag}", us, alg,
                                  {"max_abs_diff_vs_default": max(float((a - b).abs().max()) for a, b in zip(ref_g, got))}))
    return out


def bench_roi_sets(C, iters, model_npz=None, only_sets=None, only_heads=None, which=("fwd", "bwd"), images=2, tag="", layout="nchw"):
    """FPN-fused ROIAlign forward / backward on every ROI set of synth.roi_sets(): the SURVEY 8d log-uniform set, the
    trained-like set and the sets the detector itself produced (tools/dump_model_rois.py) - VERDICT r02 item 1a."""
    out = []
    feats = [torch.randn(images, 256, h, w, device="cuda") for (h, w) in synth.fpn_shapes()[:4]]
    nhwc = layout == "nhwc"    # channels-last pyramid: csrc/roi_align_nhwc.hip (box head: contiguous pooled tensor / gradient,
    if nhwc:                   # mask head: channels-last pooled tensor / gradient, as in the detector)
        feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
    scales = [1.0 / s for s in synth.FPN_STRIDES[:4]]
    shapes = [tuple(f.shape) for f in feats]
    feat_bytes = sum(f.numel() * 4 for f in feats)
    for name, sets in synth.roi_sets(model_npz).items():
        if only_sets and name not in only_sets:
            continue
        for head, ph in (("box", 7), ("mask", 14)):
            if only_heads and head not in only_heads:
                continue
            rois = sets[head]
            label = name
            if images != 2:
                # the > L3 variant of SURVEY 8d (4 img/GPU: 365.6 MB of maps against the 256 MiB Infinity Cache): the
                # 2-image ROI set repeated on image pairs (2, 3), ... — same per-image ROI statistics
                reps = []
                for r in range((images + 1) // 2):
                    rr = rois.copy()
                    rr[:, 0] = np.minimum(rr[:, 0] + 2 * r, images - 1)
                    reps.append(rr)
                rois = np.concatenate(reps)[: rois.shape[0] * images // 2]
                label = label + " x%d images" % images
            if tag:
                label = label + " | " + tag
            K = rois.shape[0]
            tr = _t(rois)
            lv = synth.level_map(rois)
            tl = _t(lv)
            alg = 4 * K * 256 * ph * ph + feat_bytes + 20 * K
            g = torch.randn(K, 256, ph, ph, device="cuda")
            ocl = nhwc and head == "mask"
            if ocl:
                g = g.contiguous(memory_format=torch.channels_last)
            if nhwc:
                label = label + " | nhwc"
            extra = {"rois_per_level": np.bincount(lv, minlength=4).tolist()}
            if "fwd" in which:
                us = dev_time_us(lambda: C.roi_align_fpn_forward(feats, tr, scales, ph, ph, 2, 2, 5, out_channels_last=ocl), iters)
                out.append(_entry(f"roi_align_fwd fpn-fused {head}-head K={K} {ph}x{ph} [{label}]", us, alg, extra))
            if "bwd" in which:
                us = dev_time_us(lambda: C.roi_align_fpn_backward(g, tr, tl, shapes, scales, ph, ph, 2, channels_last=nhwc), iters)
                out.append(_entry(f"roi_align_bwd fpn-fused {head}-head K={K} {ph}x{ph} [{label}]", us, alg, extra))
    return out


def bench_roi_pool_psroi(C, iters):
    """The two API-only pooling operators (no reference config instantiates them), once, at the box
    head's size on the stride-16 level: ROIPool 7x7 (reference csrc/cuda/ROIPool_cuda.cu:16-202) and deformable PS-ROI
    pooling (csrc/cuda/deform_pool_kernel_cuda.cu:53-264; 7x7 parts, 4 samples per part, 10 output channels per group)."""
    out = []
    H, W, Cc, K = 50, 84, 256, 512
    feat = torch.randn(2, Cc, H, W, device="cuda")
    rois = synth.fpn_rois(per_image=K // 2)
    rois = _t(rois[:K])
    fbytes = feat.numel() * 4
    alg = 4 * K * Cc * 49 + fbytes + 20 * K
    us = dev_time_us(lambda: C.roi_pool_forward(feat, rois, 1.0 / 16, 7, 7), iters)
    out.append(_entry("roi_pool_fwd 512 x 256 x 7x7 on 2x256x50x84", us, alg + 4 * K * Cc * 49))      # + argmax
    o, am = C.roi_pool_forward(feat, rois, 1.0 / 16, 7, 7)
    g = torch.randn_like(o)
    us = dev_time_us(lambda: C.roi_pool_backward(g, feat, rois, am, 1.0 / 16, 7, 7, 2, Cc, H, W), iters)
    out.append(_entry("roi_pool_bwd 512 x 256 x 7x7 on 2x256x50x84", us, alg + 4 * K * Cc * 49))
    D, P = 10, 7                                                         # C = D * P * P = 490 position-sensitive maps
    pfeat = torch.randn(2, D * P * P, H, W, device="cuda")
    trans = torch.randn(K, 2, P, P, device="cuda") * 0.1
    po = torch.empty(K, D, P, P, device="cuda")
    cnt = torch.empty_like(po)
    palg = 2 * 4 * K * D * P * P + pfeat.numel() * 4 + 20 * K + trans.numel() * 4
    us = dev_time_us(lambda: C.deform_psroi_pooling_forward(pfeat, rois, trans, po, cnt, 0, 1.0 / 16, D, P, P, P, 4, 0.1), iters)
    out.append(_entry("deform_psroi_fwd 512 rois, 10 x 7x7, 4 samples/part", us, palg))
    gi, gt = torch.zeros_like(pfeat), torch.zeros_like(trans)
    go = torch.randn_like(po)
    us = dev_time_us(lambda: C.deform_psroi_pooling_backward(go, pfeat, rois, trans, cnt, gi, gt, 0, 1.0 / 16, D, P, P, P, 4, 0.1), iters)
    out.append(_entry("deform_psroi_bwd (atomic accumulate into pre-zeroed gradients)", us, palg))
    return out


def bench_targets(C, iters):
    """IoU + Matcher and the balanced sampler at the RPN's shape (2 images x 268,569 anchors of the 800 x 1344 pyramid,
    <= 20 ground-truth boxes) and at the box head's (2 x ~2,020 proposals); bytes: boxes + matched indices."""
    out = []
    rng = np.random.RandomState(9)
    anchors = []
    for stride in (4, 8, 16, 32, 64):        # the RPN's anchor grid of a padded 800 x 1344 image: 3 ratios per location
        hh, ww = -(-800 // stride), -(-1344 // stride)
        ys, xs = np.meshgrid(np.arange(hh) * stride, np.arange(ww) * stride, indexing="ij")
        for r in (0.5, 1.0, 2.0):
            w_, h_ = 8 * stride / np.sqrt(r), 8 * stride * np.sqrt(r)
            anchors.append(np.stack([xs - w_ / 2, ys - h_ / 2, xs + w_ / 2, ys + h_ / 2], -1).reshape(hh * ww, 1, 4))
    per_level = [np.concatenate(anchors[3 * l:3 * l + 3], 1).reshape(-1, 4) for l in range(5)]
    rpn_anchors = np.concatenate(per_level).astype(np.float32)
    assert rpn_anchors.shape[0] == 268569
    for tag, K, M, B, lq in (("rpn 2x268569 anchors", 268569, 20, 256, True), ("box head 2x2020 proposals", 2020, 20, 512, False)):
        x1 = rng.uniform(0, 1200, (K,)); y1 = rng.uniform(0, 700, (K,))
        s_ = np.exp(rng.uniform(np.log(16), np.log(512), (K,)))
        boxes = torch.from_numpy(np.stack([x1, y1, x1 + s_, y1 + s_ * rng.uniform(0.5, 2, (K,))], 1).astype(np.float32)).cuda()
        if K == 268569:
            boxes = torch.from_numpy(rpn_anchors).cuda()
        gx = rng.uniform(0, 1000, (2, M)); gy = rng.uniform(0, 600, (2, M)); gs = rng.uniform(30, 400, (2, M))
        gt = torch.from_numpy(np.stack([gx, gy, gx + gs, gy + gs], 2).astype(np.float32)).cuda()
        valid = torch.ones(2, M, dtype=torch.bool, device="cuda")
        valid[1, 12:] = False
        us = dev_time_us(lambda: C.match_boxes(gt, valid, boxes, 0.7, 0.3, lq), iters)
        out.append(_entry(f"match_boxes (IoU + Matcher, low-quality rule {'on' if lq else 'off'}) {tag}", us, 16 * K + 2 * 8 * K))
        matched = C.match_boxes(gt, valid, boxes, 0.7, 0.3, lq)
        labels = (matched >= 0).float() - (matched == -2).float()
        us = dev_time_us(lambda: C.sample_labels(labels, B, B // 2, with_list=not lq), iters)
        out.append(_entry(f"sample_labels B={B} {tag}", us, 2 * K * (4 + 2)))
    return out


def bench_nms(C, iters):
    out = []
    for n, uniform in [(819, False), (2000, False), (2000, True), (6000, False)]:
        b, s = synth.nms_boxes(n, seed=2, uniform=uniform)
        tb, ts = _t(b), _t(s)
        us = dev_time_us(lambda: C.nms(tb, ts, 0.7), iters)  # includes the count readback
        k = int(C.nms(tb, ts, 0.7).numel())
        out.append(_entry(f"nms n={n} {'uniform' if uniform else 'clustered'} (with .item())", us,
                          20 * n + 8 * k, {"kept": k, "pairs_per_us": round(n * (n - 1) / 2 / us, 1)}))
    segs = synth.rpn_nms_segments()
    boxes = _t(np.concatenate([b for b, _ in segs]))
    scores = _t(np.concatenate([s for _, s in segs]))
    offs = _t(np.cumsum([0] + [len(s) for _, s in segs]).astype(np.int32))
    tot = int(boxes.size(0))
    pairs = sum(len(s) * (len(s) - 1) // 2 for _, s in segs)
    for fused, label in ((0, "one launch"), (3, "one launch, scans last"), (2, "three launches")):
        tune("nms_fused", fused)
        us = dev_time_us(lambda: C.nms_batched(boxes, scores, offs, 2000, 0.7), iters)
        out.append(_entry("nms batched 10 RPN segments, %s (no sync)" % label, us, 20 * tot,
                          {"pairs_per_us": round(pairs / us, 1)}))
    tune("nms_fused", 0)
    # the detector's calls: every segment is top-k output, i.e. already in score order (modeling/rpn/inference.py) — the sort
    # workgroups detect that and skip the network (`nms_no_presorted=1`: always sort)
    so = [np.argsort(-s, kind="stable") for _, s in segs]
    boxes_s = _t(np.concatenate([b[o] for (b, _), o in zip(segs, so)]))
    scores_s = _t(np.concatenate([s[o] for (_, s), o in zip(segs, so)]))
    for off, label in ((0, "in score order"), (1, "in score order, network forced")):
        tune("nms_no_presorted", off)
        us = dev_time_us(lambda: C.nms_batched(boxes_s, scores_s, offs, 2000, 0.7), iters)
        out.append(_entry("nms batched 10 RPN segments %s, one launch (no sync)" % label, us, 20 * tot,
                          {"pairs_per_us": round(pairs / us, 1)}))
    tune("nms_no_presorted", 0)
    return out


def bench_frozen_bn(C, iters):
    """fused FrozenBN+ReLU(+residual) vs the PyTorch elementwise chain, res2-sized activation."""
    out = []
    x = torch.randn(2, 256, 200, 336, device="cuda")
    r = torch.randn_like(x)
    scale = torch.rand(256, device="cuda") + 0.5
    bias = torch.randn(256, device="cuda")
    nb = x.numel() * 4
    us = dev_time_us(lambda: C.frozen_bn_act_forward(x, scale, bias, None, True), iters)
    out.append(_entry("frozen_bn_relu fwd fused [2,256,200,336]", us, 2 * nb))
    us = dev_time_us(lambda: C.frozen_bn_act_forward(x, scale, bias, r, True), iters)
    out.append(_entry("frozen_bn_add_relu fwd fused", us, 3 * nb))
    y = C.frozen_bn_act_forward(x, scale, bias, r, True)
    us = dev_time_us(lambda: C.frozen_bn_act_backward(r, y, scale, True, True), iters)
    out.append(_entry("frozen_bn_add_relu bwd fused (2 outputs)", us, 4 * nb))
    s4, b4 = scale.view(1, -1, 1, 1), bias.view(1, -1, 1, 1)
    us = dev_time_us(lambda: torch.relu_(x * s4 + b4), iters)
    out.append(_entry("frozen_bn_relu fwd torch chain (3 kernels)", us, 2 * nb))
    return out


def bench_group_norm(C, iters, copy_gbs=None):
    """channels-last GroupNorm + residual + ReLU: the fused kernels (csrc/group_norm.hip, through layers.GroupNorm) against
    F.group_norm + add + relu on the SAME channels-last tensors, forward and forward + backward, fp32 and bf16, at the GN
    baselines' shapes (backbone res2-res5 stages at 2 images, box head 1024 ROIs, mask head 128 ROIs).  Bytes: what the
    algorithm must move — forward x, residual, y (3 tensors); backward grad_y, x, y, grad_x, grad_residual (5 more);
    frac_of_copy = those bytes over the time, against the copy row of the same run."""
    import torch.nn.functional as F
    from maskrcnn_benchmark.layers import GroupNorm
    out = []
    shapes = [("backbone", (2, 64, 400, 672)), ("backbone", (2, 256, 200, 336)), ("backbone", (2, 512, 100, 168)),
              ("backbone", (2, 2048, 25, 42)), ("box head", (1024, 256, 7, 7)), ("mask head", (128, 256, 14, 14))]
    for where, shape in shapes:
        for dtype in (torch.float32, torch.bfloat16):
            gn = GroupNorm(32, shape[1]).cuda()
            x = torch.randn(shape, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
            r = torch.randn(shape, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
            gy = torch.randn(shape, device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
            assert gn.serves(x)
            nb = x.numel() * x.element_size()
            xg, rg = x.clone().requires_grad_(True), r.clone().requires_grad_(True)

            def torch_fwd(a, b):      # half storage: as the model runs it, under autocast (ATen's group_norm then works in fp32)
                with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
                    return torch.relu(F.group_norm(a, gn.num_groups, gn.weight, gn.bias, gn.eps) + b)

            def both(f):
                xg.grad = rg.grad = gn.weight.grad = gn.bias.grad = None
                y = f(xg, rg)
                y.backward(gy.to(y.dtype))

            rows = {}
            with torch.no_grad():
                rows["fwd fused"] = (dev_time_us(lambda: gn.fused(x, True, r), iters), 3 * nb)
                rows["fwd torch"] = (dev_time_us(lambda: torch_fwd(x, r), iters), 3 * nb)
            rows["fwd+bwd fused"] = (dev_time_us(lambda: both(lambda a, b: gn.fused(a, True, b)), iters), 8 * nb)
            rows["fwd+bwd torch"] = (dev_time_us(lambda: both(torch_fwd), iters), 8 * nb)
            tag = "group_norm+add+relu %s %s %s" % (where, "x".join(map(str, shape)), str(dtype)[6:])
            for kind in ("fwd", "fwd+bwd"):
                for impl in ("fused", "torch"):
                    us, alg = rows["%s %s" % (kind, impl)]
                    extra = {"speedup_vs_torch": round(rows[kind + " torch"][0] / us, 2)} if impl == "fused" else {}
                    if copy_gbs:
                        extra["frac_of_copy"] = round(alg / us / 1e3 / copy_gbs, 4)
                    out.append(_entry("%s %s %s" % (tag, kind, impl), us, alg, extra))
    return out


def bench_focal(C, iters):
    out = []
    for R in (200000, 403200):
        logits, targets = synth.focal_inputs(R, 80)
        tl, tt = _t(logits), _t(targets)
        d = torch.rand_like(tl)
        one = torch.ones((), device="cuda")
        us = dev_time_us(lambda: C.sigmoid_focalloss_forward(tl, tt, 80, 2.0, 0.25), iters)
        out.append(_entry(f"focal_fwd R={R}", us, 2 * 4 * R * 80 + 4 * R))
        us = dev_time_us(lambda: C.sigmoid_focalloss_backward(tl, tt, d, 80, 2.0, 0.25), iters)
        out.append(_entry(f"focal_bwd R={R}", us, 3 * 4 * R * 80 + 4 * R))
        us = dev_time_us(lambda: C.sigmoid_focalloss_forward_sum(tl, tt, 80, 2.0, 0.25), iters)
        out.append(_entry(f"focal_fwd_sum R={R}", us, 4 * R * 80 + 4 * R))
        us = dev_time_us(lambda: C.sigmoid_focalloss_backward_scalar(tl, tt, one, 80, 2.0, 0.25), iters)
        out.append(_entry(f"focal_bwd_scalar R={R}", us, 2 * 4 * R * 80 + 4 * R))
    return out


def bench_dcn_fused(C, iters):
    """deformable conv forward at the cfg-5 layer shapes, fp16 / bf16: fused implicit GEMM on MFMA (columns never
    written) vs im2col kernel + library GEMM; TFLOP/s against the 2.5 PF dense matrix peak and the bytes the
    unfused path moves through HBM for `columns` (write + read)."""
    out = []
    for (Cc, H, W) in [(128, 100, 168), (256, 50, 84), (512, 25, 42)]:
        for dt in (torch.float16, torch.bfloat16):
            x = torch.randn(2, Cc, H, W, device="cuda").to(dt)
            off = (torch.randn(2, 18, H, W, device="cuda") * 2).to(dt)
            msk = torch.rand(2, 9, H, W, device="cuda").to(dt)
            w = (torch.randn(Cc, Cc, 3, 3, device="cuda") / (3 * Cc ** 0.5)).to(dt)
            y = torch.empty(2, Cc, H, W, device="cuda", dtype=dt)
            bufs = [torch.empty(0, device="cuda", dtype=dt), torch.empty(0, device="cuda", dtype=dt)]
            flops = 2.0 * Cc * Cc * 9 * 2 * H * W
            col_bytes = 2 * Cc * 9 * 2 * H * W * 2

            def run():
                C.modulated_deform_conv_forward(x, w, None, bufs[0], off, msk, y, bufs[1], 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, False)

            res = {}
            for tag, env in (("fused MFMA", 1), ("im2col + GEMM", 2)):
                tune("dcn_fused", env)
                us = dev_time_us(run, iters)
                res[tag] = y.float().clone()
                e = _entry(f"dcn_fwd {tag} C={Cc} {H}x{W} {str(dt)[6:]}", us, 2 * (x.numel() + off.numel() + msk.numel() + y.numel()),
                           {"TFLOPs": round(flops / us / 1e6, 1), "frac_of_2.5PF": round(flops / us / 1e6 / 2500.0, 4),
                            "columns_bytes_unfused": col_bytes})
                out.append(e)
            tune("dcn_fused", 0)
            out[-1]["max_abs_diff_fused_vs_unfused"] = float((res["fused MFMA"] - res["im2col + GEMM"]).abs().max())
    return out


def bench_dcn(C, iters, experimental=False):
    out = []
    for (Cc, H, W, smooth) in [(128, 100, 168, False), (256, 50, 84, False), (512, 25, 42, False), (128, 100, 168, True)]:
        for dt, e in ((torch.float32, 4), (torch.float16, 2)):
            x = torch.randn(2, Cc, H, W, device="cuda").to(dt)
            if smooth:  # spatially smooth offsets (a conv-predicted field): low-resolution noise upsampled, ~2 px
                lo = torch.randn(2, 18, H // 8 + 2, W // 8 + 2, device="cuda") * 2
                off = torch.nn.functional.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False).to(dt)
            else:       # i.i.d. N(0, 2 px) offsets (worst case for locality)
                off = (torch.randn(2, 18, H, W, device="cuda") * 2).to(dt)
            geo = (3, 3, 1, 1, 1, 1, 1, 1, 1)
            ncol = 2 * H * W
            alg = e * (x.numel() + off.numel() + Cc * 9 * ncol)
            us = dev_time_us(lambda: C.deformable_im2col(x, off, None, *geo), iters)
            tagx = " smooth-offsets" if smooth else ""
            out.append(_entry(f"dcn_im2col C={Cc} {H}x{W} {str(dt)[6:]}{tagx}", us, alg))
            col = torch.randn(Cc * 9, ncol, device="cuda").to(dt)
            gim = torch.zeros_like(x)
            us = dev_time_us(lambda: C.deformable_col2im(col, off, None, gim, *geo), iters)
            out.append(_entry(f"dcn_col2im default C={Cc} {H}x{W} {str(dt)[6:]}{tagx}", us, alg))
            tune("dcn_col2im", 1)
            us = dev_time_us(lambda: C.deformable_col2im(col, off, None, gim, *geo), max(3, iters // 5))
            out.append(_entry(f"dcn_col2im gather (index+sort+gather, XCD-contiguous) C={Cc} {H}x{W} {str(dt)[6:]}{tagx}", us, alg))
            tune("dcn_gather_xcd", 1)
            us = dev_time_us(lambda: C.deformable_col2im(col, off, None, gim, *geo), max(3, iters // 5))
            tune("dcn_gather_xcd", 0)
            out.append(_entry(f"dcn_col2im gather (plain block order) C={Cc} {H}x{W} {str(dt)[6:]}{tagx}", us, alg))
            tune("dcn_col2im", 2)
            us = dev_time_us(lambda: C.deformable_col2im(col, off, None, gim, *geo), max(3, iters // 5))
            tune("dcn_col2im", 0)
            out.append(_entry(f"dcn_col2im scatter (LDS atomics) C={Cc} {H}x{W} {str(dt)[6:]}{tagx}", us, alg))
            if True:
                ref_g = torch.zeros_like(x)
                C.deformable_col2im(col, off, None, ref_g, *geo)
                tune("dcn_col2im", 3)
                us = dev_time_us(lambda: C.deformable_col2im(col, off, None, gim, *geo), max(3, iters // 5))
                got = torch.zeros_like(x)
                C.deformable_col2im(col, off, None, got, *geo)
                tune("dcn_col2im", 0)
                err = float((got.float() - ref_g.float()).abs().max())
                out.append(_entry(f"dcn_col2im ELL index C={Cc} {H}x{W} {str(dt)[6:]}{tagx}", us, alg,
                                  {"max_abs_diff_vs_default": err}))
            goff = torch.empty_like(off)
            us = dev_time_us(lambda: C.deformable_col2im_coord(col, x, off, None, goff, None, *geo), iters)
            out.append(_entry(f"dcn_col2im_coord C={Cc} {H}x{W} {str(dt)[6:]}{tagx}", us, alg))
    return out


def bench_dcn_block(C, iters):
    """One modulated deformable 3x3 block of cfg-5 (R-101 + DCN, fp16) at its three layer shapes, forward and backward
    through the `_C` entry points the layers call: channels-last pipeline (default) vs the reference-layout kernels
    (tuning dcn_nhwc = 2), fused MFMA forward where it applies; plus the pipeline's own kernels one by one."""
    out = []
    for (Cc, H, W) in [(128, 100, 168), (256, 50, 84), (512, 25, 42)]:
        for dt in (torch.float16, torch.float32):
            e = 2 if dt == torch.float16 else 4
            x = torch.randn(2, Cc, H, W, device="cuda").to(dt)
            off = (torch.randn(2, 18, H, W, device="cuda") * 2).to(dt)
            msk = torch.rand(2, 9, H, W, device="cuda").to(dt)
            w = (torch.randn(Cc, Cc, 3, 3, device="cuda") / (3 * Cc ** 0.5)).to(dt)
            bias = torch.zeros(Cc, device="cuda", dtype=dt)
            y = torch.empty(2, Cc, H, W, device="cuda", dtype=dt)
            go = torch.randn(2, Cc, H, W, device="cuda").to(dt)
            empty = torch.empty(0, device="cuda", dtype=dt)
            geo = (3, 3, 1, 1, 1, 1, 1, 1, 1, 1)
            flops = 2.0 * Cc * Cc * 9 * 2 * H * W
            io_bytes = e * (x.numel() + off.numel() + msk.numel() + y.numel())
            tag = f"C={Cc} {H}x{W} {str(dt)[6:]}"

            def fwd():
                C.modulated_deform_conv_forward(x, w, bias, empty, off, msk, y, empty, *geo, True)

            gi, gw, gb = torch.zeros_like(x), torch.zeros_like(w), torch.zeros_like(bias)
            goff, gm = torch.zeros_like(off), torch.zeros_like(msk)

            def bwd():
                C.modulated_deform_conv_backward(x, w, bias, empty, off, msk, empty, gi, gw, gb, goff, gm, go, *geo, True)

            res = {}
            for name, key, val in (("channels-last pipeline", "dcn_nhwc", 0), ("reference-layout kernels", "dcn_nhwc", 2)):
                tune("dcn_fused", 2)
                tune(key, val)
                us = dev_time_us(fwd, iters)
                out.append(_entry(f"dcn_block fwd [{name}] {tag}", us, io_bytes, {"TFLOPs": round(flops / us / 1e6, 1)}))
                res["fwd " + name] = y.float().clone()
                us = dev_time_us(bwd, max(3, iters // 2))
                out.append(_entry(f"dcn_block bwd [{name}] {tag}", us, 2 * io_bytes, {"TFLOPs": round(2 * flops / us / 1e6, 1)}))
                gi.zero_(); gw.zero_(); gb.zero_()
                bwd()
                res["bwd " + name] = (gi.float().clone(), gw.float().clone(), goff.float().clone(), gm.float().clone())
                gi.zero_(); gw.zero_(); gb.zero_()
                tune(key, 0)
                tune("dcn_fused", 0)
            if dt == torch.float16:
                tune("dcn_fused", 1)
                us = dev_time_us(fwd, iters)
                tune("dcn_fused", 0)
                out.append(_entry(f"dcn_block fwd [fused MFMA] {tag}", us, io_bytes, {"TFLOPs": round(flops / us / 1e6, 1)}))
            a, b = res["bwd channels-last pipeline"], res["bwd reference-layout kernels"]
            out[-1 if dt != torch.float16 else -2]["max_rel_diff_vs_reference_layout"] = [
                round(float((p - q).abs().max() / q.abs().max().clamp_min(1e-6)), 5) for p, q in zip(a, b)]
            # the pipeline's kernels, one by one
            xT = C._to_nhwc(x)
            us = dev_time_us(lambda: C._to_nhwc(x), iters)
            out.append(_entry(f"dcn nchw->nhwc {tag}", us, 2 * e * x.numel()))
            g9 = (3, 3, 1, 1, 1, 1, 1, 1, 1)
            colT = C._im2col_nhwc(xT, off, msk, 2, Cc, H, W, g9)
            us = dev_time_us(lambda: C._im2col_nhwc(xT, off, msk, 2, Cc, H, W, g9), iters)
            out.append(_entry(f"dcn im2col_nhwc {tag}", us, e * (x.numel() + off.numel() + msk.numel() + colT.numel())))
            us = dev_time_us(lambda: C._coord_nhwc(colT, xT, off, msk, goff, gm, 2, Cc, H, W, g9), iters)
            out.append(_entry(f"dcn coord_nhwc {tag}", us, e * (x.numel() + 2 * off.numel() + 2 * msk.numel() + colT.numel())))
            gT = C._to_nhwc(go)
            us = dev_time_us(lambda: C._transposed_sample(gT, off, msk, 2, Cc, H, W, Cc, g9), iters)
            out.append(_entry(f"dcn transposed_sample (index build + gather) {tag}", us, e * (go.numel() + off.numel() + msk.numel() + colT.numel())))
    return out


def bench_keypoint(C, iters):
    """the keypoint head's kernels (csrc/keypoint.hip): targets of 2 x 256 slots against 20 ground truths; the loss at
    P = 256, K = 17, M = 56 on NCHW and channels-last logits (bytes: logits read + gradient written = 109 MB, ~17 us at the
    6.29 TB/s copy ceiling); decoding of 100 detections with sides log-uniform in 32-800 px (bytes: the heatmaps + outputs)"""
    out = []
    g = torch.Generator().manual_seed(3)
    P, K, M, G = 512, 17, 56, 20
    gt = torch.rand(G, 2, generator=g) * 600
    gt = torch.cat([gt, gt + 40 + torch.rand(G, 2, generator=g) * 400], 1)
    kp = torch.cat([gt[:, None, :2] + torch.rand(G, K, 2, generator=g) * (gt[:, None, 2:] - gt[:, None, :2]),
                    torch.randint(0, 3, (G, K, 1), generator=g).float()], 2)
    matched = torch.randint(0, G, (P,), generator=g)
    boxes = gt[matched] + torch.randn(P, 4, generator=g) * 10
    labels = torch.ones(P, dtype=torch.int64)
    args = [a.cuda() for a in (boxes, matched, labels, gt, kp)]
    us = dev_time_us(lambda: C.keypoint_targets(*args, M), iters)
    out.append(_entry("keypoint_targets P=512 K=17 G=20", us, P * (16 + 8 + 8) + G * (16 + K * 12) + P * K * 9))
    P = 256
    logits = torch.randn(P, K, M, M, device="cuda") * 3
    heat = torch.randint(0, M * M, (P, K), device="cuda")
    valid = torch.rand(P, K, device="cuda") < 0.7
    for tag, x in (("nchw", logits), ("channels-last", logits.contiguous(memory_format=torch.channels_last))):
        us = dev_time_us(lambda: C.keypoint_loss(x, heat, valid), iters)
        out.append(_entry("keypoint_loss value+grad P=256 K=17 M=56 %s" % tag, us, 2 * x.numel() * 4 + P * K * 9))
    N = 100
    s_ = torch.exp(torch.empty(N, 2).uniform_(np.log(32), np.log(800), generator=g))
    xy = torch.rand(N, 2, generator=g) * 500
    dets = torch.cat([xy, xy + s_], 1).cuda()
    maps = torch.randn(N, K, M, M, generator=g).cuda()
    us = dev_time_us(lambda: C.heatmaps_to_keypoints(maps, dets), max(5, iters // 5))
    out.append(_entry("heatmaps_to_keypoints N=100 K=17 sides 32-800 px", us, maps.numel() * 4 + N * K * 16,
                      {"resized_px_per_map_mean": int((s_[:, 0].ceil() * s_[:, 1].ceil()).mean())}))
    return out


def bench_masker(C, iters):
    """masks at inference (csrc/masker.hip): 100 detections of one 800 x 1333 image, M = 28, box sides log-uniform in
    32-800 px.  Dense paste: bytes = the N * H * W planes written + the maps read (107 MB, ~17 us at the 6.29 TB/s copy
    ceiling); the same detections as uncompressed RLE (count pass, scans, the host read of the total, write pass; bytes:
    maps, column tables and counts — the planes are never stored); and paste_masks_torch on the same device tensors —
    the per-detection loop of interpolate / threshold / slice assignment a user would write today."""
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import paste_masks_torch
    g = torch.Generator().manual_seed(5)
    N, H, W, M = 100, 800, 1333, 28
    s_ = torch.exp(torch.empty(N, 2).uniform_(np.log(32), np.log(800), generator=g))
    xy = torch.rand(N, 2, generator=g) * torch.tensor([W - 32.0, H - 32.0])
    boxes = torch.cat([xy, xy + s_], 1).cuda()
    maps = torch.sigmoid(3 * torch.randn(N, 1, M, M, generator=g)).cuda()
    alg = N * H * W + N * M * M * 4
    window = (torch.minimum(xy + s_, torch.tensor([float(W), float(H)])) - xy).prod(1)
    extra = {"window_px_mean": int(window.mean())}
    out = []
    us = dev_time_us(lambda: C.paste_masks(maps, boxes, [(H, W)], 0.5, 1, counts=[N]), iters)
    out.append(_entry("paste_masks dense N=100 800x1333 M=28", us, alg, dict(extra, frac_of_copy_peak=round(alg / us / 1e3 / 6290.0, 4))))
    us = dev_time_us(lambda: C.paste_masks_rle(maps, boxes, [(H, W)], 0.5, 1, counts=[N]), iters)
    runs = int(C.paste_masks_rle(maps, boxes, [(H, W)], 0.5, 1, counts=[N])[1][-1])
    # bytes this path touches: the maps read by both passes, the column tables written, scanned and read, the counts
    rle_bytes = 2 * N * M * M * 4 + 3 * 2 * N * W * 4 + runs * 4
    out.append(_entry("paste_masks_rle N=100 800x1333 M=28", us, rle_bytes, dict(extra, runs=runs)))
    us = dev_time_us(lambda: paste_masks_torch(maps, boxes, H, W, 0.5, 1), max(3, iters // 10), warmup=2)
    out.append(_entry("paste_masks_torch loop, device tensors N=100 800x1333 M=28", us, alg, extra))
    return out


def bench_polygons(C, iters):
    """mask-head targets from polygons (csrc/polygon.hip) next to the dense path at the same slots: 20 instances of one
    800 x 1333 image as polygons of 24-200 vertices (jittered ellipses, every fourth instance two overlapping ones), 256
    slots with boxes jittered around their instances, M = 28.  polygon_mask_targets reads the packed polygons (bytes:
    vertices + offsets + boxes + targets); mask_targets crops and resizes the instances' 800 x 1333 uint8 planes (bytes: the
    box windows read + targets; the planes themselves, 21 MB, must first reach the device).  polygons_to_masks writes those
    20 planes (bytes: the planes)."""
    from maskrcnn_benchmark.structures.segmentation_mask import PolygonList
    rng = np.random.RandomState(11)
    G, S, H, W, M = 20, 256, 800, 1333, 28
    insts, ext = [], []
    for g in range(G):
        hw_, hh_ = np.exp(rng.uniform(np.log(12), np.log(330), 2))
        cx, cy = rng.uniform(hw_, W - hw_), rng.uniform(min(hh_, H / 2 - 1), max(H - hh_, H / 2 + 1))
        polys = []
        for fx, fy in ([(1.0, 1.0)] if g % 4 != 3 else [(1.0, 0.6), (0.6, 1.0)]):
            k = int(rng.randint(24, 201))
            a = np.arange(k) * (2 * np.pi / k)
            r = 1 + 0.08 * rng.uniform(-1, 1, k)
            polys.append(np.stack([cx + fx * hw_ * r * np.cos(a), cy + fy * hh_ * r * np.sin(a)], 1).reshape(-1).tolist())
        insts.append(polys)
        ext.append((cx - hw_, cy - hh_, cx + hw_, cy + hh_))
    plist = PolygonList(insts, (W, H))
    k = plist.packed().to("cuda")
    inst = torch.from_numpy(rng.randint(0, G, S)).cuda()
    e = np.array(ext)[inst.cpu().numpy()]
    side = np.stack([e[:, 2] - e[:, 0], e[:, 3] - e[:, 1]] * 2, 1)
    boxes_np = (e + rng.uniform(-0.2, 0.2, (S, 4)) * side).astype(np.float32)
    boxes_np[:, 2:] = np.maximum(boxes_np[:, 2:], boxes_np[:, :2] + 1)
    boxes = torch.from_numpy(boxes_np).cuda()
    wh = torch.tensor([[W, H]], dtype=torch.int32).expand(S, 2).contiguous().cuda()
    verts_total = int(k.V)
    extra = {"vertices": verts_total, "vertices_per_instance_mean": round(verts_total / G, 1)}
    out = []
    us = dev_time_us(lambda: C.polygon_mask_targets(k.verts, k.poly_offset, k.inst_offset, inst, boxes, wh, M), iters)
    out.append(_entry("polygon_mask_targets S=256 M=28 (20 instances, 24-200 vertices)", us,
                      k.buffer.numel() * 4 + S * (16 + 8 + 8) + S * M * M * 4, extra))
    us = dev_time_us(lambda: C.polygons_to_masks(k.verts, k.poly_offset, k.inst_offset, H, W), iters)
    out.append(_entry("polygons_to_masks G=20 800x1333", us, G * H * W, dict(extra, frac_of_copy_peak=round(G * H * W / us / 1e3 / 6290.0, 4))))
    masks = C.polygons_to_masks(k.verts, k.poly_offset, k.inst_offset, H, W)
    cb = np.clip(np.round(boxes_np), 0, [W, H, W, H])
    window = float((np.maximum(cb[:, 2] - cb[:, 0], 1) * np.maximum(cb[:, 3] - cb[:, 1], 1)).sum())
    us = dev_time_us(lambda: C.mask_targets(masks, inst, boxes, M), iters)
    out.append(_entry("mask_targets S=256 M=28 (dense 800x1333 uint8 planes, same slots)", us, int(window) + S * M * M * 4,
                      {"planes_bytes": G * H * W, "polygons_bytes": k.buffer.numel() * 4}))
    return out


def bench_input_prep(C, iters, copy_gbs=None):
    """the input path of one training batch (csrc/image_prep.hip): two 480 x 640 RGB uint8 images -> 800 x 1066, padded to
    800 x 1088 (SIZE_DIVISIBILITY 32), the default BGR-255 normalisation, one flipped.
    image_batch rows: the one launch on a device-resident buffer, HIP events; bytes = the raw images read + the fp32 batch
    written; frac_of_copy_peak = the bytes WRITTEN over the time, against the copy row of the same run.
    end-to-end rows (host clock around a device synchronise, per batch): `device` = RawImageBatch.to(cuda) from pinned
    memory (one 1.8 MB copy + the launch); `host` = the thing it replaces: the host transforms on the same two images
    (Pillow resize, flip, ToTensor, Normalize), to_image_list, and the 20.9 MB fp32 copy (+ the channels-last pass the
    detector then runs).  The host rows need Pillow; the image decode is outside both."""
    from maskrcnn_benchmark.data import transforms as T
    from maskrcnn_benchmark.data.collate_batch import BatchCollator, RawImageBatch
    rng = np.random.RandomState(3)
    yy, xx = np.mgrid[0:480, 0:640]
    srcs = [np.clip(np.stack([xx * 0.4, yy * 0.5, 128 + 100 * np.sin(0.05 * xx + 0.03 * yy + i)], 2) + rng.normal(0, 20, (480, 640, 3)),
                    0, 255).astype(np.uint8) for i in range(2)]
    mean, std, bgr = [102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0], True
    table = T.normalisation_table(mean, std, bgr)
    out = []
    written = 2 * 3 * 800 * 1088 * 4

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    for cl in (False, True):
        batch = RawImageBatch.pack([T.RawImage(srcs[0], (1066, 800), 0), T.RawImage(srcs[1], (1066, 800), 1)], table, bgr, 32, cl)
        batch.pin_memory()
        buf = batch.buffer.cuda()
        off, geom, tab = buf[:16].view(torch.int64), buf[16:56].view(torch.int32).view(2, 5), buf[56:56 + 3072].view(torch.float32).view(3, 256)
        us = dev_time_us(lambda: C.image_batch(buf, off, geom, tab, bgr, 800, 1088, channels_last=cl, geom_host=batch.geom), iters)
        extra = {"bytes_written": written}
        if copy_gbs:
            extra["frac_of_copy_peak"] = round(written / us / 1e3 / copy_gbs, 4)
        out.append(_entry("image_batch 2 x 480x640 -> 800x1066 in 800x1088 %s" % ("channels_last" if cl else "nchw"), us,
                          buf.numel() + written, extra))
        us = wall(lambda: batch.to("cuda"), max(iters, 20))
        out.append(_entry("input_prep end-to-end device (pinned copy + launch) %s" % ("channels_last" if cl else "nchw"), us,
                          buf.numel() + written, {"h2d_bytes": buf.numel()}))
    try:
        from PIL import Image
    except ImportError:
        print("input_prep: Pillow is not installed here: the host rows are not measured")
        return out
    import random
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    pil = [Image.fromarray(a, "RGB") for a in srcs]
    flips = [T.RandomHorizontalFlip(0.0), T.RandomHorizontalFlip(1.0)]
    pipes = [T.Compose([T.Resize((800,), 1333), f, T.ToTensor(), T.Normalize(mean, std, bgr)]) for f in flips]
    box = BoxList(torch.tensor([[10.0, 10.0, 100.0, 100.0]]), (640, 480))
    collate = BatchCollator(32)

    def host(cl):
        random.seed(0)
        items = [pipe(im, box) + (0,) for pipe, im in zip(pipes, pil)]
        x = collate(items)[0].to("cuda").tensors
        return x.contiguous(memory_format=torch.channels_last) if cl else x

    for cl in (False, True):
        us = wall(lambda: host(cl), 10)
        out.append(_entry("input_prep end-to-end host (Pillow + ToTensor + Normalize + pad + fp32 copy) %s" % ("channels_last" if cl else "nchw"),
                          us, 2 * 480 * 640 * 3 + written, {"h2d_bytes": written}))
    return out


def bench_color_jitter(C, iters, copy_gbs=None):
    """colour jitter of one training batch (csrc/color_jitter.hip): two 480 x 640 RGB uint8 images on a device-resident
    buffer, all four steps each, hue not last and contrast in the middle, so both launches run (the sum pass applies the
    step in front of contrast on the fly).  The operator works in place and jittered bytes are not the workload (repeated
    jitter drives an image to grey, which skips the hue path), so EVERY call starts from a pristine device copy of the
    buffer, restored outside the timed span.
    device rows: a HIP event pair per call; in front of the first event the stream is given ~0.3 ms of other work
    (torch.cuda._sleep), so the memset and both launches are queued before the device reaches them and the span holds
    device time, not the host's enqueue rate.  median and first call; bytes = the images read by the sum pass + read and
    written by the apply pass; frac_of_copy_peak = those bytes over the median, against the copy row of the same run.
    host row: the host clock around the Python wrapper call alone (no synchronise): what a call costs the host to enqueue.
    The wrapper is host-bound when the host row exceeds the device row."""
    from maskrcnn_benchmark import _color_jitter_cpu as J
    from maskrcnn_benchmark._lib import lib, ptr, stream_of
    from maskrcnn_benchmark.data import transforms as T
    from maskrcnn_benchmark.data.collate_batch import RawImageBatch
    rng = np.random.RandomState(3)
    yy, xx = np.mgrid[0:480, 0:640]
    srcs = [np.clip(np.stack([xx * 0.4, yy * 0.5, 128 + 100 * np.sin(0.05 * xx + 0.03 * yy + i)], 2) + rng.normal(0, 20, (480, 640, 3)),
                    0, 255).astype(np.uint8) for i in range(2)]
    steps = [[(J.SATURATION, 1.2), (J.CONTRAST, 0.9), (J.HUE, 13), (J.BRIGHTNESS, 1.1)],
             [(J.HUE, 243), (J.CONTRAST, 1.1), (J.BRIGHTNESS, 0.9), (J.SATURATION, 0.8)]]
    table = T.normalisation_table([102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0], True)
    batch = RawImageBatch.pack([T.RawImage(s, (1066, 800), 0, st) for s, st in zip(srcs, steps)], table, True, 32)
    pristine = batch.buffer.cuda()
    buf = pristine.clone()
    off, geom = buf[:16].view(torch.int64), buf[16:56].view(torch.int32).view(2, 5)
    jit = buf[buf.numel() - 64:].view(torch.int32).view(2, 8)
    ws = torch.empty(2, dtype=torch.int64, device="cuda")
    grey = int(sum(((s[..., 0] == s[..., 1]) & (s[..., 1] == s[..., 2])).sum() for s in srcs))   # pixels that skip the hue path

    def wrapper():
        C.color_jitter(buf, off, geom, jit, geom_host=batch.geom, jitter_host=batch.jitter)

    def entry():
        rc = lib.detops_color_jitter_u8(ptr(buf), buf.numel(), ptr(off), ptr(geom), ptr(batch.geom), ptr(jit), ptr(batch.jitter), 2,
                                        ptr(ws), 16, stream_of(buf))
        assert rc == 0, rc

    def device_us(fn, n):
        spans, host = [], []
        for _ in range(n + 3):
            buf.copy_(pristine)
            torch.cuda._sleep(600000)                      # the host runs ahead of the device
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - t0) * 1e6)
            b.record()
            torch.cuda.synchronize()
            spans.append(a.elapsed_time(b) * 1000.0)
        spans, host = spans[3:], host[3:]                  # three warm-up calls
        return float(np.median(spans)), spans[0], float(np.median(host))

    moved = 3 * 2 * 480 * 640 * 3
    out = []
    for name, fn in (("entry point", entry), ("wrapper", wrapper)):
        med, first, host = device_us(fn, iters)
        extra = {"launches": 2, "first_us": round(first, 2), "grey_source_pixels": grey}
        if copy_gbs:
            extra["frac_of_copy_peak"] = round(moved / med / 1e3 / copy_gbs, 4)
        out.append(_entry("color_jitter 2 x 480x640, 4 steps each, device time, %s" % name, med, moved, extra))
        out.append(_entry("color_jitter host time to enqueue one call, %s" % name, host, moved))
    return out


def bench_bbox_aug(C, iters, copy_gbs=None):
    """the merge of test-time box augmentation (csrc/bbox_aug.hip): N = 2 images, T = 6 passes, 1000 rows per group, 81
    classes, about 1 % of the (row, class) pairs above the score threshold.
    `merge kernels` row: the four launches (count, prefix, offsets, write) on preallocated outputs, HIP events; bytes = what they read
    (scores twice, the candidates' boxes once) + the candidates written; frac_of_copy_peak = the bytes READ over the time,
    against the copy row of the same run.  The other rows are per-call host-clock times around a device synchronise (each has
    host reads inside): _C.bbox_aug_merge as the engine calls it; merge + one segmented NMS + the per-image limit
    (engine/bbox_aug.py: merge_detections); the torch formulation of the merge on the same device tensors
    (_bbox_aug_torch.py); and the formulation there was before: PostProcessor.filter_results on each image's concatenated
    rows, every (row, class) pair padded to a dummy box, one NMS call per image (it includes NMS and the limit, like the
    merge + NMS + top-k row)."""
    from maskrcnn_benchmark import _bbox_aug_torch, _lib
    from maskrcnn_benchmark.engine.bbox_aug import merge_detections
    from maskrcnn_benchmark.modeling.roi_heads.box_head.inference import PostProcessor
    N, T, rows, NC, thresh = 2, 6, 1000, 81, 0.05
    R = N * T * rows
    rng = np.random.RandomState(7)
    frames = [[(1201, 800), (1201, 800), (600, 400), (600, 400), (1500, 1001), (1500, 1001)] for _ in range(N)]
    flips = [0, 1, 0, 1, 0, 1]
    group = np.repeat(np.arange(N * T), rows)
    wh = np.array([frames[g // T][g % T] for g in range(N * T)], np.float64)[group]
    lo = rng.uniform(-0.05, 0.8, (R, NC, 2))
    boxes = _t((np.concatenate([lo, lo + rng.uniform(0.02, 0.3, lo.shape)], -1) * np.concatenate([wh, wh], 1)[:, None, :])
               .reshape(R, 4 * NC).astype(np.float32))
    scores = _t(np.where(rng.rand(R, NC) < 0.01, rng.uniform(0.06, 1.0, (R, NC)), rng.uniform(0.0, 0.04, (R, NC))).astype(np.float32))
    row_offset = torch.arange(0, R + 1, rows, dtype=torch.int32)
    geom, ratio = _bbox_aug_torch.group_records(frames, flips)
    sizes = [f[0] for f in frames]

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    cand_boxes, cand_scores, seg_offsets, longest = C.bbox_aug_merge(boxes, scores, row_offset, geom, ratio, N, T, thresh)
    M = cand_scores.numel()
    d_off, d_geom, d_ratio = row_offset.cuda(), geom.cuda(), ratio.cuda()
    totals = torch.empty((2,), dtype=torch.int32, device="cuda")
    nbytes = int(_lib.lib.detops_bbox_aug_merge_workspace_bytes(N, NC, T * rows))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    ptr, st = _lib.ptr, _lib.stream_of

    def kernels():
        _lib.check(_lib.lib.detops_bbox_aug_merge_count(ptr(scores), ptr(d_off), ptr(row_offset), R, NC, N, T, thresh, ptr(seg_offsets),
                                                        ptr(totals), ptr(ws), nbytes, st(scores)), "count")
        _lib.check(_lib.lib.detops_bbox_aug_merge_write(ptr(boxes), ptr(scores), ptr(d_off), ptr(row_offset), ptr(d_geom), ptr(d_ratio),
                                                        R, NC, N, T, thresh, ptr(seg_offsets), M, ptr(cand_boxes), ptr(cand_scores),
                                                        ptr(ws), nbytes, st(scores)), "write")

    read = 2 * R * NC * 4 + M * 16
    us = dev_time_us(kernels, iters)
    extra = {"candidates": M, "longest_segment": longest, "bytes_read": read}
    if copy_gbs:
        extra["frac_of_copy_peak"] = round(read / us / 1e3 / copy_gbs, 4)
    out = [_entry("bbox_aug merge kernels (count, prefix, offsets, write) N=2 T=6 1000 rows C=81", us, read + M * 20, extra)]
    n = max(iters // 2, 10)
    us = wall(lambda: C.bbox_aug_merge(boxes, scores, row_offset, geom, ratio, N, T, thresh), n)
    out.append(_entry("bbox_aug _C.bbox_aug_merge (record upload, host read of M, allocation)", us, read + M * 20))
    us = wall(lambda: merge_detections(boxes, scores, row_offset, geom, ratio, sizes, T, thresh, 0.5, 100), n)
    out.append(_entry("bbox_aug merge + segmented NMS + top-k (merge_detections)", us, read + M * 20))
    us = wall(lambda: _bbox_aug_torch.bbox_aug_merge(boxes, scores, row_offset, geom, ratio, N, T, thresh), n)
    out.append(_entry("bbox_aug torch formulation of the merge, same device tensors", us, read + M * 20))
    post = PostProcessor(thresh, 0.5, 100)
    per_image = T * rows

    def padded():
        return [post.filter_results(boxes[i * per_image:(i + 1) * per_image], scores[i * per_image:(i + 1) * per_image], sizes[i])
                for i in range(N)]

    us = wall(padded, n)
    out.append(_entry("bbox_aug padded formulation: filter_results per image on the concatenated rows (NMS + top-k)", us,
                      R * NC * 20))
    return out


def bench_coco_results(C, iters, copy_gbs=None):
    """compressed RLE strings of COCO result files (csrc/rle_string.hip): the runs of bench_masker's case, 100 detections of
    one 800 x 1333 image at M = 28, straight from paste_masks_rle.
    `kernels` row: the launches of the two calls (count + offsets, write) on preallocated outputs, HIP events; bytes = the counts
    read by both passes + the strings written; bytes_written / time against the copy row of the same run is
    frac_of_copy_peak.  The other rows are host-clock times around a device synchronise, per call: _C.rle_strings plus the
    conversion to a list of str (one host read of the total, one device-to-host copy of offsets and bytes, one decode); the
    numpy statement (_rle_cpu.py) on the same counts INCLUDING the device-to-host copy of the counts and offsets it needs;
    and the literal Python loop of the definition on the first 10 detections' runs (already on the host), scaled to all."""
    from maskrcnn_benchmark import _lib, _rle_cpu
    g = torch.Generator().manual_seed(5)
    N, H, W, M = 100, 800, 1333, 28
    s_ = torch.exp(torch.empty(N, 2).uniform_(np.log(32), np.log(800), generator=g))
    xy = torch.rand(N, 2, generator=g) * torch.tensor([W - 32.0, H - 32.0])
    boxes = torch.cat([xy, xy + s_], 1).cuda()
    maps = torch.sigmoid(3 * torch.randn(N, 1, M, M, generator=g)).cuda()
    counts, run_offset = C.paste_masks_rle(maps, boxes, [(H, W)], 0.5, 1, counts=[N])
    total = counts.numel()
    data, byte_offset = C.rle_strings(counts, run_offset)
    strings = C.rle_string_list(data, byte_offset)
    B = data.numel()
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_of
    nbytes = int(lib.detops_rle_string_workspace_bytes(total))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")

    def kernels():
        _lib.check(lib.detops_rle_string_count(ptr(counts), ptr(run_offset), total, N, ptr(byte_offset), ptr(ws), nbytes, st(counts)),
                   "count")
        _lib.check(lib.detops_rle_string_write(ptr(counts), ptr(run_offset), total, N, ptr(byte_offset), ptr(data), ptr(ws), nbytes,
                                               st(counts)), "write")

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    def numpy_path():
        d, off = _rle_cpu.rle_strings(counts.cpu().numpy(), run_offset.cpu().numpy())
        return _rle_cpu.to_str_list(d, off)

    def literal(runs):
        out = []
        for i in range(len(runs)):
            x = runs[i] - runs[i - 2] if i > 2 else runs[i]
            while True:
                ch = x & 0x1f
                x >>= 5
                more = (x != -1) if ch & 0x10 else (x != 0)
                if more:
                    ch |= 0x20
                out.append(ch + 48)
                if not more:
                    break
        return bytes(out).decode("ascii")

    us = dev_time_us(kernels, iters)
    extra = {"runs": total, "string_bytes": B}
    if copy_gbs:
        extra["frac_of_copy_peak"] = round(B / us / 1e3 / copy_gbs, 6)
    out = [_entry("coco_results rle_string kernels (count, offsets, write) N=100 800x1333", us, 2 * total * 4 + B, extra)]
    assert numpy_path() == strings
    n = max(iters // 2, 10)
    dev_us = wall(lambda: C.rle_string_list(*C.rle_strings(counts, run_offset)), n)
    out.append(_entry("coco_results _C.rle_strings + list of str (host read of B, one D2H copy, decode)", dev_us, 2 * total * 4 + 2 * B))
    np_us = wall(numpy_path, n)
    out.append(_entry("coco_results numpy path on the same counts (D2H copy of counts and offsets included)", np_us,
                      2 * total * 4 + B, {"numpy_over_device": round(np_us / dev_us, 2)}))
    offs = run_offset.cpu().tolist()
    host_runs = [counts[offs[i]:offs[i + 1]].cpu().tolist() for i in range(10)]
    assert [literal(r) for r in host_runs] == strings[:10]
    t0 = time.perf_counter()
    for r in host_runs:
        literal(r)
    lit_us = (time.perf_counter() - t0) * 1e6 * total / max(offs[10], 1)
    out.append(_entry("coco_results literal Python loop, first 10 detections scaled to %d runs" % total, lit_us, total * 4 + B,
                      {"runs_timed": offs[10], "literal_over_device": round(lit_us / dev_us, 1)}))
    return out


def bench_rle_decode(C, iters):
    """reading result files back (csrc/rle_decode.hip, detops_mask_pack_rle of csrc/evaluate.hip): the strings of bench_coco_results' case, 100
    detections of one 800 x 1333 image, decoded and packed into bit rows.
    `kernels` row: the launches of the two decode calls on preallocated outputs, HIP events; bytes = the strings read by every
    pass (5) + the runs written.  Every other row is a host clock around a device synchronise, per call:
    _C.rle_string_decode_list from the list of str (one H2D copy, the host read of the total, the status check);
    _C.mask_pack_rle on device runs; the numpy statements of both on the same data (host arrays in, host arrays out); and
    the dense route to the same bit rows, _C.paste_masks + _C.mask_pack (107 MB of planes)."""
    from maskrcnn_benchmark import _eval_cpu, _lib, _rle_cpu
    g = torch.Generator().manual_seed(5)
    N, H, W, M = 100, 800, 1333, 28
    s_ = torch.exp(torch.empty(N, 2).uniform_(np.log(32), np.log(800), generator=g))
    xy = torch.rand(N, 2, generator=g) * torch.tensor([W - 32.0, H - 32.0])
    boxes = torch.cat([xy, xy + s_], 1).cuda()
    maps = torch.sigmoid(3 * torch.randn(N, 1, M, M, generator=g)).cuda()
    counts, run_offset = C.paste_masks_rle(maps, boxes, [(H, W)], 0.5, 1, counts=[N])
    total = counts.numel()
    data, byte_offset = C.rle_strings(counts, run_offset)
    strings = C.rle_string_list(data, byte_offset)
    B, hw = data.numel(), [(H, W)] * N
    hw_d = torch.tensor(hw, dtype=torch.int32).cuda()
    lib, ptr, st = _lib.lib, _lib.ptr, _lib.stream_of
    nbytes = int(lib.detops_rle_decode_workspace_bytes(B, N))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    ro, out, status = torch.zeros_like(run_offset), torch.empty_like(counts), torch.empty((N,), dtype=torch.int32, device="cuda")

    def kernels():
        _lib.check(lib.detops_rle_decode_count(ptr(data), ptr(byte_offset), B, N, ptr(ro), ptr(ws), nbytes, st(data)), "count")
        _lib.check(lib.detops_rle_decode_write(ptr(data), ptr(byte_offset), B, N, ptr(ro), total, ptr(hw_d), ptr(out), ptr(status),
                                               ptr(ws), nbytes, st(data)), "write")

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    us = dev_time_us(kernels, iters)
    assert torch.equal(out, counts) and torch.equal(ro, run_offset) and not bool(status.any())
    res = [_entry("rle_decode kernels (count, offsets, sums, write, status) N=100 800x1333", us, 5 * B + total * 4,
                  {"runs": total, "string_bytes": B})]
    n = max(iters // 2, 10)
    dev_us = wall(lambda: C.rle_string_decode_list(strings, hw, "cuda"), n)
    res.append(_entry("rle_decode _C.rle_string_decode_list, list of str -> device runs (one H2D copy, two host reads)", dev_us,
                      2 * B + total * 4))
    np_us = wall(lambda: C.rle_string_decode_list(strings, hw), n)
    res.append(_entry("rle_decode numpy path, list of str -> host runs", np_us, B + total * 4,
                      {"numpy_over_device": round(np_us / dev_us, 2)}))
    want = C.mask_pack(C.paste_masks(maps, boxes, [(H, W)], 0.5, 1, counts=[N])[1][0][:, 0])
    got = C.mask_pack_rle(counts, run_offset, hw)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    words = got[0].numel() * 8
    pack_us = wall(lambda: C.mask_pack_rle(counts, run_offset, hw), n)
    res.append(_entry("rle_decode _C.mask_pack_rle, device runs -> bit rows (no plane)", pack_us, total * 12 + words))
    c_h, ro_h = counts.cpu().numpy(), run_offset.cpu().numpy()
    np_pack = wall(lambda: _eval_cpu.mask_pack_rle(c_h, ro_h, hw), 2)
    res.append(_entry("rle_decode numpy mask_pack_rle on the same runs (host arrays)", np_pack, total * 4 + words,
                      {"numpy_over_device": round(np_pack / pack_us, 1)}))
    dense_us = wall(lambda: C.mask_pack(C.paste_masks(maps, boxes, [(H, W)], 0.5, 1, counts=[N])[1][0][:, 0]), n)
    res.append(_entry("rle_decode dense route: _C.paste_masks + _C.mask_pack (planes stored)", dense_us, 2 * N * H * W + words,
                      {"dense_over_rle": round(dense_us / pack_us, 2)}))
    return res


def bench_evaluation(C, iters):
    """detection evaluation (csrc/evaluate.hip): the 100 pasted detections of bench_masker against the 20 instances of
    bench_polygons, one 800 x 1333 image, all in one category (every pair is a problem pair: one problem of 100 x 20).
    mask_pack: bytes = the uint8 planes read + the bit rows written (frac_of_copy_peak counts the bytes READ only);
    mask_pair_counts: bytes = the words of both planes inside every pair's intersected extents; eval_iou + eval_match: the
    IoU matrix and the 40 lanes' records.  Last row: the same intersections from torch operators on the same device planes
    (planes to float, one matmul: exact, the counts stay below 2^24), written in the same run."""
    from maskrcnn_benchmark.structures.segmentation_mask import PolygonList
    g = torch.Generator().manual_seed(5)                      # bench_masker's detections
    N, H, W, M = 100, 800, 1333, 28
    s_ = torch.exp(torch.empty(N, 2).uniform_(np.log(32), np.log(800), generator=g))
    xy = torch.rand(N, 2, generator=g) * torch.tensor([W - 32.0, H - 32.0])
    boxes = torch.cat([xy, xy + s_], 1).cuda()
    maps = torch.sigmoid(3 * torch.randn(N, 1, M, M, generator=g)).cuda()
    _, views = C.paste_masks(maps, boxes, [(H, W)], 0.5, 1, counts=[N])
    dt = views[0][:, 0]
    rng = np.random.RandomState(11)                           # bench_polygons' instances
    G = 20
    insts = []
    for k in range(G):
        hw_, hh_ = np.exp(rng.uniform(np.log(12), np.log(330), 2))
        cx, cy = rng.uniform(hw_, W - hw_), rng.uniform(min(hh_, H / 2 - 1), max(H - hh_, H / 2 + 1))
        polys = []
        for fx, fy in ([(1.0, 1.0)] if k % 4 != 3 else [(1.0, 0.6), (0.6, 1.0)]):
            n = int(rng.randint(24, 201))
            a = np.arange(n) * (2 * np.pi / n)
            r = 1 + 0.08 * rng.uniform(-1, 1, n)
            polys.append(np.stack([cx + fx * hw_ * r * np.cos(a), cy + fy * hh_ * r * np.sin(a)], 1).reshape(-1).tolist())
        insts.append(polys)
    pk = PolygonList(insts, (W, H)).packed().to("cuda")
    gt = C.polygons_to_masks(pk.verts, pk.poly_offset, pk.inst_offset, H, W)
    WW = (W + 63) // 64
    out = []
    us = dev_time_us(lambda: C.mask_pack(dt), iters)
    out.append(_entry("mask_pack N=100 800x1333 (pasted detections)", us, N * H * W + N * H * WW * 8,
                      {"frac_of_copy_peak_bytes_read": round(N * H * W / us / 1e3 / 6290.0, 4)}))
    # the entry point alone, sizes and offsets already on the device (the rows above and below include the wrapper's host work)
    from maskrcnn_benchmark import _lib
    words, word_offset, hw, area, extent = C.mask_pack(dt)
    plane_offset = (torch.arange(N, dtype=torch.int64) * (H * W)).cuda()
    dt8 = dt.view(torch.uint8)
    raw = lambda: _lib.check(_lib.lib.detops_mask_pack(  # noqa: E731
        dt8.data_ptr(), plane_offset.data_ptr(), hw.data_ptr(), N, H * WW, word_offset.data_ptr(), words.data_ptr(),
        area.data_ptr(), extent.data_ptr(), _lib.stream_of(words)), "mask_pack")
    us = dev_time_us(raw, iters)
    out.append(_entry("detops_mask_pack entry point, N=100 800x1333, prebuilt offsets", us, N * H * W + N * H * WW * 8,
                      {"frac_of_copy_peak_bytes_read": round(N * H * W / us / 1e3 / 6290.0, 4)}))
    us = dev_time_us(lambda: C.mask_pack(gt), iters)
    out.append(_entry("mask_pack N=20 800x1333 (ground-truth planes)", us, G * H * W + G * H * WW * 8,
                      {"frac_of_copy_peak_bytes_read": round(G * H * W / us / 1e3 / 6290.0, 4)}))
    dp, gp = C.mask_pack(dt), C.mask_pack(gt)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()  # noqa: E731
    offs = (i32([0, N]), i32([0, G]), torch.tensor([0, N * G], dtype=torch.int64).cuda())
    pick = lambda p: (p[0], p[1], p[2], p[4])  # noqa: E731
    ed, eg = dp[4].cpu().numpy().astype(np.int64), gp[4].cpu().numpy().astype(np.int64)
    rows = np.maximum(np.minimum(ed[:, None, 1], eg[None, :, 1]) - np.maximum(ed[:, None, 0], eg[None, :, 0]) + 1, 0)
    cols = np.maximum(np.minimum(ed[:, None, 3], eg[None, :, 3]) - np.maximum(ed[:, None, 2], eg[None, :, 2]) + 1, 0)
    pair_bytes = int((rows * cols).sum()) * 16
    us = dev_time_us(lambda: C.mask_pair_counts(pick(dp), pick(gp), *offs, N * G), iters)
    out.append(_entry("mask_pair_counts 100 x 20 pairs 800x1333", us, pair_bytes,
                      {"overlapping_pairs": int(((rows * cols) > 0).sum()), "words_per_pair_mean": int((rows * cols).mean())}))
    counts = C.mask_pair_counts(pick(dp), pick(gp), *offs, N * G)
    crowd = torch.zeros((G,), dtype=torch.uint8).cuda()
    thrs = torch.from_numpy(np.linspace(0.5, 0.95, 10))
    rngs = torch.tensor([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=torch.float64)
    da, ga = dp[3].double(), gp[3].double()

    def iou_match():
        iou = C.eval_iou(C.EVAL_COCO_SEGM, *offs, N * G, counts=counts, dt_area=dp[3], gt_area=gp[3], gt_crowd=crowd)
        return C.eval_match(C.EVAL_COCO_SEGM, iou, *offs, (N, G, G), crowd, thrs, dt_area=da, gt_area=ga, area_rngs=rngs)

    us = dev_time_us(iou_match, iters)
    out.append(_entry("eval_iou + eval_match 100 x 20, 4 x 10 lanes", us, N * G * 12 + 40 * N * 5 + 4 * G))
    gt8 = gt

    def torch_counts():
        return dt8.reshape(N, -1).float() @ gt8.reshape(G, -1).float().t()

    us = dev_time_us(torch_counts, max(5, iters // 5), warmup=2)
    same = bool(torch.equal(torch_counts().to(torch.int32).reshape(-1), counts))
    out.append(_entry("torch: planes.float() matmul, same 100 x 20 intersections", us, (N + G) * H * W * 5, {"equal_counts": same}))
    return out


def bench_keypoint_oks(C, iters):
    """keypoint evaluation (csrc/eval_oks.hip): a batch of 8 images, one category, 20 detections by 8 ground truths each,
    K = 17 (1280 pairs, 21760 terms).  Rows: the entry point alone on prebuilt device arrays; _C.eval_oks through the
    wrapper (its contiguity / dtype checks, the sigma copy and two allocations included); a broadcast torch formulation of
    the same definition on the same device tensors (torch.sum adds in a tree: the last bits differ).  bytes = the keypoints,
    boxes and areas read once + the matrix and the areas written."""
    from maskrcnn_benchmark import _eval_cpu, _lib
    I, D, G, K = 8, 20, 8, 17
    rng = np.random.RandomState(3)
    gk = np.concatenate([rng.uniform(0, 600, (I * G, K, 2)), rng.randint(0, 3, (I * G, K, 1))], axis=2).astype(np.float32)
    gk[::7, :, 2] = 0                                         # some ground truths without a visible keypoint
    lo, hi = gk[:, :, :2].min(axis=1), gk[:, :, :2].max(axis=1)
    gb = np.concatenate([lo, hi], axis=1).astype(np.float32)
    ga = ((hi - lo).prod(axis=1) * 0.6).astype(np.float64)
    dk = np.repeat(gk.reshape(I, G, K, 3), 3, axis=1)[:, :D].reshape(I * D, K, 3).copy()
    dk[:, :, :2] += rng.normal(0, 12, (I * D, K, 2)).astype(np.float32)
    sig = _eval_cpu.COCO_PERSON_SIGMAS
    dto, gto = np.arange(I + 1, dtype=np.int32) * D, np.arange(I + 1, dtype=np.int32) * G
    ioo = np.arange(I + 1, dtype=np.int64) * (D * G)
    dk_d, gk_d, gb_d, ga_d, sig_d, dto_d, gto_d, ioo_d = (_t(a) for a in (dk, gk, gb, ga, sig, dto, gto, ioo))
    total = I * D * G
    alg = (dk.size + gk.size + gb.size) * 4 + ga.size * 8 + total * 8 + I * D * 8
    oks = torch.empty((total,), dtype=torch.float64, device="cuda")
    area = torch.empty((I * D,), dtype=torch.float64, device="cuda")
    raw = lambda: _lib.check(_lib.lib.detops_eval_oks(  # noqa: E731
        dk_d.data_ptr(), gk_d.data_ptr(), gb_d.data_ptr(), ga_d.data_ptr(), sig_d.data_ptr(), K, dto_d.data_ptr(), gto_d.data_ptr(),
        ioo_d.data_ptr(), I, I * D, total, oks.data_ptr(), area.data_ptr(), _lib.stream_of(oks)), "eval_oks")
    out = [_entry("detops_eval_oks entry point, 8 x (20 x 8) pairs, K=17", dev_time_us(raw, iters), alg)]
    wrapped = lambda: C.eval_oks(dk_d, gk_d, gb_d, ga_d, sig, dto_d, gto_d, ioo_d, total)  # noqa: E731
    out.append(_entry("_C.eval_oks through the wrapper, same batch", dev_time_us(wrapped, iters), alg))
    ref, ref_area = _eval_cpu.eval_oks(dk, gk, gb, ga, sig, dto, gto, ioo)
    got, got_area = wrapped()
    out[-1].update({"max_abs_diff_vs_numpy": float(np.abs(got.cpu().numpy() - ref).max()),
                    "areas_equal": bool(np.array_equal(got_area.cpu().numpy(), ref_area))})
    var = (2.0 * sig_d) * (2.0 * sig_d)

    def torch_oks():
        d, g = dk_d.view(I, D, 1, K, 3).double(), gk_d.view(I, 1, G, K, 3).double()
        vis = g[..., 2] > 0
        has = vis.any(dim=-1, keepdim=True)
        wh = ((gb_d[:, 2:] - gb_d[:, :2]) + 1).double().view(I, 1, G, 1, 2)
        xy = gb_d[:, :2].double().view(I, 1, G, 1, 2)
        p = d[..., :2]
        far = torch.clamp((xy - wh) - p, min=0) + torch.clamp(p - (xy + 2.0 * wh), min=0)
        delta = torch.where(has.unsqueeze(-1), p - g[..., :2], far)
        e = (delta[..., 0] * delta[..., 0] + delta[..., 1] * delta[..., 1]) / var / (ga_d.view(I, 1, G, 1) + 2.0 ** -52) / 2
        counts = vis | ~has
        s = torch.where(counts, torch.exp(-e), torch.zeros_like(e)).sum(dim=-1)
        xs, ys = dk_d[:, :, 0], dk_d[:, :, 1]
        a = (xs.max(dim=1)[0].double() - xs.min(dim=1)[0].double()) * (ys.max(dim=1)[0].double() - ys.min(dim=1)[0].double())
        return (s / counts.sum(dim=-1)).reshape(-1), a

    us = dev_time_us(torch_oks, iters)
    t_oks, t_area = torch_oks()
    out.append(_entry("torch: broadcast formulation on the same device tensors", us, alg,
                      {"max_abs_diff_vs_numpy": float(np.abs(t_oks.cpu().numpy() - ref).max()),
                       "areas_equal": bool(np.array_equal(t_area.cpu().numpy(), ref_area))}))
    return out


def bench_proposal_recall(C, iters):
    """proposal recall (csrc/eval_proposals.hip): 2 images, 1000 proposals and 20 ground truths each, the 2 limits x 4 area
    ranges of the `box_proposal` table (16 workgroups, 20 rounds each at most).  Rows: the entry point alone on prebuilt
    device arrays; _C.eval_proposal_overlaps through the wrapper (its dtype / contiguity checks, the copy of the limits and
    one allocation included); the reference's loop (evaluate_box_proposals) as torch operations on the same device tensors,
    once per (image, limit, area range).  bytes = the boxes, offsets and flags read once + the overlaps written."""
    from maskrcnn_benchmark import _eval_cpu, _lib
    N, P, G, limits = 2, 1000, 20, (100, 1000)
    ranges = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))
    rng = np.random.RandomState(5)
    x1, y1 = rng.uniform(0, 1100, N * G), rng.uniform(0, 600, N * G)
    side = np.exp(rng.uniform(np.log(12), np.log(400), N * G))
    gt = np.stack([x1, y1, x1 + side, y1 + side * rng.uniform(0.5, 2, N * G)], 1).astype(np.float32)
    x1, y1 = rng.uniform(0, 1200, N * P), rng.uniform(0, 700, N * P)
    dt = np.stack([x1, y1, x1 + rng.uniform(8, 400, N * P), y1 + rng.uniform(8, 400, N * P)], 1).astype(np.float32)
    near = np.repeat(gt.reshape(N, G, 4), 10, axis=1).reshape(N, G * 10, 4) + rng.uniform(-12, 12, (N, G * 10, 4))
    dt.reshape(N, P, 4)[:, :G * 10] = near                      # ten jittered copies of every ground truth among the proposals
    dt = dt.reshape(N, P, 4)[:, rng.permutation(P)].reshape(-1, 4).copy()
    dt[:, 2:] = np.maximum(dt[:, 2:], dt[:, :2] + 1)
    area = ((gt[:, 2] - gt[:, 0]) + 1) * ((gt[:, 3] - gt[:, 1]) + 1)
    valid = np.stack([(area >= lo) & (area <= hi) for lo, hi in ranges]).astype(np.uint8)
    dto, gto = (np.arange(N + 1) * P).astype(np.int32), (np.arange(N + 1) * G).astype(np.int32)
    lim = np.array(limits, np.int32)
    dt_d, gt_d, dto_d, gto_d, valid_d, lim_d = (_t(a) for a in (dt, gt, dto, gto, valid, lim))
    L, A = len(limits), len(ranges)
    alg = (dt.size + gt.size) * 4 + (dto.size + gto.size + lim.size) * 4 + valid.size + L * A * N * G * 4
    out = torch.empty((L, A, N * G), dtype=torch.float32, device="cuda")
    raw = lambda: _lib.check(_lib.lib.detops_eval_proposal_overlaps(  # noqa: E731
        dt_d.data_ptr(), gt_d.data_ptr(), dto_d.data_ptr(), gto_d.data_ptr(), valid_d.data_ptr(), lim_d.data_ptr(), N, L, A, N * P,
        N * G, P, G, out.data_ptr(), _lib.stream_of(out)), "eval_proposal_overlaps")
    name = "2 x (1000 x 20), 2 limits x 4 ranges"
    res = [_entry("detops_eval_proposal_overlaps entry point, " + name, dev_time_us(raw, iters), alg)]
    wrapped = lambda: C.eval_proposal_overlaps(dt_d, gt_d, dto_d, gto_d, valid_d, limits, max_dt=P, max_gt=G)  # noqa: E731
    res.append(_entry("_C.eval_proposal_overlaps through the wrapper, same batch", dev_time_us(wrapped, iters), alg))
    ref = _eval_cpu.eval_proposal_overlaps(dt, gt, dto, gto, valid, lim)
    res[-1].update({"equal_to_numpy": bool(np.array_equal(wrapped().cpu().numpy(), ref)),
                    "matched": int((ref > 0).sum()), "slots": int((ref >= 0).sum())})

    def torch_loop():
        result = torch.full((L, A, N * G), -1.0, device="cuda")
        for n in range(N):
            boxes, gts = dt_d[n * P:(n + 1) * P], gt_d[n * G:(n + 1) * G]
            for li, limit in enumerate(limits):
                for a in range(A):
                    keep = valid_d[a, n * G:(n + 1) * G] != 0
                    g = gts[keep]
                    if len(g) == 0:
                        continue
                    p = boxes[:limit]
                    area_p = (p[:, 2] - p[:, 0] + 1) * (p[:, 3] - p[:, 1] + 1)
                    area_g = (g[:, 2] - g[:, 0] + 1) * (g[:, 3] - g[:, 1] + 1)
                    wh = (torch.min(p[:, None, 2:], g[:, 2:]) - torch.max(p[:, None, :2], g[:, :2]) + 1).clamp(min=0)
                    inter = wh[:, :, 0] * wh[:, :, 1]
                    overlaps = inter / (area_p[:, None] + area_g - inter)
                    found = torch.zeros(len(g), device="cuda")
                    slot = torch.nonzero(keep).reshape(-1)
                    for j in range(min(len(p), len(g))):
                        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
                        gt_ovr, gt_ind = max_overlaps.max(dim=0)
                        box_ind = argmax_overlaps[gt_ind]
                        found[gt_ind] = overlaps[box_ind, gt_ind]
                        overlaps[box_ind, :] = -1
                        overlaps[:, gt_ind] = -1
                    result[li, a, n * G + slot] = found
        return result

    us = dev_time_us(torch_loop, max(iters // 10, 3), warmup=2)
    res.append(_entry("torch: the reference's loop on the same device tensors", us, alg,
                      {"equal_to_numpy": bool(np.array_equal(torch_loop().cpu().numpy(), ref))}))
    return res


def bench_cityscapes(C, iters):
    """Cityscapes window counts (csrc/cityscapes_eval.hip): one image of 1024 x 2048, D = 100 pasted predictions and G = 30
    ground truths whose planes fill ellipses in their boxes; boxes drawn like a street scene (many small, a few large), about
    300 overlapping pairs.  Rows: the entry point alone on prebuilt device arrays; _C.window_counts through the wrapper (its
    checks and four allocations included); the reference's own loop (eval_instances.py: matchGtWithPred) on the same device
    tensors: crop, mul, sum and .item() per pair and per instance, which is the yardstick.  Every row is the MEDIAN of
    `iters` samples (50 by default) after warm-up, each sample one call between two HIP events.  bytes = the window bytes the
    entry point reads: every instance's own window once, and both planes of every overlapping pair's union window."""
    from maskrcnn_benchmark import _eval_cpu, _lib
    H, W, D, G = 1024, 2048, 100, 30
    rng = np.random.RandomState(11)

    def boxes(n, jitter_of=None):
        side = np.exp(rng.uniform(np.log(16), np.log(90), n))
        side[rng.rand(n) < 0.12] *= 5                                        # a few large ones
        w, h = side * rng.uniform(0.5, 1.6, n), side * rng.uniform(0.8, 2.2, n)
        cx, cy = rng.uniform(0, W, n), rng.uniform(0.35 * H, 0.8 * H, n)       # a band around the horizon
        if jitter_of is not None:                                              # most predictions sit on a ground truth
            k = rng.randint(0, len(jitter_of), n)
            on = rng.rand(n) < 0.9
            g = jitter_of[k]
            cx, cy = np.where(on, (g[:, 0] + g[:, 2]) / 2 + rng.uniform(-8, 8, n), cx), np.where(on, (g[:, 1] + g[:, 3]) / 2 + rng.uniform(-8, 8, n), cy)
            w, h = np.where(on, (g[:, 2] - g[:, 0]) * rng.uniform(0.8, 1.25, n), w), np.where(on, (g[:, 3] - g[:, 1]) * rng.uniform(0.8, 1.25, n), h)
        b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
        return np.clip(b, 0, [W, H, W, H]).astype(np.int32)

    def ellipses(b):
        ys, xs = torch.arange(H, device="cuda").view(1, H, 1), torch.arange(W, device="cuda").view(1, 1, W)
        bt = _t(b).to(torch.float32)
        cx, cy = ((bt[:, 0] + bt[:, 2]) / 2).view(-1, 1, 1), ((bt[:, 1] + bt[:, 3]) / 2).view(-1, 1, 1)
        rx, ry = ((bt[:, 2] - bt[:, 0]) / 2).clamp(min=1).view(-1, 1, 1), ((bt[:, 3] - bt[:, 1]) / 2).clamp(min=1).view(-1, 1, 1)
        return ((((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2) <= 1).to(torch.uint8).contiguous()

    gt_box = boxes(G)
    dt_box = boxes(D, gt_box)
    dt_planes, gt_planes, dt_box_d, gt_box_d = ellipses(dt_box), ellipses(gt_box), _t(dt_box), _t(gt_box)

    def area(b):
        return np.maximum(b[..., 2] - b[..., 0], 0) * np.maximum(b[..., 3] - b[..., 1], 0)

    over = ((dt_box[:, None, :2] < gt_box[None, :, 2:]) & (gt_box[None, :, :2] < dt_box[:, None, 2:])).all(axis=2)
    union = np.concatenate([np.minimum(dt_box[:, None, :2], gt_box[None, :, :2]), np.maximum(dt_box[:, None, 2:], gt_box[None, :, 2:])], axis=2)
    alg = int(area(dt_box).sum() + area(gt_box).sum() + 2 * (area(union) * over).sum())

    def median_us(fn, warmup=5):
        for _ in range(warmup):
            fn()
        samples = []
        for _ in range(iters):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            torch.cuda.synchronize()
            samples.append(start.elapsed_time(end) * 1000.0)
        return float(np.median(samples))

    i32 = dict(dtype=torch.int32, device="cuda")
    outs = (torch.empty((D,), **i32), torch.empty((G,), **i32), torch.empty((D, G), **i32), torch.empty((D, G), **i32))
    raw = lambda: _lib.check(_lib.lib.detops_window_counts(  # noqa: E731
        dt_planes.data_ptr(), dt_box_d.data_ptr(), D, gt_planes.data_ptr(), gt_box_d.data_ptr(), G, H, W,
        *(o.data_ptr() for o in outs), _lib.stream_of(outs[0])), "window_counts")
    name = "1024 x 2048, D=100, G=30, %d overlapping pairs" % int(over.sum())
    res = [_entry("detops_window_counts entry point, " + name, median_us(raw), alg)]
    # where the time goes: the same grid with empty windows (xmax = xmin: every workgroup leaves after reading its boxes,
    # no plane is read), and one instance (the floor of the entry point's two launches)
    flat_d, flat_g = dt_box_d.clone(), gt_box_d.clone()
    flat_d[:, 2], flat_g[:, 2] = flat_d[:, 0], flat_g[:, 0]
    empty = lambda: _lib.check(_lib.lib.detops_window_counts(  # noqa: E731
        dt_planes.data_ptr(), flat_d.data_ptr(), D, gt_planes.data_ptr(), flat_g.data_ptr(), G, H, W,
        *(o.data_ptr() for o in outs), _lib.stream_of(outs[0])), "window_counts")
    res.append(_entry("  the same grid, every window empty (no plane read)", median_us(empty), 0))
    one = lambda: _lib.check(_lib.lib.detops_window_counts(  # noqa: E731
        dt_planes.data_ptr(), dt_box_d.data_ptr(), 1, gt_planes.data_ptr(), gt_box_d.data_ptr(), 0, H, W,
        *(o.data_ptr() for o in outs), _lib.stream_of(outs[0])), "window_counts")
    res.append(_entry("  one instance, no pair (two launches)", median_us(one), int(area(dt_box[:1]).sum())))
    wrapped = lambda: C.window_counts(dt_planes, dt_box_d, gt_planes, gt_box_d)  # noqa: E731
    res.append(_entry("_C.window_counts through the wrapper, same image", median_us(wrapped), alg))
    ref = _eval_cpu.window_counts(dt_planes.cpu().numpy(), dt_box, gt_planes.cpu().numpy(), gt_box)
    res[-1].update({"equal_to_numpy": bool(all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(wrapped(), ref))),
                    "overlapping_pairs": int(over.sum())})
    dt_l, gt_l = dt_box.tolist(), gt_box.tolist()

    def reference_loop():
        dt_count = [dt_planes[d][b[1]:b[3], b[0]:b[2]].sum().item() for d, b in enumerate(dt_l)]
        gt_count = [gt_planes[g][b[1]:b[3], b[0]:b[2]].sum().item() for g, b in enumerate(gt_l)]
        pair_mask = np.zeros((D, G), np.int64)
        for g, a in enumerate(gt_l):
            for d, b in enumerate(dt_l):
                if not (a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]):
                    continue
                x0, y0, x1, y1 = min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])
                pair_mask[d, g] = torch.sum(torch.mul(gt_planes[g][y0:y1, x0:x1], dt_planes[d][y0:y1, x0:x1])).item()
        return dt_count, gt_count, pair_mask

    us = median_us(reference_loop, warmup=2)
    dc, gc, pm = reference_loop()
    res.append(_entry("torch: the reference's loop (crop, mul, sum, .item()) on the same device tensors", us, alg,
                      {"equal_to_numpy": bool(np.array_equal(dc, ref[0]) and np.array_equal(gc, ref[1]) and np.array_equal(pm, ref[3])),
                       "ratio_to_entry_point": round(us / res[0]["us"], 1)}))
    return res


def copy_ceiling(iters):
    a = torch.empty(256 * 1024 * 1024 // 4, device="cuda")
    b = torch.empty_like(a)
    us = dev_time_us(lambda: b.copy_(a), iters)
    return _entry("hbm copy 256MiB (torch copy_, ceiling reference)", us, 2 * a.numel() * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default="")
    ap.add_argument("--sets", default="", help="roi_sets: comma list of ROI-set names (default all)")
    ap.add_argument("--heads", default="", help="roi_sets: box,mask (default both)")
    ap.add_argument("--dir", default="", help="roi_sets: fwd,bwd (default both)")
    ap.add_argument("--model-rois", default=None, help="npz of tools/dump_model_rois.py (default: tests/golden/model_rois.npz)")
    ap.add_argument("--layout", default="nchw", help="roi_sets: nchw | nhwc | both")
    ap.add_argument("--images", type=int, default=2, help="roi_sets: images per batch (4 = the > L3 variant: 365.6 MB of maps)")
    ap.add_argument("--tune", default="", help="library tuning switches for the whole run, key=value,key=value")
    ap.add_argument("--sweep", default="", help="roi_sets: cartesian sweep over tuning switches, 'key=v1|v2,key2=v1|v2'")
    ap.add_argument("--experimental", action="store_true",
                    help="also time the opt-in, not-yet-measured kernel variants (DESIGN.md section 7)")
    args = ap.parse_args()
    from maskrcnn_benchmark import _C as C

    only = set(filter(None, args.only.split(",")))
    res = []
    t0 = time.time()
    for kv in filter(None, args.tune.split(",")):
        k, v = kv.split("=")
        tune(k, int(v))
    if not only or "copy" in only:
        res.append(copy_ceiling(args.iters))
    if not only or "roi_align" in only:
        res += bench_roi_align(C, args.iters, experimental=args.experimental)
    if "roi_align_fpn" in only:
        res += bench_roi_align(C, args.iters, fused_only=True)
    if not only or "roi_sets" in only:
        import itertools
        axes = [(kv.split("=")[0], [int(v) for v in kv.split("=")[1].split("|")]) for kv in filter(None, args.sweep.split(","))]
        for combo in itertools.product(*[vals for _, vals in axes]):
            for (k, _), v in zip(axes, combo):
                tune(k, v)
            for lay in (("nchw", "nhwc") if args.layout == "both" else (args.layout,)):
                res += bench_roi_sets(C, args.iters, args.model_rois, set(filter(None, args.sets.split(","))),
                                      set(filter(None, args.heads.split(","))), tuple(filter(None, args.dir.split(","))) or ("fwd", "bwd"),
                                      images=args.images, tag=" ".join("%s=%d" % (k, v) for (k, _), v in zip(axes, combo)), layout=lay)
        for k, _ in axes:
            tune(k, 0)
    if "roi_align_fwd" in only:
        res += bench_roi_align(C, args.iters, which=("fwd",))
    if not only or "pool" in only:
        res += bench_roi_pool_psroi(C, args.iters)
    if not only or "nms" in only:
        res += bench_nms(C, args.iters)
    if not only or "targets" in only:
        res += bench_targets(C, args.iters)
    if not only or "keypoint" in only:
        res += bench_keypoint(C, args.iters)
    if not only or "masker" in only:
        res += bench_masker(C, args.iters)
    if not only or "polygons" in only:
        res += bench_polygons(C, args.iters)
    if not only or "evaluation" in only:
        res += bench_evaluation(C, args.iters)
    if not only or "keypoint_oks" in only:
        res += bench_keypoint_oks(C, args.iters)
    if not only or "proposal_recall" in only:
        res += bench_proposal_recall(C, args.iters)
    if not only or "cityscapes" in only:
        res += bench_cityscapes(C, args.iters)
    if not only or "coco_results" in only:
        copy_rows = [r for r in res if r["op"].startswith("hbm copy")]
        res += bench_coco_results(C, args.iters, copy_rows[0]["gbs"] if copy_rows else None)
    if not only or "rle_decode" in only:
        res += bench_rle_decode(C, args.iters)
    if not only or "input_prep" in only:
        copy_rows = [r for r in res if r["op"].startswith("hbm copy")]
        res += bench_input_prep(C, args.iters, copy_rows[0]["gbs"] if copy_rows else None)
    if not only or "color_jitter" in only:
        copy_rows = [r for r in res if r["op"].startswith("hbm copy")]
        res += bench_color_jitter(C, args.iters, copy_rows[0]["gbs"] if copy_rows else None)
    if not only or "bbox_aug" in only:
        copy_rows = [r for r in res if r["op"].startswith("hbm copy")]
        res += bench_bbox_aug(C, args.iters, copy_rows[0]["gbs"] if copy_rows else None)
    if not only or "frozen_bn" in only:
        res += bench_frozen_bn(C, args.iters)
    if not only or "group_norm" in only:
        copy_rows = [r for r in res if r["op"].startswith("hbm copy")]
        res += bench_group_norm(C, args.iters, copy_rows[0]["gbs"] if copy_rows else None)
    if not only or "focal" in only:
        res += bench_focal(C, args.iters)
    if not only or "dcn" in only:
        res += bench_dcn(C, args.iters, experimental=args.experimental)
    if not only or "dcn_fused" in only:
        res += bench_dcn_fused(C, args.iters)
    if not only or "dcn_block" in only:
        res += bench_dcn_block(C, args.iters)
    for r in res:
        print("%-70s %10.2f us  %9.1f GB/s  (%.1f%% of 8 TB/s) %s" % (
            r["op"], r["us"], r["gbs"], 100 * r["frac_of_8TBs"],
            {k: v for k, v in r.items() if k not in ("op", "us", "gbs", "frac_of_8TBs", "alg_bytes")} or ""))
    print("total %.1f s" % (time.time() - t0))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
