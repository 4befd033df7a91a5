"""Edge-shape cases of csrc/targets.hip and csrc/head_loss.hip with their references — shared by
tests/test_targets_edges_emu.py (host emulation: proves the references) and tests/test_targets_edges_gpu.py (the device).

A plain module: no tests, no fixtures.  Every builder returns numpy inputs plus the expected outputs; references are exact
integer logic (matcher, sampler, labels), the CPU composite the kernels mirror bit for bit (mask targets), or fp64 with
autograd (losses, encode).  Nothing here calls the code under test.  Builders are cached: a case and its reference are
computed once per process and must be treated as read-only.

The shapes are the smallest that reach a named branch of the kernels: kGtChunk = 256 ground-truth rows per LDS pass,
1024 boxes per matcher workgroup, the sampler's `cand <= 2 mu` switch and 2 x 256 x 256 grid-stride span, 256-thread
blocks, 64-lane waves (C below / at / above 64), kMaskSplit = 8 class planes per workgroup row."""
import functools

import numpy as np
import torch

from maskrcnn_benchmark.modeling.matcher import Matcher
from maskrcnn_benchmark.structures.boxlist_ops import box_iou_matrix

MASK64 = (1 << 64) - 1
GOLDEN64 = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------------ error measures
def rel_err(value, ref):
    """relative error of a scalar against its fp64 reference (absolute when the reference is exactly 0)"""
    value, ref = float(value), float(ref)
    return abs(value - ref) / abs(ref) if ref != 0.0 else abs(value)


def grad_err(g, ref):
    """max|g - ref| / max|ref| over any number of arrays taken together (elementwise relative error means nothing next to
    zeros); absolute when the reference is all zero"""
    gs = g if isinstance(g, (list, tuple)) else [g]
    rs = ref if isinstance(ref, (list, tuple)) else [ref]
    num = max(float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) for a, b in zip(gs, rs))
    den = max(float(np.abs(np.asarray(b, np.float64)).max()) for b in rs)
    return num / den if den > 0 else num


# ------------------------------------------------------------------------------------------ matcher
def _rand_boxes(rng, n, W=640, H=480, smin=8, smax=200):
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    w, h = rng.uniform(smin, smax, n), rng.uniform(smin, smax, n)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)


MATCHER_THRESHOLDS = ((0.7, 0.3, True), (0.5, 0.5, False))
MATCHER_SHAPES = ("1x1", "256x1023", "257x1025", "513x2049", "3x4097", "invalid_image")
FAR_GT = (5000.0, 5000.0, 5010.0, 5010.0)
PAD_GT = (-1e5, -1e5, -1e5 + 1, -1e5 + 1)


def matcher_reference(gt, valid, boxes, hi, lo, lq):
    """torch Matcher on box_iou_matrix on the CPU, invalid rows at quality -1"""
    tg, tv, tb = torch.from_numpy(gt), torch.from_numpy(valid), torch.from_numpy(boxes)
    if tb.dim() == 2:
        tb = tb.unsqueeze(0).expand(tg.shape[0], -1, -1)
    iou = box_iou_matrix(tg, tb)
    iou = torch.where(tv[:, :, None], iou, iou.new_full((), -1.0))
    return Matcher(hi, lo, allow_low_quality_matches=lq)(iou, tv)


@functools.lru_cache(maxsize=None)
def matcher_inputs(shape, batched):
    """-> dict(gt [2,M,4], valid [2,M] bool, boxes [K,4] | [2,K,4], random: the reference must hold >= 0, -1 (and -2))"""
    N = 2
    rng = np.random.RandomState(17 + 2 * MATCHER_SHAPES.index(shape) + batched)
    if shape == "1x1":
        gt = np.array([[[10, 10, 50, 60]], [[100, 100, 130, 120]]], np.float32)
        valid = np.ones((N, 1), bool)
        boxes = np.array([[[12, 11, 50, 58]], [[400, 400, 420, 420]]], np.float32) if batched else np.array([[12, 11, 50, 58]], np.float32)
        return dict(gt=gt, valid=valid, boxes=boxes, random=False)
    if shape == "invalid_image":
        M, K = 5, 300
        gt = np.stack([_rand_boxes(rng, M) for _ in range(N)])
        valid = np.ones((N, M), bool)
        valid[1] = False                     # an image without a single real row: everything is below the low threshold
        gt[~valid] = PAD_GT
        boxes = np.stack([_rand_boxes(rng, K) for _ in range(N)]) if batched else _rand_boxes(rng, K)
        return dict(gt=gt, valid=valid, boxes=boxes, random=False)
    if shape == "3x4097":
        # three ground truths far apart; every other box misses them.  Each gt's best box (IoU ~0.54: a match by the
        # low-quality rule ONLY) sits in a different 1024-box workgroup than its lesser overlaps (~0.43, ~0.33), which come
        # both before and after it: the per-gt maximum exists only once the workgroups' atomicMax have met in memory
        M, K = 3, 4097
        g1 = np.array([[100 + 200 * g, 100, 199 + 200 * g, 199] for g in range(M)], np.float32)
        gt = np.stack([g1, g1 + np.float32([0, 30, 0, 30])])

        def fill(image):
            b = _rand_boxes(rng, K, 640, 160, 8, 60)
            b[:, 1] += 300
            b[:, 3] += 300                   # y >= 270: below every ground truth
            for g, (best, mid, low) in enumerate(((1, 3, 4), (2, 0, 3), (3, 0, 1))):     # workgroups of 1024 boxes
                base = gt[image, g]
                b[best * 1024 + 7 + g] = base + np.float32([30, 0, 30, 0])
                b[mid * 1024 + 500 + g] = base + np.float32([40, 0, 40, 0])
                b[min(low * 1024 + 1000 + g, K - 1)] = base + np.float32([0, 50, 0, 50])       # workgroup 4 is box 4096 alone
            b[2 * 1024 + 77] = gt[image, 0] - np.float32([30, 0, 30, 0])     # ties gt 0's best from another workgroup
            b[3 * 1024 + 5] = gt[image, 2] + np.float32([10, 0, 10, 0])      # an ordinary match above the high threshold
            return b
        boxes = np.stack([fill(0), fill(1)]) if batched else fill(0)
        if not batched:
            gt[1] = gt[0]
        return dict(gt=gt, valid=np.ones((N, M), bool), boxes=boxes, random=False)
    M, K = (int(v) for v in shape.split("x"))
    gt = np.stack([_rand_boxes(rng, M) for _ in range(N)])
    valid = np.ones((N, M), bool)
    if shape == "513x2049":
        valid[0, M // 2:] = False            # image 0 valid only in its first half
    gt[~valid] = PAD_GT
    if M > 256:
        gt[1, 256] = gt[1, 0]                # a duplicate across the LDS chunk boundary: the first index must win
    gt[1, M - 1] = FAR_GT                    # valid, overlaps nothing: the low-quality rule then marks every IoU-0 box of image 1

    def fill(image):
        b = _rand_boxes(rng, K)
        n = K // 3                           # a third of the boxes are jittered ground truths: matches above either threshold
        src = rng.randint(0, M // 2, n)
        b[:n] = gt[image, src] + rng.uniform(-3, 3, (n, 4)).astype(np.float32)
        b[n] = gt[image, 3]                  # identical to a ground truth (IoU exactly 1)
        b[n + 1] = gt[1, 0]                  # identical to the duplicated pair of image 1
        return b
    boxes = np.stack([fill(0), fill(1)]) if batched else fill(0)
    return dict(gt=gt, valid=valid, boxes=boxes, random=True)


@functools.lru_cache(maxsize=None)
def matcher_case(shape, batched, thresholds):
    """inputs + `ref` (torch int64 [2,K])"""
    c = dict(matcher_inputs(shape, batched))
    hi, lo, lq = thresholds
    c.update(hi=hi, lo=lo, lq=lq, ref=matcher_reference(c["gt"], c["valid"], c["boxes"], hi, lo, lq))
    return c


# ------------------------------------------------------------------------------------------ sampler
def sample_keys(seed, row, n):
    """the two-round multiply-xorshift mixer of `sample_key` (csrc/targets.hip) for elements 0..n-1 of a row -> uint32 [n]"""
    m32 = np.uint64(0xFFFFFFFF)
    i = np.arange(n, dtype=np.uint64)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    h = np.full(n, (int(lo) ^ ((row * 0x9E3779B1) & 0xFFFFFFFF)), np.uint64)
    h ^= (i * np.uint64(0x85EBCA6B) + hi) & m32

    def fmix(h):
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(0x85EBCA6B)) & m32
        h ^= h >> np.uint64(13)
        h = (h * np.uint64(0xC2B2AE35)) & m32
        h ^= h >> np.uint64(16)
        return h
    h = fmix(h)
    h = (h + i) & m32
    return fmix(h).astype(np.uint32)


def sampler_reference(labels, B, max_pos, seed, word=None):
    """numpy restatement of the sampler: per row the min(#pos, max_pos) smallest (key, index) positives, then the
    min(#neg, B, B - k_pos) smallest negatives; list = positives first in ascending (key, index) order, unfilled slots
    index 0 / valid 0.  `word`: the device word mixed into the seed at run time."""
    if word is not None:
        seed = seed ^ ((word * GOLDEN64) & MASK64)
    seed &= MASK64
    N, n = labels.shape
    pos, neg = np.zeros((N, n), bool), np.zeros((N, n), bool)
    idx, val = np.zeros((N, B), np.int64), np.zeros((N, B), bool)
    for r in range(N):
        keys = sample_keys(seed, r, n).astype(np.uint64)
        order = np.argsort((keys << np.uint64(32)) | np.arange(n, dtype=np.uint64), kind="stable")
        is_pos, is_neg = labels[r] >= 1, labels[r] == 0
        k_pos = min(int(is_pos.sum()), max_pos)
        k_neg = min(int(is_neg.sum()), B, B - k_pos)
        p = order[is_pos[order]][:k_pos]
        q = order[is_neg[order]][:k_neg]
        pos[r, p], neg[r, q] = True, True
        idx[r, :k_pos], idx[r, k_pos:k_pos + k_neg] = p, q
        val[r, :k_pos + k_neg] = True
    return pos, neg, idx, val


def _labels(rng, N, n, dtype, n_pos, n_ign=None):
    """rows of zeros with n_pos[r] positives (class values 1..80) and n_ign[r] ignored (-1) at random places"""
    lab = np.zeros((N, n), dtype)
    for r in range(N):
        perm = rng.permutation(n)
        lab[r, perm[:n_pos[r]]] = rng.randint(1, 81, n_pos[r])
        k = n // 5 if n_ign is None else n_ign[r]
        lab[r, perm[n_pos[r]:n_pos[r] + k]] = -1
    return lab


SAMPLER_CASES = ("rpn_3_and_900", "no_neg_and_no_pos", "n255", "n5", "high_seed_bit", "switch_2mu", "second_stride_trip")


@functools.lru_cache(maxsize=None)
def sampler_case(name, word=None):
    """-> dict(labels, B, max_pos, seed, word, ref=(pos, neg, idx, valid))"""
    rng = np.random.RandomState(100 + SAMPLER_CASES.index(name))
    if name == "rpn_3_and_900":
        labels, B, max_pos, seed = _labels(rng, 2, 30000, np.float32, (3, 900)), 256, 128, 1234
    elif name == "no_neg_and_no_pos":
        labels = _labels(rng, 3, 777, np.int64, (40, 10, 0), (100, 767, 300))     # row 1: positives and ignored only
        B, max_pos, seed = 64, 16, (5 << 40) + 9
    elif name == "n255":
        labels, B, max_pos, seed = _labels(rng, 1, 255, np.int64, (9,)), 8, 2, 1
    elif name == "n5":
        labels, B, max_pos, seed = np.array([[1, 0, 2, -1, 0]], np.int64), 4, 4, 3
    elif name == "high_seed_bit":
        labels, B, max_pos, seed = _labels(rng, 2, 70000, np.float32, (2000, 50)), 512, 128, 2 ** 63 + 5
    elif name == "switch_2mu":
        # quota 128: mu = 128 + 8 sqrt(128) + 32 = 250.5 -> every candidate survives up to 501 of them, a key threshold
        # filters from 502 on; the negatives (3000+) are always filtered
        labels, B, max_pos, seed = _labels(rng, 4, 4000, np.int64, (500, 501, 502, 503), (400,) * 4), 256, 128, 42
    else:
        n = 2 * 256 * 256 + 300              # past gridDim.x * 256 elements: the grid-stride loops take a second trip
        labels, B, max_pos, seed = _labels(rng, 1, n, np.float32, (700,)), 256, 128, 7
    return dict(labels=labels, B=B, max_pos=max_pos, seed=seed, word=word, ref=sampler_reference(labels, B, max_pos, seed, word))


# ------------------------------------------------------------------------------------------ mask targets
MASK_IMAGES = ((1, 1), (5, 7), (33, 20))     # (H, W)
MASK_SIZES = (1, 14, 16, 17, 28)             # M * M below, equal to and above the 256-thread block
MASK_DTYPES = (torch.uint8, torch.float32, torch.bool, torch.int64, torch.int16)


@functools.lru_cache(maxsize=None)
def mask_case(H, W):
    """-> dict(masks {dtype: torch [3,H,W]}, index [P] int64, boxes [P,4]); the reference is mask_reference"""
    rng = np.random.RandomState(H * 100 + W)
    G = 3
    binary = rng.rand(G, H, W) < 0.5
    binary[0, H - 1, W - 1] = True
    binary[G - 1, H - 1, W - 1] = False
    masks = {dt: torch.from_numpy(binary).to(dt) for dt in MASK_DTYPES}
    masks[torch.float32] = torch.from_numpy(np.where(binary, rng.uniform(0.1, 1.0, binary.shape), 0.0).astype(np.float32))
    boxes = np.array([
        [-20, -30, -5, -3],                  # wholly left / above the image
        [W + 5, H + 3, W + 30, H + 40],      # wholly right / below
        [0.5, 0.5, 2.5, 3.5],                # half-to-even rounding: (0, 0, 2, 4)
        [1.5, 2.5, 1.5, 2.5],
        [3, 3, 1, 1],                        # inverted
        [-1e4, -1e4, 1e4, 1e4],
        [0, 0, W - 1, H - 1],
        [0, 0, W, H],
        [W - 1, H - 1, W - 1, H - 1],        # the last pixel alone
    ], np.float32)
    P = boxes.shape[0]
    return dict(masks=masks, index=np.repeat(np.array([0, G - 1], np.int64), P), boxes=np.concatenate([boxes, boxes]))


@functools.lru_cache(maxsize=None)
def mask_reference(H, W, M, dtype):
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.loss import project_masks_on_boxes
    c = mask_case(H, W)
    return project_masks_on_boxes(c["masks"][dtype], torch.from_numpy(c["index"]), torch.from_numpy(c["boxes"]), M)


# ------------------------------------------------------------------------------------------ encode (fp64)
def encode64(gt, boxes, weights, dtype=torch.float64):
    """BoxCoder.encode ("+1" widths) in fp64 (`dtype=torch.float32`: the same ATen composition in fp32); torch tensors [..., 4]"""
    gt, boxes = gt.to(dtype), boxes.to(dtype)
    ew, eh = boxes[..., 2] - boxes[..., 0] + 1, boxes[..., 3] - boxes[..., 1] + 1
    ex, ey = boxes[..., 0] + 0.5 * ew, boxes[..., 1] + 0.5 * eh
    gw, gh = gt[..., 2] - gt[..., 0] + 1, gt[..., 3] - gt[..., 1] + 1
    gx, gy = gt[..., 0] + 0.5 * gw, gt[..., 1] + 0.5 * gh
    wx, wy, ww, wh = weights
    return torch.stack([wx * (gx - ex) / ew, wy * (gy - ey) / eh, ww * torch.log(gw / ew), wh * torch.log(gh / eh)], -1)


def smooth_l1_64(d, beta):
    ad = d.abs()
    return torch.where(ad < beta, 0.5 * ad * ad / beta, ad - 0.5 * beta)


# ------------------------------------------------------------------------------------------ RPN loss
RPN_LOSS_CASES = ("single_anchor", "eight_levels", "nothing_sampled", "negatives_only")
RPN_UPSTREAM = (0.7, 1.3)
_EIGHT = ((1, 1), (1, 7), (7, 1), (2, 3), (5, 4), (3, 3), (6, 7), (4, 2))     # DETOPS_MAX_LEVELS uneven planes


def _flatten_levels(obj, box, A):
    """per-level [N,A,H,W] / [N,4A,H,W] -> [N,T] / [N,T,4] in the (level, y, x, anchor) order of the anchor list"""
    o = torch.cat([t.permute(0, 2, 3, 1).reshape(t.shape[0], -1) for t in obj], 1)
    b = torch.cat([t.view(t.shape[0], A, 4, t.shape[2], t.shape[3]).permute(0, 3, 4, 1, 2).reshape(t.shape[0], -1, 4)
                   for t in box], 1)
    return o, b


def _encode32(gt, an, weights):
    """the encode of the kernels in fp32 on the CPU (used only to PLANT residuals next to beta, never as a reference)"""
    f = np.float32
    ew, eh = an[2] - an[0] + f(1), an[3] - an[1] + f(1)
    ex, ey = an[0] + f(0.5) * ew, an[1] + f(0.5) * eh
    gw, gh = gt[2] - gt[0] + f(1), gt[3] - gt[1] + f(1)
    gx, gy = gt[0] + f(0.5) * gw, gt[1] + f(0.5) * gh
    return np.array([f(weights[0]) * (gx - ex) / ew, f(weights[1]) * (gy - ey) / eh, f(weights[2]) * np.log(gw / ew),
                     f(weights[3]) * np.log(gh / eh)], np.float32)


def rpn_loss_reference(obj, box, anchors, matched, pos, neg, gt, beta, weights, A, upstream=RPN_UPSTREAM, dtype=torch.float64):
    """fp64 autograd of the RPN losses over the sampled anchors, both / max(#sampled, 1); a sampled positive with a negative
    matched index regresses to ground-truth row 0 -> (objectness loss, box loss, d/d objectness per level, d/d regression per
    level).  `dtype=torch.float32`: the same ATen composition in fp32."""
    to = [torch.from_numpy(t).to(dtype).requires_grad_() for t in obj]
    tb = [torch.from_numpy(t).to(dtype).requires_grad_() for t in box]
    o, b = _flatten_levels(to, tb, A)
    tm, tp, tn = torch.from_numpy(matched), torch.from_numpy(pos), torch.from_numpy(neg)
    mg = torch.gather(torch.from_numpy(gt), 1, tm.clamp(min=0)[:, :, None].expand(-1, -1, 4))
    tg = encode64(mg, torch.from_numpy(anchors).unsqueeze(0), weights, dtype)
    ns = (tp | tn).sum().clamp(min=1).to(dtype)
    bl = smooth_l1_64(b - tg, beta).sum(-1)
    box_loss = torch.where(tp, bl, torch.zeros_like(bl)).sum() / ns
    bce = torch.nn.functional.binary_cross_entropy_with_logits(o, tp.to(dtype), reduction="none")
    obj_loss = torch.where(tp | tn, bce, torch.zeros_like(bce)).sum() / ns
    (upstream[0] * obj_loss + upstream[1] * box_loss).backward()
    return obj_loss.item(), box_loss.item(), [t.grad.numpy() for t in to], [t.grad.numpy() for t in tb]


@functools.lru_cache(maxsize=None)
def rpn_loss_case(name):
    """-> dict(obj, box (lists of numpy), anchors, matched, pos, neg, gt, beta, weights, ref=(obj loss, box loss, grads obj,
    grads box) in fp64 for the upstream gradients RPN_UPSTREAM)"""
    rng = np.random.RandomState(200 + RPN_LOSS_CASES.index(name))
    beta, weights = 1.0 / 9, (1.0, 1.0, 1.0, 1.0)
    if name == "single_anchor":
        N, A, M, shapes = 1, 1, 1, ((1, 1),)
    else:
        N, A, M, shapes = 2, 3, 4, _EIGHT
        weights = (2.0, 2.0, 0.5, 0.5) if name == "eight_levels" else weights
    T = A * sum(h * w for h, w in shapes)
    obj = [(rng.randn(N, A, h, w) * 3).astype(np.float32) for h, w in shapes]
    box = [(rng.randn(N, 4 * A, h, w) * 0.2).astype(np.float32) for h, w in shapes]
    x1, y1 = rng.uniform(0, 80, T), rng.uniform(0, 60, T)
    anchors = np.stack([x1, y1, x1 + rng.uniform(4, 60, T), y1 + rng.uniform(4, 60, T)], 1).astype(np.float32)
    gx, gy = rng.uniform(0, 70, (N, M)), rng.uniform(0, 50, (N, M))
    gt = np.stack([gx, gy, gx + rng.uniform(5, 50, (N, M)), gy + rng.uniform(5, 50, (N, M))], 2).astype(np.float32)
    # quarter-pixel coordinates below 128: widths, centres and their differences are exact in fp32, so the fp32 target is
    # one division (or one division and one log) away from the fp64 one.  The gradient d / beta of a residual under beta
    # amplifies that rounding by 1 / beta = 9; such a residual needs |target| < beta + |output| ~ 1, i.e. an error below
    # 9 x half an ulp of 1 ~ 5e-7 of a unit gradient.  With arbitrary coordinates the centre difference alone is off by
    # an ulp of 100 (8e-6) and the comparison would measure the inputs' conditioning, not the kernel
    anchors, gt = np.round(anchors * 4) / 4, np.round(gt * 4) / 4
    matched = rng.randint(-2, M, (N, T)).astype(np.int64)
    pos = (matched >= 0) & (rng.rand(N, T) < 0.4)
    neg = (matched == -1) & (rng.rand(N, T) < 0.5)
    if name == "single_anchor":
        matched[:], pos[:], neg[:] = 0, True, False
    elif name == "nothing_sampled":
        pos[:], neg[:] = False, False
    elif name == "negatives_only":
        pos[:] = False
        neg[0, :5] = True
    else:
        # a sampled positive whose matched index says "between thresholds": the kernel reads ground-truth row 0
        t = int(np.nonzero(matched[0] == -2)[0][0])
        pos[0, t], neg[0, t] = True, False
        # residuals at exactly 0, just under beta, exactly beta, just over beta (one sampled positive each, all four
        # coordinates): regression output = fp32 encode + offset
        fb = np.float32(beta)
        offs = (np.float32(0), np.nextafter(fb, np.float32(0)), fb, np.nextafter(fb, np.float32(1)))
        level0 = sum(A * h * w for h, w in shapes[:6])                     # first anchor of the 6 x 7 plane
        w6 = shapes[6][1]
        for j, off in enumerate(offs):
            loc, a = 3 + 5 * j, j % A
            t = level0 + loc * A + a
            matched[1, t], pos[1, t], neg[1, t] = j % M, True, False
            # an anchor next to its ground truth: |target| < 0.3
            anchors[t] = gt[1, j % M] + np.float32([0.5, -0.25, 1.0, 0.75])
            tg = _encode32(gt[1, j % M], anchors[t], weights)
            for k in range(4):
                box[6][1, 4 * a + k, loc // w6, loc % w6] = tg[k] + (off if k % 2 == 0 else -off)
        # saturated objectness logits on sampled anchors of either kind
        tp, tn = np.nonzero(pos[0])[0][:2], np.nonzero(neg[0])[0][:2]
        flat = [(l, y, x, a) for l, (h, w) in enumerate(shapes) for y in range(h) for x in range(w) for a in range(A)]
        for t, v in zip(list(tp) + list(tn), (90.0, -90.0, 90.0, -90.0)):
            l, y, x, a = flat[int(t)]
            obj[l][0, a, y, x] = v
    ref = rpn_loss_reference(obj, box, anchors, matched, pos, neg, gt, beta, weights, A)
    return dict(obj=obj, box=box, anchors=anchors, matched=matched, pos=pos, neg=neg, gt=gt, beta=beta, weights=weights, ref=ref)


# ------------------------------------------------------------------------------------------ RPN decode
#                 N, A, H, W, stride, top_n, min_size, (h, w) per image (None: random, anchors fit)
DECODE_CASES = {
    "single": (1, 1, 1, 1, 64, 1, 0, None),
    "all_candidates_min_size": (3, 3, 7, 9, 32, 1000, 24, None),             # k = A * H * W, many boxes under min_size
    "257_rows": (1, 3, 9, 10, 16, 257, 0, None),                             # N * k = 257: a second workgroup of one thread
    "image_smaller_than_anchors": (2, 3, 4, 5, 16, 60, 0, ((9, 7), (5, 11))),
}


@functools.lru_cache(maxsize=None)
def decode_case(name):
    """-> dict(anchors [AHW,4] torch, obj [N,A,H,W], reg [N,4A,H,W], sizes, post (RPNPostProcessor), col, off): the reference is
    post._level_candidates(anchors, obj, reg, sizes) run on the device under test"""
    from maskrcnn_benchmark.modeling.box_coder import BoxCoder
    from maskrcnn_benchmark.modeling.rpn.anchor_generator import AnchorGenerator
    from maskrcnn_benchmark.modeling.rpn.inference import RPNPostProcessor
    N, A, H, W, stride, topn, min_size, sizes = DECODE_CASES[name]
    rng = np.random.RandomState(300 + sorted(DECODE_CASES).index(name))
    if sizes is None:
        sizes = tuple((int(rng.randint(H * stride // 2, H * stride + 1)), int(rng.randint(W * stride // 2, W * stride + 1)))
                      for _ in range(N))
    gen = AnchorGenerator(sizes=(stride * 4,), aspect_ratios=tuple(np.linspace(0.5, 2.0, A).tolist()), anchor_strides=(stride,))
    anchors = gen.grid_anchors([(H, W)])[0]
    obj = torch.from_numpy(rng.randn(N, A, H, W).astype(np.float32))
    reg = torch.from_numpy((rng.randn(N, 4 * A, H, W) * 0.7).astype(np.float32))
    reg[0, 2::4] += 6.0                      # width deltas past bbox_xform_clip (log(1000 / 16) = 4.135) and past the image
    post = RPNPostProcessor(topn, topn, 0.7, min_size, BoxCoder((1.0, 1.0, 1.0, 1.0)))
    return dict(anchors=anchors, obj=obj, reg=reg, sizes=list(sizes), post=post, min_size=min_size, col=3, off=5)


# ------------------------------------------------------------------------------------------ labels and sampled slots
LABEL_SHAPES = ((1, 255), (2, 128), (1, 257))       # totals of 255, 256 and 257 elements


def match_labels_reference(matched, gt_labels, valid, dtype):
    N, K = matched.shape
    out = np.full((N, K), -1, np.int64)
    for n in range(N):
        m = matched[n]
        if gt_labels is None:
            out[n][m >= 0] = 1
        else:
            M = gt_labels.shape[1]
            ok = (m >= 0) & (m < M)
            out[n][ok] = gt_labels[n][m[ok]]              # a matched index >= M stays -1
        out[n][m == -1] = 0
    if valid is not None:
        out[~valid] = -1
    return out.astype(dtype)


@functools.lru_cache(maxsize=None)
def labels_case(N, K):
    rng = np.random.RandomState(400 + K)
    M = 6
    matched = rng.randint(-2, M + 2, (N, K)).astype(np.int64)      # M and M + 1: malformed
    return dict(matched=matched, gt_labels=rng.randint(1, 81, (N, M)).astype(np.int64), valid=rng.rand(N, K) < 0.8)


@functools.lru_cache(maxsize=None)
def slots_case(N, B, with_valid, with_obj):
    """-> inputs + ref = (boxes, labels, regression targets fp64, matched, objectness | None)"""
    rng = np.random.RandomState(500 + B + 2 * with_valid + with_obj)
    K, M = 300, 5
    weights = (10.0, 10.0, 5.0, 5.0)
    boxes = np.stack([_rand_boxes(rng, K, 200, 200, 8, 100) for _ in range(N)])
    gt = np.stack([_rand_boxes(rng, M, 200, 200, 16, 120) for _ in range(N)])
    gl = rng.randint(1, 81, (N, M)).astype(np.int64)
    matched = rng.randint(-2, M + 2, (N, K)).astype(np.int64)
    valid = (rng.rand(N, K) < 0.85) if with_valid else None
    obj = rng.rand(N, K).astype(np.float32) if with_obj else None
    idx = rng.randint(0, K, (N, B)).astype(np.int64)
    idx[0, :4] = (-3, K + 5, -1, K)          # outside [0, K): clamped, the slot is still labelled from the clamped row
    matched[0, 0], matched[0, K - 1] = 2, M + 1
    slot_valid = rng.rand(N, B) < 0.9
    slot_valid[0, :4] = True
    slot_valid[-1, B - 7:] = False           # unfilled tail
    sel = np.clip(idx, 0, K - 1)
    rows = np.arange(N)[:, None]
    m = matched[rows, sel]
    labels = match_labels_reference(matched, gl, valid, np.int64)[rows, sel]
    labels[~slot_valid] = -1
    mg = np.clip(m, 0, M - 1)
    reg = encode64(torch.from_numpy(gt[rows, mg]), torch.from_numpy(boxes[rows, sel]), weights).numpy()
    ref = (boxes[rows, sel], labels, reg, m, None if obj is None else obj[rows, sel])
    return dict(boxes=boxes, matched=matched, gt=gt, gt_labels=gl, valid=valid, idx=idx, slot_valid=slot_valid, objectness=obj,
                weights=weights, ref=ref)


# ------------------------------------------------------------------------------------------ box-head loss
#                 R, C, class-agnostic, beta, logit scale
FASTRCNN_CASES = ((1, 2, False, 1.0, 3.0), (3, 63, False, 1.0, 3.0), (5, 64, True, 0.5, 3.0), (9, 65, False, 1.0 / 9, 30.0),
                  (130, 129, False, 1.0, 30.0), (7, 81, True, 1.0, 60.0))
HEAD_UPSTREAM = (1.7, 0.6)


def fastrcnn_reference(logits, box, labels, targets, agnostic, beta, upstream, dtype=torch.float64):
    """fp64 autograd of cross-entropy + smooth-L1: rows 0 <= label < C count (and normalise), rows 0 < label < C regress;
    class-agnostic reads columns 4..7 -> (class loss, box loss, d/d logits, d/d box).  `dtype=torch.float32`: the same ATen
    composition in fp32, whose error against the fp64 result is what a bound on a new case is derived from."""
    R, C = logits.shape
    tl = torch.from_numpy(logits).to(dtype).requires_grad_()
    tb = torch.from_numpy(box).to(dtype).requires_grad_()
    L = torch.from_numpy(labels)
    row = (L >= 0) & (L < C)
    fg = (L > 0) & (L < C)
    n = row.sum().clamp(min=1).to(dtype)
    safe = torch.where(row, L, torch.zeros_like(L))
    ce = torch.logsumexp(tl, 1) - tl.gather(1, safe[:, None]).squeeze(1)
    cls = torch.where(row, ce, torch.zeros_like(ce)).sum() / n
    cols = (torch.arange(4, 8).expand(R, 4) if agnostic else 4 * torch.where(fg, L, torch.zeros_like(L))[:, None] + torch.arange(4))
    l1 = smooth_l1_64(tb.gather(1, cols) - torch.from_numpy(targets).to(dtype), beta).sum(1)
    reg = torch.where(fg, l1, torch.zeros_like(l1)).sum() / n
    (upstream[0] * cls + upstream[1] * reg).backward()
    return cls.item(), reg.item(), tl.grad.numpy(), tb.grad.numpy()


@functools.lru_cache(maxsize=None)
def fastrcnn_case(R, C, agnostic, beta, scale, unsampled=False, upstream=HEAD_UPSTREAM):
    rng = np.random.RandomState(600 + R + C)
    D = 8 if agnostic else 4 * C
    logits = (rng.randn(R, C) * scale).astype(np.float32)
    box = (rng.randn(R, D) * 0.8).astype(np.float32)
    targets = (rng.randn(R, 4) * 0.8).astype(np.float32)
    labels = rng.randint(-1, C + 1, R).astype(np.int64)            # -1 (not sampled) and the malformed C occur
    labels[: R // 2] = 0                                            # the first half is background
    if R >= 3:
        labels[R - 1], labels[R - 2], labels[R - 3] = C, -1, C - 1
        logits[R - 3, C // 2] = 88.0                                # exp(88) is next to the fp32 limit: the row maximum must be subtracted
    if R >= 5:
        logits[0, :] = -87.0                                        # a uniform (background) row far below zero
    if R >= 9:                                                      # residuals at 0 / beta of a positive row (class C - 1)
        fb = np.float32(beta)
        col0 = 4 if agnostic else 4 * (C - 1)
        box[R - 3, col0:col0 + 4] = targets[R - 3] + np.array([0, np.nextafter(fb, np.float32(0)), fb, -np.nextafter(fb, np.float32(9))], np.float32)
    if R == 1:
        labels[0] = 1
    if unsampled:
        labels[:] = -1
    ref = fastrcnn_reference(logits, box, labels, targets, agnostic, beta, upstream)
    return dict(logits=logits, box=box, labels=labels, targets=targets, agnostic=agnostic, beta=beta, ref=ref)


# ------------------------------------------------------------------------------------------ mask-head loss
#             P, C, M, logit scale
MASK_LOSS_CASES = ((1, 2, 1, 2.0), (3, 7, 14, 2.0), (5, 8, 28, 2.0), (5, 9, 17, 40.0), (4, 81, 28, 2.0), (300, 3, 2, 2.0))
MASK_UPSTREAM = 0.8


def mask_loss_reference(logits, labels, targets, upstream=MASK_UPSTREAM, dtype=torch.float64):
    """fp64 autograd of the mean BCE-with-logits over the class planes of the rows 0 < label < C -> (loss, d/d logits);
    `dtype=torch.float32`: the same ATen composition in fp32"""
    P, C, M, _ = logits.shape
    tl = torch.from_numpy(logits).to(dtype).requires_grad_()
    L = torch.from_numpy(labels)
    fg = (L > 0) & (L < C)
    own = torch.where(fg, L, torch.zeros_like(L))[:, None, None, None].expand(-1, 1, M, M)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(tl.gather(1, own).squeeze(1), torch.from_numpy(targets).to(dtype),
                                                               reduction="none")
    loss = torch.where(fg[:, None, None], bce, torch.zeros_like(bce)).sum() / (fg.sum() * (M * M)).clamp(min=1).to(dtype)
    (upstream * loss).backward()
    return loss.item(), tl.grad.numpy()


@functools.lru_cache(maxsize=None)
def mask_loss_case(P, C, M, scale, no_positives=False):
    """-> inputs + ref = (loss, d/d logits) in fp64: mean BCE-with-logits over the class planes of the rows 0 < label < C"""
    rng = np.random.RandomState(700 + P + C + M)
    logits = (rng.randn(P, C, M, M) * scale).astype(np.float32)
    targets = (rng.rand(P, M, M) < 0.4).astype(np.float32)
    labels = rng.randint(-1, C + 1, P).astype(np.int64)
    labels[0] = C - 1                                               # the last plane: own % kMaskSplit != own once C > 8
    if P >= 3:
        labels[1], labels[2] = C, 0                                 # malformed, background
    if no_positives:
        labels = np.where((labels > 0) & (labels < C), 0, labels)
    return dict(logits=logits, labels=labels, targets=targets, ref=mask_loss_reference(logits, labels, targets))
