"""The seeded random-shape cases shared by tests/test_emu_fuzz.py, tests/test_emu_fuzz_ext.py (host emulation) and
tests/test_fuzz_gpu.py, tests/test_fuzz_ext_gpu.py (MI355X).

A plain module: no tests, no fixtures, numpy only.  One generator per family; `family(seed)` returns a dict of numpy arrays
and plain Python parameters, or None where the drawn geometry has no output pixel (`deformable(0)` and
`deformable_channels_last(1)`, nothing else; no family of `EXTENSION` ever does).  Every generator draws from
`RandomState(base + seed)` in a fixed order, so a case is a function of (family, seed) alone;
tests/golden/fuzz_case_digests.json pins each one by the sha256 of `digest(case)`, and both test files run the same `SEEDS`.

What the families cover — odd map sizes, ROIs outside the map, degenerate ROIs, maps smaller than a tile, channel counts
that divide nothing, ragged NMS segments, exact IoU and score ties, focal-loss shapes on either side of the float4 /
scalar dispatch and of the grid-stride wrap — is described at each generator.  The `EXTENSION` families (the operators the
project added beyond the reference's `_C`) follow the reference's: their shapes straddle the 64-lane wave, the 256-thread
workgroup, the LDS chunk of ground truth, the 64-column and 64-detection scan tiles and the 256-row compaction round."""
import hashlib

import numpy as np

SEEDS = {"roi_align": 24, "nms": 16, "deformable": 10, "nms_batched": 8, "roi_align_fpn": 8,
         "deformable_channels_last": 6, "focal": 14,
         "targets_chain": 12, "head_losses": 12, "bbox_aug_merge": 12, "group_norm": 12, "bias_act": 12,
         "rpn_loss_decode": 10, "rpn_head_sparse": 10, "mask_chain": 12}
EMPTY = {"deformable": (0,), "deformable_channels_last": (1,)}       # seeds whose geometry has no output pixel


# ------------------------------------------------------------------------------------------ identity of a case
def _feed(h, v):
    if v is None:
        h.update(b"None;")
    elif isinstance(v, np.ndarray):
        h.update(("%s%r;" % (v.dtype.str, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (list, tuple)) and any(isinstance(e, np.ndarray) for e in v):
        h.update(("[%d;" % len(v)).encode())
        for e in v:
            _feed(h, e)
    else:
        assert not isinstance(v, np.generic), type(v)      # plain Python scalars only: their repr is the identity
        h.update((repr(v) + ";").encode())


def digest(case):
    """sha256 over the case's entries in key order: arrays by dtype, shape and bytes, everything else by repr; None for a
    case that is None"""
    if case is None:
        return None
    h = hashlib.sha256()
    for k in sorted(case):
        h.update((k + "=").encode())
        _feed(h, case[k])
    return h.hexdigest()


# ------------------------------------------------------------------------------------------ shared draws
def _rois(rng, K, N, H, W, scale):
    img_w, img_h = W / scale, H / scale
    x1 = rng.uniform(-0.3 * img_w, 1.1 * img_w, K)
    y1 = rng.uniform(-0.3 * img_h, 1.1 * img_h, K)
    w = np.exp(rng.uniform(np.log(0.5), np.log(1.5 * img_w), K))
    h = np.exp(rng.uniform(np.log(0.5), np.log(1.5 * img_h), K))
    r = np.stack([rng.randint(0, N, K), x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    if K > 2:
        r[0, 3:] = r[0, 1:3]           # zero-size ROI
        r[1, 1:] = [-1e4, -1e4, -9e3, -9e3]  # far outside
    return r


def _out_hw(H, W, k, stride, pad, dil):
    return ((H + 2 * pad - (dil * (k - 1) + 1)) // stride + 1, (W + 2 * pad - (dil * (k - 1) + 1)) // stride + 1)


# ------------------------------------------------------------------------------------------ the families
def roi_align(seed):
    """one map of 1..39 x 1..69 pixels, 1-2 images, channel counts on both sides of every chunk size, 1..70 ROIs (one of
    zero size, one far outside), the model's bin shapes and five others, every sampling ratio incl. adaptive"""
    rng = np.random.RandomState(1000 + seed)
    N = int(rng.randint(1, 3))
    C = int(rng.choice([1, 3, 4, 5, 16, 17, 33]))
    H, W = int(rng.randint(1, 40)), int(rng.randint(1, 70))
    K = int(rng.choice([1, 2, 7, 40, 70]))
    ph, pw = [(7, 7), (14, 14), (1, 1), (2, 5), (5, 2), (7, 7), (3, 3), (9, 4)][seed % 8]
    sr = int(rng.choice([0, 1, 2, 3]))
    scale = float(rng.choice([1.0, 0.5, 0.25, 0.0625]))
    x = rng.randn(N, C, H, W).astype(np.float32)
    rois = _rois(rng, K, N, H, W, scale)
    g = rng.randn(K, C, ph, pw).astype(np.float32)
    return dict(N=N, C=C, H=H, W=W, K=K, ph=ph, pw=pw, sr=sr, scale=scale, x=x, rois=rois, g=g)


def nms(seed):
    """1..513 boxes around the 64-box block sizes; odd seeds round the boxes (exact IoU == threshold ties), seed % 4 == 1
    rounds the scores (ties: stable order), seed % 4 == 2 duplicates a box; thresholds 0 and 1 included"""
    rng = np.random.RandomState(2000 + seed)
    n = int(rng.choice([1, 3, 64, 65, 127, 128, 300, 513]))
    cx, cy = rng.uniform(0, 200, n), rng.uniform(0, 200, n)
    w, h = rng.uniform(1, 80, n), rng.uniform(1, 80, n)
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
    if seed % 2:
        boxes = np.round(boxes)                     # integer boxes: many exact IoU == threshold ties
    scores = rng.rand(n).astype(np.float32)
    if seed % 4 == 1:
        scores = np.round(scores, 1)                # score ties: stable order
    if seed % 4 == 2 and n > 3:
        boxes[2] = boxes[1]; scores[2] = scores[1]  # duplicates
    thr = float(rng.choice([0.0, 0.3, 0.5, 0.7, 1.0]))
    return dict(n=n, boxes=boxes, scores=scores, thr=thr)


def deformable(seed):
    """reference-layout deformable kernels: 1-2 images, 1-2 deformable groups, 1..34 channels, maps of 3..13 x 3..19,
    1x1 and 3x3 taps with stride, padding and dilation; odd seeds are modulated; offsets of scale 0, 0.7 or 3 pixels"""
    rng = np.random.RandomState(3000 + seed)
    B = int(rng.randint(1, 3))
    dg = int(rng.choice([1, 2]))
    C = dg * int(rng.choice([1, 3, 8, 17]))
    H, W = int(rng.randint(3, 14)), int(rng.randint(3, 20))
    k = int(rng.choice([1, 3]))
    stride, pad, dil = int(rng.choice([1, 2])), int(rng.choice([0, 1, 2])), int(rng.choice([1, 2]))
    Ho, Wo = _out_hw(H, W, k, stride, pad, dil)
    if Ho < 1 or Wo < 1:
        return None
    x = rng.randn(B, C, H, W).astype(np.float32)
    off = (rng.randn(B, dg * 2 * k * k, Ho, Wo) * rng.choice([0.0, 0.7, 3.0])).astype(np.float32)
    mask = rng.rand(B, dg * k * k, Ho, Wo).astype(np.float32) if seed % 2 else None
    gcol = rng.randn(C * k * k, B * Ho * Wo).astype(np.float32)       # the column matrix's shape
    return dict(B=B, dg=dg, C=C, H=H, W=W, k=k, stride=stride, pad=pad, dil=dil, Ho=Ho, Wo=Wo, x=x, off=off, mask=mask, gcol=gcol)


def nms_batched(seed):
    """1..8 ragged segments of 0..2049 boxes over every scan width; odd seeds round the boxes, seed % 3 == 1 rounds the
    scores; an empty segment among them (seed 5)"""
    rng = np.random.RandomState(5000 + seed)
    S = int(rng.randint(1, 9))
    sizes = [int(rng.choice([0, 1, 2, 63, 64, 65, 130, 700, 1025, 1500, 2049])) for _ in range(S)]
    segs = []
    for n in sizes:
        cx, cy = rng.uniform(0, 300, n), rng.uniform(0, 300, n)
        w, h = rng.uniform(1, 90, n), rng.uniform(1, 90, n)
        b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)
        if seed % 2:
            b = np.round(b)
        s = rng.rand(n).astype(np.float32)
        if seed % 3 == 1:
            s = np.round(s, 1)
        segs.append((b.reshape(n, 4), s))
    boxes = np.concatenate([b for b, _ in segs]) if sum(sizes) else np.zeros((0, 4), np.float32)
    scores = np.concatenate([s for _, s in segs]) if sum(sizes) else np.zeros((0,), np.float32)
    offs = np.cumsum([0] + sizes).astype(np.int32)
    thr = float(rng.choice([0.3, 0.5, 0.7]))
    max_n = max(max(sizes), 1)
    return dict(S=S, sizes=sizes, boxes=boxes, scores=scores, offs=offs, thr=thr, max_n=max_n)


def segments(case):
    """the (boxes, scores) pairs of an `nms_batched` case"""
    o = case["offs"]
    return [(case["boxes"][o[i]:o[i + 1]], case["scores"][o[i]:o[i + 1]]) for i in range(case["S"])]


def roi_align_fpn(seed):
    """pyramids of 2-4 levels with odd level sizes (level 0: 24..63 x 24..79, halved and rounded up per level), 1-2 images,
    4..32 channels incl. 17, 3..150 ROIs of every scale incl. a zero-size one and one far outside; 7x7 and 14x14 bins"""
    rng = np.random.RandomState(6000 + seed)
    N = int(rng.randint(1, 3))
    C = int(rng.choice([4, 16, 17, 32]))
    L = int(rng.randint(2, 5))
    H0, W0 = int(rng.randint(24, 64)), int(rng.randint(24, 80))
    shapes = [(N, C, -(-H0 // (1 << l)), -(-W0 // (1 << l))) for l in range(L)]
    scales = [1.0 / (4 << l) for l in range(L)]
    feats = [rng.randn(*s).astype(np.float32) for s in shapes]
    K = int(rng.choice([3, 40, 150]))
    rois = _rois(rng, K, N, shapes[0][2], shapes[0][3], scales[0])
    ph = [7, 14][seed % 2]
    g = rng.randn(K, C, ph, ph).astype(np.float32)
    return dict(N=N, C=C, L=L, shapes=shapes, scales=scales, feats=feats, K=K, rois=rois, ph=ph, g=g)


def deformable_channels_last(seed):
    """shapes of the channels-last plan (fp32: channel counts / 4 a power of two >= 16), 3x3 taps with stride, padding and
    dilation on maps of 4..9 x 4..11; odd seeds are modulated"""
    rng = np.random.RandomState(7000 + seed)
    B = int(rng.randint(1, 3))
    C, Cout = int(rng.choice([64, 128])), int(rng.choice([64, 128, 256]))   # fp32: channel counts / 4 a power of two >= 16
    H, W = int(rng.randint(4, 10)), int(rng.randint(4, 12))
    k = 3
    stride, pad, dil = int(rng.choice([1, 2])), int(rng.choice([0, 1, 2])), int(rng.choice([1, 2]))
    Ho, Wo = _out_hw(H, W, k, stride, pad, dil)
    if Ho < 1 or Wo < 1:
        return None
    x = rng.randn(B, C, H, W).astype(np.float32)
    off = (rng.randn(B, 2 * k * k, Ho, Wo) * rng.choice([0.0, 0.7, 3.0])).astype(np.float32)
    mask = rng.rand(B, k * k, Ho, Wo).astype(np.float32) if seed % 2 else None
    wgt = (rng.randn(Cout, C, k, k) / np.sqrt(C * k * k)).astype(np.float32)
    go = rng.randn(B, Cout, Ho, Wo).astype(np.float32)
    return dict(B=B, C=C, Cout=Cout, H=H, W=W, k=k, stride=stride, pad=pad, dil=dil, Ho=Ho, Wo=Wo, x=x, off=off, mask=mask,
                wgt=wgt, go=go)


# focal loss: the launch takes the float4 kernels when C % 4 == 0 and every pointer is 16-byte aligned, else the scalar
# kernels; either grid is capped at FOCAL_MAX_ITEMS work items (float4 groups / elements), beyond which a thread strides
FOCAL_MAX_ITEMS = 256 * 8 * 256       # compute units * 8 workgroups * 256 threads
_FOCAL_C = [1, 3, 4, 7, 8, 80, 81]


def focal(seed):
    """seeds 0..11: R in {1, 2, 37, 255, 257, 1000}, gamma in {0, 1, 2, 1.5}, alpha in {0.25, 0.4, 0.5} drawn; C walks
    through {1, 3, 4, 7, 8, 80, 81} with the seed and `offset_floats` is 0 for seed % 3 == 1, else 1, which puts C = 4 (seeds
    2, 9), 80 (seed 5) and 8 (seed 11) on a pointer 4 bytes past a 16-byte boundary — the scalar kernels at C % 4 == 0 — and
    leaves C = 8 (seed 4) aligned.  Targets over [-1, C] with rows 0..3 forced to -1, 0, 1, C; row 0 of the logits spreads over
    [-100, 100].  Seed 12 (6554 x 81 = 530 874 elements, gamma 2) makes the scalar kernels stride a second time,
    seed 13 (26215 x 80 = 524 300 float4 groups, gamma 1.5: the smallest R that does) the float4 kernels outside the
    gamma == 2 instantiation; at `offset_floats` = 1 its 2 097 200 elements take the scalar kernels round four times."""
    rng = np.random.RandomState(8000 + seed)
    if seed == 12:
        R, C, gamma, alpha, offset_floats = 6554, 81, 2.0, 0.25, 0
    elif seed == 13:
        R, C, gamma, alpha, offset_floats = 26215, 80, 1.5, 0.25, 1
    else:
        R = int(rng.choice([1, 2, 37, 255, 257, 1000]))
        C = _FOCAL_C[seed % len(_FOCAL_C)]
        gamma = float(rng.choice([0.0, 1.0, 2.0, 1.5]))
        alpha = float(rng.choice([0.25, 0.4, 0.5]))
        offset_floats = 0 if seed % 3 == 1 else 1
    logits = (rng.randn(R, C) * 3.0).astype(np.float32)
    logits[0] = np.linspace(-100.0, 100.0, C) if C > 1 else [-100.0]
    targets = rng.randint(-1, C + 1, R).astype(np.int32)
    forced = [-1, 0, 1, C]
    targets[:min(R, 4)] = forced[:min(R, 4)]
    d_losses = rng.rand(R, C).astype(np.float32)
    d_scalar = float(np.float32(rng.uniform(0.5, 2.0) / 1234.0))      # what `.sum() / normaliser` back-propagates
    return dict(R=R, C=C, gamma=gamma, alpha=alpha, offset_floats=offset_floats, logits=logits, targets=targets,
                d_losses=d_losses, d_scalar=d_scalar)


# ------------------------------------------------------------------------------------------ the extension operators
# Families of the operators beyond the reference's `_C` (csrc/targets.hip, head_loss.hip, keypoint.hip, group_norm.hip,
# bias_act.hip, bbox_aug.hip).  None of these generators returns None: degenerate members (an image without a valid ground
# truth, no sampled row, no positive, no valid keypoint, a group without rows, a single class) are drawn on purpose and run.
# The lists below are the sizes on either side of the constants where the kernels change route; a list is walked with the seed
# (strides chosen so that every entry occurs within the family's seeds), everything else is drawn.
CHAIN_N = (1, 2, 3)
CHAIN_M = (1, 2, 63, 64, 65, 255, 256, 257, 513)       # the 64-lane wave, kGtChunk = 256 rows of ground truth per LDS pass
CHAIN_K = (1, 255, 256, 257, 1023, 1025, 2049, 4097)   # the 256-thread block, 1024 boxes per matcher workgroup
CHAIN_B = (1, 5, 64, 256, 512)
CHAIN_THRESHOLDS = ((0.7, 0.3, True), (0.5, 0.5, False))     # target_cases.MATCHER_THRESHOLDS (asserted equal by the tests)
CHAIN_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def _xywh_boxes(rng, n, W=640, H=480, smin=8, smax=200):
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    w, h = rng.uniform(smin, smax, n), rng.uniform(smin, smax, n)
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1).astype(np.float32)


def targets_chain(seed):
    """match_boxes -> match_labels -> sample_labels(with_list) -> roi_head_targets on one set of boxes: N, M, K, B walk through
    CHAIN_N / _M / _K / _B; boxes shared (even seeds) or per image (odd); the RPN rule (labels 1 / 0 / -1 as float32, no
    gt_labels) on even seeds, the box-head rule (int64 class labels) on odd ones; the thresholds alternate every second seed.
    A third of the boxes are ground truths jittered by up to 3 pixels (matches), a sixth ground truths shifted by 0.3 of their
    width (IoU ~0.54: between 0.3 and 0.7, a match at 0.5), the rest random.  About a fifth of the ground-truth rows are
    invalid and keep plausible coordinates; seed % 4 == 1 leaves the last image without a valid row.  The sampler's seed has 64
    random bits, the top one set for seed % 3 == 0; the box-validity mask and the objectness are absent for some seeds."""
    rng = np.random.RandomState(9000 + seed)
    N, M, K = CHAIN_N[seed % 3], CHAIN_M[seed % 9], CHAIN_K[(3 * seed + 1) % 8]
    B = CHAIN_B[seed % 5]
    max_pos = max(1, (B // 4, B // 2, B)[(seed // 2) % 3])
    batched, rpn_rule = bool(seed % 2), seed % 2 == 0
    hi, lo, lq = CHAIN_THRESHOLDS[(seed // 2) % 2]
    gt = np.stack([_xywh_boxes(rng, M) for _ in range(N)])
    gt_valid = rng.rand(N, M) < 0.8
    gt_valid[0, 0] = True
    if seed % 4 == 1:
        gt_valid[N - 1] = False
    gt_labels = rng.randint(1, 81, (N, M)).astype(np.int64)

    def fill(image):
        b = _xywh_boxes(rng, K)
        n = K // 3
        src = rng.randint(0, M, n)
        b[:n] = gt[image, src] + rng.uniform(-3, 3, (n, 4)).astype(np.float32)
        m = K // 6
        src = rng.randint(0, M, m)
        g = gt[image, src]
        shift = (0.3 * (g[:, 2] - g[:, 0]))[:, None] * np.float32([1, 0, 1, 0])
        b[n:n + m] = g + shift.astype(np.float32)
        return b
    boxes = np.stack([fill(i) for i in range(N)]) if batched else fill(0)
    box_valid = (rng.rand(N, K) < 0.9) if seed % 3 else None
    objectness = rng.rand(N, K).astype(np.float32) if seed % 4 < 2 else None
    sampler_seed = (int(rng.randint(0, 1 << 31)) << 33) ^ (int(rng.randint(0, 1 << 31)) << 2) ^ int(rng.randint(0, 4))
    sampler_seed = (sampler_seed | (1 << 63)) if seed % 3 == 0 else (sampler_seed & ((1 << 63) - 1))
    return dict(N=N, M=M, K=K, B=B, max_pos=max_pos, batched=batched, rpn_rule=rpn_rule, hi=hi, lo=lo, lq=lq, gt=gt,
                gt_valid=gt_valid, gt_labels=gt_labels, boxes=boxes, box_valid=box_valid, objectness=objectness,
                sampler_seed=sampler_seed, weights=CHAIN_WEIGHTS)


LOSS_R = (1, 3, 64, 65, 300, 513)          # rows on either side of the 64-lane wave and the 256-thread block
LOSS_C = (2, 3, 63, 64, 65, 81)            # classes below / at / above a wave
LOSS_BETA = (1.0, 0.5, 1.0 / 9)
MASK_P, MASK_C, MASK_M = (1, 3, 5, 300), (2, 7, 8, 9, 81), (1, 2, 14, 17, 28)     # kMaskSplit = 8 planes; M * M around 256
KP_P, KP_K, KP_HW = (1, 3, 64, 65), (1, 17), ((1, 1), (7, 5), (56, 56), (64, 64))
LOSS_ALL_UNSAMPLED, LOSS_NO_POSITIVES, LOSS_NO_VALID = 7, 5, 6        # the seeds of the three empty problems


def head_losses(seed):
    """one problem for each of fastrcnn_loss, mask_loss and keypoint_loss (keys fr_*, mk_*, kp_*).  fastrcnn: R, C walk through
    LOSS_R / LOSS_C, class-agnostic on odd seeds, beta through LOSS_BETA, logits of scale 3 or 30, labels over [-1, C] (not
    sampled .. malformed), seed 7 with every row unsampled.  mask: P, C, M through MASK_P / _C / _M, logits of scale 2 or 40,
    labels over [-1, C] with row 0 a positive of the last plane, seed 5 without positives.  keypoint: P, K, H x W through KP_P /
    _K / _HW, channels-last logits on odd seeds, about 70 % valid rows, seed 6 without a valid row."""
    rng = np.random.RandomState(10000 + seed)
    R, C = LOSS_R[seed % 6], LOSS_C[(seed + seed // 6) % 6]
    agnostic, beta, scale = bool(seed % 2), LOSS_BETA[seed % 3], (3.0, 30.0)[(seed // 2) % 2]
    fr_logits = (rng.randn(R, C) * scale).astype(np.float32)
    fr_box = (rng.randn(R, 8 if agnostic else 4 * C) * 0.8).astype(np.float32)
    fr_targets = (rng.randn(R, 4) * 0.8).astype(np.float32)
    fr_labels = rng.randint(-1, C + 1, R).astype(np.int64)
    if seed == LOSS_ALL_UNSAMPLED:
        fr_labels[:] = -1
    P, Cm, Mm = MASK_P[seed % 4], MASK_C[seed % 5], MASK_M[(2 * seed + seed // 5) % 5]
    mk_logits = (rng.randn(P, Cm, Mm, Mm) * (2.0, 40.0)[seed % 2]).astype(np.float32)
    mk_targets = (rng.rand(P, Mm, Mm) < 0.4).astype(np.float32)
    mk_labels = rng.randint(-1, Cm + 1, P).astype(np.int64)
    mk_labels[0] = Cm - 1
    if seed == LOSS_NO_POSITIVES:
        mk_labels = np.where((mk_labels > 0) & (mk_labels < Cm), 0, mk_labels)
    Pk, Kk, (H, W) = KP_P[seed % 4], KP_K[(seed // 2) % 2], KP_HW[(seed + seed // 4) % 4]
    kp_logits = (rng.randn(Pk, Kk, H, W) * 3.0).astype(np.float32)
    kp_heat = rng.randint(0, H * W, (Pk, Kk)).astype(np.int64)
    kp_valid = rng.rand(Pk, Kk) < 0.7
    if seed == LOSS_NO_VALID:
        kp_valid[:] = False
    return dict(fr_R=R, fr_C=C, fr_agnostic=agnostic, fr_beta=beta, fr_logits=fr_logits, fr_box=fr_box, fr_targets=fr_targets,
                fr_labels=fr_labels, mk_P=P, mk_C=Cm, mk_M=Mm, mk_logits=mk_logits, mk_targets=mk_targets, mk_labels=mk_labels,
                kp_P=Pk, kp_K=Kk, kp_H=H, kp_W=W, kp_channels_last=bool(seed % 2), kp_logits=kp_logits, kp_heat=kp_heat,
                kp_valid=kp_valid)


AUG_C = (1, 2, 5, 81)                      # a single class (no segment at all), 32 / 16 rows per wave step, three column tiles
AUG_ROWS = (0, 1, 31, 32, 33, 65, 128, 129, 257, 300)       # a wave's 32 rows, a workgroup's 128, several workgroups
AUG_PASS_RATE = (0.0, 0.05, 0.5, 1.0)


def bbox_aug_merge(seed):
    """the arguments of bbox_aug_cases.make_case: C through AUG_C, 1-2 images of 1-4 passes with drawn flips, 0..300 rows per
    group out of AUG_ROWS, frames of odd and differing sizes, the pass rate through AUG_PASS_RATE, class-agnostic on odd seeds"""
    rng = np.random.RandomState(15000 + seed)
    C = AUG_C[seed % 4]
    N, T = int(rng.randint(1, 3)), int(rng.randint(1, 5))
    rows = [[int(rng.choice(AUG_ROWS)) for _ in range(T)] for _ in range(N)]
    flips = [int(rng.randint(0, 2)) for _ in range(T)]
    frames = [[(int(rng.randint(40, 200)), int(rng.randint(40, 200))) for _ in range(T)] for _ in range(N)]
    return dict(seed=15000 + seed, C=C, rows=rows, frames=frames, flips=flips, pass_rate=AUG_PASS_RATE[(seed + seed // 4) % 4],
                agnostic=bool(seed % 2))


GN_G, GN_D = (1, 2, 3, 32), (1, 2, 4, 8, 256)               # groups x channels per group (the widest group the library serves)
GN_HW = ((1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (1, 1025), (25, 41))      # 1, 2, 63, 64, 65, 1025 rows and the 25 x 41 map
DTYPES = ("float32", "float16", "bfloat16")


def group_norm(seed):
    """channels-last GroupNorm (+ residual) (+ ReLU): N drawn from 1..3, G, C / G and the plane walk through GN_G, GN_D, GN_HW
    (seed 6: 2 channels per group on the 25 x 41 map, the first plane of the split regime; seed 5: one channel per group at
    1025 rows); the storage dtype walks through DTYPES, relu = seed % 2, residual = seed // 2 % 2, gamma / beta present by
    seed % 4 (both, gamma, beta, neither), the storage starts 0 or 1 element into its allocation.  Values are fp32 draws of mean
    0.5; the tests round them to the storage dtype."""
    rng = np.random.RandomState(13000 + seed)
    N = int(rng.randint(1, 4))
    G, D, (H, W) = GN_G[seed % 4], GN_D[seed % 5], GN_HW[seed % 7]
    C = G * D
    x = (rng.randn(N, C, H, W) + 0.5).astype(np.float32)
    residual = rng.randn(N, C, H, W).astype(np.float32) if (seed // 2) % 2 else None
    gy = rng.randn(N, C, H, W).astype(np.float32)
    gamma = (rng.randn(C) + 1.0).astype(np.float32)
    beta = rng.randn(C).astype(np.float32)
    return dict(N=N, C=C, G=G, H=H, W=W, dtype=DTYPES[seed % 3], relu=bool(seed % 2), x=x, residual=residual, gy=gy,
                gamma=gamma if seed % 4 in (0, 1) else None, beta=beta if seed % 4 in (0, 2) else None, offset=(seed // 3) % 2)


BIAS_C, COLSUM_C = (4, 8, 256, 1024), (1, 3, 12, 81, 255)   # widths of the fused pass (C | 1024, C % 4 == 0) / of column_sum
BIAS_ROWS = ((1, 1), (7, 9), (8, 8), (5, 13), (25, 40), (17, 241))          # 1, 63, 64, 65, 1000, 4097 rows of one image


def bias_act(seed):
    """the fused bias (+ ReLU) pass on a channels-last [1, C, H, W] activation with C through BIAS_C and its backward with the
    bias gradient, and `column_sum` of a [rows, Cs] matrix with Cs through COLSUM_C; H x W = rows walks through BIAS_ROWS; relu
    on odd seeds, the storage dtype through DTYPES"""
    rng = np.random.RandomState(14000 + seed)
    C, Cs, (H, W) = BIAS_C[seed % 4], COLSUM_C[seed % 5], BIAS_ROWS[(seed + seed // 6) % 6]
    x = rng.randn(1, C, H, W).astype(np.float32)
    bias = rng.randn(C).astype(np.float32)
    gy = rng.randn(1, C, H, W).astype(np.float32)
    m = rng.randn(H * W, Cs).astype(np.float32)
    return dict(C=C, Cs=Cs, H=H, W=W, rows=H * W, relu=bool(seed % 2), dtype=DTYPES[(seed // 2) % 3], x=x, bias=bias, gy=gy, m=m)


RPN_K = (1, 5, 64, 257, 1000)               # candidates per level before the cut to A * H * W; N * k around 256
RPN_NOTHING_SAMPLED, RPN_NEGATIVES_ONLY = 3, 5


def rpn_loss_decode(seed):
    """1..8 levels of planes 1..9 x 1..9, N in 1..3, A = 1 (odd seeds) or 3, 1..5 ground truths; anchors and ground truths on
    quarter pixels (target_cases.rpn_loss_case says why); matched indices over [-2, M); `pos` / `neg` of a drawn density, seed 3
    with nothing sampled, seed 5 with negatives only.  Per level the arguments of one rpn_decode call: the candidates k (cut to
    A * H * W by the test), min_size 0 or 24, the column / row at which the slices start, an image size per image that cuts
    some anchors down; seed % 3 == 0 pushes the width deltas of image 0 past the clip."""
    rng = np.random.RandomState(11000 + seed)
    L, N, A, M = int(rng.randint(1, 9)), int(rng.randint(1, 4)), (3, 1)[seed % 2], int(rng.randint(1, 6))
    shapes = [(int(rng.randint(1, 10)), int(rng.randint(1, 10))) for _ in range(L)]
    T = A * sum(h * w for h, w in shapes)
    obj = [(rng.randn(N, A, h, w) * 3).astype(np.float32) for h, w in shapes]
    box = [(rng.randn(N, 4 * A, h, w) * 0.2).astype(np.float32) for h, w in shapes]
    x1, y1 = rng.uniform(0, 80, T), rng.uniform(0, 60, T)
    anchors = np.stack([x1, y1, x1 + rng.uniform(4, 60, T), y1 + rng.uniform(4, 60, T)], 1).astype(np.float32)
    gx, gy = rng.uniform(0, 70, (N, M)), rng.uniform(0, 50, (N, M))
    gt = np.stack([gx, gy, gx + rng.uniform(5, 50, (N, M)), gy + rng.uniform(5, 50, (N, M))], 2).astype(np.float32)
    anchors, gt = (np.round(anchors * 4) / 4).astype(np.float32), (np.round(gt * 4) / 4).astype(np.float32)
    matched = rng.randint(-2, M, (N, T)).astype(np.int64)
    dp, dn = float(rng.choice([0.05, 0.4, 1.0])), float(rng.choice([0.05, 0.5, 1.0]))
    pos = (matched >= 0) & (rng.rand(N, T) < dp)
    neg = (matched == -1) & (rng.rand(N, T) < dn)
    if seed == RPN_NOTHING_SAMPLED:
        pos[:], neg[:] = False, False
    if seed == RPN_NEGATIVES_ONLY:
        pos[:] = False
        neg[0, 0] = True
    weights = (2.0, 2.0, 0.5, 0.5) if seed % 4 == 2 else (1.0, 1.0, 1.0, 1.0)
    # per level (k, min_size, col, off)
    decode = [(int(rng.choice(RPN_K)), (0, 24)[int(rng.randint(0, 2))], int(rng.randint(0, 6)), int(rng.randint(0, 8)))
              for _ in range(L)]
    sizes = [(int(rng.randint(30, 120)), int(rng.randint(40, 140))) for _ in range(N)]
    reg_scale = float(rng.choice([0.7, 2.0]))
    return dict(L=L, N=N, A=A, M=M, shapes=shapes, obj=obj, box=box, anchors=anchors, gt=gt, matched=matched, pos=pos, neg=neg,
                beta=1.0 / 9, weights=weights, decode=decode, sizes=sizes, reg_scale=reg_scale,
                clip=seed % 3 == 0)


SPARSE_C = (4, 8, 36, 64)                   # 16-byte rows of one, two, nine and sixteen float4
SPARSE_ROWS = (0, 1, 255, 256, 257)         # anchors with a non-zero loss gradient: around one compaction round of 256
SPARSE_OVERFLOW = 9                         # the seed whose row count is max_rows + 1


def rpn_head_sparse(seed):
    """the RPN head (3x3 conv + ReLU, two 1x1 predictors) with the sparse backward: C through SPARSE_C, 1..5 levels of planes
    1..9 x 1..9 (two 9-wide levels in front where 255+ rows need the anchors), N in {1, 2}, A = 3; the number of anchors with
    a non-zero incoming gradient through SPARSE_ROWS, placed at random; max_rows ample (even seeds) or exactly the count; seed
    9: the count is max_rows + 1"""
    rng = np.random.RandomState(16000 + seed)
    C, A, N = SPARSE_C[seed % 4], 3, int(rng.randint(1, 3))
    rows = SPARSE_ROWS[seed % 5]
    L = int(rng.randint(1, 6))
    levels = [(int(rng.randint(1, 10)), int(rng.randint(1, 10))) for _ in range(L)]
    levels = [(h, 2) if (h, w) == (1, 1) else (h, w) for h, w in levels]     # a 1 x 1 plane is not a channels-last tensor to `_C`
    if rows > 1:
        levels = [(9, 9), (9, 8)] + levels[:3]
    total = N * A * sum(h * w for h, w in levels)
    assert rows <= total
    p = {"conv.weight": (rng.randn(C, C, 3, 3) * (1.5 / (9 * C) ** 0.5)).astype(np.float32), "conv.bias": (rng.randn(C) * 0.1).astype(np.float32),
         "cls_logits.weight": (rng.randn(A, C, 1, 1) * 0.3).astype(np.float32), "cls_logits.bias": (rng.randn(A) * 0.1).astype(np.float32),
         "bbox_pred.weight": (rng.randn(4 * A, C, 1, 1) * 0.3).astype(np.float32), "bbox_pred.bias": (rng.randn(4 * A) * 0.1).astype(np.float32)}
    feats = [rng.randn(N, C, h, w).astype(np.float32) for h, w in levels]
    pick = np.sort(rng.permutation(total)[:rows])
    gobj = [np.zeros((N, A, h, w), np.float32) for h, w in levels]
    gbox = [np.zeros((N, 4 * A, h, w), np.float32) for h, w in levels]
    first = 0
    for l, (h, w) in enumerate(levels):
        n_l = N * A * h * w
        for f in pick[(pick >= first) & (pick < first + n_l)] - first:
            n, a, y, x = np.unravel_index(int(f), (N, A, h, w))
            gobj[l][n, a, y, x] = np.float32(rng.randn() * 2.5 + (3.0 if rng.rand() < 0.5 else -3.0))      # never zero
            gbox[l][n, 4 * a:4 * a + 4, y, x] = (rng.randn(4) * 0.7).astype(np.float32)
        first += n_l
    if seed == SPARSE_OVERFLOW:
        max_rows = rows - 1
    else:
        max_rows = max(rows, 1) if seed % 2 else rows + int(rng.randint(1, 40))
    return dict(C=C, A=A, N=N, rows=rows, levels=levels, max_rows=max_rows,
                params=[p[k] for k in SPARSE_PARAMS], feats=feats, gobj=gobj, gbox=gbox)


SPARSE_PARAMS = ("conv.weight", "conv.bias", "cls_logits.weight", "cls_logits.bias", "bbox_pred.weight", "bbox_pred.bias")
CHAIN_DETS = (0, 1, 2, 63, 64, 65)           # the 64-detection scan tile
CHAIN_W = (1, 31, 32, 33, 63, 64, 65, 129)   # 32 columns per workgroup row of the RLE kernels, 64-pixel words of the packs
MASK_DEBUG_THRESHOLD = 4                     # the seed with threshold -1


def _inside_box(rng, H, W):
    x, y = np.sort(rng.uniform(0, W, 2)), np.sort(rng.uniform(0, H, 2))
    return np.array([x[0], y[0], x[1] + 0.5, y[1] + 0.5])


def mask_chain(seed):
    """inference and evaluation of masks on one set of detections: CHAIN_DETS detections spread over 1..3 images of
    1..97 x CHAIN_W pixels (the widths walk through CHAIN_W), M = 14 / 28, padding 1 / 2, the storage dtype through DTYPES,
    threshold 0.5 (-1 on seed 4).  Boxes: each image's first lies inside it, the others inside, half off an edge, larger than
    the image or wholly outside it; with two or more detections the second has a NaN coordinate.  Per image 0..3 ground-truth
    planes (a rectangle plus noise), a quarter of them crowds, with the rectangle as their box."""
    rng = np.random.RandomState(12000 + seed)
    n_img = int(rng.randint(1, 4))
    sizes = [(int(rng.randint(1, 98)), CHAIN_W[(seed + 3 * i) % 8]) for i in range(n_img)]
    D = CHAIN_DETS[seed % 6]
    counts = [int(v) for v in rng.multinomial(D, [1.0 / n_img] * n_img)]
    M, padding, dtype = (14, 28)[seed % 2], (1, 2)[(seed // 2) % 2], DTYPES[seed % 3]
    maps = (1.0 / (1.0 + np.exp(-3.0 * rng.randn(D, M, M)))).astype(np.float32)
    boxes = np.zeros((D, 4), np.float64)
    k = 0
    for (H, W), n in zip(sizes, counts):
        for j in range(n):
            b = _inside_box(rng, H, W)
            kind = 0 if j == 0 else int(rng.randint(0, 4))
            if kind == 1:
                b += np.array([0.5 * W, 0.0, 0.5 * W, 0.0]) * (1 if rng.rand() < 0.5 else -1)
            elif kind == 2:
                b = np.array([-0.3 * W - 2, -0.2 * H - 2, 1.3 * W + 2, 1.4 * H + 2])
            elif kind == 3:
                b += np.array([W + 40.0, 0.0, W + 40.0, 0.0])
            boxes[k] = b
            k += 1
    boxes = boxes.astype(np.float32)
    if D >= 2:
        boxes[1, int(rng.randint(0, 4))] = np.nan
    gt_planes, gt_boxes, gt_crowd = [], [], []
    for H, W in sizes:
        G = int(rng.randint(0, 4))
        planes = np.zeros((G, H, W), np.uint8)
        gb = np.zeros((G, 4), np.float32)
        for g in range(G):
            b = _inside_box(rng, H, W)
            x0, y0, x1, y1 = int(b[0]), int(b[1]), int(np.ceil(b[2])), int(np.ceil(b[3]))
            planes[g, y0:y1 + 1, x0:x1 + 1] = 1
            planes[g] ^= (rng.rand(H, W) < 0.05).astype(np.uint8)
            gb[g] = [x0, y0, min(x1, W - 1), min(y1, H - 1)]
        gt_planes.append(planes)
        gt_boxes.append(gb)
        gt_crowd.append((rng.rand(G) < 0.25).astype(np.uint8))
    return dict(n_img=n_img, sizes=sizes, D=D, counts=counts, M=M, padding=padding, dtype=dtype,
                threshold=-1.0 if seed == MASK_DEBUG_THRESHOLD else 0.5, maps=maps, boxes=boxes, gt_planes=gt_planes,
                gt_boxes=gt_boxes, gt_crowd=gt_crowd)


FAMILIES = {"roi_align": roi_align, "nms": nms, "deformable": deformable, "nms_batched": nms_batched,
            "roi_align_fpn": roi_align_fpn, "deformable_channels_last": deformable_channels_last, "focal": focal,
            "targets_chain": targets_chain, "head_losses": head_losses, "bbox_aug_merge": bbox_aug_merge, "group_norm": group_norm,
            "bias_act": bias_act, "rpn_loss_decode": rpn_loss_decode, "rpn_head_sparse": rpn_head_sparse, "mask_chain": mask_chain}
EXTENSION = ("targets_chain", "head_losses", "rpn_loss_decode", "rpn_head_sparse", "mask_chain", "bbox_aug_merge", "group_norm",
             "bias_act")
