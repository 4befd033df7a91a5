"""The seeded random-shape cases shared by tests/test_emu_fuzz.py (host emulation) and tests/test_fuzz_gpu.py (MI355X).

A plain module: no tests, no fixtures, numpy only.  One generator per family; `family(seed)` returns a dict of numpy arrays
and plain Python parameters, or None where the drawn geometry has no output pixel (`deformable(0)` and
`deformable_channels_last(1)`, nothing else).  Every generator draws from `RandomState(base + seed)` in a fixed order, so
a case is a function of (family, seed) alone; tests/golden/fuzz_case_digests.json pins each one by the sha256 of
`digest(case)`, and both test files run the same `SEEDS`.

What the families cover — odd map sizes, ROIs outside the map, degenerate ROIs, maps smaller than a tile, channel counts
that divide nothing, ragged NMS segments, exact IoU and score ties, focal-loss shapes on either side of the float4 /
scalar dispatch and of the grid-stride wrap — is described at each generator."""
import hashlib

import numpy as np

SEEDS = {"roi_align": 24, "nms": 16, "deformable": 10, "nms_batched": 8, "roi_align_fpn": 8,
         "deformable_channels_last": 6, "focal": 14}
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


FAMILIES = {"roi_align": roi_align, "nms": nms, "deformable": deformable, "nms_batched": nms_batched,
            "roi_align_fpn": roi_align_fpn, "deformable_channels_last": deformable_channels_last, "focal": focal}
