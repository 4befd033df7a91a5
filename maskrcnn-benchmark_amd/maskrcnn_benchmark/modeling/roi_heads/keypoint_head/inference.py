"""Keypoint post-processing for inference (reference roi_heads/keypoint_head/inference.py:5-125): every detection's
heatmaps -> a "keypoints" field, PersonKeypoints [n, K, 3] of (x, y, 1) with a "logits" field of the scores [n, K].

The reference copies the heatmaps and the boxes to the host and runs cv2.resize(INTER_CUBIC) + argmax in a Python loop,
one image per batch.  Here every detection of the batch is decoded by one launch (csrc/keypoint.hip,
`detops_heatmaps_to_keypoints_f32`); `heatmaps_to_keypoints_torch` is the same computation in torch: the CPU path and the
yardstick of the kernel."""
import torch
from torch import nn

from maskrcnn_benchmark import _C
from maskrcnn_benchmark.structures.keypoint import PersonKeypoints

_A = -0.75   # OpenCV's INTER_CUBIC coefficient


def _cubic_taps(out, n):
    """OpenCV INTER_CUBIC taps of `out` output samples over `n` inputs -> (indices [out, 4] int64, weights [out, 4] fp32)"""
    d = torch.arange(out, dtype=torch.float64)
    f = ((d + 0.5) * (n / out) - 0.5).float()
    fl = f.floor()
    u = f - fl
    A = _A
    w0 = ((A * (u + 1) - 5 * A) * (u + 1) + 8 * A) * (u + 1) - 4 * A
    w1 = ((A + 2) * u - (A + 3)) * u * u + 1
    v = 1 - u
    w2 = ((A + 2) * v - (A + 3)) * v * v + 1
    w3 = 1 - w0 - w1 - w2
    idx = (fl.long()[:, None] + torch.arange(-1, 3)[None, :]).clamp(0, n - 1)
    return idx, torch.stack([w0, w1, w2, w3], dim=1)


def heatmaps_to_keypoints_torch(maps, boxes):
    """maps [N, K, H, W], boxes [N, 4] xyxy -> (keypoints [N, K, 3], scores [N, K]) on the CPU: per detection the map
    resized to ceil(max(w, 1)) x ceil(max(h, 1)) (horizontal pass, then vertical; every product and sum one fp32 rounding,
    in the kernel's order), the first row-major maximum, and ((x_int + 0.5) * (w / ceil(w)) + x1) in fp64 rounded to fp32."""
    maps, boxes = maps.detach().float().cpu(), boxes.detach().float().cpu()
    N, K, H, W = maps.shape
    kps = torch.zeros((N, K, 3), dtype=torch.float32)
    scores = torch.zeros((N, K), dtype=torch.float32)
    w = torch.clamp(boxes[:, 2] - boxes[:, 0], min=1)
    h = torch.clamp(boxes[:, 3] - boxes[:, 1], min=1)
    wc, hc = w.ceil(), h.ceil()
    for i in range(N):
        ow, oh = int(wc[i]), int(hc[i])
        xi, cx = _cubic_taps(ow, W)
        yi, cy = _cubic_taps(oh, H)
        m = maps[i]
        t = [cx[:, j] * m[:, :, xi[:, j]] for j in range(4)]
        rows = ((t[0] + t[1]) + t[2]) + t[3]                                   # [K, H, ow]
        t = [cy[:, j, None] * rows[:, yi[:, j], :] for j in range(4)]
        full = (((t[0] + t[1]) + t[2]) + t[3]).reshape(K, -1)                # [K, oh * ow]
        pos = full.argmax(dim=1)
        scores[i] = full.gather(1, pos[:, None]).squeeze(1)
        x_int, y_int = pos % ow, pos // ow
        wcorr, hcorr = float(w[i] / wc[i]), float(h[i] / hc[i])
        kps[i, :, 0] = ((x_int.double() + 0.5) * wcorr + float(boxes[i, 0])).float()
        kps[i, :, 1] = ((y_int.double() + 0.5) * hcorr + float(boxes[i, 1])).float()
        kps[i, :, 2] = 1
    return kps, scores


class KeypointPostProcessor(nn.Module):
    def forward(self, x, boxes):
        counts = [len(b) for b in boxes]
        flat = torch.cat([b.convert("xyxy").bbox for b in boxes], dim=0) if boxes else x.new_zeros((0, 4))
        if _C.on_device(x):
            kps, scores = _C.heatmaps_to_keypoints(x, flat)
        else:
            kps, scores = heatmaps_to_keypoints_torch(x, flat)
            kps, scores = kps.to(x.device), scores.to(x.device)
        results = []
        for kp, sc, b in zip(kps.split(counts, dim=0), scores.split(counts, dim=0), boxes):
            out = b.copy_with_fields(b.fields())
            field = PersonKeypoints(kp, b.size)
            field.add_field("logits", sc)
            out.add_field("keypoints", field)
            results.append(out)
        return results


def make_roi_keypoint_post_processor(cfg):
    return KeypointPostProcessor()
