"""The merge of test-time box augmentation as a composition of torch operators: the definition of include/detops.h
(detops_bbox_aug_merge_count / _write) on whatever device the tensors live on.  `_C.bbox_aug_merge` takes it for CPU tensors;
on the device it is the comparison the HIP kernels are tested and measured against.  Eager torch runs one operator per
expression, so nothing is contracted: the same fp32 roundings as the kernel."""
import torch


def group_records(frames, flips):
    """frames: per image the (w, h) of each of its T passes, first pass first; flips: the T flip bits
    -> (group_geom int32 [N*T, 3], group_ratio float32 [N*T, 2]) on the CPU.  The ratio is BoxList.resize's
    float(new) / float(old), rounded to fp32 as torch rounds a Python scalar that multiplies a float32 tensor."""
    geom, ratio = [], []
    for per_image in frames:
        w0, h0 = per_image[0]
        assert len(per_image) == len(flips)
        for (w, h), f in zip(per_image, flips):
            geom.append((int(w), int(h), int(bool(f))))
            ratio.append((float(w0) / float(w), float(h0) / float(h)))
    return (torch.tensor(geom, dtype=torch.int32).reshape(-1, 3),
            torch.tensor(ratio, dtype=torch.float64).to(torch.float32).reshape(-1, 2))


def bbox_aug_merge(boxes, scores, row_offset, group_geom, group_ratio, N, T, score_thresh):
    """boxes [R, 4C], scores [R, C] fp32; row_offset int32 [N*T + 1], group_geom int32 [N*T, 3], group_ratio fp32 [N*T, 2]
    (any device) -> (cand_boxes [M, 4], cand_scores [M], seg_offsets int32 [N*(C-1) + 1], longest segment)"""
    dev = scores.device
    R, C = scores.shape
    G, S = N * T, N * max(C - 1, 0)
    seg_offsets = torch.zeros((S + 1,), dtype=torch.int32, device=dev)
    if R == 0 or S == 0:
        return boxes.new_zeros((0, 4)), scores.new_zeros((0,)), seg_offsets, 0
    row_offset = row_offset.to(dev).long()
    g = torch.repeat_interleave(torch.arange(G, device=dev), row_offset[1:] - row_offset[:-1], output_size=R)
    geom = group_geom.to(dev)[g]
    ratio = group_ratio.to(dev)[g]
    w = geom[:, 0].to(torch.float32)[:, None]
    xhi = (geom[:, 0] - 1).to(torch.float32)
    yhi = (geom[:, 1] - 1).to(torch.float32)
    b = torch.minimum(boxes.view(R, C, 4).clamp(min=0), torch.stack([xhi, yhi, xhi, yhi], 1)[:, None, :])
    flip = (geom[:, 2] & 1).bool()[:, None]
    x1 = torch.where(flip, w - b[..., 2] - 1, b[..., 0])
    x2 = torch.where(flip, w - b[..., 0] - 1, b[..., 2])
    first = (g % T == 0)[:, None]
    rx, ry = ratio[:, 0:1], ratio[:, 1:2]
    b = torch.stack([torch.where(first, x1, x1 * rx), torch.where(first, b[..., 1], b[..., 1] * ry),
                     torch.where(first, x2, x2 * rx), torch.where(first, b[..., 3], b[..., 3] * ry)], dim=-1)
    idx = (scores[:, 1:] > score_thresh).nonzero()               # (row, class - 1), row-major
    seg = (g // T)[idx[:, 0]] * (C - 1) + idx[:, 1]
    order = torch.argsort(seg, stable=True)                      # stable: row order inside a segment
    rows, cols = idx[order, 0], idx[order, 1] + 1
    lengths = torch.bincount(seg, minlength=S)
    seg_offsets[1:] = torch.cumsum(lengths, 0).to(torch.int32)
    return b[rows, cols], scores[rows, cols], seg_offsets, int(lengths.max())
