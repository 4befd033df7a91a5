"""TEST-ONLY: the two ways the `-m "not gpu"` suite runs the detector on CPU tensors.

The product package has no CPU path (its `_C` raises on CPU tensors).  `install()` patches `_C` for the length of a
`with` block, with one of two backends:

  * "oracle": the handful of `_C` entry points the model calls are replaced by stand-ins that run the C oracle
    (oracle/detops_oracle.c) on numpy copies — an independent reference.  The model takes its host branches (proposal
    selection, target assignment, samplers and losses as ATen compositions).
  * "emu-lib": only the library handle under `_C` is swapped, for the host-emulation build of the HIP sources
    (tests/emu); every wrapper, workspace computation, ctypes call and autograd `Function` is the product's own, and
    the model takes its device branches.  `device_branches=False` keeps all of that but makes `_C.on_device` answer
    False: the host branches over the same library.

Nothing outside tests/ imports this module.
"""
import contextlib

import numpy as np
import torch

import oracle
from maskrcnn_benchmark import _C


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _roi_align_forward(input, rois, scale, ph, pw, sr):
    return torch.from_numpy(oracle.roi_align_forward(_np(input.float()), _np(rois.float()), float(scale), ph, pw, sr))


def _roi_align_backward(grad, rois, scale, ph, pw, N, C, H, W, sr):
    return torch.from_numpy(oracle.roi_align_backward(_np(grad.float()), _np(rois.float()), float(scale), ph, pw,
                                                      N, C, H, W, sr))


def _fpn_forward(inputs, rois, scales, ph, pw, sr, k_min, k_max, canonical_scale=224.0, canonical_level=4.0,
                 eps=1e-6, out_channels_last=False):
    r = _np(rois.float())
    lv = oracle.fpn_level(r, k_min, k_max, canonical_scale, canonical_level, eps)
    K, C = r.shape[0], inputs[0].shape[1]
    out = np.zeros((K, C, ph, pw), np.float32)
    for l, (f, s) in enumerate(zip(inputs, scales)):
        sel = np.nonzero(lv == l)[0]
        if sel.size:
            out[sel] = oracle.roi_align_forward(_np(f.float()), r[sel], float(s), ph, pw, sr)
    return torch.from_numpy(out), torch.from_numpy(lv.astype(np.int32))


def _fpn_backward(grad, rois, levels, shapes, scales, ph, pw, sr, prepared=None, channels_last=False):
    r, g, lv = _np(rois.float()), _np(grad.float()), _np(levels)
    outs = []
    for l, (shp, s) in enumerate(zip(shapes, scales)):
        sel = np.nonzero(lv == l)[0]
        N, C, H, W = shp
        if sel.size:
            outs.append(torch.from_numpy(oracle.roi_align_backward(g[sel], r[sel], float(s), ph, pw, N, C, H, W, sr)))
        else:
            outs.append(torch.zeros(shp))
    return outs


def _nms(dets, scores, thr):
    if dets.numel() == 0:
        return torch.empty((0,), dtype=torch.long)
    return torch.from_numpy(oracle.nms(_np(dets.float()), _np(scores.float()), float(thr)).astype(np.int64))


def _nms_batched_mask(boxes, scores, seg_offsets, max_n, thr):
    b, s, seg = _np(boxes.float()), _np(scores.float()), _np(seg_offsets)
    mask = np.zeros(b.shape[0], bool)
    num = np.zeros(len(seg) - 1, np.int32)
    for i in range(len(seg) - 1):
        lo, hi = int(seg[i]), int(seg[i + 1])
        if hi > lo:
            k = oracle.nms(b[lo:hi], s[lo:hi], float(thr))
            mask[lo + k] = True
            num[i] = len(k)
    return torch.from_numpy(mask), torch.from_numpy(num)


def _focal_sum(logits, targets, num_classes, gamma, alpha):
    return torch.from_numpy(oracle.sigmoid_focal_loss_forward(_np(logits.float()), _np(targets), gamma, alpha)).sum()


def _focal_bwd_scalar(logits, targets, d_loss, num_classes, gamma, alpha):
    d = np.full(tuple(logits.shape), float(d_loss), np.float32)
    return torch.from_numpy(oracle.sigmoid_focal_loss_backward(_np(logits.float()), _np(targets), d, gamma, alpha))


def _frozen_bn_fwd(x, scale, bias, residual, relu):
    y = x * scale.reshape(1, -1, 1, 1).to(x.dtype) + bias.reshape(1, -1, 1, 1).to(x.dtype)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


def _frozen_bn_bwd(grad_y, y, scale, relu, need_residual):
    g = grad_y * (y > 0).to(grad_y.dtype) if relu else grad_y
    return g * scale.reshape(1, -1, 1, 1).to(g.dtype), (g.clone() if need_residual else None)


_PATCHES = {
    "frozen_bn_act_forward": _frozen_bn_fwd,
    "frozen_bn_act_backward": _frozen_bn_bwd,
    "roi_align_forward": _roi_align_forward,
    "roi_align_backward": _roi_align_backward,
    "roi_align_fpn_forward": _fpn_forward,
    "roi_align_fpn_backward": _fpn_backward,
    "nms": _nms,
    "nms_batched_mask": _nms_batched_mask,
    "sigmoid_focalloss_forward_sum": _focal_sum,
    "sigmoid_focalloss_backward_scalar": _focal_bwd_scalar,
}


def _emu_lib_patches(device_branches):
    """The PRODUCT's own `_C` wrappers (argument checks, marshalling, workspaces, autograd functions) on CPU tensors: the
    library handle they call is the host-emulation build of the same HIP sources (same C ABI, host pointers), the
    CUDA-only guards are lifted and `on_device` says `device_branches`.  Nothing of `_C`'s operator surface is replaced."""
    import emu

    # emu.lib(): built when needed, bound from the table the device build is bound from (maskrcnn_benchmark/_abi.py)
    return {"lib": emu.lib(), "_need_cuda": lambda name, *tensors: None, "stream_of": lambda t: None,
            "_on_device": lambda t: _C._NOSPAN, "on_device": lambda t: device_branches}


@contextlib.contextmanager
def install(backend="oracle", device_branches=True):
    """backend = "oracle" (the stand-ins of `_PATCHES`; the model takes its host branches) or "emu-lib" (the product's
    own `_C` wrappers over the emulation library, see `_emu_lib_patches`).  `device_branches=False` with "emu-lib": the
    same wrappers and library, but the model takes its host branches (the composite side of the comparison tests)."""
    if backend == "oracle":
        patches = _PATCHES
    elif backend == "emu-lib":
        patches = _emu_lib_patches(device_branches)
    else:
        raise ValueError("unknown cpu_shim backend %r" % (backend,))
    saved = {k: getattr(_C, k) for k in patches}
    try:
        for k, v in patches.items():
            setattr(_C, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(_C, k, v)
