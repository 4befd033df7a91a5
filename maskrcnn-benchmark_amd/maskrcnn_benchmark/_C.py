"""`maskrcnn_benchmark._C` — the reference's native-operator module, re-exported over the C ABI of
libdetops_gfx950.so (include/detops.h).

Same names, argument order and ownership rules as the reference's pybind module
(reference: maskrcnn_benchmark/csrc/vision.cpp:9-25 and the dispatch headers csrc/*.h):

    nms, roi_align_forward, roi_align_backward, roi_pool_forward, roi_pool_backward,
    sigmoid_focalloss_forward, sigmoid_focalloss_backward,
    deform_conv_forward, deform_conv_backward_input, deform_conv_backward_parameters,
    modulated_deform_conv_forward, modulated_deform_conv_backward

    deform_psroi_pooling_forward, deform_psroi_pooling_backward

PyTorch is plumbing here: it owns device memory and the current HIP
stream; every computation happens in the hand-written gfx950 kernels (GEMMs of the deformable
convolution go through torch.addmm -> hipBLASLt/rocBLAS, as the reference's go through cuBLAS).

There is no CPU path: CPU tensors raise "Not implemented on the CPU" (the reference's own message
for its CUDA-only operators, e.g. csrc/ROIAlign.h:44).
"""
import ctypes
import os

import numpy as np
import torch

from . import _eval_cpu, _lib, _rle_cpu
from ._lib import check, lib, ptr, stream_of

# ------------------------------------------------------------------------------------------ helpers


def _need_cuda(name, *tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("%s: Not implemented on the CPU (HIP-only build, no fallback)" % name)


def _f32c(name, t):
    if t.dtype != torch.float32:
        raise RuntimeError("%s: expected a float32 tensor, got %s" % (name, t.dtype))
    return t.contiguous()


def on_device(t):
    """True when `t` takes the HIP operators of this module (the model code asks this instead of `t.is_cuda`, so the
    host-emulation tests can drive the same branches with CPU tensors)."""
    return t.is_cuda


def _u8(name, t):
    """bool / uint8 mask -> contiguous uint8 (a bool tensor is reinterpreted, not converted: no launch)."""
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    if t.dtype != torch.uint8:
        raise RuntimeError("%s: expected a bool or uint8 mask, got %s" % (name, t.dtype))
    return t.contiguous()


def _on_device(t):
    """Context: `t`'s device is current for the launch (a shared no-op object in the usual case — the tensor lives
    on the current device — so the launch path allocates nothing)."""
    idx = t.device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NOSPAN
    return torch.cuda.device(idx)


class KernelTimer(object):
    """Optional per-entry-point timing with HIP events recorded on the launch stream (the current
    torch stream of the tensor's device).  bench.py installs one to measure the hand-written
    kernels live inside the timed region; `results()` must be called after a device sync.
    High-frequency entry points (FrozenBN: ~100 launches per step) are SAMPLED — every `every`-th call of a name
    gets an event pair, all calls are counted — so that the timer's own host cost stays out of the step."""

    def __init__(self, every_cap=None, strides=None, count_only=False):
        self.pairs = {}
        self.calls = {}
        self.every_cap = every_cap     # upper bound on the sampling stride (short runs: enough samples per name)
        self.strides = strides or {}   # per-name sampling stride (bench.py: from the call counts of a warm-up step, so
        self.count_only = count_only   # that every name gets ~12 event pairs over the timed steps and no more: a timed
                                       # launch costs ~30-100 us of device time — the event records drain the queue)

    def span(self, name, t, every=1):
        """`name`: a string or (format, args) — kept as the key and formatted in results() (no string work per launch)"""
        n = self.calls.get(name, 0)
        self.calls[name] = n + 1
        if self.count_only:
            return _NOSPAN
        stride = self.strides.get(name)
        if stride is not None:
            every = stride
        elif self.every_cap is not None and every > self.every_cap:
            every = self.every_cap
        return _Span(self, name, t) if n % every == 0 else _NOSPAN

    def results(self):
        """name -> (calls, timed launches, total_ms of the timed launches)"""
        out = {}
        for name, pairs in self.pairs.items():
            text = name[0] % name[1] if type(name) is tuple else name
            out[text] = (self.calls.get(name, len(pairs)), len(pairs), sum(a.elapsed_time(b) for a, b in pairs))
        return out


class _Span(object):
    def __init__(self, timer, name, t):
        self.timer, self.name, self.t = timer, name, t

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record(torch.cuda.current_stream(self.t.device))

    def __exit__(self, *exc):
        self.b.record(torch.cuda.current_stream(self.t.device))
        self.timer.pairs.setdefault(self.name, []).append((self.a, self.b))


class _NoSpan(object):
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NOSPAN = _NoSpan()
KERNEL_TIMER = None  # set to a KernelTimer to collect timings


def _timed(name, t, every=1):
    """`name`: a string, or (format, args) — formatted only when a timer is installed (the launch path of an
    untimed run does no string work)"""
    if KERNEL_TIMER is None:
        return _NOSPAN
    return KERNEL_TIMER.span(name, t, every)


_ESIZE = {torch.float32: 4, torch.float16: 2, torch.bfloat16: 2}


# ------------------------------------------------------------------------------------------ double precision
# The reference dispatches its operators over float AND double (AT_DISPATCH_FLOATING_TYPES).  float64 tensors take the plain
# kernels of csrc/f64_ops.hip (device) / csrc/cpu_branch.hip (CPU tensors: nms, roi_align_forward); everything tuned in this
# library is fp32.
def _f64(t):
    return t is not None and t.dtype == torch.float64


def _f64c(name, *ts):
    for t in ts:
        if t.dtype != torch.float64:
            raise RuntimeError("%s: all floating-point tensors must be float64 (got %s)" % (name, t.dtype))
    return [t.contiguous() for t in ts]


def _nms_f64(dets, scores, threshold):
    dets, scores = _f64c("nms", dets, scores)
    n = dets.size(0)
    if dets.dim() != 2 or dets.size(1) != 4 or scores.numel() != n:
        raise RuntimeError("nms: expected dets [n,4] and scores [n]")
    if not on_device(dets):
        keep = torch.empty((n,), dtype=torch.long)
        num = torch.zeros((1,), dtype=torch.int32)
        check(lib.detops_nms_cpu_f64(ptr(dets), ptr(scores), n, float(threshold), ptr(keep), ptr(num)), "nms(cpu, f64)")
        return keep[: int(num.item())]
    _need_cuda("nms", dets, scores)
    order = torch.sort(scores, descending=True, stable=True).indices       # ties: ascending index, like the CPU path
    sorted_boxes = dets[order].contiguous()
    kept = torch.empty((n,), dtype=torch.uint8, device=dets.device)
    nbytes = int(lib.detops_nms_sorted_f64_workspace_bytes(n))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dets.device)
    with _on_device(dets):
        check(lib.detops_nms_sorted_f64(ptr(sorted_boxes), n, float(threshold), ptr(kept), ptr(ws), nbytes, stream_of(dets)), "nms(f64)")
    return torch.sort(order[kept.bool()]).values       # ascending original indices = nonzero(suppressed == 0)


def _roi_align_forward_f64(input, rois, spatial_scale, ph, pw, sr):
    input, rois = _f64c("roi_align_forward", input, rois)
    N, C, H, W = input.shape
    K = rois.size(0)
    out = torch.empty((K, C, ph, pw), dtype=torch.float64, device=input.device)
    if out.numel() == 0:
        return out
    if not on_device(input):
        check(lib.detops_roi_align_forward_cpu_f64(ptr(input), ptr(rois), ptr(out), N, C, H, W, K, ph, pw, float(spatial_scale), int(sr)),
              "roi_align_forward(cpu, f64)")
        return out
    _need_cuda("roi_align_forward", input, rois)
    with _on_device(input):
        check(lib.detops_roi_align_forward_f64(ptr(input), ptr(rois), ptr(out), N, C, H, W, K, ph, pw, float(spatial_scale), int(sr),
                                               stream_of(input)), "roi_align_forward(f64)")
    return out


def _roi_align_backward_f64(grad, rois, spatial_scale, ph, pw, N, C, H, W, sr):
    _need_cuda("roi_align_backward", grad, rois)
    grad, rois = _f64c("roi_align_backward", grad, rois)
    gin = torch.empty((N, C, H, W), dtype=torch.float64, device=grad.device)
    with _on_device(grad):
        check(lib.detops_roi_align_backward_f64(ptr(grad), ptr(rois), ptr(gin), N, C, H, W, rois.size(0), ph, pw, float(spatial_scale),
                                                int(sr), 1, stream_of(grad)), "roi_align_backward(f64)")
    return gin


def _roi_pool_forward_f64(input, rois, spatial_scale, ph, pw):
    _need_cuda("roi_pool_forward", input, rois)
    input, rois = _f64c("roi_pool_forward", input, rois)
    N, C, H, W = input.shape
    K = rois.size(0)
    out = torch.empty((K, C, ph, pw), dtype=torch.float64, device=input.device)
    argmax = torch.zeros((K, C, ph, pw), dtype=torch.int32, device=input.device)
    if out.numel():
        with _on_device(input):
            check(lib.detops_roi_pool_forward_f64(ptr(input), ptr(rois), ptr(out), ptr(argmax), N, C, H, W, K, ph, pw, float(spatial_scale),
                                                  stream_of(input)), "roi_pool_forward(f64)")
    return out, argmax


def _roi_pool_backward_f64(grad, rois, argmax, ph, pw, N, C, H, W):
    _need_cuda("roi_pool_backward", grad, rois, argmax)
    grad, rois = _f64c("roi_pool_backward", grad, rois)
    argmax = argmax.contiguous()
    gin = torch.empty((N, C, H, W), dtype=torch.float64, device=grad.device)
    with _on_device(grad):
        check(lib.detops_roi_pool_backward_f64(ptr(grad), ptr(rois), ptr(argmax), ptr(gin), N, C, H, W, rois.size(0), ph, pw, 1,
                                               stream_of(grad)), "roi_pool_backward(f64)")
    return gin


def _focal_f64(logits, targets, d_losses, num_classes, gamma, alpha):
    _need_cuda("sigmoid_focalloss", logits, targets)
    (logits,) = _f64c("sigmoid_focalloss", logits)
    if logits.dim() != 2:
        raise RuntimeError("logits should be NxClass")
    if targets.dim() != 1:
        raise RuntimeError("targets should be Nx1")
    R, Cc = logits.shape
    if Cc != num_classes or targets.numel() != R:
        raise RuntimeError("sigmoid_focalloss: inconsistent shapes")
    t32 = targets.to(torch.int32).contiguous()
    out = torch.empty_like(logits)
    with _on_device(logits):
        if d_losses is None:
            check(lib.detops_sigmoid_focal_loss_forward_f64(ptr(logits), ptr(t32), ptr(out), R, Cc, float(gamma), float(alpha),
                                                            stream_of(logits)), "sigmoid_focalloss_forward(f64)")
        else:
            (d_losses,) = _f64c("sigmoid_focalloss_backward", d_losses)
            check(lib.detops_sigmoid_focal_loss_backward_f64(ptr(logits), ptr(t32), ptr(d_losses), ptr(out), R, Cc, float(gamma),
                                                             float(alpha), stream_of(logits)), "sigmoid_focalloss_backward(f64)")
    return out


# ------------------------------------------------------------------------------------------ NMS
def nms(dets, scores, threshold):
    """reference csrc/nms.h:10-28: dets [n,4] xyxy, scores [n] -> int64 kept indices, ascending.
    CPU semantics (IoU >= threshold suppresses; csrc/cpu/nms_cpu.cpp:60)."""
    if dets.numel() == 0:  # nms.h:17-18 returns an empty CPU long tensor
        return torch.empty((0,), dtype=torch.long, device="cpu")
    if _f64(dets):
        return _nms_f64(dets, scores, threshold)
    on_cpu = not on_device(dets) and not on_device(scores)
    if not on_cpu:
        _need_cuda("nms", dets, scores)
    dets = _f32c("nms", dets)
    scores = _f32c("nms", scores)
    n = dets.size(0)
    if dets.dim() != 2 or dets.size(1) != 4 or scores.numel() != n:
        raise RuntimeError("nms: expected dets [n,4] and scores [n]")
    if on_cpu:  # the reference dispatches CPU tensors to nms_cpu (csrc/nms.h:26-27); host code of the same library
        keep = torch.empty((n,), dtype=torch.long)
        num = torch.zeros((1,), dtype=torch.int32)
        check(lib.detops_nms_cpu_f32(ptr(dets), ptr(scores), n, float(threshold), ptr(keep), ptr(num)), "nms(cpu)")
        return keep[: int(num.item())]
    keep = torch.empty((n,), dtype=torch.long, device=dets.device)
    num = torch.empty((1,), dtype=torch.int32, device=dets.device)
    ws_bytes = lib.detops_nms_workspace_bytes(n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dets.device)
    with _on_device(dets):
        check(lib.detops_nms_f32(ptr(dets), ptr(scores), n, float(threshold), ptr(keep), ptr(num),
                                 ptr(ws), ws_bytes, stream_of(dets)), "nms")
    k = int(num.item())  # the variable-length return value forces one readback
    if k < 0:
        raise RuntimeError("nms: a device-side wait of the single-launch kernel timed out (num_keep = -1): the GPU's "
                           "compute units were held by other work for seconds; no result was produced")
    return keep[:k]


_NMS_STATUS = {}


def nms_status(device):
    """The sticky device word (int32 [1]) the segmented NMS entry points pass to the library: incremented once for every
    segment the single-launch kernel gave up on and the repair launch redid (include/detops.h,
    detops_nms_batched_status_f32).  One per device, never cleared by the library, never read by the launch path."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else 0))
    t = _NMS_STATUS.get(key)
    if t is None:
        t = _NMS_STATUS[key] = torch.zeros((1,), dtype=torch.int32, device=device)
    return t


def nms_repaired_segments(device=None, reset=False):
    """Host-side read of the status words (a device->host copy: call it where a read-back happens anyway, e.g. with the
    logged losses).  Returns the number of NMS segments redone by the repair launch since the last reset."""
    total = 0
    for (typ, idx), t in list(_NMS_STATUS.items()):
        if device is not None and torch.device(device).type != typ:
            continue
        total += int(t.item())
        if reset:
            t.zero_()
    return total


def nms_batched(boxes, scores, seg_offsets, max_n, threshold):
    """Sync-free segmented NMS (extension; not in the reference `_C`).
    boxes [T,4], scores [T], seg_offsets int32 [S+1] (device).  Returns (keep [T] int64 with each
    segment's LOCAL kept indices packed at its offset, num_keep [S] int32) — all on device.
    A segment the single launch gives up on (starved producer workgroup) is redone by the library's repair launch on the
    same stream and counted in `nms_status(device)`: callers may ignore num_keep without ever losing a segment."""
    _need_cuda("nms_batched", boxes, scores, seg_offsets)
    boxes = _f32c("nms_batched", boxes)
    scores = _f32c("nms_batched", scores)
    S = seg_offsets.numel() - 1
    keep = torch.empty((boxes.size(0),), dtype=torch.long, device=boxes.device)
    num = torch.zeros((max(S, 0),), dtype=torch.int32, device=boxes.device)
    if S <= 0 or boxes.size(0) == 0:
        return keep, num
    seg_offsets = seg_offsets.to(torch.int32).contiguous()
    ws_bytes = lib.detops_nms_batched_workspace_bytes(S, int(max_n))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=boxes.device)
    with _on_device(boxes):
        check(lib.detops_nms_batched_status_f32(ptr(boxes), ptr(scores), ptr(seg_offsets), S, int(max_n),
                                                float(threshold), ptr(keep), None, ptr(num),
                                                ptr(nms_status(boxes.device)), ptr(ws), ws_bytes,
                                                stream_of(boxes)), "nms_batched")
    return keep, num


def nms_batched_mask(boxes, scores, seg_offsets, max_n, threshold):
    """Sync-free segmented NMS, dense form (extension): returns (keep_mask [T] bool,
    num_keep [S] int32), keep_mask in the ORIGINAL row order of `boxes`."""
    _need_cuda("nms_batched_mask", boxes, scores, seg_offsets)
    boxes = _f32c("nms_batched_mask", boxes)
    scores = _f32c("nms_batched_mask", scores)
    S = seg_offsets.numel() - 1
    mask = torch.zeros((boxes.size(0),), dtype=torch.uint8, device=boxes.device)
    num = torch.zeros((max(S, 0),), dtype=torch.int32, device=boxes.device)
    if S <= 0 or boxes.size(0) == 0:
        return mask.bool(), num
    if seg_offsets.dtype != torch.int32:
        seg_offsets = seg_offsets.to(torch.int32)
    seg_offsets = seg_offsets.contiguous()
    ws_bytes = lib.detops_nms_batched_workspace_bytes(S, int(max_n))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=boxes.device)
    with _on_device(boxes), _timed(("nms_batched[S=%d,max_n=%d]", (S, int(max_n))), boxes):
        check(lib.detops_nms_batched_status_f32(ptr(boxes), ptr(scores), ptr(seg_offsets), S, int(max_n),
                                                float(threshold), None, ptr(mask), ptr(num),
                                                ptr(nms_status(boxes.device)), ptr(ws), ws_bytes,
                                                stream_of(boxes)), "nms_batched_mask")
    return mask.view(torch.bool), num


# ------------------------------------------------------------------------------------------ FPN top-down step
class _UpsampleAdd(torch.autograd.Function):
    """lateral + nearest_upsample(top) in one pass (csrc/fpn_topdown.hip; reference modeling/backbone/fpn.py:59-64).
    A channels-last lateral selects the NHWC kernels and returns channels-last tensors in both directions."""

    @staticmethod
    def forward(ctx, lateral, top):
        nhwc = is_channels_last(lateral)
        fmt = torch.channels_last if nhwc else torch.contiguous_format
        lateral, top = lateral.contiguous(memory_format=fmt), top.contiguous(memory_format=fmt)
        N, C, H, W = lateral.shape
        h, w = int(top.shape[2]), int(top.shape[3])
        out = torch.empty_like(lateral)
        with _on_device(lateral), _timed(("fpn_topdown_fwd[n=%d,e=%d]", (lateral.numel(), _ESIZE[lateral.dtype])), lateral):
            if nhwc:
                check(lib.detops_fpn_topdown_forward_nhwc(ptr(lateral), ptr(top), ptr(out), _lib.DTYPE_CODE[lateral.dtype], N, C, H, W,
                                                          h, w, stream_of(lateral)), "fpn_topdown_forward_nhwc")
            else:
                check(lib.detops_fpn_topdown_forward(ptr(lateral), ptr(top), ptr(out), _lib.DTYPE_CODE[lateral.dtype], N * C, H, W, h, w,
                                                     stream_of(lateral)), "fpn_topdown_forward")
        ctx.shape = (N, C, H, W, h, w)
        ctx.nhwc = nhwc
        return out

    @staticmethod
    def backward(ctx, g):
        N, C, H, W, h, w = ctx.shape
        fmt = torch.channels_last if ctx.nhwc else torch.contiguous_format
        g = g.contiguous(memory_format=fmt)
        gtop = None
        if ctx.needs_input_grad[1]:
            gtop = torch.empty((N, C, h, w), dtype=g.dtype, device=g.device, memory_format=fmt)
            with _on_device(g), _timed(("fpn_topdown_bwd[n=%d,e=%d]", (g.numel(), _ESIZE[g.dtype])), g):
                if ctx.nhwc:
                    check(lib.detops_fpn_topdown_backward_nhwc(ptr(g), ptr(gtop), _lib.DTYPE_CODE[g.dtype], N, C, H, W, h, w,
                                                               stream_of(g)), "fpn_topdown_backward_nhwc")
                else:
                    check(lib.detops_fpn_topdown_backward(ptr(g), ptr(gtop), _lib.DTYPE_CODE[g.dtype], N * C, H, W, h, w, stream_of(g)),
                          "fpn_topdown_backward")
        return (g if ctx.needs_input_grad[0] else None), gtop


def fpn_topdown(lateral, top):
    """out = lateral + F.interpolate(top, size=lateral.shape[-2:], mode="nearest") (extension; the reference composes it from
    two ATen ops, modeling/backbone/fpn.py:59-64).  [N, C, H, W] + [N, C, h, w], one dtype (fp32 / fp16 / bf16)."""
    _need_cuda("fpn_topdown", lateral, top)
    if lateral.dtype != top.dtype or lateral.dtype not in _lib.DTYPE_CODE:
        raise RuntimeError("fpn_topdown: lateral and top must share one dtype (fp32 / fp16 / bf16)")
    if lateral.dim() != 4 or top.dim() != 4 or lateral.shape[:2] != top.shape[:2]:
        raise RuntimeError("fpn_topdown: expected [N, C, H, W] and [N, C, h, w]")
    return _UpsampleAdd.apply(lateral, top)


# ------------------------------------------------------------------------------------------ data-parallel bucket kernels
_PACK_MAX = [0]


def pack_into(dst, tensors, offsets, stream=None):
    """dst (flat fp32) [offsets[i] : offsets[i] + tensors[i].numel()] = tensors[i] — the gradients of a bucket in ONE launch
    per 48 tensors (csrc/optim.hip; reference: DistributedDataParallel's bucket copies, tools/train_net.py:45-54).
    `stream`: a torch.cuda stream (default: the current one)."""
    _need_cuda("pack_into", dst, *tensors)
    if not _PACK_MAX[0]:
        _PACK_MAX[0] = int(lib.detops_pack_max_tensors())
    if dst.dtype != torch.float32 or not dst.is_contiguous():
        raise RuntimeError("pack_into: a contiguous fp32 destination is required")
    st = stream_of(dst) if stream is None else stream.cuda_stream
    n_all = len(tensors)
    with _on_device(dst):
        for i0 in range(0, n_all, _PACK_MAX[0]):
            part = list(tensors[i0:i0 + _PACK_MAX[0]])
            n = len(part)
            srcs = (ctypes.c_void_p * n)()
            cnts = (ctypes.c_int64 * n)()
            offs = (ctypes.c_int64 * n)()
            for j, t in enumerate(part):
                if t.dtype != torch.float32 or t.device != dst.device:
                    raise RuntimeError("pack_into: fp32 tensors on the destination's device are required")
                if not t.is_contiguous():
                    t = t.contiguous()
                    part[j] = t          # keep the copy alive until the launch is enqueued
                srcs[j], cnts[j], offs[j] = t.data_ptr(), t.numel(), int(offsets[i0 + j])
                if offs[j] < 0 or offs[j] + cnts[j] > dst.numel():
                    raise RuntimeError("pack_into: slice %d leaves the destination" % (i0 + j))
            check(lib.detops_pack_f32(srcs, cnts, offs, n, ptr(dst), st), "pack_f32")
    return dst


def sgd_momentum_flat_(params, grads, momentum_buf, split, lr_weights, wd_weights, lr_biases, wd_biases, momentum, stream=None):
    """torch.optim.SGD(momentum, dampening 0) over a whole flat bucket in one pass (csrc/optim.hip; reference
    solver/build.py:7-20 + engine/trainer.py:98 `optimizer.step()`): elements [0, split) take the weights' (lr, wd), the
    rest the biases'.  In place on `params` and `momentum_buf`."""
    _need_cuda("sgd_momentum_flat_", params, grads, momentum_buf)
    for t in (params, grads, momentum_buf):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != params.numel():
            raise RuntimeError("sgd_momentum_flat_: three contiguous fp32 arrays of one length are required")
    st = stream_of(params) if stream is None else stream.cuda_stream
    with _on_device(params):
        check(lib.detops_sgd_momentum_flat_f32(ptr(params), ptr(grads), ptr(momentum_buf), params.numel(), int(split),
                                               float(lr_weights), float(wd_weights), float(lr_biases), float(wd_biases),
                                               float(momentum), st), "sgd_momentum_flat")
    return params


# ------------------------------------------------------------------------------------------ RPN loss
class _RpnLoss(torch.autograd.Function):
    """Fused RPN loss (extension; reference modeling/rpn/loss.py:92-127): one launch evaluates both losses from the
    per-level head outputs and stores d(loss sum)/d(logit) in the same layouts; backward = one scaling launch."""

    @staticmethod
    def forward(ctx, anchors, matched, pos, neg, gt, beta, weights, A, L, *heads):
        obj, box = list(heads[:L]), list(heads[L:])
        N = obj[0].size(0)
        T, M = anchors.size(0), gt.size(1)
        gobj = [torch.empty_like(t) for t in obj]
        gbox = [torch.empty_like(t) for t in box]
        out3 = torch.empty((3,), dtype=torch.float32, device=anchors.device)
        nbytes = int(lib.detops_rpn_loss_workspace_bytes())
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=anchors.device)
        Hs = (ctypes.c_int * L)(*[t.size(2) for t in obj])
        Ws = (ctypes.c_int * L)(*[t.size(3) for t in obj])
        arr = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
        w4 = (ctypes.c_float * 4)(*[float(w) for w in weights])
        with _on_device(anchors), _timed(("rpn_loss[N=%d,T=%d]", (N, T)), anchors):
            check(lib.detops_rpn_loss_f32(arr(obj), arr(box), Hs, Ws, L, int(A), ptr(anchors), ptr(matched), ptr(pos),
                                          ptr(neg), ptr(gt), N, M, T, float(beta), w4, arr(gobj), arr(gbox), ptr(out3),
                                          ptr(ws), nbytes, stream_of(anchors)), "rpn_loss")
        ctx.grads, ctx.out3, ctx.meta = (gobj, gbox), out3, (L, int(A), N, T, Hs, Ws)
        ctx.mark_non_differentiable(out3)
        return out3[0], out3[1], out3

    @staticmethod
    def backward(ctx, g_obj, g_box, _unused):
        gobj, gbox = ctx.grads
        L, A, N, T, Hs, Ws = ctx.meta
        if gobj is None:
            raise RuntimeError("rpn_loss: backward called twice (the stored gradients are scaled in place)")
        up_o = (g_obj if g_obj is not None else torch.zeros((), device=ctx.out3.device)).reshape(1).float().contiguous()
        up_b = (g_box if g_box is not None else torch.zeros((), device=ctx.out3.device)).reshape(1).float().contiguous()
        arr = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
        with _on_device(ctx.out3):
            check(lib.detops_rpn_loss_backward_f32(arr(gobj), arr(gbox), Hs, Ws, L, A, N, T, ptr(up_o), ptr(up_b),
                                                   ptr(ctx.out3[2:]), stream_of(ctx.out3)), "rpn_loss_backward")
        ctx.grads = (None, None)
        return (None,) * 9 + tuple(gobj) + tuple(gbox)


def rpn_loss(objectness, box_regression, anchors, matched_idxs, pos_mask, neg_mask, gt_boxes, beta, weights):
    """objectness / box_regression: per-level lists [N, A, H, W] / [N, 4A, H, W] (fp32, contiguous); anchors [T, 4];
    matched_idxs [N, T] int64; pos_mask / neg_mask [N, T] bool; gt_boxes [N, M, 4] -> (objectness_loss, box_loss)."""
    _need_cuda("rpn_loss", anchors, matched_idxs, pos_mask, neg_mask, gt_boxes, *objectness, *box_regression)
    L = len(objectness)
    A = box_regression[0].size(1) // 4
    heads = [_f32c("rpn_loss", t) for t in list(objectness) + list(box_regression)]
    as_u8 = lambda m: (m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)).contiguous()
    lo, lb, _ = _RpnLoss.apply(_f32c("rpn_loss", anchors), matched_idxs.to(torch.int64).contiguous(), as_u8(pos_mask),
                               as_u8(neg_mask), _f32c("rpn_loss", gt_boxes), float(beta), tuple(weights), A, L, *heads)
    return lo, lb


# ------------------------------------------------------------------------------------------ ROI-head losses
class _HeadLoss(torch.autograd.Function):
    """Shared autograd glue of the fused ROI-head losses (csrc/head_loss.hip): forward stores d loss / d input next to the
    values, backward scales the stored gradients by the upstream scalars in one launch."""

    @staticmethod
    def forward(ctx, kind, aux, *inputs):
        grads, out = _HEAD_LOSS[kind](aux, *inputs)
        ctx.grads, ctx.n_in = grads, len(inputs)
        return tuple(out[i] for i in range(out.numel()))

    @staticmethod
    def backward(ctx, *ups):
        grads = ctx.grads
        if grads is None:
            raise RuntimeError("head loss: backward called twice (the stored gradients are scaled in place)")
        dev = grads[0].device
        up = [(u if u is not None else torch.zeros((), device=dev)).reshape(1).float().contiguous() for u in ups]
        a, b = grads[0], (grads[1] if len(grads) > 1 else None)
        with _on_device(a):
            check(lib.detops_head_loss_backward_f32(ptr(a), a.numel(), ptr(up[0]), ptr(b), b.numel() if b is not None else 0,
                                                    ptr(up[1]) if b is not None else None, stream_of(a)), "head_loss_backward")
        ctx.grads = None
        return (None, None) + tuple(grads) + (None,) * (ctx.n_in - len(grads))


def _fastrcnn_loss_forward(aux, class_logits, box_regression, labels, regression_targets):
    cls_agnostic, beta = aux
    R, C = class_logits.shape
    D = box_regression.size(1)
    dev = class_logits.device
    gl, gb = torch.empty_like(class_logits), torch.empty_like(box_regression)
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    nbytes = int(lib.detops_fastrcnn_loss_workspace_bytes(R))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with _on_device(class_logits), _timed(("fastrcnn_loss[R=%d,C=%d]", (R, C)), class_logits):
        check(lib.detops_fastrcnn_loss_f32(ptr(class_logits), ptr(box_regression), ptr(labels), ptr(regression_targets), R, C, D,
                                           int(bool(cls_agnostic)), float(beta), ptr(gl), ptr(gb), ptr(out), ptr(ws), nbytes,
                                           stream_of(class_logits)), "fastrcnn_loss")
    return (gl, gb), out


def _mask_loss_forward(aux, mask_logits, labels, mask_targets):
    P, C, M, _ = mask_logits.shape
    dev = mask_logits.device
    g = torch.empty_like(mask_logits)
    out = torch.empty((1,), dtype=torch.float32, device=dev)
    nbytes = int(lib.detops_mask_loss_workspace_bytes(P))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with _on_device(mask_logits), _timed(("mask_loss[P=%d,C=%d,M=%d]", (P, C, M)), mask_logits):
        check(lib.detops_mask_loss_f32(ptr(mask_logits), ptr(labels), ptr(mask_targets), P, C, M, ptr(g), ptr(out), ptr(ws), nbytes,
                                       stream_of(mask_logits)), "mask_loss")
    return (g,), out


def _strides4(t):
    return (ctypes.c_int64 * 4)(*t.stride())


def _keypoint_loss_forward(aux, logits, heatmaps, valid):
    P, K, H, W = logits.shape
    dev = logits.device
    g = torch.empty_like(logits)
    out = torch.empty((1,), dtype=torch.float32, device=dev)
    nbytes = int(lib.detops_keypoint_loss_workspace_bytes(P, K))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with _on_device(logits), _timed(("keypoint_loss[P=%d,K=%d,M=%d]", (P, K, H)), logits):
        check(lib.detops_keypoint_loss_f32(ptr(logits), _strides4(logits), ptr(heatmaps), ptr(valid), P, K, H, W, ptr(g),
                                           _strides4(g), ptr(out), ptr(ws), nbytes, stream_of(logits)), "keypoint_loss")
    return (g,), out


_HEAD_LOSS = {"fastrcnn": _fastrcnn_loss_forward, "mask": _mask_loss_forward, "keypoint": _keypoint_loss_forward}


def fastrcnn_loss(class_logits, box_regression, labels, regression_targets, cls_agnostic=False, beta=1.0):
    """Box-head loss, value + gradient in one pass (extension; reference roi_heads/box_head/loss.py:140-193):
    class_logits [R,C], box_regression [R,4C] (or [R,>=8] class-agnostic), labels [R] int64 (-1 = not sampled),
    regression_targets [R,4] -> (classification_loss, box_loss), both / max(#sampled, 1)."""
    _need_cuda("fastrcnn_loss", class_logits, box_regression, labels, regression_targets)
    class_logits, box_regression = _f32c("fastrcnn_loss", class_logits), _f32c("fastrcnn_loss", box_regression)
    regression_targets = _f32c("fastrcnn_loss", regression_targets)
    labels = labels.to(torch.int64).contiguous()
    R, C = class_logits.shape
    D = box_regression.size(1)
    if R == 0 or labels.shape != (R,) or regression_targets.shape != (R, 4) or box_regression.size(0) != R \
            or (D < 8 if cls_agnostic else D != 4 * C):
        raise ValueError("fastrcnn_loss: inconsistent arguments")
    return _HeadLoss.apply("fastrcnn", (bool(cls_agnostic), float(beta)), class_logits, box_regression, labels,
                           regression_targets)


def mask_loss(mask_logits, labels, mask_targets):
    """Mask-head loss, value + gradient in one pass (extension; reference roi_heads/mask_head/loss.py:113-143):
    mask_logits [P,C,M,M], labels [P] int64 (> 0 = positive), mask_targets [P,M,M] -> mean BCE-with-logits of the
    positives' class planes (0 without positives)."""
    _need_cuda("mask_loss", mask_logits, labels, mask_targets)
    mask_logits, mask_targets = _f32c("mask_loss", mask_logits), _f32c("mask_loss", mask_targets)
    labels = labels.to(torch.int64).contiguous()
    P, C, M, M2 = mask_logits.shape
    if P == 0 or M != M2 or labels.shape != (P,) or mask_targets.shape != (P, M, M):
        raise ValueError("mask_loss: inconsistent arguments")
    return _HeadLoss.apply("mask", None, mask_logits, labels, mask_targets)[0]


def keypoint_loss(keypoint_logits, heatmaps, valid):
    """Keypoint-head loss, value + gradient in one pass (extension; reference roi_heads/keypoint_head/loss.py:145-169):
    keypoint_logits [P,K,H,W] fp32 (NCHW or channels-last: read through its strides, no copy), heatmaps [P,K] int64 target
    pixel, valid [P,K] bool -> mean softmax cross-entropy of the valid rows (0 without valid rows; the count never leaves
    the device)."""
    _need_cuda("keypoint_loss", keypoint_logits, heatmaps, valid)
    if keypoint_logits.dtype != torch.float32:
        raise RuntimeError("keypoint_loss: expected a float32 tensor, got %s" % keypoint_logits.dtype)
    P, K, H, W = keypoint_logits.shape
    if P == 0 or heatmaps.shape != (P, K) or valid.shape != (P, K):
        raise ValueError("keypoint_loss: inconsistent arguments")
    heatmaps = heatmaps.to(torch.int64).contiguous()
    return _HeadLoss.apply("keypoint", None, keypoint_logits, heatmaps, _u8("keypoint_loss", valid))[0]


def keypoint_targets(boxes, matched, labels, gt_boxes, gt_keypoints, heatmap_size):
    """Keypoint-head targets of every slot of the batch in one launch (extension; reference
    roi_heads/keypoint_head/loss.py:79-100 + structures/keypoint.py:154-188): boxes [P,4] xyxy, matched [P] int64 (row of
    gt_boxes [G,4] / gt_keypoints [G,K,3], global across the images, < 0 = none), labels [P] int64 -> (heatmaps [P,K] int64,
    valid [P,K] bool), bit-equal to the torch formulation."""
    _need_cuda("keypoint_targets", boxes, matched, labels, gt_boxes, gt_keypoints)
    boxes, gt_boxes = _f32c("keypoint_targets", boxes), _f32c("keypoint_targets", gt_boxes)
    gt_keypoints = _f32c("keypoint_targets", gt_keypoints)
    matched, labels = matched.to(torch.int64).contiguous(), labels.to(torch.int64).contiguous()
    P, (G, K, _) = boxes.shape[0], gt_keypoints.shape
    M = int(heatmap_size)
    heat = torch.empty((P, K), dtype=torch.int64, device=boxes.device)
    valid = torch.empty((P, K), dtype=torch.uint8, device=boxes.device)
    if P:
        with _on_device(boxes), _timed(("keypoint_targets[P=%d,K=%d,M=%d]", (P, K, M)), boxes):
            check(lib.detops_keypoint_targets(ptr(boxes), ptr(matched), ptr(labels), ptr(gt_boxes), ptr(gt_keypoints), P, G, K,
                                              M, ptr(heat), ptr(valid), stream_of(boxes)), "keypoint_targets")
    return heat, valid.view(torch.bool)


def heatmaps_to_keypoints(heatmaps, boxes):
    """Keypoint decoding of every detection of the batch (extension; reference roi_heads/keypoint_head/inference.py:40-94):
    heatmaps [N,K,H,W] (any strides), boxes [N,4] xyxy -> (keypoints [N,K,3] = (x, y, 1), scores [N,K]); the bicubic
    resize to the box size is evaluated in place, never stored."""
    _need_cuda("heatmaps_to_keypoints", heatmaps, boxes)
    heatmaps, boxes = heatmaps.float(), _f32c("heatmaps_to_keypoints", boxes)
    N, K, H, W = heatmaps.shape
    kps = torch.empty((N, K, 3), dtype=torch.float32, device=boxes.device)
    scores = torch.empty((N, K), dtype=torch.float32, device=boxes.device)
    if N:
        with _on_device(boxes), _timed(("heatmaps_to_keypoints[N=%d,K=%d]", (N, K)), boxes):
            check(lib.detops_heatmaps_to_keypoints_f32(ptr(heatmaps), _strides4(heatmaps), ptr(boxes), N, K, H, W, ptr(kps),
                                                       ptr(scores), stream_of(boxes)), "heatmaps_to_keypoints")
    return kps, scores


# ------------------------------------------------------------------------------------------ masks at inference
def _paste_args(name, masks, boxes, sizes, counts):
    """-> (masks [N,M,M] contiguous, boxes [N,4] fp32, per-image (H, W) list, per-image detection counts)"""
    _need_cuda(name, masks, boxes)
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    if masks.dim() != 3 or masks.shape[1] != masks.shape[2]:
        raise ValueError("%s: masks must be [N, 1, M, M] or [N, M, M], got %s" % (name, tuple(masks.shape)))
    if masks.dtype not in _lib.DTYPE_CODE:
        masks = masks.float()
    sizes = [(int(h), int(w)) for h, w in sizes]
    counts = [1] * len(sizes) if counts is None else [int(c) for c in counts]
    N = masks.shape[0]
    if len(counts) != len(sizes) or sum(counts) != N or tuple(boxes.shape) != (N, 4) or min(counts, default=0) < 0 \
            or any(h < 0 or w < 0 or h * w >= 2 ** 31 for h, w in sizes):
        raise ValueError("%s: inconsistent arguments" % name)
    return masks.contiguous(), _f32c(name, boxes), sizes, counts


def _det_hw(sizes, counts, device):
    hw = torch.tensor(sizes, dtype=torch.int32).reshape(-1, 2)
    return hw.repeat_interleave(torch.tensor(counts, dtype=torch.int64), dim=0).to(device)


def paste_masks(masks, boxes, sizes, threshold=0.5, padding=1, counts=None):
    """Masker for every detection of a batch in one launch (extension; reference roi_heads/mask_head/inference.py:91-199,
    include/detops.h: detops_paste_masks): masks [N,1,M,M] or [N,M,M] (fp32 / fp16 / bf16: each detection's class channel),
    boxes [N,4] xyxy.  `sizes` lists (H, W) per detection, or per image together with `counts` (detections per image, in
    order).  -> (flat uint8 buffer holding every plane, [views]): one bool view [n_i, 1, H_i, W_i] of the buffer per entry
    of `sizes`."""
    masks, boxes, sizes, counts = _paste_args("paste_masks", masks, boxes, sizes, counts)
    N, M = masks.shape[0], masks.shape[1]
    dev = masks.device
    starts, offsets, end = [], [], 0
    for (h, w), c in zip(sizes, counts):
        starts.append(end)                   # planes back to back: the buffer holds nothing else
        offsets.extend(end + k * h * w for k in range(c))
        end += c * h * w
    flat = torch.empty((end,), dtype=torch.uint8, device=dev)
    if N:
        det_hw = _det_hw(sizes, counts, dev)
        out_offset = torch.tensor(offsets, dtype=torch.int64).to(dev)
        with _on_device(masks), _timed(("paste_masks[N=%d,M=%d]", (N, M)), masks):
            check(lib.detops_paste_masks(ptr(masks), _lib.DTYPE_CODE[masks.dtype], ptr(boxes), ptr(det_hw), ptr(out_offset),
                                         N, M, int(padding), float(threshold), ptr(flat), stream_of(masks)), "paste_masks")
    else:
        check(lib.detops_paste_masks(None, 0, None, None, None, 0, max(M, 1), int(padding), float(threshold), None, None),
              "paste_masks")
    views = [flat[s:s + c * h * w].view(c, 1, h, w).view(torch.bool) for s, (h, w), c in zip(starts, sizes, counts)]
    return flat, views


def paste_masks_rle(masks, boxes, sizes, threshold=0.5, padding=1, counts=None):
    """The masks of paste_masks as uncompressed COCO RLE, without the planes (extension; include/detops.h:
    detops_paste_masks_rle_count / _write): -> (counts int32 [total], run_offset int64 [N + 1]), both on the device;
    detection n's run lengths (column-major, starting with a 0-run) are counts[run_offset[n]:run_offset[n + 1]].  One host
    read (the total) sizes `counts`."""
    masks, boxes, sizes, per_image = _paste_args("paste_masks_rle", masks, boxes, sizes, counts)
    N, M = masks.shape[0], masks.shape[1]
    dev = masks.device
    run_offset = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
    if N == 0:
        return torch.empty((0,), dtype=torch.int32, device=dev), run_offset
    det_hw = _det_hw(sizes, per_image, dev)
    max_w = max(max(w for (_, w), c in zip(sizes, per_image) if c), 1)
    nbytes = int(lib.detops_paste_masks_rle_workspace_bytes(N, max_w))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    args = (ptr(masks), _lib.DTYPE_CODE[masks.dtype], ptr(boxes), ptr(det_hw), N, M, int(padding), float(threshold), max_w)
    with _on_device(masks):
        with _timed(("paste_masks_rle_count[N=%d,M=%d]", (N, M)), masks):
            check(lib.detops_paste_masks_rle_count(*args, ptr(run_offset), ptr(ws), nbytes, stream_of(masks)),
                  "paste_masks_rle_count")
        total = int(run_offset[-1].item())
        out = torch.empty((total,), dtype=torch.int32, device=dev)
        with _timed(("paste_masks_rle_write[N=%d,M=%d]", (N, M)), masks):
            check(lib.detops_paste_masks_rle_write(*args, ptr(run_offset), ptr(out), ptr(ws), nbytes, stream_of(masks)),
                  "paste_masks_rle_write")
    return out, run_offset


def rle_strings(counts, run_offset):
    """The compressed strings of COCO result files from uncompressed runs (extension; include/detops.h: "Compressed RLE
    strings", detops_rle_string_count / _write): counts int32 [total], run_offset int64 [N + 1], as paste_masks_rle makes
    them -> (bytes uint8 [B], byte_offset int64 [N + 1]) on the inputs' device; mask n's string is
    bytes[byte_offset[n]:byte_offset[n + 1]].  One host read (the total B) sizes `bytes`.  CPU tensors take the numpy
    statement of the same definition (_rle_cpu.py)."""
    if counts.dtype != torch.int32 or run_offset.dtype != torch.int64 or counts.dim() != 1 or run_offset.dim() != 1 \
            or run_offset.numel() < 1:
        raise ValueError("rle_strings: expected counts int32 [total] and run_offset int64 [N + 1]")
    if counts.device != run_offset.device:
        raise ValueError("rle_strings: counts and run_offset live on different devices")
    if not counts.is_cuda:
        data, off = _rle_cpu.rle_strings(counts.numpy(), run_offset.numpy())
        return torch.from_numpy(data), torch.from_numpy(off)
    counts, run_offset = counts.contiguous(), run_offset.contiguous()
    total, N = counts.numel(), run_offset.numel() - 1
    dev = counts.device
    byte_offset = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
    if N == 0 or total == 0:
        return torch.empty((0,), dtype=torch.uint8, device=dev), byte_offset
    nbytes = int(lib.detops_rle_string_workspace_bytes(total))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with _on_device(counts):
        with _timed(("rle_string_count[N=%d,runs=%d]", (N, total)), counts):
            check(lib.detops_rle_string_count(ptr(counts), ptr(run_offset), total, N, ptr(byte_offset), ptr(ws), nbytes,
                                              stream_of(counts)), "rle_string_count")
        out = torch.empty((int(byte_offset[-1].item()),), dtype=torch.uint8, device=dev)
        with _timed(("rle_string_write[N=%d,runs=%d]", (N, total)), counts):
            check(lib.detops_rle_string_write(ptr(counts), ptr(run_offset), total, N, ptr(byte_offset), ptr(out), ptr(ws),
                                              nbytes, stream_of(counts)), "rle_string_write")
    return out, byte_offset


def rle_string_list(data, byte_offset):
    """(bytes, byte_offset) of rle_strings -> a list of N str.  Device tensors cross in ONE copy (the offsets in front of
    the bytes), then one bytes.decode("ascii") and slices."""
    n8 = byte_offset.numel() * 8
    if data.is_cuda:
        host = torch.cat([byte_offset.contiguous().view(torch.uint8), data]).cpu().numpy()
        return _rle_cpu.to_str_list(host[n8:], host[:n8].view(np.int64))
    return _rle_cpu.to_str_list(data.numpy(), byte_offset.numpy())


def _hw_arg(name, hw, N, device):
    if hw is None:
        return None
    hw = torch.as_tensor(hw, dtype=torch.int32).reshape(-1, 2)
    if hw.shape[0] != N:
        raise ValueError("%s: hw must be [N, 2] for N = %d masks, got %s" % (name, N, tuple(hw.shape)))
    return hw.to(device).contiguous()


def rle_string_decode_status(data, byte_offset, hw=None):
    """rle_string_decode without the check: -> (counts, run_offset, status int32 [N]); a flagged mask's runs are unspecified
    but in bounds (include/detops.h, "Reading compressed RLE strings": the DETOPS_RLE_* bits)."""
    if data.dtype != torch.uint8 or byte_offset.dtype != torch.int64 or data.dim() != 1 or byte_offset.dim() != 1 \
            or byte_offset.numel() < 1:
        raise ValueError("rle_string_decode: expected bytes uint8 [B] and byte_offset int64 [N + 1]")
    if data.device != byte_offset.device:
        raise ValueError("rle_string_decode: bytes and byte_offset live on different devices")
    B, N = data.numel(), byte_offset.numel() - 1
    hw = _hw_arg("rle_string_decode", hw, N, data.device)
    if not data.is_cuda:
        counts, run_offset, status = _rle_cpu.rle_decode(data.numpy(), byte_offset.numpy(), None if hw is None else hw.numpy())
        return torch.from_numpy(counts), torch.from_numpy(run_offset), torch.from_numpy(status)
    data, byte_offset = data.contiguous(), byte_offset.contiguous()
    dev = data.device
    run_offset = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
    if N == 0 or B == 0:        # only empty strings: nothing to launch; an empty string holds no pixel
        status = torch.zeros((N,), dtype=torch.int32, device=dev)
        if hw is not None:
            status = ((hw[:, 0].to(torch.int64) * hw[:, 1]) != 0).to(torch.int32) * _rle_cpu.BAD_SUM
        return torch.empty((0,), dtype=torch.int32, device=dev), run_offset, status
    nbytes = int(lib.detops_rle_decode_workspace_bytes(B, N))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    status = torch.empty((N,), dtype=torch.int32, device=dev)
    with _on_device(data):
        with _timed(("rle_decode_count[N=%d,bytes=%d]", (N, B)), data):
            check(lib.detops_rle_decode_count(ptr(data), ptr(byte_offset), B, N, ptr(run_offset), ptr(ws), nbytes,
                                              stream_of(data)), "rle_decode_count")
        ends = torch.stack([byte_offset[0], byte_offset[-1], run_offset[-1], (byte_offset[1:] < byte_offset[:-1]).sum()]).tolist()
        if ends[0] != 0 or ends[1] != B or ends[3] != 0:     # (the kernels stay in bounds either way; the runs would mean nothing)
            raise ValueError("rle_string_decode: byte_offset must start at 0, not decrease and end at len(bytes)")
        total = int(ends[2])
        counts = torch.empty((total,), dtype=torch.int32, device=dev)
        with _timed(("rle_decode_write[N=%d,bytes=%d]", (N, B)), data):
            check(lib.detops_rle_decode_write(ptr(data), ptr(byte_offset), B, N, ptr(run_offset), total, ptr(hw), ptr(counts),
                                              ptr(status), ptr(ws), nbytes, stream_of(data)), "rle_decode_write")
    return counts, run_offset, status


def rle_string_decode(data, byte_offset, hw=None):
    """Compressed COCO `counts` strings back to uncompressed runs: the inverse of rle_strings (extension; include/detops.h:
    "Reading compressed RLE strings", detops_rle_decode_count / _write).  bytes uint8 [B] and byte_offset int64 [N + 1] (mask
    n's string is bytes[byte_offset[n]:byte_offset[n + 1]]); hw [N, 2] (H, W), when given, must be what each mask's runs
    sum to.  -> (counts int32 [total], run_offset int64 [N + 1]) on the inputs' device.  Malformed input raises a
    ValueError that names the first flagged mask and its status bits (one more host read).  CPU tensors take the numpy
    statement of the same definition (_rle_cpu.py)."""
    counts, run_offset, status = rle_string_decode_status(data, byte_offset, hw)
    err = _rle_cpu.status_error(status.cpu().numpy())
    if err is not None:
        raise err
    return counts, run_offset


def rle_string_decode_list(strings, hw=None, device=None):
    """rle_string_decode for a list of N str, as a result file holds them; the result lives on `device` (default: the
    CPU).  The mirror of rle_string_list: ONE host-to-device copy, the offsets (and hw) in front of the bytes."""
    data, byte_offset = _rle_cpu.from_str_list(list(strings))
    N = byte_offset.size - 1
    device = torch.device("cpu" if device is None else device)
    if device.type != "cuda":
        return rle_string_decode(torch.from_numpy(data.copy()), torch.from_numpy(byte_offset), hw)
    hw_h = np.zeros((0, 2), np.int32) if hw is None else _hw_arg("rle_string_decode_list", hw, N, "cpu").numpy()
    host = np.concatenate([byte_offset.view(np.uint8), hw_h.reshape(-1).view(np.uint8), data])
    both = torch.from_numpy(host).to(device)
    n8, h8 = byte_offset.size * 8, hw_h.size * 4
    return rle_string_decode(both[n8 + h8:], both[:n8].view(torch.int64),
                             None if hw is None else both[n8:n8 + h8].view(torch.int32).reshape(-1, 2))


# ------------------------------------------------------------------------------------------ target assignment
def match_boxes(gt_boxes, gt_valid, boxes, high_threshold, low_threshold, allow_low_quality_matches):
    """Fused IoU + Matcher (extension; reference structures/boxlist_ops.py:53-89 + modeling/matcher.py:42-112):
    gt_boxes [N,M,4], gt_valid [N,M] bool, boxes [K,4] (shared) or [N,K,4] -> matched_idxs [N,K] int64."""
    _need_cuda("match_boxes", gt_boxes, gt_valid, boxes)
    gt_boxes = _f32c("match_boxes", gt_boxes)
    boxes = _f32c("match_boxes", boxes)
    valid = _u8("match_boxes", gt_valid)
    N, M = gt_boxes.shape[:2]
    batched = boxes.dim() == 3
    K = boxes.shape[-2]
    out = torch.empty((N, K), dtype=torch.int64, device=boxes.device)
    if N == 0 or K == 0:
        return out
    nbytes = int(lib.detops_match_boxes_workspace_bytes(N, M))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=boxes.device)
    with _on_device(boxes), _timed(("match_boxes[N=%d,M=%d,K=%d]", (N, M, K)), boxes):
        check(lib.detops_match_boxes_f32(ptr(gt_boxes), ptr(valid), ptr(boxes), int(batched), N, M, K,
                                         float(high_threshold), float(low_threshold), int(bool(allow_low_quality_matches)),
                                         ptr(out), ptr(ws), nbytes, stream_of(boxes)), "match_boxes")
    return out


_SAMPLER_CALLS = [0]


def _next_sampler_seed(device):
    """64-bit seed of the next sampler call, drawn from the DEVICE generator's (seed, Philox offset) — host-side state,
    no device op: the stream follows torch.cuda.manual_seed and is saved / restored with the generator state
    (torch.cuda.get_rng_state in a checkpoint), like the `torch.randperm` the reference's sampler draws from the same
    generator.  The offset is advanced by 4 per call (one Philox block)."""
    try:
        gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
        base, off = gen.initial_seed(), gen.get_offset()
        gen.set_offset(off + 4)
    except (AttributeError, RuntimeError, IndexError):   # a torch without generator offsets: per-process counter
        _SAMPLER_CALLS[0] += 1
        base, off = torch.initial_seed(), _SAMPLER_CALLS[0]
    return (base * 0x9E3779B97F4A7C15 + off * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF


# Set by engine/graph_step.py while a training step is captured into / replayed from a HIP graph: an int64 [1] device tensor that
# the captured step increments; the samplers mix it into their (frozen-at-capture) seed when they RUN.
GRAPH_SEED = None


def sample_labels(labels, batch_size_per_image, max_positives, with_list=False, seed=None):
    """BalancedPositiveNegativeSampler on device (extension; reference
    modeling/balanced_positive_negative_sampler.py:19-68): labels [N,n] float32 or int64 ->
    (pos_mask, neg_mask [N,n] bool[, idx [N,B] int64, valid [N,B] bool]).  The random subset is a pure function
    of (labels, seed); the default seed is drawn from the device generator's seed and Philox offset (no device op)."""
    _need_cuda("sample_labels", labels)
    if labels.dtype not in (torch.float32, torch.int64):
        labels = labels.to(torch.int64)
    labels = labels.contiguous()
    N, n = labels.shape
    B = int(batch_size_per_image)
    if seed is None:
        seed = _next_sampler_seed(labels.device)
    pos = torch.empty((N, n), dtype=torch.uint8, device=labels.device)
    neg = torch.empty((N, n), dtype=torch.uint8, device=labels.device)
    idx = torch.empty((N, B), dtype=torch.int64, device=labels.device) if with_list else None
    val = torch.empty((N, B), dtype=torch.uint8, device=labels.device) if with_list else None
    if N and n:
        nbytes = int(lib.detops_sample_labels_workspace_bytes(N, B))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=labels.device)
        with _on_device(labels), _timed(("sample_labels[N=%d,n=%d,B=%d]", (N, n, B)), labels):
            check(lib.detops_sample_labels_dseed(ptr(labels), 0 if labels.dtype == torch.float32 else 1, N, n, B,
                                                 int(max_positives), ctypes.c_uint64(seed), ptr(GRAPH_SEED), ptr(pos), ptr(neg),
                                                 ptr(idx), ptr(val), ptr(ws), nbytes, stream_of(labels)), "sample_labels")
    elif with_list:
        idx.zero_()
        val.zero_()
    if with_list:
        return pos.view(torch.bool), neg.view(torch.bool), idx, val.view(torch.bool)
    return pos.view(torch.bool), neg.view(torch.bool)


def mask_targets(masks, mask_index, boxes, discretization_size):
    """Mask-head targets (extension; reference roi_heads/mask_head/loss.py:11-42): masks [G,H,W] uint8 / bool /
    float32, mask_index [P] int64, boxes [P,4] xyxy -> [P,M,M] float32, bit-equal to the reference's CPU path."""
    _need_cuda("mask_targets", masks, mask_index, boxes)
    boxes = _f32c("mask_targets", boxes)
    if masks.dtype == torch.bool:
        code, m = 2, masks.contiguous().view(torch.uint8)
    elif masks.dtype == torch.uint8:
        code, m = 0, masks.contiguous()
    elif not masks.dtype.is_floating_point:
        # any other integer dtype: the reference's `.type_as(self.masks)` truncates the interpolated value for every
        # non-floating mask (segmentation_mask.py:111-158); binary masks are 0 / 1, so uint8 is the same computation
        code, m = 0, masks.to(torch.uint8).contiguous()
    else:
        code, m = 1, masks.to(torch.float32).contiguous()
    mask_index = mask_index.to(torch.int64).contiguous()
    G, H, W = m.shape
    P, M = boxes.size(0), int(discretization_size)
    out = torch.empty((P, M, M), dtype=torch.float32, device=boxes.device)
    if P:
        with _on_device(boxes), _timed(("mask_targets[P=%d,M=%d]", (P, M)), boxes):
            check(lib.detops_mask_targets(ptr(m), code, ptr(mask_index), ptr(boxes), G, H, W, P, M, ptr(out),
                                          stream_of(boxes)), "mask_targets")
    return out


def _packed_polygons(name, verts, poly_offset, inst_offset):
    if verts.dtype != torch.float32 or poly_offset.dtype != torch.int32 or inst_offset.dtype != torch.int32 \
            or verts.dim() != 2 or verts.shape[1] != 2 or poly_offset.numel() < 1 or inst_offset.numel() < 1:
        raise ValueError("%s: expected verts [V, 2] float32, poly_offset [P + 1] int32, inst_offset [G + 1] int32" % name)
    if not (verts.device == poly_offset.device == inst_offset.device):
        raise RuntimeError("%s: the packed polygons must live on one device" % name)
    return verts.contiguous(), poly_offset.contiguous(), inst_offset.contiguous()


def polygon_mask_targets(verts, poly_offset, inst_offset, slot_inst, boxes, slot_wh, discretization_size):
    """Mask-head targets from packed polygons (extension; include/detops.h: detops_polygon_mask_targets; reference
    roi_heads/mask_head/loss.py:11-42 over PolygonInstance.crop / resize / convert_to_binarymask): slot_inst [S] int64 (global
    instance index), boxes [S,4] xyxy, slot_wh [S,2] int32 = (W, H) of the slot's image -> [S,M,M] float32 of 0 / 1.  One
    launch for the whole batch.  CPU tensors take the numpy implementation of the same definition (_polygon_cpu.py)."""
    verts, poly_offset, inst_offset = _packed_polygons("polygon_mask_targets", verts, poly_offset, inst_offset)
    boxes = _f32c("polygon_mask_targets", boxes)
    slot_inst = slot_inst.to(torch.int64).contiguous()
    slot_wh = slot_wh.to(torch.int32).contiguous()
    S, M = boxes.size(0), int(discretization_size)
    if tuple(boxes.shape) != (S, 4) or tuple(slot_inst.shape) != (S,) or tuple(slot_wh.shape) != (S, 2) or M < 1:
        raise ValueError("polygon_mask_targets: inconsistent arguments")
    tensors = (verts, poly_offset, inst_offset, slot_inst, boxes, slot_wh)
    if not any(on_device(t) for t in tensors):
        from . import _polygon_cpu

        return torch.from_numpy(_polygon_cpu.polygon_mask_targets(*(t.numpy() for t in tensors), M))
    _need_cuda("polygon_mask_targets", *tensors)
    V, P, G = verts.shape[0], poly_offset.numel() - 1, inst_offset.numel() - 1
    out = torch.empty((S, M, M), dtype=torch.float32, device=boxes.device)
    if S:
        with _on_device(boxes), _timed(("polygon_mask_targets[S=%d,M=%d]", (S, M)), boxes):
            check(lib.detops_polygon_mask_targets(ptr(verts), ptr(poly_offset), ptr(inst_offset), V, P, G, ptr(slot_inst),
                                                  ptr(boxes), ptr(slot_wh), S, M, ptr(out), stream_of(boxes)),
                  "polygon_mask_targets")
    return out


def polygons_to_masks(verts, poly_offset, inst_offset, height, width):
    """Dense planes of the instances of one image (extension; include/detops.h: detops_polygons_to_masks) -> [G,H,W] uint8
    of 0 / 1 on the device of the packed polygons; CPU tensors take the numpy implementation of the same definition."""
    verts, poly_offset, inst_offset = _packed_polygons("polygons_to_masks", verts, poly_offset, inst_offset)
    H, W = int(height), int(width)
    if H < 0 or W < 0:
        raise ValueError("polygons_to_masks: negative image size")
    if not on_device(verts):
        from . import _polygon_cpu

        return torch.from_numpy(_polygon_cpu.polygons_to_masks(verts.numpy(), poly_offset.numpy(), inst_offset.numpy(), H, W))
    V, P, G = verts.shape[0], poly_offset.numel() - 1, inst_offset.numel() - 1
    out = torch.empty((G, H, W), dtype=torch.uint8, device=verts.device)
    if out.numel():
        with _on_device(verts), _timed(("polygons_to_masks[G=%d]", (G,)), verts):
            check(lib.detops_polygons_to_masks(ptr(verts), ptr(poly_offset), ptr(inst_offset), V, P, G, H, W, ptr(out),
                                               stream_of(verts)), "polygons_to_masks")
    return out


# ------------------------------------------------------------------------------------------ batch image preparation
IMAGE_PREP_MAX_KSIZE = 17             # DETOPS_IMAGE_PREP_MAX_KSIZE: a downscale by up to 8 per axis
_EINVAL = -1


def image_batch(raw, offsets, geom, table, bgr, Hp, Wp, channels_last=False, geom_host=None):
    """The batch tensor from the raw images of a batch (extension; include/detops.h: detops_image_batch_u8): raw [bytes]
    uint8 (RGB HWC images back to back), offsets [N] int64 (bytes), geom [N, 5] int32 (source h, w, destination oh, ow, flip
    bits), table [3, 256] float32 -> float32 [N, 3, Hp, Wp] (torch.channels_last memory with `channels_last`): Pillow's
    bilinear resize, flips, normalisation and zero padding in one launch.  geom_host: the CPU copy of `geom` when the
    caller has one (else it is read back).  CPU tensors take the numpy implementation of the same definition
    (_image_prep_cpu.py); so does, through the host, a device batch with a downscale beyond IMAGE_PREP_MAX_KSIZE."""
    from . import _image_prep_cpu

    Hp, Wp = int(Hp), int(Wp)
    if raw.dtype != torch.uint8 or raw.dim() != 1 or offsets.dtype != torch.int64 or geom.dtype != torch.int32 \
            or geom.dim() != 2 or geom.shape[1] != _image_prep_cpu.GEOM_FIELDS or offsets.numel() != geom.shape[0] \
            or table.dtype != torch.float32 or tuple(table.shape) != (3, 256) or Hp < 0 or Wp < 0:
        raise ValueError("image_batch: expected raw [bytes] uint8, offsets [N] int64, geom [N, 5] int32, table [3, 256] float32")
    tensors = (raw, offsets, geom, table)
    N = geom.shape[0]
    fmt = torch.channels_last if channels_last else torch.contiguous_format

    def host(device):
        out = torch.from_numpy(_image_prep_cpu.image_batch(*(t.cpu().numpy() for t in tensors), bool(bgr), Hp, Wp))
        return out.to(device).contiguous(memory_format=fmt)

    if not any(on_device(t) for t in tensors):
        return host(raw.device)
    _need_cuda("image_batch", *tensors)
    raw, offsets, geom, table = (t.contiguous() for t in tensors)
    geom_host = (geom.cpu() if geom_host is None else geom_host.to(torch.int32)).contiguous()
    if geom_host.is_cuda or tuple(geom_host.shape) != tuple(geom.shape):
        raise ValueError("image_batch: geom_host is the CPU copy of geom")
    out = torch.empty((N, 3, Hp, Wp), dtype=torch.float32, device=raw.device, memory_format=fmt)
    if out.numel():
        with _on_device(raw), _timed(("image_batch[N=%d,%dx%d]", (N, Hp, Wp)), raw):
            rc = lib.detops_image_batch_u8(ptr(raw), raw.numel(), ptr(offsets), ptr(geom), ptr(geom_host), N, ptr(table),
                                           int(bool(bgr)), Hp, Wp, int(bool(channels_last)), ptr(out), stream_of(raw))
        g = geom_host.numpy()
        if rc == _EINVAL and g[:, :4].min(initial=1) >= 1 and (g[:, 2] <= Hp).all() and (g[:, 3] <= Wp).all() \
                and max(_image_prep_cpu.axis_ksize(r[a], r[a + 2]) for r in g for a in (0, 1)) > IMAGE_PREP_MAX_KSIZE:
            return host(raw.device)                   # well-formed, only the downscale is beyond the kernel
        check(rc, "image_batch")
    return out


def color_jitter(raw, offsets, geom, jitter, geom_host=None, jitter_host=None):
    """Colour jitter of the raw images of a batch, IN PLACE on `raw` (extension; include/detops.h: detops_color_jitter_u8):
    raw, offsets, geom as image_batch; jitter [N, 8] int32 per image: four step codes in the order they run (0 none,
    1 brightness, 2 contrast, 3 saturation, 4 hue) and their four parameters (the fp32 bits of the factor, or hue's byte
    shift k).  Pillow's ImageEnhance and HSV arithmetic, byte for byte.  geom_host, jitter_host: the CPU copies when the
    caller has them (else they are read back).  Returns raw.  CPU tensors take the numpy implementation of the same
    definition (_color_jitter_cpu.py)."""
    from . import _color_jitter_cpu, _image_prep_cpu

    if raw.dtype != torch.uint8 or raw.dim() != 1 or offsets.dtype != torch.int64 or offsets.dim() != 1 \
            or geom.dtype != torch.int32 or geom.dim() != 2 or geom.shape[1] != _image_prep_cpu.GEOM_FIELDS \
            or jitter.dtype != torch.int32 or jitter.dim() != 2 or jitter.shape[1] != _color_jitter_cpu.FIELDS \
            or not offsets.numel() == geom.shape[0] == jitter.shape[0]:
        raise ValueError("color_jitter: expected raw [bytes] uint8, offsets [N] int64, geom [N, 5] int32, jitter [N, 8] int32")
    tensors = (raw, offsets, geom, jitter)
    N = geom.shape[0]
    if not any(on_device(t) for t in tensors):
        if not raw.is_contiguous():
            raise ValueError("color_jitter: raw is changed in place and must be contiguous")
        _color_jitter_cpu.color_jitter(raw.numpy(), offsets.numpy(), geom.numpy(), jitter.numpy())
        return raw
    _need_cuda("color_jitter", *tensors)
    if not raw.is_contiguous():
        raise ValueError("color_jitter: raw is changed in place and must be contiguous")
    offsets, geom, jitter = (t.contiguous() for t in (offsets, geom, jitter))
    geom_host = (geom.cpu() if geom_host is None else geom_host.to(torch.int32)).contiguous()
    jitter_host = (jitter.cpu() if jitter_host is None else jitter_host.to(torch.int32)).contiguous()
    if geom_host.is_cuda or tuple(geom_host.shape) != tuple(geom.shape) or jitter_host.is_cuda \
            or tuple(jitter_host.shape) != tuple(jitter.shape):
        raise ValueError("color_jitter: geom_host and jitter_host are the CPU copies of geom and jitter")
    if N == 0:
        return raw
    with _on_device(raw), _timed(("color_jitter[N=%d,%d bytes]", (N, raw.numel())), raw):
        ws = torch.empty(N, dtype=torch.int64, device=raw.device)
        rc = lib.detops_color_jitter_u8(ptr(raw), raw.numel(), ptr(offsets), ptr(geom), ptr(geom_host), ptr(jitter),
                                        ptr(jitter_host), N, ptr(ws), ws.numel() * 8, stream_of(raw))
    if rc == _EINVAL:                                  # the entry point validated the records (nothing was launched):
        _color_jitter_cpu.check_records(jitter_host.numpy())       # its refusal with the reason, off the per-batch path
    check(rc, "color_jitter")
    return raw


# ------------------------------------------------------------------------------------------ test-time box augmentation
def bbox_aug_merge(boxes, scores, row_offset, group_geom, group_ratio, N, T, score_thresh):
    """The merge of test-time box augmentation (extension; include/detops.h: detops_bbox_aug_merge_count / _write): boxes
    [R, 4C] and scores [R, C] fp32 are the unfiltered rows of every (image, pass) group, image-major; row_offset int32
    [N*T + 1], group_geom int32 [N*T, 3] (frame w, h, flip bit) and group_ratio float32 [N*T, 2] are CPU tensors
    (_bbox_aug_torch.group_records makes the last two).  -> (cand_boxes [M, 4] in the frame of each image's first pass,
    cand_scores [M], seg_offsets int32 [N*(C-1) + 1] on the device, the longest segment): one NMS segment per (image,
    class >= 1), pass order then row order inside it.  One host read (M and the longest segment).  CPU tensors take the
    torch formulation of the same definition (_bbox_aug_torch.py)."""
    from . import _bbox_aug_torch

    N, T = int(N), int(T)
    if boxes.dim() != 2 or scores.dim() != 2 or boxes.shape[0] != scores.shape[0] or boxes.shape[1] != 4 * scores.shape[1] \
            or N < 0 or T < 1 or row_offset.dtype != torch.int32 or row_offset.numel() != N * T + 1 \
            or group_geom.dtype != torch.int32 or tuple(group_geom.shape) != (N * T, 3) \
            or group_ratio.dtype != torch.float32 or tuple(group_ratio.shape) != (N * T, 2) \
            or row_offset.is_cuda or group_geom.is_cuda or group_ratio.is_cuda:
        raise ValueError("bbox_aug_merge: expected boxes [R, 4C], scores [R, C] and the CPU records row_offset [N*T + 1] int32, "
                         "group_geom [N*T, 3] int32, group_ratio [N*T, 2] float32")
    boxes = _f32c("bbox_aug_merge", boxes)
    scores = _f32c("bbox_aug_merge", scores)
    if not on_device(boxes) and not on_device(scores):
        return _bbox_aug_torch.bbox_aug_merge(boxes, scores, row_offset, group_geom, group_ratio, N, T, float(score_thresh))
    _need_cuda("bbox_aug_merge", boxes, scores)
    if boxes.data_ptr() % 16:                         # the kernel reads a box as one 16-byte load: a view at an odd offset is copied
        boxes = boxes.clone()
    dev = scores.device
    R, C = scores.shape
    row_offset = row_offset.contiguous()
    per_image = row_offset[::T]
    longest_image = int((per_image[1:] - per_image[:-1]).max()) if N else 0
    d_off = row_offset.to(dev, non_blocking=True)
    d_geom = group_geom.contiguous().to(dev, non_blocking=True)
    d_ratio = group_ratio.contiguous().to(dev, non_blocking=True)
    seg_offsets = torch.empty((N * max(C - 1, 0) + 1,), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int32, device=dev)
    nbytes = int(lib.detops_bbox_aug_merge_workspace_bytes(N, C, max(longest_image, 0)))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    with _on_device(scores):
        with _timed(("bbox_aug_merge_count[R=%d,C=%d]", (R, C)), scores):
            check(lib.detops_bbox_aug_merge_count(ptr(scores), ptr(d_off), ptr(row_offset), R, C, N, T, float(score_thresh),
                                                  ptr(seg_offsets), ptr(totals), ptr(ws), nbytes, stream_of(scores)),
                  "bbox_aug_merge_count")
        M, longest = totals.tolist()                  # the variable-length result forces one readback
        cand_boxes = torch.empty((M, 4), dtype=torch.float32, device=dev)
        cand_scores = torch.empty((M,), dtype=torch.float32, device=dev)
        with _timed(("bbox_aug_merge_write[R=%d,C=%d]", (R, C)), scores):
            check(lib.detops_bbox_aug_merge_write(ptr(boxes), ptr(scores), ptr(d_off), ptr(row_offset), ptr(d_geom), ptr(d_ratio),
                                                  R, C, N, T, float(score_thresh), ptr(seg_offsets), M, ptr(cand_boxes),
                                                  ptr(cand_scores), ptr(ws), nbytes, stream_of(scores)), "bbox_aug_merge_write")
    return cand_boxes, cand_scores, seg_offsets, longest


# ------------------------------------------------------------------------------------------ detection evaluation
EVAL_COCO_SEGM, EVAL_COCO_BBOX, EVAL_VOC = 0, 1, 2
EVAL_MAX_GT = _eval_cpu.MAX_GT        # DETOPS_EVAL_MAX_GT: the largest G_p detops_eval_match serves
_EGTCAP = -4


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _problem_args(name, dt_offset, gt_offset, iou_offset):
    if dt_offset.dtype != torch.int32 or gt_offset.dtype != torch.int32 or iou_offset.dtype != torch.int64 \
            or not (dt_offset.numel() == gt_offset.numel() == iou_offset.numel() >= 1):
        raise ValueError("%s: expected dt_offset / gt_offset [P + 1] int32 and iou_offset [P + 1] int64" % name)
    return dt_offset.contiguous(), gt_offset.contiguous(), iou_offset.contiguous(), dt_offset.numel() - 1


def mask_pack(planes):
    """Bit rows, pixel counts and tight extents of uint8 / bool planes (extension; include/detops.h: detops_mask_pack).
    planes: a tensor [n, H, W] or a list of such tensors (the images of a batch differ in size) -> (words int64 [total]: the
    64-bit words, word_offset int64 [N], hw int32 [N, 2], area int32 [N], extent int32 [N, 4]).  One launch per tensor of
    the list (tensors that are views of ONE buffer, as paste_masks returns them, share a launch); contiguous planes are read
    in place.  The host builds the per-plane sizes and offsets and copies them to the device (three small copies, one more
    per launch).  CPU tensors take the numpy implementation (_eval_cpu.py)."""
    if isinstance(planes, torch.Tensor):
        planes = [planes]
    groups = []
    for t in planes:
        if t.dim() != 3 or t.dtype not in (torch.uint8, torch.bool):
            raise ValueError("mask_pack: planes must be [n, H, W] uint8 or bool, got %s %s" % (tuple(t.shape), t.dtype))
        if t.shape[1] * t.shape[2] >= 2 ** 31:
            raise ValueError("mask_pack: a plane must hold fewer than 2^31 pixels")
        t = t.contiguous()
        groups.append(t.view(torch.uint8) if t.dtype == torch.bool else t)
    if not any(on_device(t) for t in groups):
        from . import _eval_cpu

        w, off, hw, area, ext = _eval_cpu.mask_pack([t.numpy() for t in groups])
        return (torch.from_numpy(w.view(np.int64)), torch.from_numpy(off), torch.from_numpy(hw), torch.from_numpy(area),
                torch.from_numpy(ext))
    _need_cuda("mask_pack", *groups)
    dev = groups[0].device
    hw_l, off_l, base_l, total = [], [], [], 0
    for t in groups:
        n, H, W = t.shape
        per = H * ((W + 63) // 64)
        hw_l.extend([(H, W)] * n)
        off_l.extend(total + k * per for k in range(n))
        base_l.extend(t.data_ptr() + k * H * W for k in range(n))
        total += n * per
    N = len(hw_l)
    words = torch.empty((total,), dtype=torch.int64, device=dev)
    area = torch.empty((N,), dtype=torch.int32, device=dev)
    extent = torch.empty((N, 4), dtype=torch.int32, device=dev)
    hw = torch.tensor(hw_l, dtype=torch.int32).reshape(-1, 2).to(dev)
    word_offset = torch.tensor(off_l, dtype=torch.int64).to(dev)
    if N:
        # one launch per underlying buffer: plane addresses are offsets from the buffer's first plane
        runs, start = [], 0
        stores = [t.untyped_storage().data_ptr() for t in groups for _ in range(t.shape[0])]
        for k in range(1, N + 1):
            if k == N or stores[k] != stores[start]:
                runs.append((start, k))
                start = k
        with _on_device(groups[0]), _timed(("mask_pack[N=%d]", (N,)), groups[0]):
            for a, b in runs:
                base = min(base_l[a:b])
                plane_offset = torch.tensor([v - base for v in base_l[a:b]], dtype=torch.int64).to(dev)
                max_words = max(h * ((w + 63) // 64) for h, w in hw_l[a:b])
                check(lib.detops_mask_pack(base, ptr(plane_offset), hw[a:b].data_ptr(), b - a, max_words,
                                           word_offset[a:b].data_ptr(), ptr(words), area[a:b].data_ptr(),
                                           extent[a:b].data_ptr(), stream_of(words)), "mask_pack")
    return words, word_offset, hw, area, extent


MASK_PACK_RLE_MAX_H = _lib._abi.MASK_PACK_RLE_MAX_H


def mask_pack_rle(counts, run_offset, hw):
    """mask_pack from uncompressed RLE, no plane stored (extension; include/detops.h: detops_mask_pack_rle).  counts int32
    [total] and run_offset int64 [N + 1] as paste_masks_rle or rle_string_decode make them (column-major runs starting
    with a 0-run), hw [N, 2] (H, W) per mask -> the five tensors of mask_pack.  A call with a plane taller than
    MASK_PACK_RLE_MAX_H, and CPU tensors, take the numpy implementation (_eval_cpu.py)."""
    if counts.dtype != torch.int32 or run_offset.dtype != torch.int64 or counts.dim() != 1 or run_offset.dim() != 1 \
            or run_offset.numel() < 1:
        raise ValueError("mask_pack_rle: expected counts int32 [total] and run_offset int64 [N + 1]")
    if counts.device != run_offset.device:
        raise ValueError("mask_pack_rle: counts and run_offset live on different devices")
    N, total, dev = run_offset.numel() - 1, counts.numel(), counts.device
    hw_h = torch.as_tensor(hw).detach().cpu().to(torch.int32).reshape(-1, 2)
    if hw_h.shape[0] != N or (N and (int(hw_h.min()) < 0 or int((hw_h[:, 0].long() * hw_h[:, 1].long()).max()) >= 2 ** 31)):
        raise ValueError("mask_pack_rle: hw must be [N, 2] sizes of fewer than 2^31 pixels for N = %d masks" % N)
    max_h, max_w = (int(hw_h[:, 0].max()), int(hw_h[:, 1].max())) if N else (0, 0)
    if not counts.is_cuda or max_h > MASK_PACK_RLE_MAX_H:
        w, off, hw_o, area, ext = _eval_cpu.mask_pack_rle(_np(counts), _np(run_offset), hw_h.numpy())
        return tuple(torch.from_numpy(a).to(dev) for a in (w.view(np.int64), off, hw_o, area, ext))
    counts, run_offset = counts.contiguous(), run_offset.contiguous()
    per = hw_h[:, 0].to(torch.int64) * ((hw_h[:, 1].to(torch.int64) + 63) // 64)
    ends = torch.cumsum(per, 0)
    n_words = int(ends[-1]) if N else 0
    words = torch.empty((n_words,), dtype=torch.int64, device=dev)
    area = torch.empty((N,), dtype=torch.int32, device=dev)
    extent = torch.empty((N, 4), dtype=torch.int32, device=dev)
    # one host-to-device copy: the word offsets in front of the sizes
    both = torch.cat([(ends - per).view(torch.int32), hw_h.reshape(-1)]).to(dev)
    word_offset, hw_d = both[:2 * N].view(torch.int64), both[2 * N:].reshape(N, 2)
    if N:
        nbytes = int(lib.detops_mask_pack_rle_workspace_bytes(total))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        with _on_device(counts), _timed(("mask_pack_rle[N=%d,runs=%d]", (N, total)), counts):
            check(lib.detops_mask_pack_rle(ptr(counts), ptr(run_offset), total, ptr(hw_d), N, max_h, max_w, ptr(word_offset),
                                           ptr(words), ptr(area), ptr(extent), ptr(ws), nbytes, stream_of(counts)),
                  "mask_pack_rle")
    return words, word_offset, hw_d, area, extent


def mask_pair_counts(dt_pack, gt_pack, dt_offset, gt_offset, iou_offset, total_pairs):
    """Pixels set in both planes of every (detection, ground truth) pair of every problem (extension; include/detops.h:
    detops_mask_pair_counts).  dt_pack / gt_pack: (words, word_offset, hw, extent) with the per-plane arrays in SORTED
    (problem) order -> int32 [total_pairs]."""
    dt_offset, gt_offset, iou_offset, P = _problem_args("mask_pair_counts", dt_offset, gt_offset, iou_offset)
    total_pairs = int(total_pairs)
    dw, dwo, dhw, dex = (t.contiguous() for t in dt_pack)
    gw, gwo, ghw, gex = (t.contiguous() for t in gt_pack)
    tensors = (dw, dwo, dhw, dex, gw, gwo, ghw, gex, dt_offset, gt_offset, iou_offset)
    if not any(on_device(t) for t in tensors):
        from . import _eval_cpu

        out = _eval_cpu.mask_pair_counts(dw.numpy().view(np.uint64), dwo.numpy(), dhw.numpy(), dex.numpy(),
                                         gw.numpy().view(np.uint64), gwo.numpy(), ghw.numpy(), gex.numpy(), dt_offset.numpy(),
                                         gt_offset.numpy(), iou_offset.numpy())
        return torch.from_numpy(out)
    _need_cuda("mask_pair_counts", *tensors)
    if dwo.dtype != torch.int64 or gwo.dtype != torch.int64 or any(t.dtype != torch.int32 for t in (dhw, dex, ghw, gex)) \
            or dw.dtype != torch.int64 or gw.dtype != torch.int64:
        raise ValueError("mask_pair_counts: packs must come from mask_pack")
    counts = torch.empty((total_pairs,), dtype=torch.int32, device=dt_offset.device)
    if total_pairs:
        with _on_device(counts), _timed(("mask_pair_counts[pairs=%d]", (total_pairs,)), counts):
            check(lib.detops_mask_pair_counts(ptr(dw), ptr(dwo), ptr(dhw), ptr(dex), ptr(gw), ptr(gwo), ptr(ghw), ptr(gex),
                                              ptr(dt_offset), ptr(gt_offset), ptr(iou_offset), P, total_pairs, ptr(counts),
                                              stream_of(counts)), "mask_pair_counts")
    return counts


def eval_iou(mode, dt_offset, gt_offset, iou_offset, total_pairs, counts=None, dt_area=None, gt_area=None, dt_boxes=None,
             gt_boxes=None, gt_crowd=None):
    """The fp64 IoU matrices of every problem (extension; include/detops.h: detops_eval_iou).  EVAL_COCO_SEGM: counts
    [total_pairs] int32 and int32 areas; EVAL_COCO_BBOX / EVAL_VOC: fp32 xyxy boxes; gt_crowd uint8 / bool (COCO modes).
    Everything in sorted (problem) order -> float64 [total_pairs]."""
    dt_offset, gt_offset, iou_offset, P = _problem_args("eval_iou", dt_offset, gt_offset, iou_offset)
    total_pairs, mode = int(total_pairs), int(mode)
    if mode == EVAL_COCO_SEGM:
        counts, dt_area, gt_area = (t.to(torch.int32).contiguous() for t in (counts, dt_area, gt_area))
        dt_boxes = gt_boxes = None
    else:
        dt_boxes, gt_boxes = (t.to(torch.float32).contiguous().reshape(-1, 4) for t in (dt_boxes, gt_boxes))
        counts = dt_area = gt_area = None
    if gt_crowd is not None:
        gt_crowd = gt_crowd.to(torch.uint8).contiguous()
    tensors = [t for t in (dt_offset, gt_offset, iou_offset, counts, dt_area, gt_area, dt_boxes, gt_boxes, gt_crowd)
               if t is not None]
    if not any(on_device(t) for t in tensors):
        from . import _eval_cpu

        return torch.from_numpy(_eval_cpu.eval_iou(mode, _np(counts), _np(dt_area), _np(gt_area), _np(dt_boxes), _np(gt_boxes),
                                                   _np(gt_crowd), dt_offset.numpy(), gt_offset.numpy(), iou_offset.numpy()))
    _need_cuda("eval_iou", *tensors)
    if counts is not None and counts.numel() != total_pairs:
        raise ValueError("eval_iou: counts must hold total_pairs elements")
    iou = torch.empty((total_pairs,), dtype=torch.float64, device=dt_offset.device)
    if total_pairs:
        with _on_device(iou), _timed(("eval_iou[pairs=%d]", (total_pairs,)), iou):
            check(lib.detops_eval_iou(mode, ptr(counts), ptr(dt_area), ptr(gt_area), ptr(dt_boxes), ptr(gt_boxes), ptr(gt_crowd),
                                      ptr(dt_offset), ptr(gt_offset), ptr(iou_offset), P, total_pairs, ptr(iou), stream_of(iou)),
                  "eval_iou")
    return iou


def eval_match(mode, iou, dt_offset, gt_offset, iou_offset, counts_host, gt_flag, iou_thrs, dt_area=None, gt_area=None,
               area_rngs=None):
    """Greedy matching of every problem (extension; include/detops.h: detops_eval_match).  counts_host = (D_total, G_total,
    max G_p) as Python ints; gt_flag: iscrowd (COCO modes) or difficult (EVAL_VOC); iou_thrs [T] and area_rngs [A, 2]
    float64.  COCO modes -> (dt_match int32 [A, T, D_total], dt_ignore uint8 [A, T, D_total], gt_ignore uint8 [A, G_total]);
    EVAL_VOC -> match int8 [D_total].  Problems with more than EVAL_MAX_GT ground truths are computed on the host
    (_eval_cpu.py) and patched into the device result."""
    dt_offset, gt_offset, iou_offset, P = _problem_args("eval_match", dt_offset, gt_offset, iou_offset)
    mode = int(mode)
    D_total, G_total, max_gt = (int(v) for v in counts_host)
    iou = iou.to(torch.float64).contiguous()
    gt_flag = gt_flag.to(torch.uint8).contiguous()
    iou_thrs = torch.as_tensor(iou_thrs, dtype=torch.float64).reshape(-1).contiguous()
    coco = mode != EVAL_VOC
    if coco:
        area_rngs = torch.as_tensor(area_rngs, dtype=torch.float64).reshape(-1, 2).contiguous()
        dt_area, gt_area = dt_area.to(torch.float64).contiguous(), gt_area.to(torch.float64).contiguous()
        A, T = area_rngs.shape[0], iou_thrs.numel()
        if dt_area.numel() != D_total or gt_area.numel() != G_total:
            raise ValueError("eval_match: areas do not match the problem sizes")
    else:
        area_rngs = dt_area = gt_area = None
    if gt_flag.numel() != G_total or iou_thrs.numel() < 1:
        raise ValueError("eval_match: inconsistent arguments")
    tensors = [iou, dt_offset, gt_offset, iou_offset, gt_flag] + ([dt_area, gt_area] if coco else [])
    from . import _eval_cpu

    def host(only=None):
        return _eval_cpu.eval_match(mode, _np(iou), _np(dt_offset), _np(gt_offset), _np(iou_offset), _np(dt_area), _np(gt_area),
                                    _np(gt_flag), iou_thrs.cpu().numpy(), None if area_rngs is None else area_rngs.cpu().numpy(),
                                    only=only)

    if not any(on_device(t) for t in tensors):
        out = host()
        return torch.from_numpy(out) if not coco else tuple(torch.from_numpy(o) for o in out)
    _need_cuda("eval_match", *tensors)
    dev = iou.device
    iou_thrs = iou_thrs.to(dev)
    if coco:
        area_rngs = area_rngs.to(dev)
        dtm = torch.full((A, T, D_total), -1, dtype=torch.int32, device=dev)
        dti = torch.zeros((A, T, D_total), dtype=torch.uint8, device=dev)
        gti = torch.zeros((A, G_total), dtype=torch.uint8, device=dev)
        vm = None
    else:
        A = T = 0
        dtm = dti = gti = None
        vm = torch.zeros((D_total,), dtype=torch.int8, device=dev)
    rc = 0
    if P:
        with _on_device(iou), _timed(("eval_match[P=%d]", (P,)), iou):
            rc = lib.detops_eval_match(mode, ptr(iou), ptr(dt_offset), ptr(gt_offset), ptr(iou_offset), P, D_total, G_total, max_gt, ptr(dt_area),
                                       ptr(gt_area), ptr(gt_flag), ptr(iou_thrs), T, ptr(area_rngs), A, ptr(dtm), ptr(dti),
                                       ptr(gti), ptr(vm), stream_of(iou))
        if rc != _EGTCAP:
            check(rc, "eval_match")
    if rc == _EGTCAP:       # the problems beyond the cap: numpy, patched in
        g = gt_offset.cpu().numpy()
        big = [p for p in range(P) if int(g[p + 1]) - int(g[p]) > EVAL_MAX_GT]
        out = host(only=big)
        d = dt_offset.cpu().numpy()
        for p in big:
            d0, d1, g0, g1 = int(d[p]), int(d[p + 1]), int(g[p]), int(g[p + 1])
            if coco:
                dtm[:, :, d0:d1] = torch.from_numpy(out[0][:, :, d0:d1]).to(dev)
                dti[:, :, d0:d1] = torch.from_numpy(out[1][:, :, d0:d1]).to(dev)
                gti[:, g0:g1] = torch.from_numpy(out[2][:, g0:g1]).to(dev)
            else:
                vm[d0:d1] = torch.from_numpy(out[d0:d1]).to(dev)
    return (dtm, dti, gti) if coco else vm


EVAL_OKS_MAX_K = _lib._abi.EVAL_OKS_MAX_K        # DETOPS_EVAL_OKS_MAX_K: the largest K detops_eval_oks serves


def eval_oks(dt_kpts, gt_kpts, gt_boxes, gt_area, sigmas, dt_offset, gt_offset, iou_offset, total_pairs):
    """The fp64 OKS matrices of every problem and the detections' keypoint-extent areas (extension; include/detops.h:
    detops_eval_oks).  dt_kpts [D_total, K, 3] / gt_kpts [G_total, K, 3] fp32 rows of (x, y, v), gt_boxes fp32 xyxy
    [G_total, 4], gt_area fp64 [G_total], everything in sorted (problem) order; sigmas fp64 [K] -> (oks float64
    [total_pairs], dt_area float64 [D_total]).  Device tensors go to the kernel; CPU tensors, and K above EVAL_OKS_MAX_K,
    take the numpy form of the same definition (_eval_cpu.eval_oks)."""
    dt_offset, gt_offset, iou_offset, P = _problem_args("eval_oks", dt_offset, gt_offset, iou_offset)
    total_pairs = int(total_pairs)
    sigmas = torch.as_tensor(sigmas, dtype=torch.float64).reshape(-1).contiguous()
    K = sigmas.numel()
    if K < 1 or dt_kpts.dim() != 3 or gt_kpts.dim() != 3 or tuple(dt_kpts.shape[1:]) != (K, 3) or tuple(gt_kpts.shape[1:]) != (K, 3):
        raise ValueError("eval_oks: expected keypoints [*, K, 3] for K = %d sigmas, got %s and %s"
                         % (K, tuple(dt_kpts.shape), tuple(gt_kpts.shape)))
    dt_kpts, gt_kpts = dt_kpts.to(torch.float32).contiguous(), gt_kpts.to(torch.float32).contiguous()
    gt_boxes = gt_boxes.to(torch.float32).contiguous().reshape(-1, 4)
    gt_area = gt_area.to(torch.float64).contiguous().reshape(-1)
    D_total, G_total = dt_kpts.shape[0], gt_kpts.shape[0]
    if gt_boxes.shape[0] != G_total or gt_area.numel() != G_total:
        raise ValueError("eval_oks: gt_boxes and gt_area do not match the %d ground truths" % G_total)
    tensors = (dt_kpts, gt_kpts, gt_boxes, gt_area, dt_offset, gt_offset, iou_offset)
    dev = dt_offset.device
    if not any(on_device(t) for t in tensors) or K > EVAL_OKS_MAX_K:
        oks, area = _eval_cpu.eval_oks(_np(dt_kpts), _np(gt_kpts), _np(gt_boxes), _np(gt_area), sigmas.cpu().numpy(),
                                       _np(dt_offset), _np(gt_offset), _np(iou_offset))
        return torch.from_numpy(oks).to(dev), torch.from_numpy(area).to(dev)
    _need_cuda("eval_oks", *tensors)
    sigmas = sigmas.to(dev)
    oks = torch.empty((total_pairs,), dtype=torch.float64, device=dev)
    area = torch.empty((D_total,), dtype=torch.float64, device=dev)
    if total_pairs or D_total:
        with _on_device(oks), _timed(("eval_oks[pairs=%d,K=%d]", (total_pairs, K)), oks):
            check(lib.detops_eval_oks(ptr(dt_kpts), ptr(gt_kpts), ptr(gt_boxes), ptr(gt_area), ptr(sigmas), K, ptr(dt_offset),
                                      ptr(gt_offset), ptr(iou_offset), P, D_total, total_pairs, ptr(oks), ptr(area),
                                      stream_of(oks)), "eval_oks")
    return oks, area


EVAL_PROPOSALS_MAX_DT = _lib._abi.EVAL_PROPOSALS_MAX_DT      # DETOPS_EVAL_PROPOSALS_MAX_DT / _MAX_GT: the largest number of
EVAL_PROPOSALS_MAX_GT = _lib._abi.EVAL_PROPOSALS_MAX_GT      # proposals taking part / ground truths of one image served


def eval_proposal_overlaps(dt_boxes, gt_boxes, dt_offset, gt_offset, gt_valid, limits, max_dt=None, max_gt=None):
    """The greedy matching behind the average recall of proposals, for every (limit, area range) of a batch in one launch
    (include/detops.h: detops_eval_proposal_overlaps).  dt_boxes [D_total, 4] fp32 xyxy, image after image and in
    objectness order (descending) inside an image; gt_boxes [G_total, 4]; dt_offset / gt_offset [N + 1] int32; gt_valid
    [A, G_total] bool / uint8; limits: a sequence of L ints (<= 0 or None: no limit) -> float32 [L, A, G_total]: the IoU a
    ground truth is matched with, 0 where no round reaches it, -1 where gt_valid is 0.
    max_dt / max_gt: the largest number of proposals / ground truths of one image, where the caller knows them on the host
    (None: read from the offsets).  Device tensors go to the kernel; CPU tensors, and images beyond
    EVAL_PROPOSALS_MAX_DT proposals taking part or EVAL_PROPOSALS_MAX_GT ground truths, take the numpy form of the same
    definition (_eval_cpu.eval_proposal_overlaps)."""
    if dt_offset.dtype != torch.int32 or gt_offset.dtype != torch.int32 or not (dt_offset.numel() == gt_offset.numel() >= 1):
        raise ValueError("eval_proposal_overlaps: expected dt_offset / gt_offset [N + 1] int32")
    dt_offset, gt_offset = dt_offset.contiguous(), gt_offset.contiguous()
    N = dt_offset.numel() - 1
    dt_boxes, gt_boxes = (t.to(torch.float32).contiguous().reshape(-1, 4) for t in (dt_boxes, gt_boxes))
    D_total, G_total = dt_boxes.shape[0], gt_boxes.shape[0]
    limits = [0 if v is None else int(v) for v in limits]
    if not limits or gt_valid.dim() != 2 or gt_valid.shape[0] < 1 or gt_valid.shape[1] != G_total:
        raise ValueError("eval_proposal_overlaps: expected at least one limit and gt_valid [A >= 1, %d], got %d and %s"
                         % (G_total, len(limits), tuple(gt_valid.shape)))
    gt_valid = _u8("eval_proposal_overlaps", gt_valid)
    L, A = len(limits), gt_valid.shape[0]
    tensors = (dt_boxes, gt_boxes, dt_offset, gt_offset, gt_valid)
    dev = gt_boxes.device
    if max_dt is None or max_gt is None:
        do, go = _np(dt_offset).astype(np.int64), _np(gt_offset).astype(np.int64)
        max_dt = int(np.diff(do).max()) if N else 0
        max_gt = int(np.diff(go).max()) if N else 0
    part = max(min(int(max_dt), v) if v > 0 else int(max_dt) for v in limits)       # the largest P' of the call
    if not any(on_device(t) for t in tensors) or part > EVAL_PROPOSALS_MAX_DT or int(max_gt) > EVAL_PROPOSALS_MAX_GT:
        out = _eval_cpu.eval_proposal_overlaps(_np(dt_boxes), _np(gt_boxes), _np(dt_offset), _np(gt_offset), _np(gt_valid), limits)
        return torch.from_numpy(out).to(dev)
    _need_cuda("eval_proposal_overlaps", *tensors)
    out = torch.empty((L, A, G_total), dtype=torch.float32, device=dev)
    if N and G_total:
        lim = torch.tensor(limits, dtype=torch.int32).to(dev)
        with _on_device(out), _timed(("eval_proposal_overlaps[N=%d,D=%d,G=%d]", (N, D_total, G_total)), out):
            check(lib.detops_eval_proposal_overlaps(ptr(dt_boxes), ptr(gt_boxes), ptr(dt_offset), ptr(gt_offset), ptr(gt_valid),
                                                    ptr(lim), N, L, A, D_total, G_total, part, int(max_gt), ptr(out),
                                                    stream_of(out)), "eval_proposal_overlaps")
    return out


WINDOW_COUNTS_MAX_ITEMS = _lib._abi.WINDOW_COUNTS_MAX_ITEMS      # DETOPS_WINDOW_COUNTS_MAX_ITEMS: D + G + D * G stays below it


def window_counts(dt_planes, dt_box, gt_planes, gt_box):
    """The counts behind the Cityscapes AP of ONE image in one call (include/detops.h: detops_window_counts).
    dt_planes [D, H, W], gt_planes [G, H, W] bool / uint8 (a non-zero byte is a set pixel); dt_box [D, 4], gt_box [G, 4]
    int32 (xmin, ymin, xmax, ymax), the maxima exclusive -> (dt_count [D], gt_count [G], pair_box [D, G], pair_mask [D, G]),
    all int32: the planes' set pixels inside their own boxes, and for every pair whose boxes overlap the box intersection
    and the pixels set in both planes inside the union box; 0 for the other pairs.  Windows are clamped to the image.
    Device tensors go to the kernel; CPU tensors take the numpy form of the same definition (_eval_cpu.window_counts)."""
    if dt_planes.dim() != 3 or gt_planes.dim() != 3 or tuple(dt_planes.shape[1:]) != tuple(gt_planes.shape[1:]):
        raise ValueError("window_counts: expected planes [D, H, W] and [G, H, W] of one image, got %s and %s"
                         % (tuple(dt_planes.shape), tuple(gt_planes.shape)))
    dt_planes, gt_planes = _u8("window_counts", dt_planes), _u8("window_counts", gt_planes)
    (D, H, W), G = dt_planes.shape, gt_planes.shape[0]
    if dt_box.dtype != torch.int32 or gt_box.dtype != torch.int32 or tuple(dt_box.shape) != (D, 4) or tuple(gt_box.shape) != (G, 4):
        raise ValueError("window_counts: expected int32 boxes [%d, 4] and [%d, 4], got %s %s and %s %s"
                         % (D, G, dt_box.dtype, tuple(dt_box.shape), gt_box.dtype, tuple(gt_box.shape)))
    if H * W >= 2 ** 31 or D + G + D * G >= WINDOW_COUNTS_MAX_ITEMS:
        raise ValueError("window_counts: H * W = %d must stay below 2^31 and D + G + D * G = %d below %d"
                         % (H * W, D + G + D * G, WINDOW_COUNTS_MAX_ITEMS))
    dt_box, gt_box = dt_box.contiguous(), gt_box.contiguous()
    tensors = (dt_planes, dt_box, gt_planes, gt_box)
    dev = dt_planes.device
    if not any(on_device(t) for t in tensors):
        out = _eval_cpu.window_counts(_np(dt_planes), _np(dt_box), _np(gt_planes), _np(gt_box))
        return tuple(torch.from_numpy(o) for o in out)
    _need_cuda("window_counts", *tensors)
    i32 = dict(dtype=torch.int32, device=dev)
    out = (torch.empty((D,), **i32), torch.empty((G,), **i32), torch.empty((D, G), **i32), torch.empty((D, G), **i32))
    if D + G:
        with _on_device(dt_planes), _timed(("window_counts[D=%d,G=%d,H=%d,W=%d]", (D, G, H, W)), out[0]):
            check(lib.detops_window_counts(ptr(dt_planes), ptr(dt_box), D, ptr(gt_planes), ptr(gt_box), G, H, W,
                                           *(ptr(o) for o in out), stream_of(dt_planes)), "window_counts")
    return out


def match_labels(matched, gt_labels=None, valid=None, dtype=torch.int64):
    """Matcher output [N,K] -> labels in one launch (extension; reference modeling/rpn/loss.py:70-88,
    roi_heads/box_head/loss.py:56-72): matched >= 0 -> gt_labels[n, matched] (1 when gt_labels is None), -1 -> 0,
    -2 -> -1, and -1 where `valid` [N,K] is false.  dtype float32 or int64."""
    _need_cuda("match_labels", matched, gt_labels, valid)
    if matched.dtype != torch.int64 or matched.dim() != 2 or dtype not in (torch.float32, torch.int64):
        raise ValueError("match_labels: matched must be [N, K] int64 and dtype float32 / int64")
    matched = matched.contiguous()
    N, K = matched.shape
    M = 0
    if gt_labels is not None:
        gt_labels = gt_labels.to(torch.int64).contiguous()
        M = gt_labels.size(1)
        if gt_labels.size(0) != N:
            raise ValueError("match_labels: gt_labels must be [N, M]")
    if valid is not None:
        valid = _u8("match_labels", valid)
        if valid.shape != matched.shape:
            raise ValueError("match_labels: valid must be [N, K]")
    out = torch.empty((N, K), dtype=dtype, device=matched.device)
    if N * K:
        with _on_device(matched), _timed(("match_labels[N=%d,K=%d]", (N, K)), matched):
            check(lib.detops_match_labels(ptr(matched), ptr(gt_labels) if gt_labels is not None else None,
                                          ptr(valid) if valid is not None else None, N, K, M,
                                          0 if dtype == torch.float32 else 1, ptr(out), stream_of(matched)), "match_labels")
    return out


def roi_head_targets(boxes, matched, gt_boxes, gt_labels, valid, idx, slot_valid, objectness, weights):
    """The box head's sampled slots in one launch (extension; reference roi_heads/box_head/loss.py:56-110):
    boxes [N,K,4], matched [N,K], gt_boxes [N,M,4], gt_labels [N,M], valid [N,K] | None, idx / slot_valid [N,B],
    objectness [N,K] | None -> (boxes [N,B,4], labels [N,B] int64, regression_targets [N,B,4], matched [N,B],
    objectness [N,B] | None)."""
    _need_cuda("roi_head_targets", boxes, matched, gt_boxes, gt_labels, valid, idx, slot_valid, objectness)
    boxes = _f32c("roi_head_targets", boxes)
    gt_boxes = _f32c("roi_head_targets", gt_boxes)
    matched, idx = matched.contiguous(), idx.contiguous()
    gt_labels = gt_labels.to(torch.int64).contiguous()
    slot_valid = _u8("roi_head_targets", slot_valid)
    N, K = matched.shape
    M, B = gt_boxes.size(1), idx.size(1)
    if matched.dtype != torch.int64 or idx.dtype != torch.int64 or boxes.shape != (N, K, 4) or gt_boxes.shape != (N, M, 4) \
            or gt_labels.shape != (N, M) or idx.shape != (N, B) or slot_valid.shape != (N, B):
        raise ValueError("roi_head_targets: inconsistent arguments")
    if valid is not None:
        valid = _u8("roi_head_targets", valid)
        if valid.shape != (N, K):
            raise ValueError("roi_head_targets: valid must be [N, K]")
    if objectness is not None:
        objectness = _f32c("roi_head_targets", objectness)
        if objectness.shape != (N, K):
            raise ValueError("roi_head_targets: objectness must be [N, K]")
    dev = boxes.device
    ob = torch.empty((N, B, 4), dtype=torch.float32, device=dev)
    oreg = torch.empty((N, B, 4), dtype=torch.float32, device=dev)
    ol = torch.empty((N, B), dtype=torch.int64, device=dev)
    om = torch.empty((N, B), dtype=torch.int64, device=dev)
    oo = torch.empty((N, B), dtype=torch.float32, device=dev) if objectness is not None else None
    if N * B:
        if K == 0 or M == 0:
            raise ValueError("roi_head_targets: no proposals / ground truth rows to take the slots from")
        wx, wy, ww, wh = (float(w) for w in weights)
        with _on_device(boxes), _timed(("roi_head_targets[N=%d,B=%d]", (N, B)), boxes):
            check(lib.detops_roi_head_targets_f32(
                ptr(boxes), ptr(matched), ptr(gt_boxes), ptr(gt_labels), ptr(valid) if valid is not None else None, ptr(idx),
                ptr(slot_valid), ptr(objectness) if objectness is not None else None, N, K, M, B, wx, wy, ww, wh, ptr(ob),
                ptr(ol), ptr(oreg), ptr(om), ptr(oo) if oo is not None else None, stream_of(boxes)), "roi_head_targets")
    return ob, ol, oreg, om, oo


def rpn_decode(box_regression, topk_idx, topk_scores, anchors, image_hw, weights, bbox_xform_clip, min_size,
               boxes, scores, col, nms_boxes, nms_scores, ok, off):
    """Box path of RPN proposal selection for one level in ONE launch (extension; reference
    modeling/rpn/inference.py:75-110 + box_coder.py:61-95): decodes the top-k anchors straight from the head output
    [N,4A,H,W] and writes boxes[:, col:col+k] / scores[:, col:col+k] of the image-major result and rows
    [off, off+N*k) of the level-major NMS input (nms_boxes, nms_scores, ok uint8)."""
    _need_cuda("rpn_decode", box_regression, topk_idx, topk_scores, anchors, image_hw, boxes, scores)
    reg = _f32c("rpn_decode", box_regression)
    topk_scores = _f32c("rpn_decode", topk_scores)
    anchors = _f32c("rpn_decode", anchors)
    topk_idx = topk_idx.contiguous()
    N, A4, H, W = reg.shape
    k = topk_idx.size(1)
    if topk_idx.dtype != torch.int64 or A4 % 4 or anchors.size(0) != (A4 // 4) * H * W or image_hw.shape != (N, 2):
        raise ValueError("rpn_decode: inconsistent arguments")
    for t in (boxes, scores, nms_boxes, nms_scores, ok):
        if not t.is_contiguous():
            raise ValueError("rpn_decode: outputs must be contiguous")
    if boxes.dtype != torch.float32 or scores.dtype != torch.float32 or ok.dtype != torch.uint8 \
            or col + k > boxes.size(1) or off + N * k > nms_scores.numel():
        raise ValueError("rpn_decode: outputs do not fit")
    if N * k == 0:
        return
    wx, wy, ww, wh = (float(w) for w in weights)
    with _on_device(reg), _timed(("rpn_decode[N=%d,k=%d]", (N, k)), reg):
        check(lib.detops_rpn_decode_f32(
            ptr(reg), ptr(topk_idx), ptr(topk_scores), ptr(anchors), ptr(image_hw), N, A4 // 4, H, W, k, wx, wy, ww, wh,
            float(bbox_xform_clip), float(min_size), boxes.data_ptr() + 16 * col, 4 * boxes.size(1),
            scores.data_ptr() + 4 * col, scores.size(1), nms_boxes.data_ptr() + 16 * off, nms_scores.data_ptr() + 4 * off,
            ok.data_ptr() + off, stream_of(reg)), "rpn_decode")


# ------------------------------------------------------------------------------------------ ROIAlign
def roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio):
    """reference csrc/ROIAlign.h:11-25 -> [K,C,PH,PW]."""
    if _f64(input):
        return _roi_align_forward_f64(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio)
    if not on_device(input) and not on_device(rois):
        return _roi_align_forward_cpu(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio)
    _need_cuda("roi_align_forward", input, rois)
    input = _f32c("roi_align_forward", input)
    rois = _f32c("roi_align_forward", rois)
    N, C, H, W = input.shape
    K = rois.size(0)
    out = torch.empty((K, C, pooled_height, pooled_width), dtype=input.dtype, device=input.device)
    if out.numel() == 0:
        return out
    with _on_device(input):
        ws, nbytes = _fwd_workspace(input.device, K, pooled_height, pooled_width, sampling_ratio)
        check(lib.detops_roi_align_forward_ws_f32(ptr(input), ptr(rois), ptr(out), N, C, H, W, K,
                                                  pooled_height, pooled_width, float(spatial_scale),
                                                  int(sampling_ratio), ptr(ws), nbytes, stream_of(input)),
              "roi_align_forward")
    return out


def _roi_align_forward_cpu(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio):
    """CPU tensors: the reference dispatches to ROIAlign_forward_cpu (csrc/ROIAlign.h:19-24); host code of the
    same library (csrc/cpu_branch.hip).  Not a fallback of the device path: CUDA tensors never come here."""
    input = _f32c("roi_align_forward", input)
    rois = _f32c("roi_align_forward", rois)
    N, C, H, W = input.shape
    K = rois.size(0)
    out = torch.empty((K, C, pooled_height, pooled_width), dtype=torch.float32)
    if out.numel() == 0:
        return out
    check(lib.detops_roi_align_forward_cpu_f32(ptr(input), ptr(rois), ptr(out), N, C, H, W, K, pooled_height,
                                               pooled_width, float(spatial_scale), int(sampling_ratio)),
          "roi_align_forward(cpu)")
    return out


def _fwd_workspace(device, K, ph, pw, sr):
    """Scratch for the forward's pre-pass (per-ROI sample records; the ROI visiting order for K >= 384), from
    torch's stream-ordered caching allocator; (None, 0) when this shape is served without a pre-pass."""
    nbytes = int(lib.detops_roi_align_forward_workspace_bytes(int(K), int(ph), int(pw), int(sr)))
    if nbytes <= 0:
        return None, 0
    return torch.empty((nbytes,), dtype=torch.uint8, device=device), nbytes


def roi_align_backward(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels,
                       height, width, sampling_ratio):
    """reference csrc/ROIAlign.h:27-45 -> zero-initialised [bs,ch,h,w] with the scattered grads."""
    if _f64(grad):
        return _roi_align_backward_f64(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height, width,
                                       sampling_ratio)
    _need_cuda("roi_align_backward", grad, rois)
    grad = _f32c("roi_align_backward", grad)
    rois = _f32c("roi_align_backward", rois)
    K = rois.size(0)
    gin = torch.empty((batch_size, channels, height, width), dtype=grad.dtype, device=grad.device)
    with _on_device(grad):
        Hs, Ws = (ctypes.c_int * 1)(height), (ctypes.c_int * 1)(width)
        ws, nbytes = _bwd_workspace(grad.device, Hs, Ws, 1, batch_size, channels, K, pooled_height, pooled_width)
        check(lib.detops_roi_align_backward_ws_f32(ptr(grad), ptr(rois), ptr(gin), batch_size, channels,
                                                   height, width, K, pooled_height, pooled_width,
                                                   float(spatial_scale), int(sampling_ratio), 1, ptr(ws), nbytes,
                                                   stream_of(grad)), "roi_align_backward")
    return gin


def _bwd_workspace(device, Hs, Ws, L, N, C, K, ph, pw):
    """Scratch for the binned ROIAlign backward (per-ROI adjoint rows + per-tile hit lists), from
    torch's stream-ordered caching allocator; (None, 0) when the shape uses the workspace-free kernels."""
    nbytes = int(lib.detops_roi_align_backward_workspace_bytes(Hs, Ws, L, int(N), int(C), int(K), int(ph), int(pw)))
    if nbytes <= 0:
        return None, 0
    return torch.empty((nbytes,), dtype=torch.uint8, device=device), nbytes


def _host_arrays(tensors, scales):
    L = len(tensors)
    ptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in tensors])
    Hs = (ctypes.c_int * L)(*[t.size(2) for t in tensors])
    Ws = (ctypes.c_int * L)(*[t.size(3) for t in tensors])
    sc = (ctypes.c_float * L)(*[float(s) for s in scales])
    return ptrs, Hs, Ws, sc


def _nhwc_host_arrays(tensors, scales):
    """(pointer array, H array, W array, scale array) of channels-last [N, C, H, W] tensors (stored [N, H, W, C])"""
    return _host_arrays(tensors, scales)


def roi_align_fpn_forward(inputs, rois, scales, pooled_height, pooled_width, sampling_ratio, k_min,
                          k_max, canonical_scale=224.0, canonical_level=4.0, eps=1e-6, out_channels_last=False):
    """Multi-level ROIAlign in one launch (extension): the device-side form of
    modeling/poolers.py:91-121.  Returns (out [K,C,PH,PW], levels int32 [K]).
    A channels-last pyramid (every level stored NHWC) is read in place by the NHWC kernels (csrc/roi_align_nhwc.hip: same
    values, bit for bit); `out_channels_last` then returns the pooled tensor channels-last as well (for a convolutional
    head) instead of contiguous (for the box head's FC layer)."""
    _need_cuda("roi_align_fpn_forward", rois, *inputs)
    if all(is_channels_last(t) for t in inputs) and inputs[0].dtype == torch.float32:
        return _roi_align_fpn_forward_nhwc(inputs, rois, scales, pooled_height, pooled_width, sampling_ratio, k_min, k_max,
                                           canonical_scale, canonical_level, eps, out_channels_last)
    inputs = [_f32c("roi_align_fpn_forward", t) for t in inputs]
    rois = _f32c("roi_align_fpn_forward", rois)
    N, C = inputs[0].shape[:2]
    K = rois.size(0)
    out = torch.empty((K, C, pooled_height, pooled_width), dtype=torch.float32, device=rois.device)
    levels = torch.empty((K,), dtype=torch.int32, device=rois.device)
    if K == 0:
        return out, levels
    ptrs, Hs, Ws, sc = _host_arrays(inputs, scales)
    with _on_device(rois), _timed(("roi_align_fpn_fwd[K=%d,C=%d,%dx%d]", (K, C, pooled_height, pooled_width)), rois):
        ws, nbytes = _fwd_workspace(rois.device, K, pooled_height, pooled_width, sampling_ratio)
        check(lib.detops_roi_align_fpn_forward_ws_f32(
            ptrs, Hs, Ws, sc, len(inputs), ptr(rois), ptr(out), ptr(levels), N, C, K, pooled_height,
            pooled_width, int(sampling_ratio), int(k_min), int(k_max), float(canonical_scale),
            float(canonical_level), float(eps), ptr(ws), nbytes, stream_of(rois)), "roi_align_fpn_forward")
    return out, levels


def _roi_align_fpn_forward_nhwc(inputs, rois, scales, pooled_height, pooled_width, sampling_ratio, k_min, k_max,
                                canonical_scale, canonical_level, eps, out_channels_last):
    rois = _f32c("roi_align_fpn_forward", rois)
    N, C = inputs[0].shape[:2]
    K = rois.size(0)
    fmt = torch.channels_last if out_channels_last else torch.contiguous_format
    out = torch.empty((K, C, pooled_height, pooled_width), dtype=torch.float32, device=rois.device, memory_format=fmt)
    levels = torch.empty((K,), dtype=torch.int32, device=rois.device)
    if K == 0:
        return out, levels
    ptrs, Hs, Ws, sc = _nhwc_host_arrays(inputs, scales)
    with _on_device(rois), _timed(("roi_align_fpn_fwd[K=%d,C=%d,%dx%d]", (K, C, pooled_height, pooled_width)), rois):
        nbytes = int(lib.detops_roi_align_fpn_forward_nhwc_workspace_bytes(int(K)))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=rois.device) if nbytes > 0 else None
        check(lib.detops_roi_align_fpn_forward_nhwc_f32(
            ptrs, Hs, Ws, sc, len(inputs), ptr(rois), ptr(out), int(bool(out_channels_last)), ptr(levels), N, C, K,
            pooled_height, pooled_width, int(sampling_ratio), int(k_min), int(k_max), float(canonical_scale),
            float(canonical_level), float(eps), ptr(ws), nbytes, stream_of(rois)), "roi_align_fpn_forward_nhwc")
    return out, levels


_SIDE_STREAMS = {}


def _side_stream(device):
    """one auxiliary stream per device for work that only has to be finished by the backward pass"""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    s = _SIDE_STREAMS.get(idx)
    if s is None:
        s = _SIDE_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return s


def roi_align_fpn_backward_prepare(rois, levels, shapes, scales, pooled_height, pooled_width, sampling_ratio):
    """The backward's pre-pass (per-ROI adjoint rows + per-tile hit lists: a function of the ROIs and the map shapes only),
    issued at FORWARD time on a side stream so that it is off the backward pass's critical path.  Returns an opaque
    handle for roi_align_fpn_backward(prepared=...), or None when the shape is served by the one-call kernels."""
    K = rois.size(0)
    if K == 0 or not on_device(rois):
        return None
    N, C = shapes[0][:2]
    L = len(shapes)
    Hs = (ctypes.c_int * L)(*[s[2] for s in shapes])
    Ws = (ctypes.c_int * L)(*[s[3] for s in shapes])
    sc = (ctypes.c_float * L)(*[float(s) for s in scales])
    nbytes = int(lib.detops_roi_align_backward_workspace_bytes(Hs, Ws, L, int(N), int(C), int(K), int(pooled_height), int(pooled_width)))
    if nbytes <= 0:
        return None
    main = torch.cuda.current_stream(rois.device)
    side = _side_stream(rois.device)
    side.wait_stream(main)                       # the ROIs and their levels are produced on the main stream
    with torch.cuda.stream(side):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=rois.device)
        with _timed(("roi_align_fpn_bwd_prepare[K=%d,C=%d,%dx%d]", (K, C, pooled_height, pooled_width)), rois):
            rc = lib.detops_roi_align_fpn_backward_prepare_f32(
                ptr(rois), ptr(levels), Hs, Ws, sc, L, int(N), int(C), int(K), int(pooled_height), int(pooled_width),
                int(sampling_ratio), ptr(ws), nbytes, side.cuda_stream)
        if rc == -3:                             # DETOPS_EUNSUPPORTED: the other kernels serve this shape
            return None
        check(rc, "roi_align_fpn_backward_prepare")
        done = torch.cuda.Event()
        done.record(side)
    ws.record_stream(main)                       # used by the backward pass on the main stream
    rois.record_stream(side)
    levels.record_stream(side)
    return ws, nbytes, done


def roi_align_fpn_backward(grad, rois, levels, shapes, scales, pooled_height, pooled_width,
                           sampling_ratio, prepared=None, channels_last=False):
    """Backward of roi_align_fpn_forward: returns one zero-initialised gradient map per level.  `prepared`: the handle of
    roi_align_fpn_backward_prepare (the pre-pass already ran): only the main kernel is launched.  `channels_last`: the
    forward read a channels-last pyramid — the gradient maps are produced channels-last by the NHWC kernel
    (csrc/roi_align_nhwc.hip), from a contiguous or a channels-last pooled gradient alike."""
    _need_cuda("roi_align_fpn_backward", grad, rois, levels)
    if channels_last:
        return _roi_align_fpn_backward_nhwc(grad, rois, levels, shapes, scales, pooled_height, pooled_width, sampling_ratio)
    grad = _f32c("roi_align_fpn_backward", grad)
    K = rois.size(0)
    gins = [torch.empty(tuple(s), dtype=torch.float32, device=grad.device) for s in shapes]
    N, C = shapes[0][:2]
    ptrs, Hs, Ws, sc = _host_arrays(gins, scales)
    if prepared is not None:
        ws, nbytes, done = prepared
        with _on_device(grad):
            torch.cuda.current_stream(grad.device).wait_event(done)
            with _timed(("roi_align_fpn_bwd[K=%d,C=%d,%dx%d]", (K, C, pooled_height, pooled_width)), grad):
                check(lib.detops_roi_align_fpn_backward_prepared_f32(
                    ptr(grad), ptrs, Hs, Ws, sc, len(gins), N, C, K, pooled_height, pooled_width, 1, ptr(ws), nbytes,
                    stream_of(grad)), "roi_align_fpn_backward(prepared)")
        return gins
    with _on_device(grad):
        ws, nbytes = _bwd_workspace(grad.device, Hs, Ws, len(gins), N, C, K, pooled_height, pooled_width)
        with _timed(("roi_align_fpn_bwd[K=%d,C=%d,%dx%d]", (K, C, pooled_height, pooled_width)), grad):
            check(lib.detops_roi_align_fpn_backward_ws_f32(
                ptr(grad), ptr(rois), ptr(levels), ptrs, Hs, Ws, sc, len(gins), N, C, K, pooled_height,
                pooled_width, int(sampling_ratio), 1, ptr(ws), nbytes, stream_of(grad)), "roi_align_fpn_backward")
    return gins


NHWC_BACKWARD = os.environ.get("DETOPS_ROIALIGN_NHWC_BWD", "auto")   # auto | ring | native  (A/B switch)


def _roi_align_fpn_backward_nhwc(grad, rois, levels, shapes, scales, pooled_height, pooled_width, sampling_ratio):
    """Channels-last gradient maps.  Two kernels serve this: the pixel-owner ring kernel of the NCHW path with a channels-last
    store epilogue (csrc/roi_align_bwd.hip: 7 x 7 / 14 x 14 bins on launches that fill the chip — the model's shapes; the
    pooled gradient is read as [K, C, PH, PW]), and the NHWC-native hit-parallel kernel (csrc/roi_align_nhwc.hip: any shape,
    contiguous or channels-last pooled gradient).  "auto": the ring kernel where its plan applies (measured 3x faster at the
    model's shapes, profiles/r06*), the native kernel otherwise."""
    if grad.dtype != torch.float32:
        raise RuntimeError("roi_align_fpn_backward: expected a float32 gradient, got %s" % grad.dtype)
    rois = _f32c("roi_align_fpn_backward", rois)
    K = rois.size(0)
    gins = [torch.empty(tuple(s), dtype=torch.float32, device=grad.device, memory_format=torch.channels_last) for s in shapes]
    N, C = shapes[0][:2]
    ptrs, Hs, Ws, sc = _nhwc_host_arrays(gins, scales)
    with _on_device(grad):
        if NHWC_BACKWARD != "native" and K > 0:
            g = grad.contiguous()          # [K, C, PH, PW] (a channels-last pooled gradient is converted: 51 MB for the mask head)
            ws, nbytes = _bwd_workspace(grad.device, Hs, Ws, len(gins), N, C, K, pooled_height, pooled_width)
            if ws is not None:
                with _timed(("roi_align_fpn_bwd[K=%d,C=%d,%dx%d]", (K, C, pooled_height, pooled_width)), g):
                    rc = lib.detops_roi_align_fpn_backward_ring_nhwc_f32(
                        ptr(g), ptr(rois), ptr(levels), ptrs, Hs, Ws, sc, len(gins), N, C, K, pooled_height, pooled_width,
                        int(sampling_ratio), 1, ptr(ws), nbytes, stream_of(g))
                if rc == 0:
                    return gins
                if rc != -3:      # DETOPS_EUNSUPPORTED: the ring plan does not serve this shape
                    check(rc, "roi_align_fpn_backward_ring_nhwc")
            if NHWC_BACKWARD == "ring":
                raise RuntimeError("roi_align_fpn_backward: the ring plan does not serve this shape (DETOPS_ROIALIGN_NHWC_BWD=ring)")
        g_nhwc = is_channels_last(grad)
        if not g_nhwc:
            grad = grad.contiguous()
        nbytes = int(lib.detops_roi_align_fpn_backward_nhwc_workspace_bytes(Hs, Ws, len(gins), N, C, K, pooled_height, pooled_width))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=grad.device) if nbytes > 0 else None
        with _timed(("roi_align_fpn_bwd[K=%d,C=%d,%dx%d]", (K, C, pooled_height, pooled_width)), grad):
            check(lib.detops_roi_align_fpn_backward_nhwc_f32(
                ptr(grad), int(g_nhwc), ptr(rois), ptr(levels), ptrs, Hs, Ws, sc, len(gins), N, C, K, pooled_height,
                pooled_width, int(sampling_ratio), 1, ptr(ws), nbytes, stream_of(grad)), "roi_align_fpn_backward_nhwc")
    return gins


# ------------------------------------------------------------------------------------------ ROIPool
def roi_pool_forward(input, rois, spatial_scale, pooled_height, pooled_width):
    """reference csrc/ROIPool.h:11-24 -> (output, argmax int32)."""
    if _f64(input):
        return _roi_pool_forward_f64(input, rois, spatial_scale, pooled_height, pooled_width)
    _need_cuda("roi_pool_forward", input, rois)
    input = _f32c("roi_pool_forward", input)
    rois = _f32c("roi_pool_forward", rois)
    N, C, H, W = input.shape
    K = rois.size(0)
    out = torch.empty((K, C, pooled_height, pooled_width), dtype=input.dtype, device=input.device)
    argmax = torch.zeros((K, C, pooled_height, pooled_width), dtype=torch.int32, device=input.device)
    if out.numel() == 0:
        return out, argmax
    with _on_device(input):
        check(lib.detops_roi_pool_forward_f32(ptr(input), ptr(rois), ptr(out), ptr(argmax), N, C, H,
                                              W, K, pooled_height, pooled_width,
                                              float(spatial_scale), stream_of(input)),
              "roi_pool_forward")
    return out, argmax


def roi_pool_backward(grad, input, rois, argmax, spatial_scale, pooled_height, pooled_width,
                      batch_size, channels, height, width):
    """reference csrc/ROIPool.h:26-45 (`input` is unused there too)."""
    if _f64(grad):
        return _roi_pool_backward_f64(grad, rois, argmax, pooled_height, pooled_width, batch_size, channels, height, width)
    _need_cuda("roi_pool_backward", grad, rois, argmax)
    grad = _f32c("roi_pool_backward", grad)
    rois = _f32c("roi_pool_backward", rois)
    argmax = argmax.contiguous()
    K = rois.size(0)
    gin = torch.empty((batch_size, channels, height, width), dtype=grad.dtype, device=grad.device)
    with _on_device(grad):
        check(lib.detops_roi_pool_backward_f32(ptr(grad), ptr(rois), ptr(argmax), ptr(gin),
                                               batch_size, channels, height, width, K, pooled_height,
                                               pooled_width, 1, stream_of(grad)), "roi_pool_backward")
    return gin


# ------------------------------------------------------------------------------------------ focal
def _focal_args(name, logits, targets, num_classes):
    _need_cuda(name, logits, targets)
    if logits.dim() != 2:
        raise RuntimeError("logits should be NxClass")  # SigmoidFocalLoss_cuda.cu:112
    logits = _f32c(name, logits)
    if targets.dtype != torch.int32:
        raise RuntimeError("%s: targets must be int32 (reference kernel reads `const int*`)" % name)
    targets = targets.contiguous()
    if targets.numel() != logits.size(0) or logits.size(1) != num_classes:
        raise RuntimeError("%s: shape mismatch" % name)
    return logits, targets


def sigmoid_focalloss_forward(logits, targets, num_classes, gamma, alpha):
    """reference csrc/SigmoidFocalLoss.h:10-24 -> losses [R,C]."""
    if _f64(logits):
        return _focal_f64(logits, targets, None, num_classes, gamma, alpha)
    logits, targets = _focal_args("sigmoid_focalloss_forward", logits, targets, num_classes)
    losses = torch.empty_like(logits)
    with _on_device(logits):
        check(lib.detops_sigmoid_focal_loss_forward_f32(ptr(logits), ptr(targets), ptr(losses),
                                                        logits.size(0), num_classes, float(gamma),
                                                        float(alpha), stream_of(logits)),
              "sigmoid_focalloss_forward")
    return losses


def sigmoid_focalloss_backward(logits, targets, d_losses, num_classes, gamma, alpha):
    """reference csrc/SigmoidFocalLoss.h:26-41 -> d_logits [R,C]."""
    if _f64(logits):
        return _focal_f64(logits, targets, d_losses, num_classes, gamma, alpha)
    logits, targets = _focal_args("sigmoid_focalloss_backward", logits, targets, num_classes)
    _need_cuda("sigmoid_focalloss_backward", d_losses)
    d_losses = _f32c("sigmoid_focalloss_backward", d_losses)
    if d_losses.shape != logits.shape:
        raise RuntimeError("sigmoid_focalloss_backward: d_losses must be [R,C]")
    d_logits = torch.empty_like(logits)
    with _on_device(logits):
        check(lib.detops_sigmoid_focal_loss_backward_f32(ptr(logits), ptr(targets), ptr(d_losses),
                                                         ptr(d_logits), logits.size(0), num_classes,
                                                         float(gamma), float(alpha),
                                                         stream_of(logits)),
              "sigmoid_focalloss_backward")
    return d_logits


def sigmoid_focalloss_forward_sum(logits, targets, num_classes, gamma, alpha):
    """Extension: sum(losses) without materialising [R,C] (what SigmoidFocalLoss.forward needs).  Two launches
    (per-workgroup sums, then one fixed-order reduction) and nothing else: no zero-fill, no torch reduction."""
    logits, targets = _focal_args("sigmoid_focalloss_forward_sum", logits, targets, num_classes)
    nbytes = int(lib.detops_sigmoid_focal_loss_sum_workspace_bytes())
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=logits.device)
    total = torch.empty((), dtype=torch.float32, device=logits.device)
    with _on_device(logits), _timed(("focal_fwd_sum[R=%d,C=%d]", (logits.size(0), num_classes)), logits):
        check(lib.detops_sigmoid_focal_loss_forward_sum_ws_f32(
            ptr(logits), ptr(targets), None, ptr(total), logits.size(0), num_classes, float(gamma), float(alpha),
            ptr(ws), nbytes, stream_of(logits)), "sigmoid_focalloss_forward_sum")
    return total


def sigmoid_focalloss_backward_scalar(logits, targets, d_loss, num_classes, gamma, alpha):
    """Extension: backward of the summed loss; d_loss is a 0-dim / 1-element device tensor."""
    logits, targets = _focal_args("sigmoid_focalloss_backward_scalar", logits, targets, num_classes)
    _need_cuda("sigmoid_focalloss_backward_scalar", d_loss)
    d_loss = d_loss.reshape(1).to(torch.float32).contiguous()
    d_logits = torch.empty_like(logits)
    with _on_device(logits), _timed(("focal_bwd_scalar[R=%d,C=%d]", (logits.size(0), num_classes)), logits):
        check(lib.detops_sigmoid_focal_loss_backward_scalar_f32(
            ptr(logits), ptr(targets), ptr(d_loss), ptr(d_logits), logits.size(0), num_classes,
            float(gamma), float(alpha), stream_of(logits)), "sigmoid_focalloss_backward_scalar")
    return d_logits


# ------------------------------------------------------------------------------------------ frozen BN
def is_channels_last(t):
    """4-d tensor stored NHWC (and not at the same time plain-contiguous, e.g. C == 1 or H == W == 1)"""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def frozen_bn_act_forward(x, scale, bias, residual, relu):
    """Extension: y = [relu](x * scale[c] + bias[c] [+ residual]) in one pass.  NCHW-contiguous input -> NCHW output; a
    channels-last (NHWC) input is processed in place of its layout and returns a channels-last output (no transpose)."""
    _need_cuda("frozen_bn_act_forward", x, scale, bias, residual)
    code = _lib.DTYPE_CODE[x.dtype]
    nhwc = is_channels_last(x)
    if not nhwc:
        x = x.contiguous()
    if residual is not None:
        if residual.dtype != x.dtype or residual.shape != x.shape:
            raise RuntimeError("frozen_bn_act_forward: residual must match x")
        residual = residual.contiguous(memory_format=torch.channels_last) if nhwc else residual.contiguous()
    N, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(N * C, 1)
    y = torch.empty_like(x)      # preserves the memory format
    with _on_device(x), _timed(("frozen_bn_fwd[n=%d,nc=%d,e=%d,res=%d]", (x.numel(), N * C, _ESIZE[x.dtype], residual is not None)), x, every=8):
        if nhwc:
            check(lib.detops_frozen_bn_act_forward_nhwc(ptr(x), ptr(scale), ptr(bias), ptr(residual), ptr(y), code, N * HW, C,
                                                        int(bool(relu)), stream_of(x)), "frozen_bn_act_forward_nhwc")
        else:
            check(lib.detops_frozen_bn_act_forward(ptr(x), ptr(scale), ptr(bias), ptr(residual), ptr(y), code, N, C, HW,
                                                   int(bool(relu)), stream_of(x)), "frozen_bn_act_forward")
    return y


def frozen_bn_act_backward(grad_y, y, scale, relu, need_residual):
    """Extension: (grad_x, grad_residual or None) of frozen_bn_act_forward.  The layout follows the saved output `y` when
    there is one (ReLU), otherwise the incoming gradient's."""
    _need_cuda("frozen_bn_act_backward", grad_y, scale)
    code = _lib.DTYPE_CODE[grad_y.dtype]
    nhwc = is_channels_last(y) if (relu and y is not None) else is_channels_last(grad_y)
    grad_y = grad_y.contiguous(memory_format=torch.channels_last) if nhwc else grad_y.contiguous()
    N, C = grad_y.shape[0], grad_y.shape[1]
    HW = grad_y.numel() // max(N * C, 1)
    gx = torch.empty_like(grad_y)
    gres = torch.empty_like(grad_y) if need_residual else None
    with _on_device(grad_y), _timed(("frozen_bn_bwd[n=%d,nc=%d,e=%d,res=%d,relu=%d]", (grad_y.numel(), N * C, _ESIZE[grad_y.dtype], bool(need_residual), bool(relu))),
                                     grad_y, every=8):
        if nhwc:
            check(lib.detops_frozen_bn_act_backward_nhwc(ptr(grad_y), ptr(y) if relu else None, ptr(scale), ptr(gx), ptr(gres),
                                                         code, N * HW, C, int(bool(relu)), stream_of(grad_y)),
                  "frozen_bn_act_backward_nhwc")
        else:
            if relu and y is not None and not y.is_contiguous():
                y = y.contiguous()
            check(lib.detops_frozen_bn_act_backward(ptr(grad_y), ptr(y) if relu else None, ptr(scale), ptr(gx), ptr(gres),
                                                    code, N, C, HW, int(bool(relu)), stream_of(grad_y)),
                  "frozen_bn_act_backward")
    return gx, gres


# ------------------------------------------------------------------------------------------ group norm
# A/B switch DETOPS_GROUP_NORM: "fused" (default) channels-last GroupNorm (+ residual) (+ ReLU) runs in csrc/group_norm.hip |
# "torch" every GroupNorm layer calls F.group_norm (+ add) (+ relu).  Read once at import; layers.GroupNorm asks it per call.
GROUP_NORM = os.environ.get("DETOPS_GROUP_NORM", "fused")
if GROUP_NORM not in ("fused", "torch"):
    raise RuntimeError("DETOPS_GROUP_NORM must be 'fused' or 'torch', got %r" % GROUP_NORM)


GROUP_NORM_MAX_GROUP_WIDTH = 256      # kGnMaxD of csrc/group_norm.hip


def group_norm_serves(C, G):
    """the rule of detops_group_norm_supported, answered on the host (the routing of a layer that the library does not
    serve costs no library call; tests/test_group_norm_gpu.py holds the two against each other)"""
    D = C // G if G > 0 and C % G == 0 else 0
    return 0 < D <= GROUP_NORM_MAX_GROUP_WIDTH and D & (D - 1) == 0


def group_norm_supported(x, G):
    """True when group_norm_forward serves `x` with G groups: a non-empty fp32 / fp16 / bf16 channels-last 4-d device
    activation whose (C, G) the library serves (C % G == 0, a power-of-two group width of at most 256 channels)."""
    return (on_device(x) and x.dtype in _lib.DTYPE_CODE and is_channels_last(x) and x.numel() > 0
            and group_norm_serves(int(x.shape[1]), int(G)) and hasattr(lib, "detops_group_norm_forward_nhwc"))


def _gn_workspace(x, N, HW, C, G):
    nbytes = int(lib.detops_group_norm_workspace_bytes(N, HW, C, G))
    return torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=x.device), nbytes


def group_norm_forward(x, G, gamma, beta, eps, residual, relu):
    """Extension: (y, mean, rstd) with y = [relu](group_norm(x, G, gamma, beta, eps) [+ residual]) for a channels-last
    [N, C, H, W] activation, in the storage dtype of `x`; mean / rstd are fp32 [N, G].  gamma / beta: fp32 [C] or None."""
    _need_cuda("group_norm_forward", x, gamma, beta, residual)
    if not is_channels_last(x):
        raise RuntimeError("group_norm_forward: expected a channels-last 4-d activation")
    code = _lib.DTYPE_CODE[x.dtype]
    N, C = int(x.shape[0]), int(x.shape[1])
    HW = int(x.shape[2]) * int(x.shape[3])
    if residual is not None:
        if residual.dtype != x.dtype or residual.shape != x.shape:
            raise RuntimeError("group_norm_forward: residual must match x")
        residual = residual.contiguous(memory_format=torch.channels_last)
    gamma = None if gamma is None else _f32c("group_norm_forward", gamma)
    beta = None if beta is None else _f32c("group_norm_forward", beta)
    y = torch.empty_like(x)      # preserves the memory format
    mean = torch.empty((N, G), dtype=torch.float32, device=x.device)
    rstd = torch.empty((N, G), dtype=torch.float32, device=x.device)
    ws, nbytes = _gn_workspace(x, N, HW, C, G)
    with _on_device(x), _timed(("group_norm_fwd[n=%d,C=%d,G=%d,e=%d,res=%d]", (x.numel(), C, G, _ESIZE[x.dtype], residual is not None)), x, every=8):
        check(lib.detops_group_norm_forward_nhwc(ptr(x), ptr(gamma), ptr(beta), ptr(residual), ptr(y), ptr(mean), ptr(rstd), code,
                                                 N, HW, C, int(G), float(eps), int(bool(relu)), ptr(ws), nbytes, stream_of(x)),
              "group_norm_forward")
    return y, mean, rstd


def group_norm_backward(grad_y, x, y, G, gamma, mean, rstd, relu, need_residual, need_gamma, need_beta):
    """Extension: (grad_x, grad_residual or None, grad_gamma or None, grad_beta or None) of group_norm_forward.  `y` (the
    forward's output) is read only with relu.  Deterministic."""
    _need_cuda("group_norm_backward", grad_y, x, gamma, mean, rstd)
    code = _lib.DTYPE_CODE[x.dtype]
    if grad_y.dtype != x.dtype:
        grad_y = grad_y.to(x.dtype)
    grad_y = grad_y.contiguous(memory_format=torch.channels_last)
    N, C = int(x.shape[0]), int(x.shape[1])
    HW = int(x.shape[2]) * int(x.shape[3])
    gx = torch.empty_like(x)
    gres = torch.empty_like(x) if need_residual else None
    ggamma = torch.empty((C,), dtype=torch.float32, device=x.device) if need_gamma else None
    gbeta = torch.empty((C,), dtype=torch.float32, device=x.device) if need_beta else None
    ws, nbytes = _gn_workspace(x, N, HW, C, G)
    with _on_device(x), _timed(("group_norm_bwd[n=%d,C=%d,G=%d,e=%d,relu=%d]", (x.numel(), C, G, _ESIZE[x.dtype], bool(relu))), x, every=8):
        check(lib.detops_group_norm_backward_nhwc(ptr(grad_y), ptr(x), ptr(y) if relu else None, ptr(gamma), ptr(mean), ptr(rstd),
                                                  ptr(gx), ptr(gres), ptr(ggamma), ptr(gbeta), code, N, HW, C, int(G),
                                                  int(bool(relu)), ptr(ws), nbytes, stream_of(x)), "group_norm_backward")
    return gx, gres, ggamma, gbeta


# ------------------------------------------------------------------------------------------ 1x1 conv + frozen BN
# A/B switch DETOPS_CONV1X1_BN: "1" (default) the library's routing table decides per shape | "0" every backbone 1x1
# convolution stays on convolution + frozen_bn_act_forward (two launches) | "t32" / "t16" every shape the kernels serve takes
# that tile configuration (tests, per-shape measurements).  As a value: None off | 0 routing table | 1 | 2.
CONV1X1_BN = {"0": None, "1": 0, "t32": 1, "t16": 2}[os.environ.get("DETOPS_CONV1X1_BN", "1")]
_CONV1X1_BN_ROUTE = {}


def conv1x1_bn_config(x, weight, stride, residual=None, config=0):
    """-> the tile configuration (1 | 2) with which conv1x1_bn_forward serves `conv2d(x, weight, stride=stride)` followed by
    the FrozenBN epilogue, 0 = the two-launch path runs (not an fp32 channels-last device activation, an autocast region,
    a shape the kernel does not serve, or — config 0 — one the library's routing table measured no faster)."""
    if not (x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 4 and weight.dim() == 4 and on_device(x)
            and x.numel() > 0 and x.is_contiguous(memory_format=torch.channels_last)
            and weight.shape[2] == 1 and weight.shape[3] == 1 and weight.shape[1] == x.shape[1]
            and (weight.is_contiguous() or weight.is_contiguous(memory_format=torch.channels_last))
            and not torch.is_autocast_enabled() and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0
            and (residual is None or residual.data_ptr() % 16 == 0)):
        return 0
    N, C, H, W = x.shape
    key = (N, C, H, W, weight.shape[0], stride, residual is not None, config, x.device.index)
    cfg = _CONV1X1_BN_ROUTE.get(key)
    if cfg is None:
        query = getattr(lib, "detops_conv1x1_frozen_bn_act_supported", None)     # (not part of the host emulation build)
        if query is None:
            return 0
        with _on_device(x):
            cfg = _CONV1X1_BN_ROUTE[key] = int(query(N, C, H, W, weight.shape[0], int(stride), int(residual is not None),
                                                     int(config)))
    return cfg


def conv1x1_bn_forward(x, weight, scale, bias, residual, relu, stride, config):
    """Extension: y = [relu](conv2d(x, weight, stride=stride) * scale[k] + bias[k] [+ residual]) in ONE launch
    (csrc/conv1x1_bn.hip).  `config` is a non-zero answer of conv1x1_bn_config for the same arguments."""
    _need_cuda("conv1x1_bn_forward", x, weight, scale, bias, residual)
    N, C, H, W = x.shape
    K = weight.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((N, K, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    if residual is not None:
        if residual.dtype != y.dtype or residual.shape != y.shape:
            raise RuntimeError("conv1x1_bn_forward: residual must match the output")
        residual = residual.contiguous(memory_format=torch.channels_last)
    with _on_device(x), _timed(("conv1x1_bn_fwd[n=%d,C=%d,K=%d,s=%d,res=%d]", (N * Ho * Wo, C, K, stride, residual is not None)), x, every=8):
        check(lib.detops_conv1x1_frozen_bn_act_forward_nhwc_f32(ptr(x), ptr(weight), ptr(scale), ptr(bias), ptr(residual), ptr(y),
                                                               N, C, H, W, K, int(stride), int(bool(relu)), int(config),
                                                               stream_of(x)), "conv1x1_bn_forward")
    return y


_ONES = {}


def _ones(C, device):
    key = (int(C), str(device))
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones((C,), dtype=torch.float32, device=device)
    return t


def bias_act_supported(x, bias):
    """bias_act serves fp32 channels-last activations on the device (any channel count: widths dividing 1024 through the
    fused kernels of csrc/bias_act.hip, the others — the RPN's 3 / 12 and the mask logits' 81 channels — through an in-place
    add and a matrix-vector product for the bias gradient)"""
    return (bias is not None and on_device(x) and x.dtype in _lib.DTYPE_CODE and bias.dtype == torch.float32 and x.dim() == 4
            and is_channels_last(x))


def _bias_act_forward(x, bias, relu):
    """-> ([relu](x + bias[c]), served by the fused kernel?) — `x` may be overwritten"""
    fused = bool(lib.detops_bias_act_supported(int(x.shape[1])))
    if fused:
        y = frozen_bn_act_forward(x, _ones(x.shape[1], x.device), bias.contiguous(), None, relu)
    else:
        bb = bias.to(x.dtype).view(1, -1, 1, 1)
        y = x.add_(bb) if not x.requires_grad else x + bb
        if relu:
            y = y.relu_()
    return y, fused


class _BiasAct(torch.autograd.Function):
    """y = [relu](x + bias[c]) on a channels-last activation (csrc/bias_act.hip).  The point is the BACKWARD: the bias
    gradient of a channels-last gradient is a column sum over [N*H*W, C]; PyTorch's `sum((0, 2, 3))` runs it through a generic
    strided reduce kernel at ~0.1 TB/s."""

    @staticmethod
    def forward(ctx, x, bias, relu):
        y, ctx.fused = _bias_act_forward(x, bias, relu)
        ctx.relu = relu
        ctx.save_for_backward(y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = gy.contiguous(memory_format=torch.channels_last)
        N, C, H, W = gy.shape
        rows = N * H * W
        if not ctx.fused:
            gx = torch.ops.aten.threshold_backward(gy, y, 0) if ctx.relu else gy      # relu's backward (NaN y passes)
            return gx, column_sum(gx.permute(0, 2, 3, 1).reshape(rows, C)), None    # (a view of the channels-last storage)
        gb = torch.empty((C,), dtype=torch.float32, device=gy.device)
        gx = torch.empty_like(gy) if ctx.relu else gy
        nbytes = int(lib.detops_bias_act_backward_workspace_bytes(rows, C))
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=gy.device)
        with _on_device(gy), _timed(("bias_act_bwd[n=%d,C=%d,e=%d,relu=%d]", (gy.numel(), C, _ESIZE[gy.dtype], bool(ctx.relu))), gy, every=4):
            check(lib.detops_bias_act_backward_nhwc(ptr(gy), ptr(y) if ctx.relu else None, ptr(gx), ptr(gb), _lib.DTYPE_CODE[gy.dtype],
                                                    rows, C, int(bool(ctx.relu)), ptr(ws), nbytes, stream_of(gy)), "bias_act_backward")
        return gx, gb, None


def column_sum(x2d):
    """[rows, C] row-major fp32 / fp16 / bf16 -> fp32 [C] column sums (extension, csrc/bias_act.hip; C <= 256), deterministic"""
    _need_cuda("column_sum", x2d)
    if x2d.dtype not in _lib.DTYPE_CODE:
        raise RuntimeError("column_sum: unsupported dtype %s" % x2d.dtype)
    x2d = x2d.contiguous()
    rows, C = x2d.shape
    out = torch.empty((C,), dtype=torch.float32, device=x2d.device)
    if C > 256:
        return x2d.float().sum(0)
    nbytes = int(lib.detops_column_sum_workspace_bytes(rows, C))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=x2d.device)
    with _on_device(x2d):
        check(lib.detops_column_sum(ptr(x2d), ptr(out), _lib.DTYPE_CODE[x2d.dtype], rows, C, ptr(ws), nbytes, stream_of(x2d)), "column_sum")
    return out


def bias_act(x, bias, relu=False):
    """[relu](x + bias[c]) for a channels-last fp32 activation (extension; see bias_act_supported).  `x` may be overwritten
    (it is the caller's fresh convolution output)."""
    _need_cuda("bias_act", x, bias)
    return _BiasAct.apply(x, bias, bool(relu))


# ------------------------------------------------------------------------------------------ sparse RPN-head backward
_RPN_SPARSE_STATUS = {}


def rpn_sparse_status(device):
    """The sticky device word (int32 [1]) of the sparse RPN-head backward: incremented by every backward that found more
    non-zero gradient rows than its static capacity (that step's conv-weight gradient is NaN).  One per device, never
    cleared by the library, never read by the launch path."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else 0))
    t = _RPN_SPARSE_STATUS.get(key)
    if t is None:
        t = _RPN_SPARSE_STATUS[key] = torch.zeros((1,), dtype=torch.int32, device=device)
    return t


def rpn_sparse_overflows(device=None, reset=False):
    """Host-side read of the status words (a device->host copy: call it where a read-back happens anyway).  Returns the
    number of sparse RPN-head backward passes whose row list overflowed since the last reset."""
    total = 0
    for (typ, idx), t in list(_RPN_SPARSE_STATUS.items()):
        if device is not None and torch.device(device).type != typ:
            continue
        total += int(t.item())
        if reset:
            t.zero_()
    return total


def _conv_bias_act_plain(x, weight, bias, padding, relu):
    """layers.misc.conv_bias_act's channels-last branch without autograd: bias-free convolution, then the bias (+ ReLU) pass"""
    y = torch.nn.functional.conv2d(x, weight, None, 1, padding)
    if bias_act_supported(y, bias):
        return _bias_act_forward(y, bias, relu)[0]
    y = y + bias.to(y.dtype).view(1, -1, 1, 1)
    return torch.relu(y) if relu else y


class _RpnHeadSparse(torch.autograd.Function):
    """The whole RPN head (shared 3x3 conv + ReLU, 1x1 objectness, 1x1 box deltas) over every level as ONE node whose
    backward touches only the anchors that carry gradient (csrc/targets.hip, "sparse RPN-head backward").  The forward is
    the dense head's; `max_rows` bounds the non-zero rows of the incoming gradients (see modeling/rpn/rpn.py)."""

    @staticmethod
    def forward(ctx, max_rows, w_conv, b_conv, w_cls, b_cls, w_box, b_box, *features):
        xs, ts, obj, box = [], [], [], []
        for x in features:
            x = x.contiguous(memory_format=torch.channels_last)
            t = _conv_bias_act_plain(x, w_conv, b_conv, 1, True).contiguous(memory_format=torch.channels_last)
            obj.append(_conv_bias_act_plain(t, w_cls, b_cls, 0, False).contiguous())
            box.append(_conv_bias_act_plain(t, w_box, b_box, 0, False).contiguous())
            xs.append(x)
            ts.append(t)
        ctx.max_rows, ctx.levels = int(max_rows), len(features)
        ctx.save_for_backward(w_conv, w_cls, w_box, *(xs + ts))
        return tuple(obj + box)

    @staticmethod
    def backward(ctx, *grads):
        L, R = ctx.levels, ctx.max_rows
        w_conv, w_cls, w_box = ctx.saved_tensors[:3]
        xs, ts = ctx.saved_tensors[3:3 + L], ctx.saved_tensors[3 + L:]
        N, C = int(xs[0].shape[0]), int(xs[0].shape[1])
        A = int(w_cls.shape[0])
        dev = xs[0].device
        gobj = [(g.float().contiguous() if g is not None else torch.zeros((N, A) + tuple(x.shape[2:]), device=dev))
                for g, x in zip(grads[:L], xs)]
        gbox = [(g.float().contiguous() if g is not None else torch.zeros((N, 4 * A) + tuple(x.shape[2:]), device=dev))
                for g, x in zip(grads[L:], xs)]
        Hs = (ctypes.c_int * L)(*[int(x.shape[2]) for x in xs])
        Ws = (ctypes.c_int * L)(*[int(x.shape[3]) for x in xs])
        T = A * sum(int(x.shape[2]) * int(x.shape[3]) for x in xs)
        # the kernels read the 3x3 weight as [C_out, ky, kx, C_in] — the channels-last parameter's own storage (no copy)
        wk = w_conv.permute(0, 2, 3, 1).contiguous()
        wc = w_cls.reshape(A, C).contiguous()
        wb = w_box.reshape(4 * A, C).contiguous()
        gwk = torch.empty((C, 3, 3, C), dtype=torch.float32, device=dev)
        gb_conv = torch.empty((C,), dtype=torch.float32, device=dev)
        gw_cls = torch.empty((A, C), dtype=torch.float32, device=dev)
        gb_cls = torch.empty((A,), dtype=torch.float32, device=dev)
        gw_box = torch.empty((4 * A, C), dtype=torch.float32, device=dev)
        gb_box = torch.empty((4 * A,), dtype=torch.float32, device=dev)
        dxs = [torch.empty_like(x) for x in xs]
        nbytes = int(lib.detops_rpn_head_backward_workspace_bytes(N, T, R, C))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        arr = lambda tensors: (ctypes.c_void_p * L)(*[t.data_ptr() for t in tensors])
        with _on_device(xs[0]), _timed(("rpn_head_bwd[N=%d,R=%d,C=%d]", (N, R, C)), xs[0]):
            check(lib.detops_rpn_head_backward_f32(arr(gobj), arr(gbox), arr(xs), arr(ts), arr(dxs), Hs, Ws, L, A, N, C, T, R,
                                                   ptr(wk), ptr(wc), ptr(wb), ptr(gwk), ptr(gb_conv), ptr(gw_cls), ptr(gb_cls),
                                                   ptr(gw_box), ptr(gb_box), ptr(rpn_sparse_status(dev)), ptr(ws), nbytes,
                                                   stream_of(xs[0])), "rpn_head_backward")
        # each weight gradient in its parameter's memory format (the data-parallel bucket views carry those strides)
        gw_conv = gwk.permute(0, 3, 1, 2)
        if w_conv.is_contiguous():
            gw_conv = gw_conv.contiguous()
        need = ctx.needs_input_grad
        return (None, gw_conv, gb_conv, gw_cls.view(w_cls.shape), gb_cls, gw_box.view(w_box.shape), gb_box) + tuple(
            d if need[7 + i] else None for i, d in enumerate(dxs))


def rpn_head_sparse_supported(features, params):
    """fp32 channels-last features and fp32 parameters on the device, C a multiple of 4 (the kernels' 16-byte rows)"""
    return (all(on_device(t) and t.dtype == torch.float32 for t in list(features) + list(params))
            and all(f.dim() == 4 and f.numel() > 0 and is_channels_last(f) for f in features)
            and int(features[0].shape[1]) % 4 == 0 and 0 < len(features) <= 8)


def rpn_head_sparse(features, w_conv, b_conv, w_cls, b_cls, w_box, b_box, max_rows):
    """(objectness per level [N, A, H, W], box deltas per level [N, 4A, H, W]) of the RPN head with the sparse backward
    (extension).  `max_rows` >= the number of anchors of the batch whose loss gradient is non-zero."""
    params = (w_conv, b_conv, w_cls, b_cls, w_box, b_box)
    _need_cuda("rpn_head_sparse", *(list(features) + list(params)))
    if not rpn_head_sparse_supported(features, params):
        raise RuntimeError("rpn_head_sparse: fp32 channels-last features and fp32 parameters are required")
    out = _RpnHeadSparse.apply(int(max_rows), *params, *features)
    L = len(features)
    return list(out[:L]), list(out[L:])


# ------------------------------------------------------------------------------------------ deformable conv
def _dcn_check(name, *tensors):
    _need_cuda(name, *tensors)
    dt = tensors[0].dtype
    if dt not in _lib.DTYPE_CODE:
        raise RuntimeError("%s: unsupported dtype %s" % (name, dt))
    for t in tensors:
        if t is not None and t.dtype != dt:
            raise RuntimeError("%s: all tensors must share one dtype" % name)
    return _lib.DTYPE_CODE[dt]


def _out_hw(H, W, kH, kW, padH, padW, dH, dW, dilH, dilW):
    return ((H + 2 * padH - (dilH * (kH - 1) + 1)) // dH + 1,
            (W + 2 * padW - (dilW * (kW - 1) + 1)) // dW + 1)


def _shape_check(input, offset, grad_output, weight, kH, kW, dH, dW, padH, padW, dilH, dilW, group,
                 deformable_group):
    """reference csrc/cuda/deform_conv_cuda.cu:67-156 (same conditions, RuntimeError)."""
    if weight.dim() != 4:
        raise RuntimeError("4D weight tensor (nOutputPlane,nInputPlane,kH,kW) expected, but got: %d" % weight.dim())
    if not weight.is_contiguous() and not is_channels_last(weight):
        raise RuntimeError("weight tensor has to be contiguous")
    if kW <= 0 or kH <= 0:
        raise RuntimeError("kernel size should be greater than zero, but got kH: %d kW: %d" % (kH, kW))
    if weight.size(2) != kH or weight.size(3) != kW:
        raise RuntimeError("kernel size should be consistent with weight")
    if dW <= 0 or dH <= 0:
        raise RuntimeError("stride should be greater than zero, but got dH: %d dW: %d" % (dH, dW))
    if dilW <= 0 or dilH <= 0:
        raise RuntimeError("dilation should be greater than 0")
    if input.dim() != 4:
        raise RuntimeError("3D or 4D input tensor expected but got: %d" % input.dim())
    nIn = weight.size(1) * group
    H, W = input.size(2), input.size(3)
    Ho, Wo = _out_hw(H, W, kH, kW, padH, padW, dH, dW, dilH, dilW)
    if nIn % deformable_group != 0:
        raise RuntimeError("input channels must divide deformable group size")
    if Wo < 1 or Ho < 1:
        raise RuntimeError("Given input size: (%d x %d x %d). Calculated output size: (%d x %d x %d). "
                           "Output size is too small" % (nIn, H, W, weight.size(0), Ho, Wo))
    if input.size(1) != nIn:
        raise RuntimeError("invalid number of input planes, expected: %d, but got: %d" % (nIn, input.size(1)))
    if H < kH or W < kW:
        raise RuntimeError("input image is smaller than kernel")
    if offset.size(2) != Ho or offset.size(3) != Wo:
        raise RuntimeError("invalid spatial size of offset, expected height: %d width: %d, but got "
                           "height: %d width: %d" % (Ho, Wo, offset.size(2), offset.size(3)))
    if offset.size(1) != deformable_group * 2 * kH * kW:
        raise RuntimeError("invalid number of channels of offset")
    if offset.size(0) != input.size(0):
        raise RuntimeError("invalid batch size of offset")
    if grad_output is not None:
        if grad_output.size(1) != weight.size(0):
            raise RuntimeError("invalid number of gradOutput planes, expected: %d, but got: %d"
                               % (weight.size(0), grad_output.size(1)))
        if grad_output.size(2) != Ho or grad_output.size(3) != Wo:
            raise RuntimeError("invalid size of gradOutput")
    return Ho, Wo


def deformable_im2col(im, offset, mask, kH, kW, padH, padW, dH, dW, dilH, dilW, dg):
    """col [C*kH*kW, B*Ho*Wo] (deform_conv_kernel_cuda.cu:197-250 / :577-640)."""
    code = _dcn_check("deformable_im2col", im, offset, mask)
    B, C, H, W = im.shape
    Ho, Wo = _out_hw(H, W, kH, kW, padH, padW, dH, dW, dilH, dilW)
    col = torch.empty((C * kH * kW, B * Ho * Wo), dtype=im.dtype, device=im.device)
    with _on_device(im), _timed(("dcn_im2col[B=%d,C=%d,%dx%d,k=%d,e=%d,m=%d]", (B, C, H, W, kH, _ESIZE[im.dtype], mask is not None)), im, every=8):
        check(lib.detops_deformable_im2col(ptr(im), ptr(offset), ptr(mask), ptr(col), code, B, C, H, W, kH, kW, padH, padW,
                                           dH, dW, dilH, dilW, dg, stream_of(im)), "deformable_im2col")
    return col


def deformable_col2im(col, offset, mask, grad_im, kH, kW, padH, padW, dH, dW, dilH, dilW, dg):
    """accumulates into grad_im [B,C,H,W] (deform_conv_kernel_cuda.cu:286-342 / :642-700)."""
    code = _dcn_check("deformable_col2im", col, offset, mask, grad_im)
    B, C, H, W = grad_im.shape
    geom = (B, C, H, W, kH, kW, padH, padW, dH, dW, dilH, dilW, dg)
    with _on_device(col):
        # gather lists for the atomic-free path live in a scratch tensor (torch's caching allocator:
        # stream-ordered reuse, no hipMalloc per call); 0 bytes = shape outside the index plan
        nbytes = int(lib.detops_deformable_col2im_workspace_bytes(*geom))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=col.device) if nbytes > 0 else None
        with _timed(("dcn_col2im[B=%d,C=%d,%dx%d,k=%d,e=%d,m=%d]", (B, C, H, W, kH, _ESIZE[col.dtype], mask is not None)), col, every=8):
            check(lib.detops_deformable_col2im_ws(ptr(col), ptr(offset), ptr(mask), ptr(grad_im), code, *geom,
                                                  ptr(ws), nbytes, stream_of(col)), "deformable_col2im")


def deformable_col2im_coord(col, im, offset, mask, grad_offset, grad_mask, kH, kW, padH, padW, dH,
                            dW, dilH, dilW, dg):
    """overwrites grad_offset (and grad_mask) (deform_conv_kernel_cuda.cu:380-443 / :702-774)."""
    code = _dcn_check("deformable_col2im_coord", col, im, offset, mask, grad_offset, grad_mask)
    B, C, H, W = im.shape
    with _on_device(col), _timed(("dcn_col2im_coord[B=%d,C=%d,%dx%d,k=%d,e=%d,m=%d]", (B, C, H, W, kH, _ESIZE[col.dtype], mask is not None)), col, every=8):
        check(lib.detops_deformable_col2im_coord(ptr(col), ptr(im), ptr(offset), ptr(mask),
                                                 ptr(grad_offset), ptr(grad_mask), code, B, C, H, W, kH, kW, padH, padW,
                                                 dH, dW, dilH, dilW, dg, stream_of(col)), "deformable_col2im_coord")


def _fused_dcn_forward(input, weight, offset, mask, bias, out, kH, kW, padH, padW, dH, dW, dilH, dilW, group, dg):
    """Fused implicit-GEMM forward on the matrix cores (csrc/deform_conv.hip: the deformed operand tile is built
    in LDS, `columns` is never written).  Returns False when the shape is outside the fused plan (fp32 storage,
    grouped convolution, channels per deformable group not a multiple of 32) or tuning dcn_fused = 2."""
    if group != 1 or input.dtype not in (torch.float16, torch.bfloat16) or _lib.tuning_get("dcn_fused") == 2:
        return False
    B, C, H, W = input.shape
    Cout = weight.size(0)
    code = 1 if input.dtype == torch.float16 else 2
    geo = (code, B, C, H, W, Cout, kH, kW, padH, padW, dH, dW, dilH, dilW, dg)
    nbytes = int(lib.detops_deform_conv_forward_fused_workspace_bytes(*geo))
    if nbytes == 0:
        return False
    with _on_device(input):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=input.device)
        with _timed(("dcn_fused_fwd[B=%d,C=%d,%dx%d,Cout=%d,k=%d,e=2,m=%d]", (B, C, H, W, Cout, kH, mask is not None)), input, every=8):
            check(lib.detops_deform_conv_forward_fused(ptr(input), ptr(weight), ptr(offset), ptr(mask), ptr(bias),
                                                       ptr(out), *geo, ptr(ws), nbytes, stream_of(input)),
                  "deform_conv_forward_fused")
    return True


# ---- channels-last pipeline (csrc/deform_conv.hip, "channels-last pipeline"): every per-sampling-point operand is
# channel-fastest, the GEMMs are plain library GEMMs on those layouts, the input gradient uses the transposed
# sampling operator + a GEMM instead of the col2im scatter.  Served shapes: conv groups == 1, deformable_group == 1,
# channel counts that are power-of-two multiples of a 16-byte vector (all model shapes).
def _nhwc_ok(input, weight, group, dg, geom=None):
    """channels-last pipeline applicable?  With `geom` (kH, kW, padH, padW, dH, dW, dilH, dilW, dg) the backward's index
    plan is checked too (empty batches and shapes beyond its 32-bit limits return 0 bytes): callers then take the
    reference-layout kernels BEFORE anything is launched instead of failing half way."""
    if group != 1 or dg != 1 or input.dtype not in _lib.DTYPE_CODE or _lib.tuning_get("dcn_nhwc") == 2:
        return False
    if input.numel() == 0:
        return False
    if not lib.detops_deformable_nhwc_supported(_lib.DTYPE_CODE[input.dtype], input.size(1), weight.size(0), dg):
        return False
    if geom is not None:
        B, C, H, W = input.shape
        if int(lib.detops_deformable_transposed_sample_workspace_bytes(B, C, H, W, *geom)) == 0:
            return False
    return True


def _dcn_in(x):
    """a channels-last tensor stays as it is (the channels-last pipeline reads it in place); anything else is made contiguous"""
    return x if is_channels_last(x) else x.contiguous()


def _to_nhwc(x):
    """[B, C, H, W] -> [B, H*W, C] (contiguous).  A channels-last tensor IS that layout: a view, no launch."""
    B, C, H, W = x.shape
    if is_channels_last(x):
        return x.permute(0, 2, 3, 1).reshape(B, H * W, C)
    x = x.contiguous()
    out = torch.empty((B, H * W, C), dtype=x.dtype, device=x.device)
    if out.numel():
        with _on_device(x), _timed(("dcn_to_nhwc[n=%d,e=%d]", (x.numel(), _ESIZE[x.dtype])), x, every=8):
            check(lib.detops_nchw_to_nhwc(ptr(x), ptr(out), _lib.DTYPE_CODE[x.dtype], B, C, H * W, stream_of(x)), "nchw_to_nhwc")
    return out


def _im2col_nhwc(xT, offset, mask, B, C, H, W, geom):
    kH, kW = geom[0], geom[1]
    Ho, Wo = _out_hw(H, W, *geom[:8])
    colT = torch.empty((B * Ho * Wo, kH * kW * C), dtype=xT.dtype, device=xT.device)
    if colT.numel():
        with _on_device(xT), _timed(("dcn_im2col_nhwc[B=%d,C=%d,%dx%d,k=%d,e=%d,m=%d]", (B, C, H, W, kH, _ESIZE[xT.dtype], mask is not None)), xT, every=8):
            check(lib.detops_deformable_im2col_nhwc(ptr(xT), ptr(offset), ptr(mask), ptr(colT), _lib.DTYPE_CODE[xT.dtype],
                                                    B, C, H, W, *geom, stream_of(xT)), "deformable_im2col_nhwc")
    return colT


def _coord_nhwc(colsG, xT, offset, mask, grad_offset, grad_mask, B, C, H, W, geom):
    with _on_device(xT), _timed(("dcn_coord_nhwc[B=%d,C=%d,%dx%d,k=%d,e=%d,m=%d]", (B, C, H, W, geom[0], _ESIZE[xT.dtype], mask is not None)), xT, every=8):
        check(lib.detops_deformable_coord_nhwc(ptr(colsG), ptr(xT), ptr(offset), ptr(mask), ptr(grad_offset), ptr(grad_mask),
                                               _lib.DTYPE_CODE[xT.dtype], B, C, H, W, *geom, stream_of(xT)), "deformable_coord_nhwc")


def _transposed_sample(gT, offset, mask, B, C, H, W, Cout, geom):
    """S_T [B*H*W, kh*kw*Cout]: per gradient-map pixel and tap, the weighted sum of the output-gradient vectors of the
    sampling points that touch the pixel."""
    kH, kW = geom[0], geom[1]
    S_T = torch.empty((B * H * W, kH * kW * Cout), dtype=gT.dtype, device=gT.device)
    nbytes = int(lib.detops_deformable_transposed_sample_workspace_bytes(B, C, H, W, *geom))
    if nbytes == 0:
        raise RuntimeError("deformable_transposed_sample: shape outside the index plan")
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=gT.device)
    with _on_device(gT), _timed(("dcn_transposed_sample[B=%d,Cout=%d,%dx%d,k=%d,e=%d,m=%d]", (B, Cout, H, W, kH, _ESIZE[gT.dtype], mask is not None)), gT, every=8):
        check(lib.detops_deformable_transposed_sample(ptr(gT), ptr(offset), ptr(mask), ptr(S_T), _lib.DTYPE_CODE[gT.dtype],
                                                      B, C, H, W, Cout, *geom, ptr(ws), nbytes, stream_of(gT)),
              "deformable_transposed_sample")
    return S_T


DCN_INPUT_GRAD = os.environ.get("DETOPS_DCN_INPUT_GRAD", "col2im")   # col2im | transposed  (A/B switch)


def _col2im_nhwc(colsG, offset, mask, B, C, H, W, geom):
    """grad_in_T [B, H*W, C] from the channel-fastest column gradient [B*Ho*Wo, kh*kw*C]: col2im as a gather over the inverted
    index (csrc/deform_conv.hip col2im_nhwc_gather_kernel); None when the shape is outside the kernel's plan."""
    kH = geom[0]
    nbytes = int(lib.detops_deformable_transposed_sample_workspace_bytes(B, C, H, W, *geom))
    if nbytes == 0 or C // (8 if _ESIZE[colsG.dtype] == 2 else 4) > 256:
        return None
    ginT = torch.empty((B, H * W, C), dtype=colsG.dtype, device=colsG.device)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=colsG.device)
    with _on_device(colsG), _timed(("dcn_col2im_nhwc[B=%d,C=%d,%dx%d,k=%d,e=%d,m=%d]", (B, C, H, W, kH, _ESIZE[colsG.dtype], mask is not None)), colsG, every=8):
        rc = lib.detops_deformable_col2im_nhwc(ptr(colsG), ptr(offset), ptr(mask), ptr(ginT), _lib.DTYPE_CODE[colsG.dtype],
                                               B, C, H, W, *geom, ptr(ws), nbytes, stream_of(colsG))
    if rc == -3:
        return None
    check(rc, "deformable_col2im_nhwc")
    return ginT


def _w_tap_major(weight):
    """[Cout, C, kh, kw] -> W2 [Cout, kh*kw*C] (tap-major, channel-fastest: the column order of colT)"""
    Cout = weight.size(0)
    return weight.permute(0, 2, 3, 1).reshape(Cout, -1)


def _nhwc_forward(input, weight, offset, mask, bias, out, geom):
    """-> (xT, colT): the channel-fastest copy of the input and the column matrix, which the backward pass of the same
    layer needs again (deform_conv_backward_all(saved=...))"""
    B, C, H, W = input.shape
    Cout = weight.size(0)
    xT = _to_nhwc(input)
    colT = _im2col_nhwc(xT, offset, mask, B, C, H, W, geom)
    # (a bias goes into the GEMM: sum + bias is rounded to the storage type once, as in the fused kernel's epilogue; added to the
    #  GEMM's half output it would be rounded twice)
    bias = None if bias is None else bias.to(out.dtype)
    if is_channels_last(out):
        # channels-last output: ONE GEMM over the whole batch straight into the output's storage ([B*Ho*Wo, Cout])
        out2 = out.permute(0, 2, 3, 1).reshape(-1, Cout)
        if bias is None:
            torch.mm(colT, _w_tap_major(weight).t(), out=out2)
        else:
            torch.addmm(bias, colT, _w_tap_major(weight).t(), out=out2)
    else:
        w2, cols = _w_tap_major(weight).unsqueeze(0).expand(B, -1, -1), colT.view(B, -1, colT.size(1)).transpose(1, 2)
        if bias is None:
            torch.bmm(w2, cols, out=out.view(B, Cout, -1))
        else:
            torch.baddbmm(bias.view(1, -1, 1), w2, cols, out=out.view(B, Cout, -1))
    return xT, colT


def _w_cin_major(weight):
    """[Cout, C, kh, kw] -> W2T [C, kh*kw*Cout] (the column order of S_T)"""
    return weight.permute(1, 2, 3, 0).reshape(weight.size(1), -1)


def _nhwc_backward_core(xT, colT, gT, weight, offset, mask, B, C, H, W, geom, need_input, need_weight, need_bias,
                        grad_offset=None, grad_mask=None):
    """The channels-last backward pass that deform_conv_backward_all (the layers) and the reference-named entry points both
    run; each adds only its final layout step.  `xT` [B, H*W, C] / `gT` [B, Ho*Wo, Cout]: channel-fastest input and output
    gradient; `colT`: the forward's kept column matrix, or None (rebuilt for the weight gradient); `grad_offset` /
    `grad_mask`: the caller's buffers, or None (fresh ones).  -> (ginT, S_T, grad_offset, grad_mask, gw2, grad_bias), None where
    not asked for: the input gradient is `ginT` [B, H*W, C], or (DCN_INPUT_GRAD == "transposed", shapes outside the gather's
    plan) `S_T` [B*H*W, kh*kw*Cout] for the caller to multiply with _w_cin_major(weight); `gw2` is [Cout, kh*kw*C]."""
    Cout = gT.size(2)
    g2 = gT.view(-1, Cout)
    ginT = S_T = gw2 = grad_bias = None
    if need_input:
        colsG = torch.mm(g2, _w_tap_major(weight))               # column gradient, channel-fastest: [B*Ho*Wo, K*C]
        if grad_offset is None:
            grad_offset = torch.empty_like(offset)               # written in full by the coordinate kernel
            grad_mask = torch.empty_like(mask) if mask is not None else None
        _coord_nhwc(colsG, xT, offset, mask, grad_offset, grad_mask, B, C, H, W, geom)
        # input gradient: col2im of the column gradient as a gather (no S_T, no second conv-sized GEMM); the transposed
        # sampling of the output gradient + GEMM of rounds 3-5 stays as the A/B form and for shapes outside the gather's plan
        ginT = _col2im_nhwc(colsG, offset, mask, B, C, H, W, geom) if DCN_INPUT_GRAD == "col2im" else None
        del colsG
        if ginT is None:
            S_T = _transposed_sample(gT, offset, mask, B, C, H, W, Cout, geom)     # [B*H*W, K*Cout]
    if need_weight:
        if colT is None:
            colT = _im2col_nhwc(xT, offset, mask, B, C, H, W, geom)  # [B*Ho*Wo, K*C]
        gw2 = torch.mm(g2.t(), colT)
    if need_bias:
        grad_bias = g2.sum(0)
    return ginT, S_T, grad_offset, grad_mask, gw2, grad_bias


def _nhwc_backward(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, grad_bias,
                   geom, scale=1.0):
    """the reference-named backward entry points on the channels-last plan: accumulates into grad_input / grad_weight /
    grad_bias, the coordinate kernel overwrites grad_offset / grad_mask in place.  Either half (input+offset(+mask) /
    weight(+bias)) may be None: the v1 entry points ask for them in two calls."""
    B, C, H, W = input.shape
    ginT, S_T, _, _, gw2, gb = _nhwc_backward_core(
        _to_nhwc(input), None, _to_nhwc(grad_output), weight, offset, mask, B, C, H, W, geom, grad_input is not None,
        grad_weight is not None, grad_weight is not None and grad_bias is not None, grad_offset, grad_mask)
    if ginT is not None:       # [B, H*W, C]: accumulated into the caller's NCHW gradient
        grad_input.view(B, C, -1).add_(ginT.transpose(1, 2))
    elif S_T is not None:
        grad_input.view(B, C, -1).baddbmm_(_w_cin_major(weight).unsqueeze(0).expand(B, -1, -1), S_T.view(B, H * W, -1).transpose(1, 2))
    if gw2 is not None:
        grad_weight.add_(gw2.view(-1, geom[0], geom[1], C).permute(0, 3, 1, 2), alpha=float(scale))
    if gb is not None:
        grad_bias += gb


def deform_conv_backward_all(input, offset, mask, weight, grad_output, kH, kW, padH, padW, dH, dW, dilH, dilW, group,
                             deformable_group, need_input=True, need_weight=True, need_bias=False, saved=None):
    """Extension (not a name of the reference's `_C`): every gradient of one deformable convolution (v1: mask None;
    v2: modulated) from ONE pass over the channels-last pipeline.  The reference API (deform_conv_backward_input +
    deform_conv_backward_parameters, below: the same _nhwc_backward_core) asks for them in two calls, each of which must
    rebuild the channel-fastest copies of the input and of the output gradient and accumulates into caller-zeroed tensors:
    per layer that is two extra transposes, three fills and an accumulate — about a third of the launches of a host-bound
    step (R-101 + DCN under fp16).

    `saved` = what the forward pass of the same layer kept (`keep=[]` of deform_conv_forward /
    modulated_deform_conv_forward: the channel-fastest input copy and the column matrix): neither is rebuilt then
    (one transpose and one im2col launch less per layer: 35-55 us of device time at the cfg-5 shapes, for 9x the
    layer input in memory until its backward pass has run).

    -> (grad_input, grad_offset, grad_mask, grad_weight, grad_bias), None where not asked for / not applicable;
    returns None when the shape is outside the channels-last plan (the caller then uses the reference entry points)."""
    _dcn_check("deform_conv_backward_all", input, offset, weight, grad_output)
    geom = (kH, kW, padH, padW, dH, dW, dilH, dilW, deformable_group)
    if not _nhwc_ok(input, weight, group, deformable_group, geom):
        return None
    cl_in = is_channels_last(input)
    cl_w = is_channels_last(weight)          # channels-last parameter: its tap-major matrix is a view, and so is its gradient
    input, offset, weight, grad_output = _dcn_in(input), offset.contiguous(), _dcn_in(weight), _dcn_in(grad_output)
    if mask is not None:
        mask = mask.contiguous()
    B, C, H, W = input.shape
    xT, colT = saved if saved is not None else (_to_nhwc(input), None)
    ginT, S_T, grad_offset, grad_mask, grad_weight, grad_bias = _nhwc_backward_core(
        xT, colT, _to_nhwc(grad_output), weight, offset, mask, B, C, H, W, geom, need_input, need_weight, need_bias)
    grad_input = None
    if ginT is not None:
        if cl_in:  # the input was channels-last: so is its gradient ([B, H*W, C] viewed as [B, C, H, W])
            grad_input = ginT.view(B, H, W, C).permute(0, 3, 1, 2)
        else:      # [B, H*W, C] -> [B, C, H*W]: the same tile transpose with the roles of C and H*W swapped
            grad_input = torch.empty((B, C, H, W), dtype=ginT.dtype, device=ginT.device)
            with _on_device(ginT):
                check(lib.detops_nchw_to_nhwc(ptr(ginT), ptr(grad_input), _lib.DTYPE_CODE[ginT.dtype], B, H * W, C,
                                              stream_of(ginT)), "nhwc_to_nchw")
    elif S_T is not None:
        W2T = _w_cin_major(weight)                               # [C, K*Cout]
        if cl_in:     # the input was channels-last: so is its gradient ([B*H*W, C] from one GEMM, viewed as [B, C, H, W])
            grad_input = torch.mm(S_T, W2T.t()).view(B, H, W, C).permute(0, 3, 1, 2)
        else:
            grad_input = torch.bmm(W2T.unsqueeze(0).expand(B, -1, -1), S_T.view(B, H * W, -1).transpose(1, 2)).view(B, C, H, W)
    if grad_weight is not None:
        grad_weight = grad_weight.view(-1, kH, kW, C).permute(0, 3, 1, 2)   # [Cout, C, kH, kW], channels-last strides
        if not cl_w:
            grad_weight = grad_weight.contiguous()
    return grad_input, grad_offset, grad_mask, grad_weight, grad_bias


def _grouped_weight_times_cols(weight, col, group, out, bias=None):
    """out[g] = W[g] @ col[g] (+ bias[g] per row); out is [Cout, ncol] (written), fp32/half via rocBLAS/hipBLASLt.  The bias goes
    into the GEMM: sum + bias is rounded to the storage type once, as in the fused kernel's epilogue."""
    Cout = weight.size(0)
    Mg = Cout // group
    Kg = col.size(0) // group
    w2 = weight.reshape(group, Mg, Kg)
    for g in range(group):
        if bias is None:
            torch.mm(w2[g], col[g * Kg:(g + 1) * Kg], out=out[g * Mg:(g + 1) * Mg])
        else:
            torch.addmm(bias[g * Mg:(g + 1) * Mg].unsqueeze(1), w2[g], col[g * Kg:(g + 1) * Kg], out=out[g * Mg:(g + 1) * Mg])


def _sl(t, sl):
    return None if t is None else t[sl]


def _dcn_forward(input, weight, offset, mask, bias, output, geom, group, im2col_step, keep):
    """what deform_conv_forward (mask and bias None) and modulated_deform_conv_forward share once their arguments are
    checked and in `geom` order (kH, kW, padH, padW, dH, dW, dilH, dilW, dg): fused MFMA kernel -> channels-last
    pipeline -> reference-layout kernels, `im2col_step` images at a time."""
    B, _, H, W = input.shape
    Cout = weight.size(0)
    Ho, Wo = _out_hw(H, W, *geom[:8])
    out = output.view(B, Cout, Ho, Wo)
    if (not is_channels_last(input) and out.is_contiguous()
            and _fused_dcn_forward(input, weight.contiguous(), offset, mask, None if bias is None else bias.to(input.dtype).contiguous(),
                                   out, *geom[:8], group, geom[8])):
        return
    if (out.is_contiguous() or is_channels_last(out)) and _nhwc_ok(input, weight, group, geom[8]):
        kept = _nhwc_forward(input, weight, offset, mask, bias, out, geom)
        if keep is not None:
            keep.append(kept)
        return
    input, weight = input.contiguous(), weight.contiguous()
    bias = None if bias is None else bias.to(input.dtype)
    for b0 in range(0, B, im2col_step):
        sl = slice(b0, b0 + im2col_step)
        col = deformable_im2col(input[sl], offset[sl], _sl(mask, sl), *geom)
        buf = torch.empty((Cout, im2col_step * Ho * Wo), dtype=input.dtype, device=input.device)
        _grouped_weight_times_cols(weight, col, group, buf, bias)
        out[sl].copy_(buf.view(Cout, im2col_step, Ho, Wo).transpose(0, 1))


def _ref_backward_input(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, geom, group, im2col_step):
    """reference-layout kernels: columns = W^T * gradOut (deform_conv_cuda.cu:338-341 / :628-631), then col2im_coord
    (overwrites grad_offset / grad_mask) and col2im (accumulates into grad_input), `im2col_step` images at a time"""
    B, C = input.shape[:2]
    Cout = weight.size(0)
    n = im2col_step * grad_output.size(2) * grad_output.size(3)
    Mg, Kg = Cout // group, (C // group) * geom[0] * geom[1]
    w2 = weight.reshape(group, Mg, Kg)
    for b0 in range(0, B, im2col_step):
        sl = slice(b0, b0 + im2col_step)
        go = grad_output[sl].transpose(0, 1).reshape(Cout, n)
        col = torch.empty((group * Kg, n), dtype=input.dtype, device=input.device)
        for g in range(group):
            torch.mm(w2[g].t(), go[g * Mg:(g + 1) * Mg], out=col[g * Kg:(g + 1) * Kg])
        deformable_col2im_coord(col, input[sl], offset[sl], _sl(mask, sl), grad_offset[sl], _sl(grad_mask, sl), *geom)
        deformable_col2im(col, offset[sl], _sl(mask, sl), grad_input[sl], *geom)


def _ref_backward_parameters(input, offset, mask, grad_output, grad_weight, grad_bias, geom, group, scale, im2col_step):
    """reference-layout kernels: grad_weight += scale * gradOut * cols^T (deform_conv_cuda.cu:466-472 / :666-670) and
    grad_bias += gradOut * ones (:671-676), `im2col_step` images at a time"""
    B, C = input.shape[:2]
    Cout = grad_weight.size(0)
    n = im2col_step * grad_output.size(2) * grad_output.size(3)
    Mg, Kg = Cout // group, (C // group) * geom[0] * geom[1]
    gw = grad_weight.view(group, Mg, Kg)
    for b0 in range(0, B, im2col_step):
        sl = slice(b0, b0 + im2col_step)
        col = deformable_im2col(input[sl], offset[sl], _sl(mask, sl), *geom)
        go = grad_output[sl].transpose(0, 1).reshape(Cout, n)
        for g in range(group):
            gw[g].addmm_(go[g * Mg:(g + 1) * Mg], col[g * Kg:(g + 1) * Kg].t(), beta=1.0, alpha=float(scale))
        if grad_bias is not None:
            grad_bias += go.sum(1)


def deform_conv_forward(input, weight, offset, output, columns, ones, kW, kH, dW, dH, padW, padH,
                        dilationW, dilationH, group, deformable_group, im2col_step, keep=None):
    """reference csrc/deform_conv.h:11-42 / csrc/cuda/deform_conv_cuda.cu:158-266.
    Writes `output` in place; note the W-before-H argument order.  Returns 1.
    `keep` (extension): a list that receives what deform_conv_backward_all(saved=...) can reuse, when the
    channels-last pipeline served the call."""
    _dcn_check("deform_conv_forward", input, weight, offset, output)
    # (a channels-last weight — a model switched to channels-last carries its 4-d parameters that way — IS the tap-major matrix
    #  the channels-last pipeline multiplies with: _w_tap_major is a view of it, no copy launch)
    input, offset, weight = _dcn_in(input), offset.contiguous(), _dcn_in(weight)
    _shape_check(input, offset, None, weight, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group)
    if input.size(0) % im2col_step != 0:
        raise RuntimeError("im2col step must divide batchsize")
    _dcn_forward(input, weight, offset, None, None, output, (kH, kW, padH, padW, dH, dW, dilationH, dilationW, deformable_group),
                 group, im2col_step, keep)
    return 1


def deform_conv_backward_input(input, offset, gradOutput, gradInput, gradOffset, weight, columns, kW,
                               kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group,
                               im2col_step):
    """reference csrc/deform_conv.h:45-77 / deform_conv_cuda.cu:268-380: accumulates into the
    caller-zeroed gradInput, overwrites gradOffset.  Returns 1."""
    _dcn_check("deform_conv_backward_input", input, offset, gradOutput, gradInput, gradOffset, weight)
    input, offset = input.contiguous(), offset.contiguous()
    gradOutput, weight = gradOutput.contiguous(), weight.contiguous()
    _shape_check(input, offset, gradOutput, weight, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group)
    geom = (kH, kW, padH, padW, dH, dW, dilationH, dilationW, deformable_group)
    if gradInput.is_contiguous() and gradOffset.is_contiguous() and _nhwc_ok(input, weight, group, deformable_group, geom):
        _nhwc_backward(input, weight, offset, None, gradOutput, gradInput, gradOffset, None, None, None, geom)
    else:
        _ref_backward_input(input, weight, offset, None, gradOutput, gradInput, gradOffset, None, geom, group, im2col_step)
    return 1


def deform_conv_backward_parameters(input, offset, gradOutput, gradWeight, columns, ones, kW, kH, dW,
                                    dH, padW, padH, dilationW, dilationH, group, deformable_group,
                                    scale, im2col_step):
    """reference csrc/deform_conv.h:80-112 / deform_conv_cuda.cu:382-494:
    gradWeight += scale * gradOut * cols^T.  Returns 1."""
    _dcn_check("deform_conv_backward_parameters", input, offset, gradOutput, gradWeight)
    input, offset, gradOutput = input.contiguous(), offset.contiguous(), gradOutput.contiguous()
    _shape_check(input, offset, gradOutput, gradWeight, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group)
    geom = (kH, kW, padH, padW, dH, dW, dilationH, dilationW, deformable_group)
    if gradWeight.is_contiguous() and _nhwc_ok(input, gradWeight, group, deformable_group):
        _nhwc_backward(input, None, offset, None, gradOutput, None, None, None, gradWeight, None, geom, scale=scale)
    else:
        _ref_backward_parameters(input, offset, None, gradOutput, gradWeight, None, geom, group, scale, im2col_step)
    return 1


def _modulated_check(input, weight, kernel_h, kernel_w, group, channels_last_too):
    """the reference's v2 checks (same texts); `channels_last_too`: the forward also takes a channels-last input and
    weight (a model switched to channels-last carries its 4-d parameters that way)"""
    if not input.is_contiguous() and not (channels_last_too and is_channels_last(input)):
        raise RuntimeError("input tensor has to be contiguous")
    if not weight.is_contiguous() and not (channels_last_too and is_channels_last(weight)):
        raise RuntimeError("weight tensor has to be contiguous")
    if weight.size(2) != kernel_h or weight.size(3) != kernel_w:
        raise RuntimeError("Input shape and kernel shape wont match: (%d x %d vs %d x %d)."
                           % (kernel_h, kernel_w, weight.size(2), weight.size(3)))
    if input.size(1) != weight.size(1) * group:
        raise RuntimeError("Input shape and kernel channels wont match: (%d vs %d)." % (input.size(1), weight.size(1) * group))


def modulated_deform_conv_forward(input, weight, bias, ones, offset, mask, output, columns, kernel_h,
                                  kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w,
                                  group, deformable_group, with_bias, keep=None):
    """reference csrc/deform_conv.h:115-149 / deform_conv_cuda.cu:496-575 (H-before-W order).
    `keep` (extension): see deform_conv_forward.
    The reference loops per image; one im2col + one GEMM per group over the whole batch gives the
    same sums."""
    _dcn_check("modulated_deform_conv_forward", input, weight, offset, mask, output)
    _modulated_check(input, weight, kernel_h, kernel_w, group, True)
    _dcn_forward(input, weight, offset.contiguous(), mask.contiguous(), bias if with_bias else None, output,
                 (kernel_h, kernel_w, pad_h, pad_w, stride_h, stride_w, dilation_h, dilation_w, deformable_group),
                 group, max(input.size(0), 1), keep)


def modulated_deform_conv_backward(input, weight, bias, ones, offset, mask, columns, grad_input,
                                   grad_weight, grad_bias, grad_offset, grad_mask, grad_output,
                                   kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                                   dilation_w, group, deformable_group, with_bias):
    """reference csrc/deform_conv.h:152-191 / deform_conv_cuda.cu:577-691.  grad_input /
    grad_weight / grad_bias are accumulated into (caller passes zeros); grad_offset / grad_mask are
    overwritten."""
    _dcn_check("modulated_deform_conv_backward", input, weight, offset, mask, grad_input, grad_weight,
               grad_offset, grad_mask, grad_output)
    _modulated_check(input, weight, kernel_h, kernel_w, group, False)
    offset, mask, grad_output = offset.contiguous(), mask.contiguous(), grad_output.contiguous()
    geom = (kernel_h, kernel_w, pad_h, pad_w, stride_h, stride_w, dilation_h, dilation_w, deformable_group)
    grad_bias = grad_bias if with_bias else None
    if (grad_input.is_contiguous() and grad_weight.is_contiguous() and grad_offset.is_contiguous() and grad_mask.is_contiguous()
            and _nhwc_ok(input, weight, group, deformable_group, geom)):
        _nhwc_backward(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, grad_bias, geom)
    else:
        step = max(input.size(0), 1)
        _ref_backward_input(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, geom, group, step)
        _ref_backward_parameters(input, offset, mask, grad_output, grad_weight, grad_bias, geom, group, 1.0, step)


def _psroi_args(name, input, bbox, trans, no_trans, part_size):
    _need_cuda(name, input, bbox)
    if not input.is_contiguous():  # deform_pool_cuda.cu:45
        raise RuntimeError("input tensor has to be contiguous")
    input = _f32c(name, input)
    bbox = _f32c(name, bbox)
    if no_trans:
        return input, bbox, None, 2  # deform_pool_cuda.cu:51 (`channels_trans = no_trans ? 2 : trans.size(1)`)
    _need_cuda(name, trans)
    trans = _f32c(name, trans)
    if trans.dim() != 4 or trans.size(0) != bbox.size(0) or trans.size(2) != part_size or trans.size(3) != part_size:
        raise RuntimeError("%s: trans must be [num_bbox, 2*num_classes, part_size, part_size]" % name)
    return input, bbox, trans, trans.size(1)


def deform_psroi_pooling_forward(input, bbox, trans, out, top_count, no_trans, spatial_scale, output_dim,
                                 group_size, pooled_size, part_size, sample_per_part, trans_std):
    """reference csrc/deform_pool.h:11-38 -> deform_pool_cuda.cu:38-62.  Writes into the
    caller-allocated `out` / `top_count` [num_bbox, output_dim, pooled_size, pooled_size]."""
    name = "deform_psroi_pooling_forward"
    input, bbox, trans, ct = _psroi_args(name, input, bbox, trans, no_trans, part_size)
    N, C, H, W = input.shape
    K = bbox.size(0)
    if K != out.size(0):  # deform_pool_cuda.cu:54-56
        raise RuntimeError("Output shape and bbox number wont match: (%d vs %d)." % (out.size(0), K))
    _need_cuda(name, out, top_count)
    if not (out.is_contiguous() and top_count.is_contiguous() and out.dtype == torch.float32
            and top_count.dtype == torch.float32):
        raise RuntimeError("%s: out/top_count must be contiguous float32" % name)
    with _on_device(input), _timed(("psroi_fwd[K=%d,D=%d,P=%d]", (K, output_dim, pooled_size)), input):
        check(lib.detops_deform_psroi_pool_forward_f32(
            ptr(input), ptr(bbox), ptr(trans), ptr(out), ptr(top_count), N, C, H, W, K, ct,
            int(bool(no_trans)), float(spatial_scale), output_dim, group_size, pooled_size, part_size,
            sample_per_part, float(trans_std), stream_of(input)), name)


def deform_psroi_pooling_backward(out_grad, input, bbox, trans, top_count, input_grad, trans_grad,
                                  no_trans, spatial_scale, output_dim, group_size, pooled_size,
                                  part_size, sample_per_part, trans_std):
    """reference csrc/deform_pool.h:41-70 -> deform_pool_cuda.cu:64-87.  Accumulates into the
    caller's (zeroed) `input_grad` / `trans_grad` like the reference's atomicAdd kernel."""
    name = "deform_psroi_pooling_backward"
    _need_cuda(name, out_grad, top_count, input_grad)
    if not out_grad.is_contiguous():  # deform_pool_cuda.cu:71
        raise RuntimeError("out_grad tensor has to be contiguous")
    out_grad = _f32c(name, out_grad)
    input, bbox, trans, ct = _psroi_args(name, input, bbox, trans, no_trans, part_size)
    top_count = _f32c(name, top_count)
    N, C, H, W = input.shape
    K = bbox.size(0)
    if K != out_grad.size(0):  # deform_pool_cuda.cu:80-82
        raise RuntimeError("Output shape and bbox number wont match: (%d vs %d)." % (out_grad.size(0), K))
    if not (input_grad.is_contiguous() and input_grad.dtype == torch.float32):
        raise RuntimeError("%s: input_grad must be contiguous float32" % name)
    if not no_trans and not (on_device(trans_grad) and trans_grad.is_contiguous()
                             and trans_grad.dtype == torch.float32 and trans_grad.shape == trans.shape):
        raise RuntimeError("%s: trans_grad must be a contiguous float32 CUDA tensor shaped like trans" % name)
    with _on_device(input), _timed(("psroi_bwd[K=%d,D=%d,P=%d]", (K, output_dim, pooled_size)), input):
        check(lib.detops_deform_psroi_pool_backward_f32(
            ptr(out_grad), ptr(input), ptr(bbox), ptr(trans), ptr(top_count), ptr(input_grad),
            None if no_trans else ptr(trans_grad), N, C, H, W, K, ct, int(bool(no_trans)),
            float(spatial_scale), output_dim, group_size, pooled_size, part_size, sample_per_part,
            float(trans_std), 0, stream_of(input)), name)
