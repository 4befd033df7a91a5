"""GroupNorm (`nn.GroupNorm` with the reference's constructor and `weight` / `bias` keys, so its checkpoints load unchanged).

`forward(x)` is the module call; `fused(x, relu, residual)` is the form the GN models use here: normalisation (+ residual
add) (+ ReLU) in ONE pass of the hand-written HIP kernel (csrc/group_norm.hip), with a deterministic backward.  The kernel
serves channels-last 4-d activations on the device (fp32, or fp16 / bf16 as stored: the output keeps the storage dtype and the
statistics are fp32 — ATen under autocast would return fp32), for the (C, G) `_C.group_norm_supported` answers, while the
switch `_C.GROUP_NORM` is "fused".  Everything else — CPU tensors, NCHW, 2-d inputs (the box head's FC layers), empty
tensors, unserved shapes, the switch on "torch" — calls F.group_norm (+ residual) (+ ReLU), composed as the model always
composed them."""
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from maskrcnn_benchmark import _C


class _GroupNormAct(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, G, eps, relu):
        y, mean, rstd = _C.group_norm_forward(x, G, weight, bias, eps, residual, relu)
        ctx.G, ctx.relu = G, relu
        ctx.save_for_backward(x, mean, rstd, weight, y if relu else None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, mean, rstd, weight, y = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx, gres, gw, gb = _C.group_norm_backward(grad_y, x, y, ctx.G, weight, mean, rstd, ctx.relu, need[3],
                                                  weight is not None and need[1], need[2])
        return (gx if need[0] else None), gw, gb, gres, None, None, None


def _f32(p):
    return None if p is None else (p if p.dtype.is_floating_point and p.dtype.itemsize == 4 else p.float())


class GroupNorm(nn.GroupNorm):
    def serves(self, x):
        """True when `x` takes the HIP kernel"""
        return _C.GROUP_NORM == "fused" and x.dim() == 4 and _C.on_device(x) and _C.group_norm_supported(x, self.num_groups)

    def forward(self, x):
        if self.serves(x):
            return _GroupNormAct.apply(x, _f32(self.weight), _f32(self.bias), None, self.num_groups, self.eps, False)
        return super(GroupNorm, self).forward(x)

    def fused(self, x, relu=False, residual=None):
        """[relu](group_norm(x) [+ residual])"""
        if self.serves(x):
            if residual is not None and residual.dtype != x.dtype:
                residual = residual.to(x.dtype)
            return _GroupNormAct.apply(x, _f32(self.weight), _f32(self.bias), residual, self.num_groups, self.eps, bool(relu))
        out = super(GroupNorm, self).forward(x)
        if residual is not None:
            out += residual
        return F.relu_(out) if relu else out
