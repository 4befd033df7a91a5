"""FrozenBatchNorm2d (reference layers/batch_norm.py:6-31): fixed statistics and affine.

`forward(x)` is the reference's module (x * scale + bias).  `fused(x, relu, residual)` is the form
the backbone uses here: affine (+ residual add) (+ ReLU) in ONE pass of the hand-written HIP
kernel (csrc/frozen_bn.hip) instead of three to four PyTorch elementwise launches per convolution,
with a one-pass backward; the folded scale / bias are cached until a buffer changes.  `conv1x1_fused(conv, x, relu,
residual)` goes one step further for the bottleneck's 1x1 convolutions: the affine (+ residual) (+ ReLU) runs as the
epilogue of the convolution kernel itself (csrc/conv1x1_bn.hip), one launch instead of two, where the library serves the
shape; everything else takes `fused(conv(x), ...)`."""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from maskrcnn_benchmark import _C


class _FrozenBNAct(Function):
    @staticmethod
    def forward(ctx, x, scale, bias, residual, relu):
        y = _C.frozen_bn_act_forward(x, scale, bias, residual, relu)
        ctx.relu = relu
        ctx.save_for_backward(y if relu else None, scale)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        y, scale = ctx.saved_tensors
        need_x, need_res = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        gx, gres = _C.frozen_bn_act_backward(grad_y, y, scale, ctx.relu, need_res)
        return (gx if need_x else None), None, None, gres, None


class _Conv1x1FrozenBNAct(Function):
    """y = [relu](conv2d(x, weight, stride) * scale[k] + bias[k] [+ residual]), forward in one launch.  The backward is the
    two-launch path's: the FrozenBN backward, then the convolution's input / weight gradients."""

    @staticmethod
    def forward(ctx, x, weight, scale, bias, residual, relu, stride, config):
        y = _C.conv1x1_bn_forward(x, weight, scale, bias, residual, relu, stride, config)
        ctx.relu, ctx.stride = relu, stride
        ctx.conv_grads = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]     # a frozen stage asks for neither
        ctx.save_for_backward(y if relu else None, scale, *((x, weight) if ctx.conv_grads else ()))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        y, scale = ctx.saved_tensors[:2]
        need_x, need_w, need_res = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[4]
        g, gres = _C.frozen_bn_act_backward(grad_y, y, scale, ctx.relu, need_res)
        gx = gw = None
        if ctx.conv_grads:
            x, weight = ctx.saved_tensors[2:]
            s = ctx.stride
            gx, gw, _ = torch.ops.aten.convolution_backward(g, x, weight, None, [s, s], [0, 0], [1, 1], False, [0, 0], 1,
                                                            [need_x, need_w, False])
        return gx, gw, None, None, gres, None, None, None


def _plain_conv1x1(conv):
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and conv.bias is None and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.stride[0] == conv.stride[1])


class FrozenBatchNorm2d(nn.Module):
    def __init__(self, n):
        super(FrozenBatchNorm2d, self).__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))
        self._folded = None

    def folded(self):
        """(scale, bias) fp32 [C]: scale = weight * rsqrt(var), bias = bias - mean * scale.  Cached; the key checked on
        the hot path is the four buffers' version counters (in-place writes, `load_state_dict`) AND their storage addresses
        (`buf.data = x`, `module._buffers[name] = t`, which bypass `__setattr__` / `_apply`).  The one write no key can
        see is an in-place write through the `.data` alias (`buf.data.copy_(x)` bumps no counter and moves nothing):
        call `invalidate()` after it."""
        b = self._buffers      # (nn.Module.__getattr__ costs ~0.5 us per buffer access)
        w, bi, m, v = b["weight"], b["bias"], b["running_mean"], b["running_var"]
        version = (w._version + bi._version + m._version + v._version, w.data_ptr(), bi.data_ptr(), m.data_ptr(), v.data_ptr())
        f = self._folded
        if f is None or f[0] != version:
            with torch.no_grad():
                scale = self.weight.float() * self.running_var.float().rsqrt()
                bias = self.bias.float() - self.running_mean.float() * scale
            f = self._folded = (version, scale.contiguous(), bias.contiguous())
        return f[1], f[2]

    def invalidate(self):
        """drop the cached folded scale / bias (needed only after in-place writes through `.data`, see folded())"""
        self._folded = None

    def _apply(self, fn, *args, **kwargs):
        self._folded = None
        return super(FrozenBatchNorm2d, self)._apply(fn, *args, **kwargs)

    def __setattr__(self, name, value):
        if name in ("weight", "bias", "running_mean", "running_var"):
            object.__setattr__(self, "_folded", None)
        super(FrozenBatchNorm2d, self).__setattr__(name, value)

    def forward(self, x):
        # the folded scale/bias follow the activation dtype (reference casts the buffers to half)
        scale, bias = self.folded()
        return x * scale.reshape(1, -1, 1, 1).to(x.dtype) + bias.reshape(1, -1, 1, 1).to(x.dtype)

    def fused(self, x, relu=False, residual=None):
        scale, bias = self.folded()
        if residual is not None and residual.dtype != x.dtype:
            residual = residual.to(x.dtype)
        return _FrozenBNAct.apply(x, scale, bias, residual, relu)

    def conv1x1_fused(self, conv, x, relu=False, residual=None):
        """`self.fused(conv(x), relu, residual)` for a bias-free 1x1 convolution module — as ONE launch where
        _C.conv1x1_bn_config serves the case (fp32, channels-last, on the device, a routed shape; the switch
        _C.CONV1X1_BN turns it off or picks a tile configuration instead of the routing table), as those two calls otherwise."""
        mode = _C.CONV1X1_BN
        if mode is not None and _plain_conv1x1(conv):
            if residual is not None and residual.dtype != x.dtype:
                residual = residual.to(x.dtype)
            cfg = _C.conv1x1_bn_config(x, conv.weight, conv.stride[0], residual, mode)
            if cfg:
                scale, bias = self.folded()
                return _Conv1x1FrozenBNAct.apply(x, conv.weight, scale, bias, residual, relu, conv.stride[0], cfg)
        return self.fused(conv(x), relu=relu, residual=residual)
