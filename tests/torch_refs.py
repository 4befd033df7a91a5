"""Independent PyTorch / numpy formulations used to cross-check the oracle's restatements of the
reference's CUDA-only operators (ROIAlign backward, ROIPool, deformable conv).  They are written
from the operator DEFINITIONS, vectorised and differentiable, i.e. not a
transcription of either the reference kernels or of oracle/detops_oracle.c.
"""
import math

import numpy as np
import torch


def _axis_table(start, bin_size, P, grid, size, dtype):
    """Per-axis sample table for ROIAlign: for p in [0,P), i in [0,grid):
    returns (low idx, high idx, w_low, w_high, valid) each of shape [P*grid]."""
    p = torch.arange(P, dtype=dtype).repeat_interleave(grid)
    i = torch.arange(grid, dtype=dtype).repeat(P)
    c = start + p * bin_size + (i + 0.5) * bin_size / grid
    valid = ~((c < -1.0) | (c > size))
    c = c.clamp(min=0)
    low = c.floor().long()
    edge = low >= size - 1
    low = torch.where(edge, torch.full_like(low, size - 1), low)
    high = torch.where(edge, low, low + 1)
    c = torch.where(edge, low.to(dtype), c)
    frac = c - low.to(dtype)
    return low, high, (1 - frac) * valid, frac * valid


def roi_align_torch(x, rois, scale, PH, PW, sampling_ratio):
    """x [N,C,H,W] (double), rois [K,5]; separable-matrix formulation:
    out[k,c] = Ay[k] @ x[b_k, c] @ Ax[k]^T / count."""
    N, C, H, W = x.shape
    outs = []
    for r in rois:
        b = int(r[0])
        sw, sh, ew, eh = [float(v) * scale for v in r[1:]]
        rw, rh = max(ew - sw, 1.0), max(eh - sh, 1.0)
        gh = sampling_ratio if sampling_ratio > 0 else int(math.ceil(rh / PH))
        gw = sampling_ratio if sampling_ratio > 0 else int(math.ceil(rw / PW))
        yl, yh, wyl, wyh = _axis_table(sh, rh / PH, PH, gh, H, x.dtype)
        xl, xh, wxl, wxh = _axis_table(sw, rw / PW, PW, gw, W, x.dtype)
        Ay = torch.zeros(PH * gh, H, dtype=x.dtype)
        Ay.scatter_add_(1, yl[:, None], wyl[:, None])
        Ay.scatter_add_(1, yh[:, None], wyh[:, None])
        Ax = torch.zeros(PW * gw, W, dtype=x.dtype)
        Ax.scatter_add_(1, xl[:, None], wxl[:, None])
        Ax.scatter_add_(1, xh[:, None], wxh[:, None])
        Ay = Ay.view(PH, gh, H).sum(1)
        Ax = Ax.view(PW, gw, W).sum(1)
        if bool(torch.isfinite(x[b]).all()):
            outs.append(torch.einsum("ph,chw,qw->cpq", Ay, x[b], Ax) / (gh * gw))
            continue
        # a non-finite plane: a sample outside [-1, size] counts as 0 WITHOUT reading anything (the operator returns before
        # it touches the map), and a pixel no sample of a bin touches is not read for that bin — so a zero entry of Ay / Ax
        # must contribute 0, not 0 * Inf
        rows = torch.where((Ay != 0)[None, :, :, None], Ay[None, :, :, None] * x[b][:, None, :, :], x.new_zeros(())).sum(2)
        outs.append(torch.where((Ax != 0)[None, None, :, :], Ax[None, None, :, :] * rows[:, :, None, :],
                                x.new_zeros(())).sum(3) / (gh * gw))
    if not outs:
        return x.new_zeros((0, C, PH, PW))
    return torch.stack(outs)


def _c_round(v):
    """C roundf: half away from zero."""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def roi_pool_py(inp, rois, scale, PH, PW):
    N, C, H, W = inp.shape
    K = rois.shape[0]
    out = np.zeros((K, C, PH, PW), np.float32)
    amax = np.full((K, C, PH, PW), -1, np.int32)
    f32 = np.float32
    for k in range(K):
        b = int(rois[k, 0])
        x1, y1, x2, y2 = [_c_round(float(f32(v) * f32(scale))) for v in rois[k, 1:]]
        rw, rh = max(x2 - x1 + 1, 1), max(y2 - y1 + 1, 1)
        bh, bw = f32(rh) / f32(PH), f32(rw) / f32(PW)
        for ph in range(PH):
            hs = min(max(int(np.floor(f32(ph) * bh)) + y1, 0), H)
            he = min(max(int(np.ceil(f32(ph + 1) * bh)) + y1, 0), H)
            for pw in range(PW):
                ws = min(max(int(np.floor(f32(pw) * bw)) + x1, 0), W)
                we = min(max(int(np.ceil(f32(pw + 1) * bw)) + x1, 0), W)
                if he <= hs or we <= ws:
                    continue
                win = inp[b, :, hs:he, ws:we].reshape(C, -1)
                # the maximum starts at -FLT_MAX and only a greater value replaces it: a NaN, -inf or -FLT_MAX never does
                with np.errstate(invalid="ignore"):
                    cand = np.where(win > np.float32(-np.finfo(np.float32).max), win, -np.inf)
                j = cand.argmax(1)  # first maximum in row-major order
                none = np.isneginf(cand[np.arange(C), j])
                out[k, :, ph, pw] = np.where(none, np.float32(-np.finfo(np.float32).max), win[np.arange(C), j])
                amax[k, :, ph, pw] = np.where(none, -1, (hs + j // (we - ws)) * W + ws + j % (we - ws))
    return out, amax


def deform_conv_torch(x, offset, mask, weight, bias, stride, pad, dil, group, dg):
    """Differentiable deformable conv (v1 when mask is None, v2 otherwise).
    x [B,C,H,W], offset [B,dg*2*k*k,Ho,Wo] (dh at 2*(i*kw+j), dw at +1), mask [B,dg*k*k,Ho,Wo]."""
    B, C, H, W = x.shape
    Cout, Cg, kh, kw = weight.shape
    Ho = (H + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1
    dt = x.dtype
    ho = torch.arange(Ho, dtype=dt).view(1, 1, Ho, 1)
    wo = torch.arange(Wo, dtype=dt).view(1, 1, 1, Wo)
    cols = []
    cpg = C // dg
    for i in range(kh):
        for j in range(kw):
            tap = i * kw + j
            per_g = []
            for g in range(dg):
                dh = offset[:, g * 2 * kh * kw + 2 * tap].unsqueeze(1)
                dw = offset[:, g * 2 * kh * kw + 2 * tap + 1].unsqueeze(1)
                hh = ho * stride - pad + i * dil + dh  # [B,1,Ho,Wo]
                ww = wo * stride - pad + j * dil + dw
                inside = (hh > -1) & (ww > -1) & (hh < H) & (ww < W)
                h0 = hh.detach().floor()
                w0 = ww.detach().floor()
                lh, lw = hh - h0, ww - w0
                xs = x[:, g * cpg:(g + 1) * cpg]
                val = 0
                for (hi, wi, wt) in ((h0, w0, (1 - lh) * (1 - lw)), (h0, w0 + 1, (1 - lh) * lw),
                                     (h0 + 1, w0, lh * (1 - lw)), (h0 + 1, w0 + 1, lh * lw)):
                    ok = (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1) & inside
                    idx = (hi.clamp(0, H - 1) * W + wi.clamp(0, W - 1)).long()  # [B,1,Ho,Wo]
                    v = xs.flatten(2).gather(2, idx.view(B, 1, -1).expand(B, cpg, -1))
                    val = val + v.view(B, cpg, Ho, Wo) * (wt * ok)
                if mask is not None:
                    val = val * mask[:, g * kh * kw + tap].unsqueeze(1)
                per_g.append(val)
            cols.append(torch.cat(per_g, 1))  # [B,C,Ho,Wo]
    col = torch.stack(cols, 2)  # [B,C,kh*kw,Ho,Wo]
    Mg = Cout // group
    outs = []
    for g in range(group):
        cg = col[:, g * Cg:(g + 1) * Cg].reshape(B, Cg * kh * kw, Ho * Wo)
        wg = weight[g * Mg:(g + 1) * Mg].reshape(Mg, Cg * kh * kw)
        outs.append(torch.einsum("mk,bkp->bmp", wg, cg))
    out = torch.cat(outs, 1).view(B, Cout, Ho, Wo)
    if bias is not None:
        out = out + bias.view(1, -1, 1, 1)
    return out


def deform_psroi_pool_torch(data, rois, trans, no_trans, scale, output_dim, group_size, P, part_size,
                            S, trans_std):
    """Deformable PS-ROI pooling from its definition (Deformable ConvNets, eq. 5-6 as the reference
    discretises it): data [N,C,H,W] double, rois [K,5], trans [K,2*ncls,part,part] or None.
    Differentiable in `data` and `trans`; the border clamp is straight-through (the operator's
    offset gradient ignores the clamp).  Returns (out, count) [K,output_dim,P,P]."""
    N, C, H, W = data.shape
    dt = data.dtype
    ncls = 1 if no_trans else trans.shape[1] // 2
    cec = output_dim if no_trans else output_dim // ncls
    ar = torch.arange(P, dtype=dt)
    # the cell and group of a bin are integer decisions the operator takes in fp32 (its scalar type): 7 / 23 * 23 is
    # 6.9999995 there and floors to 6, whatever a wider type would say
    ar32 = torch.arange(P, dtype=torch.float32)
    part = torch.floor(ar32 / P * part_size).long()
    grp = torch.floor(ar32 * group_size / P).long().clamp(0, group_size - 1)
    sub = torch.arange(S, dtype=dt)
    cls_of = torch.arange(output_dim) // cec
    # position-sensitive plane of (ctop, ph, pw)
    plane = (torch.arange(output_dim)[:, None, None] * group_size + grp[None, :, None]) * group_size + grp[None, None, :]
    outs, cnts = [], []
    for k in range(rois.shape[0]):
        b = int(rois[k, 0])
        x1, y1, x2, y2 = [float(_c_round(float(v))) for v in rois[k, 1:]]
        sw, sh = x1 * scale - 0.5, y1 * scale - 0.5
        ew, eh = (x2 + 1.0) * scale - 0.5, (y2 + 1.0) * scale - 0.5
        rw, rh = max(ew - sw, 0.1), max(eh - sh, 0.1)
        bw, bh = rw / P, rh / P
        if no_trans:
            tx = torch.zeros(output_dim, P, P, dtype=dt)
            ty = torch.zeros(output_dim, P, P, dtype=dt)
        else:
            t = trans[k].view(ncls, 2, part_size, part_size)[cls_of]          # [D,2,part,part]
            t = t[:, :, part][:, :, :, part]                                 # [D,2,P,P]
            tx, ty = t[:, 0] * trans_std, t[:, 1] * trans_std
        ws = ar[None, None, :] * bw + sw + tx * rw                            # [D,P,P]
        hs = ar[None, :, None] * bh + sh + ty * rh
        w = ws[..., None, None] + sub[None, None, None, None, :] * (bw / S)   # [D,P,P,S,S] (ih, iw)
        h = hs[..., None, None] + sub[None, None, None, :, None] * (bh / S)
        w, h = torch.broadcast_tensors(w, h)
        valid = ~((w < -0.5) | (w > W - 0.5) | (h < -0.5) | (h > H - 0.5))
        wc = w + (w.clamp(0, W - 1) - w).detach()
        hc = h + (h.clamp(0, H - 1) - h).detach()
        x0, x1i = wc.detach().floor().long(), wc.detach().ceil().long()
        y0, y1i = hc.detach().floor().long(), hc.detach().ceil().long()
        x0, x1i, y0, y1i = [v.clamp(0, m) for v, m in ((x0, W - 1), (x1i, W - 1), (y0, H - 1), (y1i, H - 1))]
        dx, dy = wc - x0.to(dt), hc - y0.to(dt)
        img = data[b].reshape(C, H * W)
        pl = plane[..., None, None].expand_as(x0)

        def tap(yy, xx):
            return img[pl, yy * W + xx]

        val = ((1 - dx) * (1 - dy) * tap(y0, x0) + (1 - dx) * dy * tap(y1i, x0)
               + dx * (1 - dy) * tap(y0, x1i) + dx * dy * tap(y1i, x1i))
        val = torch.where(valid, val, torch.zeros_like(val))
        cnt = valid.sum((-1, -2)).to(dt)
        outs.append(torch.where(cnt > 0, val.sum((-1, -2)) / cnt.clamp(min=1), torch.zeros_like(cnt)))
        cnts.append(cnt)
    if not outs:
        z = data.new_zeros((0, output_dim, P, P))
        return z, z
    return torch.stack(outs), torch.stack(cnts)


# ---------------------------------------------------------------------------------------------- fused ReLU, non-finite values
def _exact(got, want, what):
    """same dtype, same NaN positions, every other element equal (+0 == -0)"""
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    torch.testing.assert_close(got, want, rtol=0, atol=0, equal_nan=True, msg=lambda m: "%s: %s" % (what, m))


def check_fused_relu_non_finite(device, dtype, channels_last):
    """The fused ReLU of FrozenBatchNorm2d.fused (csrc/frozen_bn.hip) and of _C.bias_act (csrc/bias_act.hip) follows
    torch.relu on non-finite values: NaN stays NaN in the forward, and the backward is aten.threshold_backward(g, y, 0),
    which passes the gradient where y is NaN.  Inputs hold NaN, +-inf, -0.0 and inf + (-inf) through the residual; the
    reference is the fp32 composition on the same dtype-rounded values, one rounding at the end."""
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.layers import FrozenBatchNorm2d
    N, C, H, W = 2, 8, 4, 6
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    g = torch.Generator().manual_seed(11 + int(channels_last))
    inf, nan = float("inf"), float("nan")
    x = torch.randn(N, C, H, W, generator=g)
    r = torch.randn(N, C, H, W, generator=g)
    x[:, :, 0, :5] = torch.tensor([nan, inf, -inf, -0.0, 0.0])
    x[:, :, 1, :4] = torch.tensor([inf, -inf, 1.0, inf])
    r[:, :, 1, :4] = torch.tensor([-inf, inf, nan, inf])          # inf + (-inf) = NaN, NaN residual, inf + inf
    r[:, :, 2, :2] = torch.tensor([-0.0, -inf])
    x, r = x.to(dtype), r.to(dtype)
    gy = torch.randn(N, C, H, W, generator=g).to(dtype)

    bn = FrozenBatchNorm2d(C)
    bn.weight.copy_(torch.linspace(-1.5, 1.5, C))                 # signed scales: +-inf swap sign in some channels
    bn.bias.copy_(torch.randn(C, generator=g))
    bn.running_mean.copy_(torch.randn(C, generator=g))
    bn.running_var.copy_(torch.rand(C, generator=g) + 0.3)
    bn = bn.to(device)
    scale, bias = (t.cpu().reshape(1, -1, 1, 1) for t in bn.folded())
    for res in (False, True):
        xd = x.to(device).clone(memory_format=fmt).requires_grad_()
        rd = r.to(device).clone(memory_format=fmt).requires_grad_() if res else None
        y = bn.fused(xd, relu=True, residual=rd)
        y.backward(gy.to(device).contiguous(memory_format=fmt))
        assert _C.is_channels_last(y) == channels_last and _C.is_channels_last(xd.grad) == channels_last
        t = x.float() * scale + bias
        if res:
            t = t + r.float()
        want = torch.relu(t).to(dtype)
        assert int(want.isnan().sum()) > 0 and int(torch.isinf(want).sum()) > 0
        _exact(y.detach().cpu(), want, "frozen_bn forward res=%d" % res)
        m = torch.ops.aten.threshold_backward(gy.float(), want.float(), 0)
        _exact(xd.grad.cpu(), (m * scale).to(dtype), "frozen_bn grad_x res=%d" % res)
        if res:
            _exact(rd.grad.cpu(), m.to(dtype), "frozen_bn grad_residual")

    if not channels_last:
        return
    # bias_act: the FrozenBN stream with scale 1 forward; its own backward pass (mask, grad_x, fp32 column sums).  C = 8 takes
    # the fused kernels, C = 12 the generic path (in-place add + column_sum).
    for Cb in (8, 12):
        xb = torch.cat([x, x[:, :Cb - C]], 1) if Cb > C else x
        gb = torch.cat([gy, gy[:, :Cb - C]], 1) if Cb > C else gy
        b = torch.randn(Cb, generator=g)
        xd = xb.to(device).clone(memory_format=torch.channels_last).requires_grad_()
        bd = b.to(device).clone().requires_grad_()
        y = _C.bias_act(xd.clone(memory_format=torch.channels_last), bd, True)
        y.backward(gb.to(device).contiguous(memory_format=torch.channels_last))
        # (the generic path adds the bias in the activation's dtype, as the convolution's own bias would)
        bias_as = b if Cb == 8 else b.to(dtype).float()
        want = torch.relu(xb.float() + bias_as.reshape(1, -1, 1, 1)).to(dtype)
        _exact(y.detach().cpu(), want, "bias_act forward C=%d" % Cb)
        m = torch.ops.aten.threshold_backward(gb.float(), want.float(), 0)
        _exact(xd.grad.cpu(), m.to(dtype), "bias_act grad_x C=%d" % Cb)
        terms = m.double()
        # fp32 sums of n terms in any order: |error| <= n * eps32 * sum |terms|
        colsum, bound = terms.sum((0, 2, 3)), terms[:, 0].numel() * 2.0 ** -24 * terms.abs().sum((0, 2, 3))
        got = bd.grad.cpu().double()
        assert bool(((got - colsum).abs() <= bound).all()), ("bias_act grad_bias C=%d" % Cb, got, colsum)


# ---------------------------------------------------------------------------------------------- deformable conv, channels-last plan
import contextlib  # noqa: E402


@contextlib.contextmanager
def launches():
    """-> dict, filled on exit: calls per `_C._timed` name (the part of its format before "[") made inside the block,
    counted by a `_C.KernelTimer(count_only=True)` (no events: works on CPU tensors under the host emulation too)"""
    from maskrcnn_benchmark import _C
    counts = {}
    timer = _C.KernelTimer(count_only=True)
    prev, _C.KERNEL_TIMER = _C.KERNEL_TIMER, timer
    try:
        yield counts
    finally:
        _C.KERNEL_TIMER = prev
        for name, n in timer.calls.items():
            key = (name[0] if type(name) is tuple else name).split("[")[0]
            counts[key] = counts.get(key, 0) + n


# the smallest shape inside the channels-last plan in fp32 (64 channels = 16 vectors of 16 bytes), odd map sides
DCN_IN_PLAN = dict(B=2, C=64, H=9, W=11, k=3)


def _dcn_in_plan_case(modulated, seed):
    import synth
    g = DCN_IN_PLAN
    x, off, mask, wgt = synth.dcn_inputs(g["B"], g["C"], g["H"], g["W"], g["C"], g["k"], 1, modulated, seed=seed)
    go = np.random.RandomState(seed + 1).randn(*x.shape).astype(np.float32)      # 3x3, pad 1, stride 1: output = input size
    return x, off, mask, wgt, go


def _near(got, want, tol, what):
    err = float(np.abs(got.detach().cpu().numpy() - want).max())      # NaN (a buffer not overwritten) fails the comparison
    assert err <= tol * max(1.0, float(np.abs(want).max())), (what, err)


def check_dcn_reference_names_in_plan(device, modulated, tol):
    """The reference-named backward entry points of `_C` (v1: deform_conv_backward_input + deform_conv_backward_parameters with
    scale 0.5; v2: modulated_deform_conv_backward) on a shape the channels-last pipeline serves, against the oracle, with
    the reference's ownership rules: gradInput / gradWeight / grad_bias are accumulated into (pre-filled with ones: the
    result is 1 + gradient), gradOffset / grad_mask are overwritten in full (pre-filled with NaN); and the launches."""
    import oracle
    from maskrcnn_benchmark import _C
    g = DCN_IN_PLAN
    B, C, k = g["B"], g["C"], g["k"]
    x, off, mask, wgt, go = _dcn_in_plan_case(modulated, 41)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    tx, toff, tw, tgo = t(x), t(off), t(wgt), t(go)
    e = torch.empty(0, device=device)
    gi, gw, gb = torch.ones_like(tx), torch.ones_like(tw), torch.ones(C, device=device)
    goff, gm = torch.full_like(toff, float("nan")), None
    geo = (k, k, 1, 1, 1, 1, 1, 1, 1, 1)           # kernel, stride, pad, dilation (square: either argument order), group, dg
    with launches() as calls:
        if modulated:
            tm = t(mask)
            gm = torch.full_like(tm, float("nan"))
            _C.modulated_deform_conv_backward(tx, tw, torch.zeros(C, device=device), e, toff, tm, e, gi, gw, gb, goff, gm, tgo,
                                              *geo, True)
        else:
            assert _C.deform_conv_backward_input(tx, toff, tgo, gi, goff, tw, e, *geo, B) == 1
            assert _C.deform_conv_backward_parameters(tx, toff, tgo, gw, e, e, *geo, 0.5, B) == 1
    # v1 asks in two calls, each of which transposes the input and the output gradient again
    assert calls == {"dcn_to_nhwc": 2 if modulated else 4, "dcn_coord_nhwc": 1, "dcn_col2im_nhwc": 1, "dcn_im2col_nhwc": 1}, calls
    rin, roff, rmask, rw, rb = oracle.deform_conv_backward(x, off, mask, wgt, go, modulated, (1, 1), (1, 1), (1, 1), 1, 1)
    _near(gi, 1.0 + rin, tol, "gradInput")
    _near(goff, roff, tol, "gradOffset")
    _near(gw, 1.0 + (1.0 if modulated else 0.5) * rw, tol, "gradWeight")
    if modulated:
        _near(gm, rmask, tol, "grad_mask")
        _near(gb, 1.0 + rb, tol, "grad_bias")


def check_dcn_layer_in_plan(device, modulated, channels_last, tol, input_grad_kernel="dcn_col2im_nhwc"):
    """deform_conv / modulated_deform_conv (layers/dcn) forward + backward on a shape the channels-last pipeline serves,
    NCHW or everything (input, offset, mask, weight, upstream gradient) channels-last: the oracle's output and gradients,
    and the launch sequence — one im2col (the forward's column matrix is kept for the backward pass), the coordinate kernel,
    `input_grad_kernel`, and the two layout transposes (input, output gradient) that only NCHW tensors need."""
    import oracle
    from maskrcnn_benchmark import _C
    from maskrcnn_benchmark.layers import deform_conv, modulated_deform_conv
    x, off, mask, wgt, go = _dcn_in_plan_case(modulated, 43)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    t = lambda a: torch.from_numpy(a).to(device).contiguous(memory_format=fmt)  # noqa: E731
    tx, toff, tw = (t(a).requires_grad_() for a in (x, off, wgt))
    tm = t(mask).requires_grad_() if modulated else None
    with launches() as calls:
        y = modulated_deform_conv(tx, toff, tm, tw, None, 1, 1, 1, 1, 1) if modulated else deform_conv(tx, toff, tw, 1, 1, 1, 1, 1)
        y.backward(t(go))
    want = {"dcn_im2col_nhwc": 1, "dcn_coord_nhwc": 1, input_grad_kernel: 1}
    if not channels_last:
        want["dcn_to_nhwc"] = 2
    assert {k: v for k, v in calls.items() if k.startswith("dcn_")} == want, calls
    assert _C.is_channels_last(y) == channels_last and _C.is_channels_last(tx.grad) == channels_last
    og = ((1, 1), (1, 1), (1, 1), 1, 1)
    _near(y, oracle.deform_conv_forward(x, off, mask, wgt, None, *og), tol, "output")
    rin, roff, rmask, rw, _ = oracle.deform_conv_backward(x, off, mask, wgt, go, False, *og)
    _near(tx.grad, rin, tol, "input gradient")
    _near(toff.grad, roff, tol, "offset gradient")
    _near(tw.grad, rw, tol, "weight gradient")
    if modulated:
        _near(tm.grad, rmask, tol, "mask gradient")
