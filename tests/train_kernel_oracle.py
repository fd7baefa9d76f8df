"""Plain torch restatements of the non-convolution training kernels (csrc/bn_train.hip, csrc/ln_train.hip,
csrc/train_ew.hip, csrc/attn_spatial_train.hip, csrc/channel_gate_train.hip, csrc/ubf_train.hip, csrc/roi_align.hip),
one function per kernel family.

Every function is dtype-generic: it computes in the dtype of its floating inputs.  The GPU tests call each one
twice on the same inputs (already rounded to the kernel's compute dtype): once in float64 -- the reference -- and
once in float32, whose element-wise distance from the float64 result (`e32`) is the yardstick of the bounds.
Gradients come from autograd, except where the forward's own choice has to be replayed (the spatial attention's
max channel and the max-pool's window maximum are routed through an explicit first-maximum index).

The Dropout2d mask oracle is exact integer arithmetic (splitmix64), no floating point.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_GELU, ACT_SWISH = range(6)


def act_fn(v, act, beta=1.0):
    """include/hiseg.h hiseg_act at the pre-activation v."""
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v * (1.0 / math.sqrt(2.0))))
    if act == ACT_SWISH:
        return v * torch.sigmoid(beta * v)
    raise ValueError(act)


def _leaf(t):
    return t.detach().clone().requires_grad_(True)


def _grads(outs, wrt, gouts):
    """d sum_i <outs_i, gouts_i> / d wrt (zeros where unused)."""
    loss = sum((o * g).sum() for o, g in zip(outs, gouts))
    gs = torch.autograd.grad(loss, wrt, allow_unused=True)
    return [torch.zeros_like(w) if g is None else g for g, w in zip(gs, wrt)]


# ----------------------------------------------------------------------------------------- element-wise
# Tensors are [P][C] (the live channels of a view); chan_mul is [N][C], pixel p belongs to image p // HW.
def relu_bwd(dy, y, chan_mul, HW):
    g = dy
    if chan_mul is not None:
        g = g * chan_mul.repeat_interleave(HW, dim=0)
    return torch.where(y > 0, g, torch.zeros_like(g))


def sigmoid_bwd(dy, s):
    return dy * s * (1 - s)


def gate_fwd(a, g):
    return a * g


def gate_bwd(dy, a, g):
    """(da, dzg) of out = a * g with g = sigmoid(zg)."""
    return dy * g, dy * a * g * (1 - g)


def act_bwd_cvt(dy, y, act):
    """dy * act'(.) recovered from the activation's OUTPUT y (none, ReLU, sigmoid)."""
    if act == ACT_NONE:
        return dy.clone()
    if act == ACT_RELU:
        return torch.where(y > 0, dy, torch.zeros_like(dy))
    if act == ACT_SIGMOID:
        return dy * y * (1 - y)
    raise ValueError("the derivative of a smooth activation is not a function of its output")


def act_bwd_pre(dy, z, act, beta=1.0):
    """dy * act'(z) at the pre-activation z, by autograd."""
    zl = _leaf(z)
    (g,) = _grads([act_fn(zl, act, beta)], [zl], [dy])
    return g


def add(dst, src):
    return dst + src


# ----------------------------------------------------------------------------------------- pooling / resampling
def maxpool2x2_bwd(x, dy):
    """x [N][H][W][C], dy [N][H/2][W/2][C] -> dx: dy routed to the FIRST maximum of each window in the order
    (0,0), (0,1), (1,0), (1,1)."""
    N, H, W, C = x.shape
    win = [x[:, i::2, j::2, :] for i in (0, 1) for j in (0, 1)]
    best = torch.full_like(win[0], -math.inf)
    arg = torch.zeros(win[0].shape, dtype=torch.long)
    for k, v in enumerate(win):
        upd = v > best
        best = torch.where(upd, v, best)
        arg = torch.where(upd, torch.full_like(arg, k), arg)
    dx = torch.zeros_like(x)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, i::2, j::2, :] = torch.where(arg == k, dy, torch.zeros_like(dy))
    return dx


def upsample2x_bwd(dy):
    """dy [N][2h][2w][C] -> [N][h][w][C]: the sum of each pixel's 2x2 children (nearest x2 upsample backward)."""
    N, H, W, C = dy.shape
    return dy.reshape(N, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4))


def _resize_matrix(out, inp, dtype):
    """[out][inp] row-stochastic matrix of bilinear interpolation, align_corners=False."""
    scale = torch.tensor(inp, dtype=dtype) / torch.tensor(out, dtype=dtype)
    o = torch.arange(out, dtype=dtype)
    s = torch.clamp(scale * (o + 0.5) - 0.5, min=0)
    i0 = torch.floor(s).long().clamp(max=inp - 1)
    i1 = torch.clamp(i0 + 1, max=inp - 1)
    l1 = s - i0.to(dtype)
    A = torch.zeros(out, inp, dtype=dtype)
    rows = torch.arange(out)
    A.index_put_((rows, i0), 1 - l1, accumulate=True)
    A.index_put_((rows, i1), l1, accumulate=True)
    return A


def resize_bilinear_fwd(x, H, W):
    """x [NC][h][w] -> [NC][H][W], F.interpolate(mode='bilinear', align_corners=False)."""
    Ay, Ax = _resize_matrix(H, x.shape[1], x.dtype), _resize_matrix(W, x.shape[2], x.dtype)
    return torch.einsum("Yy,nyx,Xx->nYX", Ay, x, Ax)


def resize_bilinear_bwd(dy, h, w):
    """dy [NC][H][W] -> dx [NC][h][w]: the adjoint of resize_bilinear_fwd."""
    Ay, Ax = _resize_matrix(dy.shape[1], h, dy.dtype), _resize_matrix(dy.shape[2], w, dy.dtype)
    return torch.einsum("Yy,nYX,Xx->nyx", Ay, dy, Ax)


# ----------------------------------------------------------------------------------------- attention modules
def first_argmax(x):
    """Index of the first maximal entry along the last axis."""
    C = x.shape[-1]
    mx = x.max(dim=-1, keepdim=True).values
    idx = torch.where(x == mx, torch.arange(C), torch.full((1,), C, dtype=torch.long))
    return idx.min(dim=-1).values


def spatial_attention(x, w7, chan_mul, dout=None, dw7_old=None):
    """x [N][H][W][C], w7 [2][k][k], chan_mul [N][C] or None.
    out = x * sigmoid(conv_kxk([mean_c x, max_c x])) * chan_mul; the max-channel gradient goes to the first
    maximal channel."""
    k = w7.shape[-1]
    xl, wl = _leaf(x), _leaf(w7)
    am = first_argmax(x)
    mean = xl.mean(dim=-1)
    mx = xl.gather(-1, am.unsqueeze(-1)).squeeze(-1)
    pre = F.conv2d(torch.stack([mean, mx], dim=1), wl.unsqueeze(0), padding=k // 2)[:, 0]
    att = torch.sigmoid(pre)
    out = xl * att.unsqueeze(-1)
    if chan_mul is not None:
        out = out * chan_mul[:, None, None, :]
    r = {"out": out.detach(), "att": att.detach(), "mean": mean.detach(), "max": mx.detach(), "argmax": am}
    if dout is not None:
        dx, dw = _grads([out], [xl, wl], [dout])
        r["dx"] = dx
        r["dw7"] = dw + (0 if dw7_old is None else dw7_old)
    return r


def channel_attention(x, w1, b1, w2, b2, act, beta, chan_mul, dout=None, old=None):
    """x [N][HW][C], w1 [Cr][C], w2 [C][Cr], biases or None (ChannelAttentionModule has none, SqueezeExcite has
    both): out = x * sigmoid(W2 act(W1 gap(x) + b1) + b2) * chan_mul.  old: dict of preloaded parameter gradients
    the backward adds to."""
    xl = _leaf(x)
    ps = {"w1": _leaf(w1), "w2": _leaf(w2)}
    if b1 is not None:
        ps["b1"], ps["b2"] = _leaf(b1), _leaf(b2)
    gap = xl.mean(dim=1)
    hpre = gap @ ps["w1"].t()
    if b1 is not None:
        hpre = hpre + ps["b1"]
    s = act_fn(hpre, act, beta) @ ps["w2"].t()
    if b1 is not None:
        s = s + ps["b2"]
    gate = torch.sigmoid(s)
    out = xl * gate.unsqueeze(1)
    if chan_mul is not None:
        out = out * chan_mul.unsqueeze(1)
    r = {"gap": gap.detach(), "hpre": hpre.detach(), "gate": gate.detach(), "out": out.detach()}
    if dout is not None:
        names = list(ps)
        gs = _grads([out], [xl] + [ps[n] for n in names], [dout])
        r["dx"] = gs[0]
        for n, g in zip(names, gs[1:]):
            r["d" + n] = g + (0 if old is None else old["d" + n])
    return r


# ----------------------------------------------------------------------------------------- upsample_bg_fg head
UBF_PARAMS = ("ut_w", "ut_b", "gamma", "beta", "u1_w", "u1_b")


def ubf_head(low, p, tfeat, t_w, t_b, act, beta, layernorm, eps=1e-5, momentum=0.1, running=None, grads=None,
             old=None):
    """include/hiseg_head_train.h hiseg_ubf_desc: low [N][h][w][2]; p: dict of ut_w [2][32][2][2], ut_b, gamma,
    beta [32], u1_w [2][32], u1_b [2]; tfeat [N][2h][2w][Ct], t_w [2][Ct], t_b [2].
      z = ConvTranspose2d(2, 32, 2, 2)(low);  a = act(z * scale + shift) with the fold of train-mode BatchNorm2d
      (statistics over N, H, W) or LayerNorm2d (per sample over C, H, W);  b = Conv2d(32, 2, 1)(a);
      t = Conv2d(Ct, 2, 1)(tfeat);  p_fg = softmax(b)[1];  logits = (b0, b1 + t0 p_fg, b1 + t1 p_fg).
    running: (running_mean, running_var) before the step (BatchNorm).  grads: (dlogits, dbgfg_ext or None,
    dtn_ext or None), all NCHW; old: preloaded parameter gradients the backward adds to."""
    ll = _leaf(low)
    q = {n: _leaf(p[n]) for n in UBF_PARAMS}
    N = low.shape[0]
    z = F.conv_transpose2d(ll.permute(0, 3, 1, 2), q["ut_w"], q["ut_b"], stride=2)
    r = {}
    if layernorm:
        mean = z.mean(dim=(1, 2, 3))
        var = ((z - mean.view(N, 1, 1, 1)) ** 2).mean(dim=(1, 2, 3))
        invstd = 1 / torch.sqrt(var + eps)
        scale = q["gamma"].view(1, 32) * invstd.view(N, 1)
        shift = q["beta"].view(1, 32) - mean.view(N, 1) * scale
        pre = z * scale.view(N, 32, 1, 1) + shift.view(N, 32, 1, 1)
    else:
        P = z.numel() // 32
        mean = z.mean(dim=(0, 2, 3))
        var = ((z - mean.view(1, 32, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        invstd = 1 / torch.sqrt(var + eps)
        scale = q["gamma"] * invstd
        shift = q["beta"] - mean * scale
        pre = z * scale.view(1, 32, 1, 1) + shift.view(1, 32, 1, 1)
        if running is not None:
            r["running_mean"] = (1 - momentum) * running[0] + momentum * mean.detach()
            r["running_var"] = (1 - momentum) * running[1] + momentum * var.detach() * P / (P - 1)
    a = act_fn(pre, act, beta)
    b = F.conv2d(a, q["u1_w"].view(2, 32, 1, 1), q["u1_b"])
    tn = (tfeat @ t_w.t() + t_b).permute(0, 3, 1, 2)
    tn = _leaf(tn)
    pf = torch.softmax(b, dim=1)[:, 1:2]
    logits = torch.cat([b[:, 0:1], b[:, 1:2] + tn * pf], dim=1)
    r.update(logits=logits.detach(), bgfg=b.detach(), tn=tn.detach(), mean=mean.detach(), invstd=invstd.detach(),
             scale=scale.detach(), shift=shift.detach(), pre=pre.detach())
    if grads is not None:
        dlogits, dbgfg, dtn = grads
        outs, gouts = [logits], [dlogits]
        if dbgfg is not None:
            outs.append(b), gouts.append(dbgfg)
        if dtn is not None:
            outs.append(tn), gouts.append(dtn)
        gs = _grads(outs, [ll, tn] + [q[n] for n in UBF_PARAMS], gouts)
        r["dlow"] = gs[0]
        r["dtn_out"] = gs[1].permute(0, 2, 3, 1).reshape(-1, 2)     # [P][2] as the kernel writes it
        for n, g in zip(UBF_PARAMS, gs[2:]):
            r["d" + n] = g + (0 if old is None else old["d" + n])
    return r


def pw2_bwd(tfeat, dtn, w, old_dw=None, old_db=None):
    """Backward of Conv2d(Ct, 2, 1): tfeat [P][Ct], dtn [P][2], w [2][Ct] -> dt [P][Ct], dw [2][Ct], db [2]."""
    dt = dtn @ w
    dw = dtn.t() @ tfeat
    db = dtn.sum(dim=0)
    return dt, dw + (0 if old_dw is None else old_dw), db + (0 if old_db is None else old_db)


# ----------------------------------------------------------------------------------------- RoIAlign into an affine
def _linspace01(S, dtype):
    if S == 1:
        return torch.zeros(1, dtype=dtype)
    step = torch.tensor(1.0, dtype=dtype) / (S - 1)
    j = torch.arange(S)
    return torch.where(j < S // 2, step * j.to(dtype), 1 - step * (S - 1 - j).to(dtype))


def roi_sample_coords(rois, oh, ow, scale_h, scale_w, H, W, aligned):
    """Unnormalised sampling coordinates (ix [N][ow], iy [N][oh]) of DynamicRoIAlign: a linspace over the scaled
    box, normalised for grid_sample and un-normalised again by it."""
    dt = rois.dtype
    x1, y1, x2, y2 = (rois[:, 1] * scale_w, rois[:, 2] * scale_h, rois[:, 3] * scale_w, rois[:, 4] * scale_h)
    fx = x1[:, None] + _linspace01(ow, dt)[None, :] * (x2 - x1)[:, None]
    fy = y1[:, None] + _linspace01(oh, dt)[None, :] * (y2 - y1)[:, None]
    if aligned:
        ix = (fx / (W - 1) * 2 - 1 + 1) * ((W - 1) / 2)
        iy = (fy / (H - 1) * 2 - 1 + 1) * ((H - 1) / 2)
    else:
        ix = (fx / W * 2 - 1 + 1) * (W / 2) - 0.5
        iy = (fy / H * 2 - 1 + 1) * (H / 2) - 0.5
    return ix, iy


def roi_align_bwd_affine(u, rois, g, oh, ow, scale_h, scale_w, aligned, old_dw=None, old_db=None):
    """u [B][1][H][W], rois [N][5] (batch, x1, y1, x2, y2), g [N][oh][ow][2] the gradient of the roi logits
    r_c = interp(w_c u + b_c): dw_c = sum g_c interp(u), db_c = sum g_c interp(1), an explicit loop over the four
    bilinear taps with taps outside the map counted as 0."""
    B, _, H, W = u.shape
    dt = u.dtype
    ix, iy = roi_sample_coords(rois, oh, ow, scale_h, scale_w, H, W, aligned)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    lx, ly = ix - x0, iy - y0
    b = rois[:, 0].long()
    vu = torch.zeros(rois.shape[0], oh, ow, dtype=dt)
    ws = torch.zeros_like(vu)
    for dy_, wy in ((0, 1 - ly), (1, ly)):
        for dx_, wx in ((0, 1 - lx), (1, lx)):
            yy = (y0.long() + dy_)[:, :, None].expand(-1, -1, ow)
            xx = (x0.long() + dx_)[:, None, :].expand(-1, oh, -1)
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            wgt = wy[:, :, None] * wx[:, None, :]
            val = u[b[:, None, None], 0, yy.clamp(0, H - 1), xx.clamp(0, W - 1)]
            zero = torch.zeros_like(wgt)
            vu = vu + torch.where(ok, wgt * val, zero)
            ws = ws + torch.where(ok, wgt, zero)
    dw = (g * vu.unsqueeze(-1)).sum(dim=(0, 1, 2))
    db = (g * ws.unsqueeze(-1)).sum(dim=(0, 1, 2))
    return dw + (0 if old_dw is None else old_dw), db + (0 if old_db is None else old_db)


# ----------------------------------------------------------------------------------------- LayerNorm2d
def layernorm2d(z, gamma, beta, eps, act, act_beta, residual=None, chan_mul=None, dy=None):
    """z [N][HW][C]: per-sample mean / biased variance over (HW, C); the folded tables scale [N][C] = gamma *
    invstd_n, shift = beta - mean_n * scale; y = act(z * scale + shift + residual) * chan_mul.
    With dy: dz, dres (the residual's gradient), dgamma, dbeta and dconv_bias = sum of dz over (N, HW)."""
    N, HW, C = z.shape
    zl, gl, bl = _leaf(z), _leaf(gamma), _leaf(beta)
    rl = None if residual is None else _leaf(residual)
    mean = zl.mean(dim=(1, 2))
    var = ((zl - mean.view(N, 1, 1)) ** 2).mean(dim=(1, 2))
    invstd = 1 / torch.sqrt(var + eps)
    scale = gl.view(1, C) * invstd.view(N, 1)
    shift = bl.view(1, C) - mean.view(N, 1) * scale
    pre = zl * scale.unsqueeze(1) + shift.unsqueeze(1)
    if rl is not None:
        pre = pre + rl
    y = act_fn(pre, act, act_beta)
    if chan_mul is not None:
        y = y * chan_mul.unsqueeze(1)
    r = {"mean": mean.detach(), "invstd": invstd.detach(), "scale": scale.detach(), "shift": shift.detach(),
         "y": y.detach()}
    if dy is not None:
        wrt = [zl, gl, bl] + ([] if rl is None else [rl])
        gs = _grads([y], wrt, [dy])
        r["dz"], r["dgamma"], r["dbeta"] = gs[0], gs[1], gs[2]
        r["dconv_bias"] = gs[0].sum(dim=(0, 1))
        if rl is not None:
            r["dres"] = gs[3]
    return r


# ----------------------------------------------------------------------------------------- Dropout2d masks
_M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def dropout2d_mask(n: int, p: float, seed: int) -> np.ndarray:
    """dropout2d_mask_kernel: element i is 0 if u_i < p else 1 / (1 - p), u_i = top 24 bits of
    splitmix64(seed ^ splitmix64(i)) / 2^24; p and the comparison in float32 as on the device."""
    p32 = np.float32(p)
    keep = np.float32(1.0) / (np.float32(1.0) - p32)
    out = np.empty(n, dtype=np.float32)
    for i in range(n):
        u = np.float32(splitmix64((seed & _M64) ^ splitmix64(i)) >> 40) * np.float32(1.0 / 16777216.0)
        out[i] = np.float32(0.0) if u < p32 else keep
    return out


def dropout2d_dev_seed(base: int, offset: int) -> int:
    """dropout2d_mask_dev_kernel's seed from the device-resident base."""
    return ((base * 0x9E3779B1 + offset) & _M64) & ((1 << 48) - 1)


def dropout2d_mask_dev(n: int, p: float, base: int, offset: int) -> np.ndarray:
    return dropout2d_mask(n, p, dropout2d_dev_seed(base, offset))
