"""Plain torch restatements of the inference non-convolution kernels of csrc/misc.hip, one function per kernel.

Every function is dtype-generic: it computes in the dtype of its floating inputs.  The GPU tests call each one twice
on the same inputs (already rounded to the kernel's compute dtype): once in float64 -- the reference -- and once in
float32, whose element-wise distance from the float64 result (`e32`) is the yardstick of the bounds.  Activations are
NHWC as the kernels take them.  Where order or tie-breaking decides the result (window maxima, first argmax, the
sign of a zero maximum) it is spelled out; sums are plain sums.

Functions whose kernel goes through the fast exp / sigmoid intrinsics also return the argument of that intrinsic
(`arg`, or the pre-activations), from which the GPU tests derive the extra error term.
"""
import torch

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
    if act == ACT_SWISH:
        return v * torch.sigmoid(beta * v)
    raise ValueError(act)


# ------------------------------------------------------------------------------------------- pool, attention
def maxpool2x2(x):
    """MaxPool2d(2) on [N, H, W, C]: an odd last row / column is dropped."""
    Ho, Wo = x.shape[1] // 2, x.shape[2] // 2
    x = x[:, :2 * Ho, :2 * Wo]
    top = torch.maximum(x[:, 0::2, 0::2], x[:, 0::2, 1::2])
    bot = torch.maximum(x[:, 1::2, 0::2], x[:, 1::2, 1::2])
    return torch.maximum(top, bot)


def attn_map(x, w):
    """SpatialAttentionModule's map of x [N, H, W, C] with the [2][k][k] kernel w (zero padding k // 2, no bias):
    the per-pixel channel mean and max, the conv's sum `arg`, and att = sigmoid(arg)."""
    N, H, W, C = x.shape
    k = w.shape[-1]
    r = k // 2
    mean, mx = x.sum(-1) / C, x.max(-1).values
    pad = torch.zeros(N, 2, H + 2 * r, W + 2 * r, dtype=x.dtype)
    pad[:, 0, r:r + H, r:r + W], pad[:, 1, r:r + H, r:r + W] = mean, mx
    arg = torch.zeros(N, H, W, dtype=x.dtype)
    for c in range(2):
        for ky in range(k):
            for kx in range(k):
                arg = arg + w[c, ky, kx] * pad[:, c, ky:ky + H, kx:kx + W]
    return {"mean": mean, "max": mx, "arg": arg, "att": torch.sigmoid(arg)}


def pixel_scale(x, att):
    """x [..., C] times the per-pixel att [...]."""
    return x * att.unsqueeze(-1)


def attn_spatial(x, w):
    r = attn_map(x, w)
    r["out"] = pixel_scale(x, r["att"])
    return r


# ------------------------------------------------------------------------------------------- SqueezeExcite
def gap_partials(x, splits):
    """Per-split channel sums of x [N, HW, C]: split s takes pixels [HW s / splits, HW (s + 1) / splits)."""
    N, HW, C = x.shape
    out = torch.zeros(N, splits, C, dtype=x.dtype)
    for s in range(splits):
        out[:, s] = x[:, HW * s // splits:HW * (s + 1) // splits].sum(1)
    return out


def se_gate(partial, HW, w1, b1, w2, b2, act, beta=1.0):
    """gate = sigmoid(W2 act(W1 mean + b1) + b2) from the pool partials [N, splits, C]; z1 / z2 are the two
    pre-activations."""
    mean = partial.sum(1) / HW
    z1 = mean @ w1.t()
    if b1 is not None:
        z1 = z1 + b1
    hid = act_fn(z1, act, beta)
    z2 = hid @ w2.t()
    if b2 is not None:
        z2 = z2 + b2
    return {"mean": mean, "z1": z1, "hid": hid, "z2": z2, "gate": torch.sigmoid(z2)}


def channel_scale(x, gate):
    """x [N, HW, C] times gate [N, C]."""
    return x * gate.unsqueeze(1)


# ------------------------------------------------------------------------------------------- input prologue
def image_max_bits(x):
    """The maximum of a float32 tensor as its bit pattern (int), with -0.0 below +0.0: the maximum of the
    order-preserving integer key of every element (IEEE totalOrder on non-NaN values)."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    return key_to_bits(int(key.max()))


def key_to_bits(k):
    """The float32 bit pattern of an order-preserving key: hiseg_image_max_fwd leaves the key, not the float, in its
    buffer (hiseg_input_norm_fwd decodes it)."""
    return k - 0x80000000 if k >= 0x80000000 else 0xFFFFFFFF - k


def input_norm(x, mean, std, cpad):
    """normalize_input of x [B, C, H, W]: x / 255 when max(x) > 1, then (x - mean_c) / std_c, as NHWC with the
    channels zero-padded to cpad."""
    B, C, H, W = x.shape
    v = x / 255.0 if bool(x.max() > 1.0) else x
    v = (v - mean.view(1, C, 1, 1)) / std.view(1, C, 1, 1)
    out = torch.zeros(B, H, W, cpad, dtype=x.dtype)
    out[..., :C] = v.permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------- hierarchical head
def conv_transpose_2x2(low, ut_w):
    """ConvTranspose2d(2, 32, 2, stride 2) without bias: low [N, h, w, 2], ut_w [ci][co][dy][dx] -> [N, 32, 2h, 2w].
    Output pixel (Y, X) has the single parent (Y // 2, X // 2) and the tap (Y % 2, X % 2)."""
    N, h, w, _ = low.shape
    lo = low.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)   # [N, 2h, 2w, 2]
    tap = ut_w.repeat(1, 1, h, w)                                       # [2, 32, 2h, 2w]: [.., Y, X] = ut_w[.., Y%2, X%2]
    return lo[..., 0].unsqueeze(1) * tap[0].unsqueeze(0) + lo[..., 1].unsqueeze(1) * tap[1].unsqueeze(0)


def hier_combine(low, tfeat, tn2, ut_w, ut_scale, ut_shift, ut_act, ut_beta, u1_w, u1_b, t_w, t_b):
    """The head's combine at mask resolution.  ut_scale / ut_shift are [32] (shared) or [N][32] (per sample);
    the target pair comes from tfeat [N, 2h, 2w, Ct] through t_w [2][Ct] / t_b, or directly as tn2 [N, 2h, 2w, 2].
    Returns logits [N, 3, 2h, 2w], bgfg and tn [N, 2, 2h, 2w], and pre (the activation's argument), d = b0 - b1."""
    z = conv_transpose_2x2(low, ut_w)
    pre = z * ut_scale.reshape(-1, 32, 1, 1) + ut_shift.reshape(-1, 32, 1, 1)
    hs = act_fn(pre, ut_act, ut_beta)
    b = u1_b.view(1, 2, 1, 1) + torch.einsum("kc,nchw->nkhw", u1_w, hs)
    if tn2 is not None:
        t = tn2.permute(0, 3, 1, 2)
    else:
        t = t_b.view(1, 2, 1, 1) + torch.einsum("nhwc,kc->nkhw", tfeat, t_w)
    b0, b1 = b[:, 0], b[:, 1]
    mx = torch.maximum(b0, b1)
    e0, e1 = torch.exp(b0 - mx), torch.exp(b1 - mx)
    pfg = e1 / (e0 + e1)
    logits = torch.stack([b0, b1 + t[:, 0] * pfg, b1 + t[:, 1] * pfg], dim=1)
    return {"logits": logits, "bgfg": b, "tn": t.contiguous(), "pfg": pfg, "pre": pre, "hs": hs, "d": b0 - b1}


def ubf_ln_tables(low, ut_w, ut_b, gamma, beta, eps, fold_bias):
    """LayerNorm2d statistics of z = ConvTranspose(low) (+ ut_b) over (32, 2h, 2w) per sample, and the folded
    tables act(z * scale + shift); with fold_bias the tables apply to the bias-free ConvTranspose sum."""
    z = conv_transpose_2x2(low, ut_w)
    if ut_b is not None:
        z = z + ut_b.view(1, 32, 1, 1)
    N = z.shape[0]
    M = z[0].numel()
    mean = z.reshape(N, -1).sum(1) / M
    var = ((z - mean.view(N, 1, 1, 1)) ** 2).reshape(N, -1).sum(1) / M
    invstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones(32, dtype=low.dtype) if gamma is None else gamma
    bt = torch.zeros(32, dtype=low.dtype) if beta is None else beta
    scale = g.view(1, 32) * invstd.view(N, 1)
    m = mean.view(N, 1).expand(N, 32)
    if fold_bias and ut_b is not None:
        m = m - ut_b.view(1, 32)
    return {"mean": mean, "invstd": invstd, "scale": scale, "shift": bt.view(1, 32) - m * scale}


# ------------------------------------------------------------------------------------------- layout
def nchw_to_nhwc(x, cpad):
    N, C, H, W = x.shape
    out = torch.zeros(N, H, W, cpad, dtype=x.dtype)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out


def nhwc_to_nchw(buf, C, coff):
    """Channels [coff, coff + C) of buf [N, H, W, cstride] as [N, C, H, W]."""
    return buf[..., coff:coff + C].permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------- export masks
def softmax3_p1(logits):
    mx = torch.maximum(logits[:, 0], torch.maximum(logits[:, 1], logits[:, 2]))
    e = torch.exp(logits - mx.unsqueeze(1))
    return e[:, 1] / (e[:, 0] + e[:, 1] + e[:, 2])


def instance_masks(logits, dilation):
    """(argmax_c logits == 1) of logits [N, 3, mh, mw] after MaskDilationModule: the target logit gains 2 where the
    maximum of the target probability over the clipped (2 d + 1)^2 window exceeds the pixel's own by more than 0.1.
    argmax takes the first maximum.  margin = (window max - p1) - 0.1 and gap = the distance between the two largest
    logits after the bump are returned for the input checks."""
    N, _, mh, mw = logits.shape
    l0, l1, l2 = logits[:, 0], logits[:, 1], logits[:, 2]
    margin = None
    if dilation > 0:
        p1 = softmax3_p1(logits)
        win = torch.full_like(p1, -float("inf"))
        for dy in range(-dilation, dilation + 1):
            for dx in range(-dilation, dilation + 1):
                ys, ye = max(0, -dy), min(mh, mh - dy)
                xs, xe = max(0, -dx), min(mw, mw - dx)
                if ys >= ye or xs >= xe:
                    continue
                win[:, ys:ye, xs:xe] = torch.maximum(win[:, ys:ye, xs:xe], p1[:, ys + dy:ye + dy, xs + dx:xe + dx])
        margin = (win - p1) - 0.1
        l1 = torch.where(margin > 0, l1 + 2.0, l1)
    cls = torch.zeros_like(l0, dtype=torch.int64)
    best = l0
    cls = torch.where(l1 > best, torch.ones_like(cls), cls)
    best = torch.maximum(best, l1)
    cls = torch.where(l2 > best, torch.full_like(cls, 2), cls)
    s = torch.sort(torch.stack([l0, l1, l2], 1), dim=1, descending=True).values
    return {"inst": (cls == 1).to(logits.dtype).unsqueeze(1), "margin": margin, "gap": s[:, 0] - s[:, 1]}


def output_conv(u, w, b):
    """The UNet head's 1 -> 2 1x1 conv: u [B, H, W] -> [B, 2, H, W]."""
    return torch.stack([w[0] * u + b[0], w[1] * u + b[1]], dim=1)


def binary_masks(u, w, b):
    """softmax(output_conv(u))[:, 0] of u [...]; d = a0 - a1 is the softmax's argument."""
    a0, a1 = w[0] * u + b[0], w[1] * u + b[1]
    m = torch.maximum(a0, a1)
    e0, e1 = torch.exp(a0 - m), torch.exp(a1 - m)
    return {"binary": e0 / (e0 + e1), "d": a0 - a1}


def distance_mask(x, thr):
    arg = (x - thr) * 10.0
    return {"arg": arg, "mask": torch.sigmoid(arg)}


def resize_bilinear(x, Ho, Wo):
    """F.interpolate(mode='bilinear', align_corners=False) of x [NC, H, W]: source coordinate
    (o + 0.5) in / out - 0.5 clamped at 0, the +1 neighbour clamped at the last row / column."""
    NC, H, W = x.shape

    def axis(n_in, n_out):
        o = torch.arange(n_out, dtype=x.dtype)
        s = ((o + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
        i0 = s.floor().long().clamp_max(n_in - 1)
        i1 = (i0 + 1).clamp_max(n_in - 1)
        return i0, i1, s - i0.to(x.dtype)

    y0, y1, ly = axis(H, Ho)
    x0, x1, lx = axis(W, Wo)
    ly, lx = ly.view(1, Ho, 1), lx.view(1, 1, Wo)
    r0, r1 = x[:, y0], x[:, y1]
    top = (1 - lx) * r0[:, :, x0] + lx * r0[:, :, x1]
    bot = (1 - lx) * r1[:, :, x0] + lx * r1[:, :, x1]
    return (1 - ly) * top + ly * bot


# ------------------------------------------------------------------------------------------- constructed inputs
# Inputs whose float64 result sits away from every decision the kernels take, so that exact comparisons need no
# exclusions.  tests/test_infer_kernel_oracle.py asserts the stated properties of every case listed here.
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}

# (N, mh, mw, dilation): 286 pixels span two blocks; the 2x5 mask is smaller than the dilation-3 window
INSTANCE_CASES = [(2, 13, 11, 0), (2, 13, 11, 1), (2, 13, 11, 2), (1, 2, 5, 3)]
INSTANCE_MARGIN = 1e-3


def instance_logits(N, mh, mw, dilation):
    """float32-exact logits, redrawn until every pixel's dilation margin and top-two logit gap are at least
    INSTANCE_MARGIN from their decisions in float64 and (dilation > 0) both outcomes of the dilation rule occur."""
    for seed in range(1000):
        g = torch.Generator().manual_seed(7000 + 131 * dilation + seed)
        lg = (2.0 * torch.randn(N, 3, mh, mw, generator=g, dtype=torch.float64)).float().double()
        r = instance_masks(lg, dilation)
        if r["gap"].min() < INSTANCE_MARGIN:
            continue
        if dilation > 0 and (r["margin"].abs().min() < INSTANCE_MARGIN or not (r["margin"] > 0).any()
                             or not (r["margin"] < 0).any()):
            continue
        return lg
    raise AssertionError("no admissible instance-mask input")


def instance_tie_logits():
    """The dilation-0 input with two exact ties set by hand: pixel (0, 0, 0) has l0 == l1 > l2 (class 0), pixel
    (0, 0, 1) has l1 == l2 > l0 (class 1)."""
    lg = instance_logits(2, 13, 11, 0).clone()
    lg[0, :, 0, 0] = torch.tensor([1.5, 1.5, -0.25], dtype=torch.float64)
    lg[0, :, 0, 1] = torch.tensor([-0.5, 0.75, 0.75], dtype=torch.float64)
    return lg


# name: (N, HW, C, Cr, act, beta, bias); C is a multiple of 8 so that both dtypes take every case
SE_RELU_MARGIN = 2.0 ** -6
SE_CASES = {
    "wide_pool":   (3, 33, 1024, 10, ACT_RELU, 1.0, False),    # f32: nch = 256, the one-thread-per-chunk pool
    "nch10":       (3, 70, 40, 6, ACT_SILU, 1.0, True),        # f32: nch = 10, 256 % nch != 0; two even splits
    "nch10_b":     (3, 70, 80, 6, ACT_RELU, 1.0, True),        # bf16: nch = 10
    "tail40":      (3, 31, 104, 10, ACT_RELU, 1.0, True),      # last channel block 40 wide; one split, 31 pixels
    "one_pixel":   (3, 1, 104, 6, ACT_SWISH, 1.5, False),
    "splits64":    (3, 2100, 104, 260, ACT_RELU, 1.0, False),  # 64 splits; Cr > 256 threads; Cr % 4 == 0
    "splits64_s":  (2, 2100, 128, 16, ACT_SILU, 1.0, True),    # full 64-wide blocks, vector W1 / W2 paths
    "no_fit":      (3, 16, 72, 18, ACT_RELU, 1.0, False),      # Cr > splits x (last block's 8 columns): three launches
}


# hiseg_se_gate_partials_fwd is called with the oracle's own per-split sums: splits -> case (HW = 4 splits + 3)
SE_PARTIAL_CASES = {
    "part1":   (3, 7, 104, 10, ACT_RELU, 1.0, True),
    "part37":  (3, 151, 104, 10, ACT_SILU, 1.0, False),
    "part130": (3, 523, 104, 10, ACT_RELU, 1.0, False),
    "part512": (3, 2051, 104, 10, ACT_RELU, 1.0, True),
}
SE_PARTIAL_SPLITS = {"part1": 1, "part37": 37, "part130": 130, "part512": 512}


def se_inputs(name, dt):
    """x [N, HW, C] (rounded to dt), w1, b1, w2, b2 (float32-exact), redrawn until in float64 every hidden unit is at
    least SE_RELU_MARGIN from zero, every image has a live and a dead unit, and both sigmoid arguments stay
    within +-16.  Images have means of different size and sign, so their hidden patterns differ."""
    N, HW, C, Cr, act, beta, bias = {**SE_CASES, **SE_PARTIAL_CASES}[name]
    for seed in range(200):
        g = torch.Generator().manual_seed(9000 + seed)
        off = torch.tensor([1.0, -0.8, 1.4])[:N].double().view(N, 1, 1)
        x = (off + torch.randn(N, HW, C, generator=g, dtype=torch.float64)).to(DTYPES[dt]).double()
        sign = torch.where(torch.rand(Cr, generator=g) < 0.5, -1.0, 1.0).double()
        sign[0], sign[Cr - 1] = 1.0, -1.0
        amp = 0.5 + 2.5 * torch.rand(Cr, generator=g, dtype=torch.float64)
        w1 = (sign * amp).view(Cr, 1) * (0.5 + torch.randn(Cr, C, generator=g, dtype=torch.float64).abs()) / C
        w2 = 1.5 * torch.randn(C, Cr, generator=g, dtype=torch.float64) / Cr ** 0.5
        b1 = 0.1 * torch.randn(Cr, generator=g, dtype=torch.float64) if bias else None
        b2 = 0.5 * torch.randn(C, generator=g, dtype=torch.float64) if bias else None
        w1, w2 = w1.float().double(), w2.float().double()
        b1 = None if b1 is None else b1.float().double()
        b2 = None if b2 is None else b2.float().double()
        r = se_gate(gap_partials(x, 1), HW, w1, b1, w2, b2, act, beta)
        if se_inputs_ok(r, beta):
            return x, w1, b1, w2, b2
    raise AssertionError(f"no admissible SqueezeExcite input for {name}")


def se_inputs_ok(r, beta):
    z1 = r["z1"]
    return bool(z1.abs().min() >= SE_RELU_MARGIN and (z1 > 0).any(1).all() and (z1 < 0).any(1).all()
                and (beta * z1).abs().max() <= 16 and r["z2"].abs().max() <= 16)
