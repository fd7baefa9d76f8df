"""A plain oracle of hiseg_conv2d_fwd, written from the descriptor's semantics (include/hiseg.h) on NCHW tensors.  It
never calls the library and uses no torch convolution: tests/test_conv_kernel_oracle.py holds it against
F.conv2d / F.conv_transpose2d / F.interpolate, tests/test_gpu_conv_kernels.py holds every forward conv kernel
against it.

    A   = nearest-upsample(source A, a_up); with a gate (in_scale): A = round_to_compute_dtype(fl32(A * gate[n][c]))
    X   = A ++ B along channels
    acc = sum over taps and channels X[n, c, y*stride - pad + ky, x*stride - pad + kx] * W[co, c, ky, kx]
          (ConvTranspose 2x2 / stride 2: out[n, co, 2y + dy, 2x + dx] = sum_c X[n, c, y, x] * W[c, co, dy, dx])
    v   = act(acc * scale[co] + shift[co] + residual) * mul
    out = v in the output dtype, out2 = v in the compute dtype

Every step runs in the dtype of `compute` (float64: the reference; float32: torch's own float32 evaluation, the e32
of the error bound).  S is the same pipeline over absolute values, |X| * |W| * |scale| + |shift| + |residual|: the
magnitude every partial sum of the pre-activation is bounded by, for the exactness premise of tier A and the derived
worst-case rounding bound.
"""
import torch

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_GELU, ACT_SWISH = range(6)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def act_fn(v, act, beta=1.0):
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    if act in (ACT_SILU, ACT_SWISH):
        b = beta if act == ACT_SWISH else 1.0
        return v / (1.0 + torch.exp(-b * v))
    raise ValueError(f"activation {act}")


def upsample_nearest(x, f):
    """out[..., y, x] = in[..., y // f, x // f]."""
    if f == 1:
        return x
    N, C, H, W = x.shape
    iy = torch.arange(H * f) // f
    ix = torch.arange(W * f) // f
    return x[:, :, iy][:, :, :, ix]


def gather_input(xa, xb, a_up, gate, dt):
    """The GEMM's input X (float64 values the loader reads), from source A, its gate, source B."""
    a = upsample_nearest(xa.double(), a_up)
    if gate is not None:
        g = gate.double()
        assert torch.equal(a.float().double(), a) and torch.equal(g.float().double(), g)
        a = (a.float() * g.float()[:, :, None, None]).to(DTYPES[dt]).double()   # fl32 product, then the compute dtype
    if xb is not None:
        assert xb.shape[0] == a.shape[0] and xb.shape[2:] == a.shape[2:]
        a = torch.cat([a, xb.double()], 1)
    return a


def _taps(x, w, stride, pad):
    """sum over taps and channels, one tap at a time (x [N, C, H, W], w [Co, C, KH, KW]) in x's dtype."""
    N, C, H, W = x.shape
    Co, Cw, KH, KW = w.shape
    assert Cw == C
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    xp = torch.zeros(N, C, H + 2 * pad, W + 2 * pad, dtype=x.dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    acc = torch.zeros(N, Co, Ho, Wo, dtype=x.dtype)
    for ky in range(KH):
        for kx in range(KW):
            win = xp[:, :, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            acc += torch.einsum("nchw,oc->nohw", win, w[:, :, ky, kx])
    return acc


def _gemm(x, w, stride, pad, convT):
    if not convT:
        return _taps(x, w, stride, pad)
    N, C, H, W = x.shape
    Cw, Co, KH, KW = w.shape
    assert Cw == C and KH == 2 and KW == 2 and stride == 1 and pad == 0
    out = torch.zeros(N, Co, 2 * H, 2 * W, dtype=x.dtype)
    for dy in range(2):
        for dx in range(2):
            out[:, :, dy::2, dx::2] = torch.einsum("nchw,co->nohw", x, w[:, :, dy, dx])   # 1x1 GEMM + pixel shuffle
    return out


def conv(xa, w, scale, shift, *, xb=None, a_up=1, gate=None, stride=1, pad=0, residual=None, act=ACT_NONE, beta=1.0,
         mul=None, convT=False, dt="bf16", out_dt=None, compute=torch.float64):
    """The whole operation.  Inputs are float64 tensors holding values of the compute dtype `dt` (scale / shift / gate:
    float32 values).  Returns a dict: `v` the result in `compute`, `pre` the pre-activation, `S` the absolute-value
    pipeline, `out` / `out2` the result rounded (by torch, to nearest even) to the output / compute dtype."""
    out_dt = out_dt or dt
    X = gather_input(xa, xb, a_up, gate, dt)
    c = lambda t: None if t is None else t.double().to(compute)
    bc = lambda t: c(t)[None, :, None, None]
    acc = _gemm(c(X), c(w), stride, pad, convT)
    pre = acc * bc(scale) + bc(shift)
    S = _gemm(X.abs(), w.double().abs(), stride, pad, convT) * scale.double().abs()[None, :, None, None] \
        + shift.double().abs()[None, :, None, None]
    if residual is not None:
        assert residual.shape == pre.shape
        pre = pre + c(residual)
        S = S + residual.double().abs()
    v = act_fn(pre, act, beta)
    if mul is not None:
        v = v * c(mul)
    return {"v": v, "pre": pre, "S": S, "X": X,
            "out": v.float().to(DTYPES[out_dt]), "out2": v.float().to(DTYPES[dt])}


# ------------------------------------------------------------------------------------------- inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, *shape, lo=-2, hi=2):
    """iid integers in {lo..hi} as float64."""
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def pick(g, values, *shape):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def rnd(g, dt, *shape, scale=1.0):
    """float64 normal values exactly representable in the compute dtype."""
    return (scale * torch.randn(*shape, generator=g, dtype=torch.float64)).to(DTYPES[dt]).double()


TIER_A_SCALES = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
TIER_A_GATES = (0.5, 1.0, 2.0)


def make_inputs(case, tier, dt, seed=0):
    """The tensors of a case (a dict, see CASE_DEFAULTS) as float64 NCHW.

    Tier A: activations, weights, residual, mul iid integers in {-2..2}, shift integers in {-3..3}, scale from
    {+-0.5, +-1, +-2}, gates from {0.5, 1, 2}.  Every term is a multiple of 1/4 (a gate of 1/2 times a scale of 1/2)
    bounded by S, and so is every partial sum in any order: S < 2^22 makes all of them exactly representable in
    float32 (and in an FMA's or an MFMA's wider intermediate), so a correct kernel returns the exact value whatever its
    summation order, tile shape or K split.  A gated bf16 source holds |x| * gate <= 4, exact in bf16.  S <= 16 K + 5
    by construction (K = taps x channels <= 2^17 in every case here), never a matter of the seed.
    Tier B: normal values rounded to the compute dtype, weights scaled by 1 / sqrt(K), gates k / 128 with k in 64..255
    (8 significant bits: fl32(x * gate) is exact for a bf16 x, so its rounding to bf16 is unambiguous)."""
    c = dict(CASE_DEFAULTS, **case)
    g = gen(1000 + seed)
    N, Ca, Cb, Cout, H, W, k = c["N"], c["Ca"], c["Cb"], c["Cout"], c["H"], c["W"], c["k"]
    up = c["a_up"]
    assert H % up == 0 and W % up == 0
    if c["convT"]:
        oH, oW, K = 2 * H, 2 * W, Ca
        wshape = (Ca, Cout, 2, 2)
    else:
        oH = (H + 2 * c["pad"] - k) // c["stride"] + 1
        oW = (W + 2 * c["pad"] - k) // c["stride"] + 1
        K = k * k * (Ca + Cb)
        wshape = (Cout, Ca + Cb, k, k)
    t = {}
    if tier == "A":
        assert c["act"] in (ACT_NONE, ACT_RELU) and K <= 2 ** 17
        t["xa"] = ints(g, N, Ca, H // up, W // up)
        t["xb"] = ints(g, N, Cb, H, W) if Cb else None
        t["w"] = ints(g, *wshape)
        t["scale"] = pick(g, TIER_A_SCALES, Cout)
        t["shift"] = ints(g, Cout, lo=-3, hi=3)
        t["gate"] = pick(g, TIER_A_GATES, N, Ca) if c["gate"] else None
        t["residual"] = ints(g, N, Cout, oH, oW) if c["residual"] else None
        t["mul"] = ints(g, N, Cout, oH, oW) if c["mul"] else None
    else:
        t["xa"] = rnd(g, dt, N, Ca, H // up, W // up)
        t["xb"] = rnd(g, dt, N, Cb, H, W) if Cb else None
        t["w"] = rnd(g, dt, *wshape, scale=K ** -0.5)
        t["scale"] = (0.5 + torch.rand(Cout, generator=g, dtype=torch.float64)).float().double()
        t["shift"] = (0.2 * torch.randn(Cout, generator=g, dtype=torch.float64)).float().double()
        t["gate"] = torch.randint(64, 256, (N, Ca), generator=g).double() / 128 if c["gate"] else None
        t["residual"] = rnd(g, dt, N, Cout, oH, oW) if c["residual"] else None
        t["mul"] = rnd(g, dt, N, Cout, oH, oW) if c["mul"] else None
    return c, t


def run(c, t, dt, out_dt=None, compute=torch.float64):
    return conv(t["xa"], t["w"], t["scale"], t["shift"], xb=t["xb"], a_up=c["a_up"], gate=t["gate"],
                stride=c["stride"], pad=c["pad"], residual=t["residual"], act=c["act"], beta=c["beta"], mul=t["mul"],
                convT=c["convT"], dt=dt, out_dt=out_dt, compute=compute)


CASE_DEFAULTS = dict(N=2, Cb=0, k=3, stride=1, pad=1, a_up=1, gate=False, residual=False, mul=False, out2=False,
                     act=ACT_NONE, beta=1.0, convT=False, a_view=None, out_view=None, f32_out=False, split_k_3x3=False)
