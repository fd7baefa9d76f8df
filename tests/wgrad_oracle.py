"""A plain float64 oracle of the convolution weight gradient, its split reduction and the per-step weight packing,
written from include/hiseg_train.h (hiseg_conv2d_wgrad, hiseg_conv2d_wgrad_reduce, hiseg_pack_weights).  It never
calls the library and uses no torch convolution: tests/test_wgrad_oracle.py holds it against float64 autograd of
F.conv2d / F.conv_transpose2d, tests/test_gpu_wgrad_kernels.py holds every weight-gradient kernel, both reducers and
the packing kernel against it.

A case is a dict in the vocabulary of conv_kernel_oracle (N, Ca, Cb, Cout, H, W, k, stride, pad, a_up, convT): Ca / Cb
/ Cout are the REAL channel counts (ConvTranspose: Cout output channels, 4 Cout GEMM columns), H x W the full-resolution
input grid (source A holds H / a_up x W / a_up).  The library's K layout pads each source to the dtype's 16-byte
chunk (8 bf16 / 4 f32 channels):

    k = tap * (ca + cb) + cp,  tap = ky * KW + kx,  cp < ca: source A's channel cp (zero past ca_real), else source B's
    X[p][k] = the input the forward conv reads for output pixel p = (n, oy, ox) at that tap (zero outside the image)
    ws[s][j][k]    = sum over the pixels p of split s of dy[p][j] * X[p][k]
    ws[s][j][Ktot] = sum over the same pixels of dy[p][j]                         (want_bias)

with j the GEMM column (ConvTranspose: j = q * Cout + co, q = 2 dy + dx the sub-pixel, dy[p][j] the gradient at output
pixel (2 oy + dy, 2 ox + dx)).  Pixels are split in blocks of 64 (bf16) or 32 (f32) in flat (n, oy, ox) order, `bps`
blocks per split (wgrad_geometry, csrc/train_conv.hip); the halo tile walks 8 x 16 pixel tiles instead
(halo_partition).
"""
import numpy as np
import torch

import conv_kernel_oracle as O

CHUNK = {"f32": 4, "bf16": 8}
PIXEL_BLOCK = {"f32": 32, "bf16": 64}
PACK_FRAG, PACK_BIAS = 8, 4


def rup(x, m):
    return (x + m - 1) // m * m


def geometry(c, dt, want_bias):
    """The padded GEMM geometry of a case: include/hiseg_train.h's Cg / Kg and the K layout's channel counts."""
    c = dict(O.CASE_DEFAULTS, **c)
    ch = CHUNK[dt]
    ca, cb = rup(c["Ca"], ch), rup(c["Cb"], ch)
    kh = kw = 1 if c["convT"] else c["k"]
    cols = 4 * c["Cout"] if c["convT"] else c["Cout"]
    if c["convT"]:
        Ho, Wo = c["H"], c["W"]
    else:
        Ho = (c["H"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1
        Wo = (c["W"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1
    Ktot = kh * kw * (ca + cb)
    return dict(ca=ca, cb=cb, ca_real=c["Ca"], cb_real=c["Cb"], KH=kh, KW=kw, cols=cols, Ho=Ho, Wo=Wo,
                M=c["N"] * Ho * Wo, Ktot=Ktot, Kg=rup(Ktot + (1 if want_bias else 0), 64), Cg=rup(cols, 16),
                PB=PIXEL_BLOCK[dt], convT=bool(c["convT"]))


def im2col(c, X, dt):
    """[M][Ktot] float64: row p = (n, oy, ox), column k = tap * (ca + cb) + cp as above, from the gathered input X
    (conv_kernel_oracle.gather_input: NCHW, real channels, source A upsampled)."""
    g = geometry(c, dt, False)
    c = dict(O.CASE_DEFAULTS, **c)
    N, Cr, H, W = X.shape
    assert Cr == g["ca_real"] + g["cb_real"] and (H, W) == (c["H"], c["W"])
    if g["convT"]:
        stride, pad = 1, 0
    else:
        stride, pad = c["stride"], c["pad"]
    Ho, Wo, cin = g["Ho"], g["Wo"], g["ca"] + g["cb"]
    xp = torch.zeros(N, H + 2 * pad, W + 2 * pad, cin, dtype=torch.float64)
    xp[:, pad:pad + H, pad:pad + W, :g["ca_real"]] = X[:, :g["ca_real"]].permute(0, 2, 3, 1)
    xp[:, pad:pad + H, pad:pad + W, g["ca"]:g["ca"] + g["cb_real"]] = X[:, g["ca_real"]:].permute(0, 2, 3, 1)
    out = torch.zeros(N, Ho, Wo, g["KH"] * g["KW"], cin, dtype=torch.float64)
    for ky in range(g["KH"]):
        for kx in range(g["KW"]):
            out[:, :, :, ky * g["KW"] + kx] = xp[:, ky:ky + (Ho - 1) * stride + 1:stride,
                                                 kx:kx + (Wo - 1) * stride + 1:stride]
    return out.reshape(g["M"], g["Ktot"])


def dy_matrix(c, dy, dt):
    """[M][GEMM columns] float64 from dy NCHW (ConvTranspose: [N][Cout][2H][2W], column q * Cout + co)."""
    g = geometry(c, dt, False)
    if not g["convT"]:
        return dy.double().permute(0, 2, 3, 1).reshape(g["M"], g["cols"])
    parts = [dy.double()[:, :, q >> 1::2, q & 1::2].permute(0, 2, 3, 1) for q in range(4)]
    return torch.cat(parts, 3).reshape(g["M"], g["cols"])


def block_partition(M, PB, splits, bps):
    """Split s takes pixel blocks [s bps, (s + 1) bps) of PB pixels each."""
    parts = [torch.arange(min(s * bps * PB, M), min((s + 1) * bps * PB, M)) for s in range(splits)]
    assert sum(len(p) for p in parts) == M, "the splits do not cover the pixels"
    return parts


def halo_partition(N, H, W, splits):
    """wgrad_hwc.hip: 8 x 16 pixel tiles in (n, tile row, tile column) order, ceil(tiles / splits) tiles per split."""
    nty, ntx = (H + 7) // 8, (W + 15) // 16
    NT = N * nty * ntx
    tps = (NT + splits - 1) // splits
    pix = torch.arange(N * H * W).view(N, H, W)
    parts = []
    for s in range(splits):
        idx = []
        for t in range(s * tps, min((s + 1) * tps, NT)):
            tx, ty, n = t % ntx, (t // ntx) % nty, t // (ntx * nty)
            idx.append(pix[n, ty * 8:ty * 8 + 8, tx * 16:tx * 16 + 16].reshape(-1))
        parts.append(torch.cat(idx) if idx else torch.zeros(0, dtype=torch.long))
    assert sum(len(p) for p in parts) == N * H * W
    return parts


def partials(c, X, dy, want_bias, splits, bps, dt="bf16", compute=torch.float64, partition=None, absolute=False):
    """ws [splits][GEMM columns][Ktot + want_bias] in `compute` (float64: the reference; float32: the e32 of the error
    bound).  `partition`: the pixel indices of each split (default: block_partition)."""
    g = geometry(c, dt, want_bias)
    Xm, Ym = im2col(c, X, dt), dy_matrix(c, dy, dt)
    if want_bias:
        Xm = torch.cat([Xm, torch.ones(g["M"], 1, dtype=torch.float64)], 1)
    if absolute:
        Xm, Ym = Xm.abs(), Ym.abs()
    Xm, Ym = Xm.to(compute), Ym.to(compute)
    parts = partition if partition is not None else block_partition(g["M"], g["PB"], splits, bps)
    assert len(parts) == splits
    return torch.stack([Ym[p].t() @ Xm[p] for p in parts])


def S(c, X, dy, want_bias, dt="bf16"):
    """The same sums over absolute values, all pixels: what every partial sum of an element is bounded by."""
    return partials(c, X, dy, want_bias, 1, 1 << 30, dt, absolute=True)[0]


def reduce(ws, m, acc_into=None):
    """hiseg_conv2d_wgrad_reduce: ws [splits][>= Cout][>= Ktot + want_bias] summed over the splits and scattered into
    the reference layouts (gw, gb) -- conv [Cout][ca_real + cb_real][KH][KW], convT [ca_real][Cout / 4][2][2] with the
    bias summed over the 4 sub-pixel columns.  m: the hiseg_wgrad_map fields.  acc_into = (gw0, gb0): accumulate."""
    cin = m["ca"] + m["cb"]
    Ktot = m["KH"] * m["KW"] * cin
    tot = ws.sum(0)
    J = m["Cout"]
    if m["convT"]:
        assert m["KH"] == 1 and m["KW"] == 1 and m["cb"] == 0 and J % 4 == 0
        C = J // 4
        gw = torch.zeros(m["ca_real"], C, 2, 2, dtype=ws.dtype)
        for q in range(4):
            for co in range(C):
                gw[:, co, q >> 1, q & 1] = tot[q * C + co, :m["ca_real"]]
        gb = sum(tot[q * C:(q + 1) * C, Ktot] for q in range(4)) if m["want_bias"] else None
    else:
        cr = m["ca_real"] + m["cb_real"]
        gw = torch.zeros(J, cr, m["KH"], m["KW"], dtype=ws.dtype)
        for ky in range(m["KH"]):
            for kx in range(m["KW"]):
                base = (ky * m["KW"] + kx) * cin
                gw[:, :m["ca_real"], ky, kx] = tot[:J, base:base + m["ca_real"]]
                gw[:, m["ca_real"]:, ky, kx] = tot[:J, base + m["ca"]:base + m["ca"] + m["cb_real"]]
        gb = tot[:J, Ktot].clone() if m["want_bias"] else None
    if acc_into is not None:
        gw = gw + acc_into[0].to(ws.dtype)
        if gb is not None and acc_into[1] is not None:
            gb = gb + acc_into[1].to(ws.dtype)
    return gw, gb


def wgrad_map(c, dt, want_bias):
    g = geometry(c, dt, want_bias)
    return dict(Cout=g["cols"], KH=g["KH"], KW=g["KW"], ca=g["ca"], ca_real=g["ca_real"], cb=g["cb"],
                cb_real=g["cb_real"], convT=int(g["convT"]), Cg=g["Cg"], Kg=g["Kg"], want_bias=int(want_bias))


def _real_channel(e, cp):
    """Padded K-layout channel -> reference input channel, -1 for a pad."""
    ca, cb = e["ca"], e["cb"]
    a = np.where(cp < e["ca_real"], cp, -1)
    b = np.where(cp - ca < e["cb_real"], e["ca_real"] + cp - ca, -1)
    return np.where(cp < ca, a, b)


def pack(e):
    """hiseg_pack_weights for one table entry (a dict of hiseg_pack_entry's fields, src a float tensor in the
    reference layout): the `total` = rows * K_pad packed values as float64 (the caller rounds to the entry's dtype).

      mode 0  conv forward   P[co][tap * (ca + cb) + cp]   = W[co][ci(cp)][ky][kx]
      mode 1  conv dgrad     P[cp][tap' * cop + co]        = W[co][ci(cp)][KH - 1 - ky'][KW - 1 - kx']
      mode 2  convT forward  P[q * Cout + co][ci]          = W[ci][co][q >> 1][q & 1]
      mode 3  convT dgrad    P[ci][tap * cop + co]         = W[ci][co][tap >> 1][tap & 1]    (the 2x2 / stride 2 conv)
      BIAS    dst[i] = src[i % Cout]
      | FRAG  the same matrix in MFMA A-fragment order: [rows / 16][K channels / 64][tap][2][64 lanes][8], lane l
              holding row l & 15, channels 8 (l >> 4) .. + 7 of k-step s's 32
    everything else zero."""
    mode = e["mode"] & 7
    src = e["src"].double().reshape(-1).numpy()
    idx = np.arange(e["total"], dtype=np.int64)
    KH, KW, Cout, cinr = e["KH"], e["KW"], e["Cout"], e["Cin_real"]
    cinp = e["ca"] + e["cb"]
    if mode == PACK_BIAS:
        return torch.from_numpy(src[idx % Cout])
    if e["mode"] & PACK_FRAG:
        assert mode in (0, 1)
        kc = cinp if mode == 0 else e["cop"]
        taps, ncb = KH * KW, kc // 64
        el, lane, s = idx % 8, idx // 8 % 64, idx // 512 % 2
        tap, cb, ct = idx // 1024 % taps, idx // (1024 * taps) % ncb, idx // (1024 * taps * ncb)
        row = ct * 16 + (lane & 15)
        k = tap * kc + cb * 64 + s * 32 + (lane >> 4) * 8 + el
    else:
        row, k = idx // e["K_pad"], idx % e["K_pad"]
    out = np.zeros(e["total"])

    def put(ok, off):
        out[ok] = src[off[ok]]

    if mode == 0:
        tap, cp = k // cinp, k % cinp
        ci = _real_channel(e, cp)
        put((row < Cout) & (k < KH * KW * cinp) & (ci >= 0), (row * cinr + ci) * KH * KW + tap)
    elif mode == 1:
        cop = e["cop"]
        tap2, co = k // cop, k % cop
        ci = np.where(row < cinp, _real_channel(e, np.minimum(row, cinp - 1)), -1)
        ky, kx = KH - 1 - tap2 // KW, KW - 1 - tap2 % KW
        put((ci >= 0) & (k < KH * KW * cop) & (co < Cout), ((co * cinr + ci) * KH + ky) * KW + kx)
    elif mode == 2:
        q, co = row // Cout, row % Cout
        put((row < 4 * Cout) & (k < cinr), (k * Cout + co) * 4 + q)
    else:
        cop = e["cop"]
        tap, co = k // cop, k % cop
        put((row < cinr) & (k < 4 * cop) & (co < Cout), (row * Cout + co) * 4 + tap)
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------- inputs
def make_inputs(case, tier, dt, seed=0):
    """(case with defaults, xa, xb, dy) as float64 NCHW.  Tier A: integers in {-2..2}; tier B: normal values rounded
    to the compute dtype (dy scaled by 1 / sqrt(M))."""
    c = dict(O.CASE_DEFAULTS, **case)
    g = geometry(c, dt, False)
    gen = O.gen(2000 + seed)
    N, up = c["N"], c["a_up"]
    assert c["H"] % up == 0 and c["W"] % up == 0
    dshape = (N, c["Cout"], 2 * c["H"], 2 * c["W"]) if c["convT"] else (N, c["Cout"], g["Ho"], g["Wo"])
    if tier == "A":
        xa = O.ints(gen, N, c["Ca"], c["H"] // up, c["W"] // up)
        xb = O.ints(gen, N, c["Cb"], c["H"], c["W"]) if c["Cb"] else None
        dy = O.ints(gen, *dshape)
    else:
        xa = O.rnd(gen, dt, N, c["Ca"], c["H"] // up, c["W"] // up)
        xb = O.rnd(gen, dt, N, c["Cb"], c["H"], c["W"]) if c["Cb"] else None
        dy = O.rnd(gen, dt, *dshape, scale=g["M"] ** -0.5)
    return c, xa, xb, dy


def tier_a_bound(case, dt, want_bias):
    """From the shape alone: every partial sum of a tier A weight-gradient element is an integer of magnitude at most
    4 M (|x|, |dy| <= 2 over M pixels), 4 M for the bias column's sum of dy too (2 M), times 4 for the ConvTranspose
    bias, which the reducer sums over four columns."""
    g = geometry(case, dt, want_bias)
    return 4 * g["M"] * (4 if g["convT"] and want_bias else 1)
