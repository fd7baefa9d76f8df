"""Tensor-level wrappers over the libhiseg C ABI.

Activations live in HBM as NHWC tensors whose channel dimension is padded to whole 16-byte
chunks (8 bf16 / 4 f32).  An :class:`Act` is a view (tensor, grid, real channels, channel
stride, channel offset) so that concatenations are produced in place: a producer writes its
channels at an offset of the consumer's buffer and no concat copy is ever made.

Every function launches on ``torch.cuda.current_stream()`` and requires CUDA (HIP) tensors:
there is no CPU fallback in the product path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as L

_TORCH_TO_HISEG = {torch.float32: L.HISEG_F32, torch.bfloat16: L.HISEG_BF16}


def chunk_elems(dtype: torch.dtype) -> int:
    return 8 if dtype == torch.bfloat16 else 4


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def hdtype(dtype: torch.dtype) -> int:
    try:
        return _TORCH_TO_HISEG[dtype]
    except KeyError:
        raise TypeError(f"hiseg supports float32 and bfloat16 activations, got {dtype}") from None


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _require_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("hiseg kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")


@dataclass
class Act:
    """NHWC activation view: element (n, y, x, c) at t[((n*H + y)*W + x)*cstride + coff + c]."""
    t: torch.Tensor
    N: int
    H: int
    W: int
    C: int
    cstride: int
    coff: int = 0

    @staticmethod
    def new(N, H, W, C, dtype, device, cpad=None, zero=None) -> "Act":
        ce = chunk_elems(dtype)
        cs = round_up(C, ce) if cpad is None else cpad
        if zero is None:
            zero = cs != C
        alloc = torch.zeros if zero else torch.empty
        t = alloc(N * H * W * cs, dtype=dtype, device=device)
        return Act(t, N, H, W, C, cs, 0)

    def slice(self, coff: int, C: int) -> "Act":
        return Act(self.t, self.N, self.H, self.W, C, self.cstride, self.coff + coff)

    @property
    def dtype(self):
        return self.t.dtype

    @property
    def cpad(self) -> int:
        return round_up(self.C, chunk_elems(self.t.dtype))

    def ptr(self) -> int:
        return self.t.data_ptr()

    def to_nchw(self) -> torch.Tensor:
        out = torch.empty(self.N, self.C, self.H, self.W, dtype=torch.float32, device=self.t.device)
        L.check(L.lib().hiseg_nhwc_to_nchw_fwd(hdtype(self.dtype), self.ptr(), self.N, self.H, self.W, self.C,
                                               self.cstride, self.coff, out.data_ptr(), L.stream_ptr()),
                "nhwc_to_nchw")
        return out

    @staticmethod
    def from_nchw(x: torch.Tensor, dtype: torch.dtype) -> "Act":
        _require_gpu(x)
        x = x.contiguous().float()
        N, C, H, W = x.shape
        a = Act.new(N, H, W, C, dtype, x.device, zero=False)
        L.check(L.lib().hiseg_nchw_to_nhwc_fwd(hdtype(dtype), x.data_ptr(), N, C, H, W, a.ptr(), a.cstride,
                                               L.stream_ptr()), "nchw_to_nhwc")
        return a


# ---------------------------------------------------------------------------------------- RoIAlign
def roi_align(feat: torch.Tensor, rois: torch.Tensor, oh: int, ow: int, scale_h: float, scale_w: float,
              aligned: bool, out: Optional[Act] = None, aff_w: Optional[torch.Tensor] = None,
              aff_b: Optional[torch.Tensor] = None, nchw_out: Optional[torch.Tensor] = None,
              zero_to: int = 0) -> None:
    """DynamicRoIAlign.forward (dynamic_roi_align.py:56-171) into an NHWC Act or an NCHW f32 tensor."""
    _require_gpu(feat, rois)
    assert feat.dtype == torch.float32 and feat.is_contiguous() and feat.dim() == 4
    rois = rois.contiguous().float()
    assert rois.dim() == 2 and rois.shape[1] == 5
    B, C, H, W = feat.shape
    d = L.RoiAlignDesc()
    d.feat, d.B, d.C, d.H, d.W = feat, B, C, H, W
    d.rois, d.N = rois, rois.shape[0]
    d.oh, d.ow = int(oh), int(ow)
    d.scale_h, d.scale_w = float(scale_h), float(scale_w)
    d.aligned = int(bool(aligned))
    if aff_w is not None:
        d.aff_w, d.aff_b, d.n_aff = aff_w, (aff_b), aff_w.numel()
    if nchw_out is not None:
        assert nchw_out.dtype == torch.float32 and nchw_out.is_contiguous()
        d.out, d.out_dtype, d.o_nchw = nchw_out, L.HISEG_F32, 1
        d.o_cstride = 1
    else:
        d.out, d.out_dtype, d.o_cstride, d.o_coff = out, hdtype(out.dtype), out.cstride, out.coff
        d.zero_to = zero_to
    L.check(L.lib().hiseg_roi_align_fwd(ctypes.byref(d), L.stream_ptr()), "roi_align")


# ---------------------------------------------------------------------------------------- conv
class LaunchProbe:
    """Optional per-launch HIP-event timing of selected conv launches (used by bench.py's roofline).

    ``select(desc) -> key or None`` picks launches; events are recorded on the launch stream.
    """

    def __init__(self, select):
        self.select = select
        self.events = []  # (key, start, end, flops)

    def around(self, key, flops, launch):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        st = launch()
        e.record()
        self.events.append((key, s, e, flops))
        return st

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for key, s, e, fl in self.events:
            d = out.setdefault(key, {"launches": 0, "ms": 0.0, "flops": fl})
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
        for d in out.values():
            d["avg_ms"] = d["ms"] / d["launches"]
        return out


PROBE: Optional[LaunchProbe] = None
# Serving-schedule hook (hiseg.model.StreamPipelinedExport(gate=True)): ``GATE.before()`` / ``GATE.after()`` run on the
# host around every conv launch of at least ``GATE.min_flops``, on the launching stream.
GATE = None
# Developer hook (tools/layer_profile.py): when a list, every conv launch appends
# (descriptor copy, tensors kept alive, flops).
RECORD: Optional[list] = None


@dataclass
class ConvPlan:
    """A conv (or ConvTranspose 2x2/s2) layer packed for hiseg_conv2d_fwd."""
    weight: torch.Tensor  # [Cout_pad, K_pad]
    scale: torch.Tensor   # f32 [Cout_pad]
    shift: torch.Tensor   # f32 [Cout_pad]
    kh: int
    kw: int
    stride: int
    pad: int
    ca: int               # padded channels read from source A
    cb: int               # padded channels read from source B
    cout: int             # real output channels (per output pixel)
    gemm_cols: int        # = cout, or 4*cout for convT
    cout_pad: int
    k_pad: int
    act: int
    convT: bool = False
    weight_frag: Optional[torch.Tensor] = None  # MFMA-fragment order (3x3 halo kernel), bf16 only


def pack_conv(weight: torch.Tensor, bias: Optional[torch.Tensor], bn: Optional[torch.nn.BatchNorm2d], act: int,
              dtype: torch.dtype, device, stride: int = 1, pad: int = 0, split=None) -> ConvPlan:
    """Pack an nn.Conv2d weight [Cout, Cin, kh, kw] (+ eval BN + bias) for the implicit GEMM.

    ``split`` = (ca_real, cb_real) partitions the input channels into the two loader sources
    (each padded to whole chunks); default: all channels from source A.  A third entry pads source B's
    channels further (zero weights) to that count -- a skip feature stored with a 64-multiple channel
    stride so the decoder conv takes the halo-tiled kernels (engine.effunet_forward).
    """
    ce = chunk_elems(dtype)
    w = weight.detach().float()
    cout, cin, kh, kw = w.shape
    ca_r, cb_r = split[:2] if split is not None else (cin, 0)
    assert ca_r + cb_r == cin
    ca, cb = round_up(ca_r, ce), round_up(cb_r, ce)
    if split is not None and len(split) > 2:
        cb = max(cb, int(split[2]))
    wk = torch.zeros(cout, kh, kw, ca + cb, dtype=torch.float32, device=w.device)
    wt = w.permute(0, 2, 3, 1)
    wk[..., :ca_r] = wt[..., :ca_r]
    if cb_r:
        wk[..., ca:ca + cb_r] = wt[..., ca_r:]
    k = kh * kw * (ca + cb)
    k_pad = round_up(k, 64)
    cout_pad = round_up(cout, 16)
    wp = torch.zeros(cout_pad, k_pad, dtype=torch.float32, device=w.device)
    wp[:cout, :k] = wk.reshape(cout, k)
    scale, shift = fold_affine(cout, bias, bn, w.device)
    sc = torch.zeros(cout_pad, dtype=torch.float32, device=w.device)
    sh = torch.zeros(cout_pad, dtype=torch.float32, device=w.device)
    sc[:cout], sh[:cout] = scale, shift
    frag = None
    if dtype == torch.bfloat16 and kh == 3 and kw == 3 and stride == 1 and ca % 64 == 0 and cb % 64 == 0 and k == k_pad:
        frag = frag_pack(wp, kh * kw, ca + cb).to(device=device, dtype=dtype).contiguous()
    return ConvPlan(wp.to(device=device, dtype=dtype).contiguous(), sc.to(device), sh.to(device), kh, kw, stride, pad,
                    ca, cb, cout, cout, cout_pad, k_pad, act, weight_frag=frag)


def frag_pack(wp: torch.Tensor, taps: int, cin: int) -> torch.Tensor:
    """[Cout_pad][taps*cin] -> MFMA A-fragment order [Cout_pad/16][cb][tap][s][lane(64)][8].

    K blocks run channel-block-major, tap-minor (the halo kernel's loop order); inside a K block,
    k-step s covers channels 32s..32s+31 and lane l holds row l&15, channels 8(l>>4)..+7
    (v_mfma_f32_16x16x32_bf16 A-operand map, cdna_hip_programming.md §3).
    """
    cp = wp.shape[0]
    v = wp.reshape(cp // 16, 16, taps, cin // 64, 2, 4, 8)      # ct, row, tap, cb, s, lg, e
    v = v.permute(0, 3, 2, 4, 5, 1, 6)                           # ct, cb, tap, s, lg, row, e
    return v.reshape(-1)


def pack_convT2x2(weight: torch.Tensor, bias: Optional[torch.Tensor], bn, act: int, dtype, device) -> ConvPlan:
    """Pack nn.ConvTranspose2d(k=2, s=2) weight [Cin, Cout, 2, 2] as a 1x1 GEMM with 4*Cout columns."""
    ce = chunk_elems(dtype)
    w = weight.detach().float()
    cin, cout, kh, kw = w.shape
    assert kh == 2 and kw == 2 and cout % 4 == 0
    ca = round_up(cin, ce)
    cols = 4 * cout
    k_pad = round_up(ca, 64)
    cout_pad = round_up(cols, 16)
    wp = torch.zeros(cout_pad, k_pad, dtype=torch.float32, device=w.device)
    # column q*cout + co  <->  (dy, dx) = (q // 2, q % 2)
    wp[:cols, :cin] = w.permute(2, 3, 1, 0).reshape(cols, cin)
    scale, shift = fold_affine(cout, bias, bn, w.device)
    sc = torch.zeros(cout_pad, dtype=torch.float32, device=w.device)
    sh = torch.zeros(cout_pad, dtype=torch.float32, device=w.device)
    sc[:cols], sh[:cols] = scale.repeat(4), shift.repeat(4)
    return ConvPlan(wp.to(device=device, dtype=dtype).contiguous(), sc.to(device), sh.to(device), 1, 1, 1, 0,
                    ca, 0, cout, cols, cout_pad, k_pad, act, convT=True)


def fold_affine(cout: int, bias: Optional[torch.Tensor], bn, device):
    """scale/shift such that bn(conv(x) + bias) == conv(x)*scale + shift (eval-mode BN)."""
    scale = torch.ones(cout, dtype=torch.float32, device=device)
    shift = torch.zeros(cout, dtype=torch.float32, device=device)
    if bias is not None:
        shift = bias.detach().float().to(device).clone()
    if bn is not None:
        g = bn.weight.detach().float() if bn.weight is not None else torch.ones(cout, device=device)
        b = bn.bias.detach().float() if bn.bias is not None else torch.zeros(cout, device=device)
        inv = g / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        shift = (shift - bn.running_mean.detach().float()) * inv + b
        scale = inv
    return scale, shift


@dataclass
class Head2:
    """A trailing 1x1 conv Cout -> 2 for conv2d(head2=...): w f32 [2, Cout], b f32 [2].  After the call ``out`` is
    its f32 [N*Ho*Wo, 2] result when the conv's epilogue applied it (the conv output itself is then not stored and
    conv2d returns None), or None when the layer has no such kernel and ran as usual."""
    w: torch.Tensor
    b: torch.Tensor
    out: Optional[torch.Tensor] = None


def conv2d(p: ConvPlan, xa: Act, xb: Optional[Act] = None, out: Optional[Act] = None, *, a_up: int = 1,
           residual: Optional[Act] = None, mul: Optional[Act] = None, out2: Optional[Act] = None,
           in_scale: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
           variant: int = 0, out_cpad: Optional[int] = None, split_k_3x3: bool = False,
           px_scale: Optional[torch.Tensor] = None, head2: Optional[Head2] = None,
           a_gate: Optional[torch.Tensor] = None, res_gate: Optional[torch.Tensor] = None) -> Optional[Act]:
    """hiseg_conv2d_fwd.  Returns the output Act (allocated when ``out`` is None; ``out_cpad``: its channel
    stride, the pad channels zero).

    ``a_gate`` (f32 [N, Ca]) / ``res_gate`` (f32 [N, Cout]): source A / the residual is read as
    bf16(x * gate[image][channel]) -- inside the kernel where the layer has that form (hiseg_conv2d_fused_ok; the
    residual's only beside ``head2``), through a channel_scale pass otherwise; the same bits either way.

    ``px_scale`` (f32, one value per source pixel): source A is read as bf16(xa * px_scale[pixel]) -- inside the
    kernel's loader where the layer has that form (hiseg_conv2d_fused_ok), through a pixel_scale pass otherwise; the
    same bits either way.  ``head2``: see :class:`Head2`.

    ``variant`` != 0 forces a kernel variant (hiseg_conv2d_fwd_variant; -1 = generic kernel).  ``split_k_3x3``
    passes the split-K workspace to a 3x3 layer too (images of <= 256 pixels, K >= 1536: the library then splits
    its K loop; the train engine's small-batch choice, off on the inference path).
    """
    dt = xa.dtype
    H, W = xa.H * a_up, xa.W * a_up
    if xb is not None:
        assert xb.dtype == dt and (xb.H, xb.W, xb.N) == (H, W, xa.N)
    if p.convT:
        Ho, Wo = H, W
        oH, oW = 2 * H, 2 * W
    else:
        Ho = (H + 2 * p.pad - p.kh) // p.stride + 1
        Wo = (W + 2 * p.pad - p.kw) // p.stride + 1
        oH, oW = Ho, Wo
    if a_gate is not None:
        assert px_scale is None and head2 is None and res_gate is None
        if variant or out2 is not None or not _fused_ok(p, xa, xb, residual, mul, in_scale, None, None,
                                                        out_dtype or dt, a_up, a_gate=a_gate):
            xa, a_gate = channel_scale(xa, a_gate), None
    if res_gate is not None:
        assert residual is not None
        if head2 is None or variant or out is not None or out2 is not None or \
                not _fused_ok(p, xa, xb, residual, mul, in_scale, None, head2, out_dtype or dt, a_up,
                              res_gate=res_gate):
            residual, res_gate = channel_scale(residual, res_gate), None
    fused = (px_scale is not None or head2 is not None) and not variant and out is None and out2 is None
    if fused:
        assert px_scale is None or head2 is None
        fused = _fused_ok(p, xa, xb, residual, mul, in_scale, px_scale, head2, out_dtype or dt, a_up,
                          res_gate=res_gate)
    assert res_gate is None or fused
    if px_scale is not None and not fused:
        xa = pixel_scale(xa, px_scale)
    if head2 is not None:
        head2.out = None
    if out is None and not (fused and head2 is not None):
        out = Act.new(xa.N, oH, oW, p.cout, out_dtype or dt, xa.t.device, cpad=out_cpad,
                      zero=None if out_cpad is None else out_cpad != p.cout)
    assert out is None or (out.N, out.H, out.W) == (xa.N, oH, oW), ((out.N, out.H, out.W), (xa.N, oH, oW))
    assert xa.C <= p.ca and (xb is None or xb.C <= p.cb)
    if out is None:   # (head2 in the epilogue: the output tile is not stored)
        head2.out = torch.empty(xa.N * oH * oW, 2, dtype=torch.float32, device=xa.t.device)
    d = _conv_desc(p, xa, xb, residual, mul, out, a_up=a_up, in_scale=in_scale, out_dtype=out_dtype, out2=out2,
                   px_scale=px_scale if fused else None, head2=head2 if out is None else None,
                   head2_out=head2.out if out is None else None, a_gate=a_gate, res_gate=res_gate)
    ws = None
    if dt == torch.bfloat16 and not p.convT and ((p.kh * p.kw == 1 and p.k_pad >= 384) or
                                                 (split_k_3x3 and p.kh * p.kw == 9)):
        # small-grid, long-K 1x1 layers (the EfficientNet's deep SE-gated projections) split their K loop over
        # workgroups into this stream-ordered workspace (hiseg_conv2d_workspace_bytes: 0 when the layer does not).
        # (The 3x3 small-image split is the train engine's alone: it pays only for a small batch, and the inference
        # path's kernel choice must not depend on the batch.)
        nbytes = L.lib().hiseg_conv2d_workspace_bytes(ctypes.byref(d))
        if nbytes > 0:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=xa.t.device)
            d.workspace, d.workspace_bytes = ws, nbytes
    if RECORD is not None:
        dc = d.copy()
        keep = [t for t in (xa, xb, out, residual, mul, out2, ws, px_scale, a_gate, res_gate) if t is not None]
        RECORD.append((dc, keep, p, _conv_flops(d, p, xa, xb)))
    gate = GATE
    if gate is not None:
        if _conv_flops(d, p, xa, xb) >= gate.min_flops and not variant:
            gate.before()
            _launch_conv(d, p, xa, xb)
            gate.after()
            return out
        gate.light()
    _launch_conv(d, p, xa, xb, variant)
    return out


def _conv_desc(p, xa, xb, residual, mul, out, *, a_up=1, in_scale=None, out_dtype=None, out2=None, px_scale=None,
               head2=None, head2_out=None, a_gate=None, res_gate=None):
    """The Conv2dDesc of one layer, for a launch (conv2d) or a plan (_fused_ok).  ``out`` None: no output tile is
    described beyond a dense [.., Cout] view of ``out_dtype`` -- head2 stores ``head2_out`` instead, and a plan has
    no output yet."""
    dt = xa.dtype
    H, W = xa.H * a_up, xa.W * a_up
    d = L.Conv2dDesc()
    d.dtype, d.out_dtype = hdtype(dt), hdtype(out.dtype if out is not None else (out_dtype or dt))
    d.N, d.H, d.W = xa.N, H, W
    if p.convT:
        d.Ho, d.Wo = H, W
    else:
        d.Ho = (H + 2 * p.pad - p.kh) // p.stride + 1
        d.Wo = (W + 2 * p.pad - p.kw) // p.stride + 1
    d.KH, d.KW, d.stride, d.pad = p.kh, p.kw, p.stride, p.pad
    d.srcA, d.a_cstride, d.a_coff, d.Ca, d.a_up = xa, xa.cstride, xa.coff, p.ca, a_up
    if xb is not None:
        d.srcB, d.b_cstride, d.b_coff, d.Cb = xb, xb.cstride, xb.coff, p.cb
    if in_scale is not None:
        d.in_scale = in_scale
    d.weight, d.Cout, d.Cout_pad, d.K_pad = p.weight, p.gemm_cols, p.cout_pad, p.k_pad
    d.scale, d.shift, d.act, d.act_beta = p.scale, p.shift, int(p.act), L.act_beta(p.act)
    if residual is not None:
        d.residual, d.r_cstride, d.r_coff = residual, residual.cstride, residual.coff
    if mul is not None:
        d.mul, d.m_cstride, d.m_coff = mul, mul.cstride, mul.coff
    if out is not None:
        d.out, d.o_cstride, d.o_coff = out, out.cstride, out.coff
    else:
        d.o_cstride, d.o_coff = p.cout, 0
    if head2 is not None:
        d.head2_w, d.head2_b, d.head2_out = head2.w, head2.b, head2_out
    if px_scale is not None:
        d.px_scale = px_scale
    if a_gate is not None:
        d.a_gate = a_gate
    if res_gate is not None:
        d.res_gate = res_gate
    if out2 is not None:
        assert out2.dtype == dt
        d.out2, d.o2_cstride, d.o2_coff = out2, out2.cstride, out2.coff
    d.convT = int(p.convT)
    if p.weight_frag is not None:
        d.weight_frag = p.weight_frag
    return d


def _conv_flops(d, p, xa, xb) -> float:
    """Multiply-adds x 2 of one launch over the channels the sources really hold (RECORD, GATE and PROBE)."""
    return 2.0 * d.N * d.Ho * d.Wo * p.gemm_cols * p.kh * p.kw * (xa.C + (xb.C if xb is not None else 0))


def _fused_ok(p, xa, xb, residual, mul, in_scale, px_scale, head2, out_dtype, a_up, a_gate=None, res_gate=None) -> bool:
    """Whether the library has a kernel that applies px_scale / head2 / a_gate / res_gate (all that are given) inside
    this layer (planning only, no launch)."""
    if xa.dtype != torch.bfloat16 or out_dtype != torch.bfloat16 or xb is not None or mul is not None or \
            in_scale is not None or a_up != 1:
        return False
    for gt, c in ((a_gate, p.ca), (res_gate, p.cout)):
        if gt is not None:
            assert gt.dtype == torch.float32 and gt.is_contiguous() and tuple(gt.shape) == (xa.N, c), \
                (gt.dtype, tuple(gt.shape), (xa.N, c))
    if a_gate is not None and xa.C != p.ca:
        return False
    if px_scale is not None:
        assert px_scale.dtype == torch.float32 and px_scale.is_contiguous() and px_scale.numel() == xa.N * xa.H * xa.W
    if head2 is not None:
        if p.convT or residual is None:
            return False
        assert head2.w.dtype == torch.float32 and head2.w.is_contiguous() and tuple(head2.w.shape) == (2, p.cout)
        assert head2.b.dtype == torch.float32 and head2.b.numel() == 2
    # (head2.w for head2_out: the plan looks at its alignment only, and nothing is launched)
    d = _conv_desc(p, xa, None, residual, None, None, out_dtype=out_dtype, px_scale=px_scale, head2=head2,
                   head2_out=head2.w if head2 is not None else None, a_gate=a_gate, res_gate=res_gate)
    if px_scale is not None or a_gate is not None:
        d.out = xa   # (any aligned address: the plan looks at the output's alignment only)
    return bool(L.lib().hiseg_conv2d_fused_ok(ctypes.byref(d)))


def resblock(p1: ConvPlan, p2: ConvPlan, x: Act) -> Optional[Act]:
    """A 64-channel ResidualBlock act2(conv2(act1(conv1(x))) + x) in one launch (hiseg_resblock_fwd): the bits of
    conv2d(p2, conv2d(p1, x), residual=x), the intermediate never stored.  Returns None -- nothing launched -- where
    the library has no such kernel for the pair (hiseg_resblock_fused_ok) or a launch hook (RECORD, GATE) wants the
    layers one by one; the caller then runs the two launches."""
    if RECORD is not None or GATE is not None or x.dtype != torch.bfloat16 or p1.convT or p2.convT or \
            p1.cout != 64 or p2.cout != 64 or x.C != 64:
        return None
    out = Act.new(x.N, x.H, x.W, p2.cout, x.dtype, x.t.device, zero=None)
    d1 = _conv_desc(p1, x, None, None, None, None, out_dtype=x.dtype)
    d2 = _conv_desc(p2, x, None, x, None, out)   # (srcA stands in for the intermediate: same shape, never read)
    if not L.lib().hiseg_resblock_fused_ok(ctypes.byref(d1), ctypes.byref(d2)):
        return None
    L.check(L.lib().hiseg_resblock_fwd(ctypes.byref(d1), ctypes.byref(d2), L.stream_ptr()), "resblock")
    return out


def _launch_conv(d, p, xa, xb, variant=0):
    if PROBE is not None:
        key = PROBE.select(d)
        if key is not None:
            L.check(PROBE.around(key, _conv_flops(d, p, xa, xb), lambda: L.lib().hiseg_conv2d_fwd(ctypes.byref(d), L.stream_ptr())),
                    "conv2d")
            return
    if variant:
        L.check(L.lib().hiseg_conv2d_fwd_variant(ctypes.byref(d), variant, L.stream_ptr()), "conv2d")
    else:
        L.check(L.lib().hiseg_conv2d_fwd(ctypes.byref(d), L.stream_ptr()), "conv2d")


# ---------------------------------------------------------------------------------------- misc
def maxpool2x2(x: Act) -> Act:
    assert x.coff == 0 and x.cstride == x.cpad
    out = Act.new(x.N, x.H // 2, x.W // 2, x.C, x.dtype, x.t.device, cpad=x.cstride, zero=False)
    L.check(L.lib().hiseg_maxpool2x2_fwd(hdtype(x.dtype), x.ptr(), x.N, x.H, x.W, x.cstride, out.ptr(),
                                         L.stream_ptr()), "maxpool2x2")
    return out


def attn_spatial(x: Act, w7: torch.Tensor) -> Act:
    """SpatialAttentionModule (attention_modules.py:92-113)."""
    assert x.coff == 0 and x.cstride == x.C
    P = x.N * x.H * x.W
    stats = torch.empty(P * 2, dtype=torch.float32, device=x.t.device)
    att = torch.empty(P, dtype=torch.float32, device=x.t.device)
    out = Act.new(x.N, x.H, x.W, x.C, x.dtype, x.t.device, zero=False)
    k = w7.shape[-1]
    L.check(L.lib().hiseg_attn_spatial_fwd(hdtype(x.dtype), x.ptr(), x.N, x.H, x.W, x.C, w7.data_ptr(), k,
                                           stats.data_ptr(), att.data_ptr(), out.ptr(), L.stream_ptr()),
            "attn_spatial")
    return out


def attn_map(x: Act, w7: torch.Tensor) -> torch.Tensor:
    """The attention map of SpatialAttentionModule alone: sigmoid(conv7x7([mean_c x, max_c x])), f32 [N*H*W]."""
    assert x.coff == 0 and x.cstride == x.C
    P = x.N * x.H * x.W
    stats = torch.empty(P * 2, dtype=torch.float32, device=x.t.device)
    att = torch.empty(P, dtype=torch.float32, device=x.t.device)
    L.check(L.lib().hiseg_attn_map_fwd(hdtype(x.dtype), x.ptr(), x.N, x.H, x.W, x.C, w7.data_ptr(), w7.shape[-1],
                                       stats.data_ptr(), att.data_ptr(), L.stream_ptr()), "attn_map")
    return att


def pixel_scale(x: Act, att: torch.Tensor) -> Act:
    """x * att[pixel] (attention_modules.py:113); att f32 [N*H*W]."""
    assert x.coff == 0 and x.cstride == x.C and att.dtype == torch.float32 and att.numel() == x.N * x.H * x.W
    out = Act.new(x.N, x.H, x.W, x.C, x.dtype, x.t.device, zero=False)
    L.check(L.lib().hiseg_pixel_scale_fwd(hdtype(x.dtype), x.ptr(), x.N * x.H * x.W, x.C, att.data_ptr(), out.ptr(),
                                          L.stream_ptr()), "pixel_scale")
    return out


def se_gate(x: Act, w1, b1, w2, b2, act: int) -> torch.Tensor:
    """GAP -> 1x1 -> act -> 1x1 -> sigmoid; returns gate [N, C] f32."""
    assert x.coff == 0 and x.cstride == x.C
    HW = x.H * x.W
    lib = L.lib()
    splits = lib.hiseg_gap_splits(HW)
    partial = torch.empty(x.N * splits * x.C, dtype=torch.float32, device=x.t.device)
    gate = torch.empty(x.N, x.C, dtype=torch.float32, device=x.t.device)
    cr = w1.shape[0]
    L.check(lib.hiseg_se_gate_fwd(hdtype(x.dtype), x.ptr(), x.N, HW, x.C, w1.data_ptr(), _ptr(b1), cr,
                                  w2.data_ptr(), _ptr(b2), int(act), L.act_beta(act), partial.data_ptr(), gate.data_ptr(),
                                  L.stream_ptr()), "se_gate")
    return gate


def channel_scale(x: Act, gate: torch.Tensor) -> Act:
    assert x.coff == 0 and x.cstride == x.C
    out = Act.new(x.N, x.H, x.W, x.C, x.dtype, x.t.device, zero=False)
    L.check(L.lib().hiseg_channel_scale_fwd(hdtype(x.dtype), x.ptr(), x.N, x.H * x.W, x.C, gate.data_ptr(),
                                            out.ptr(), L.stream_ptr()), "channel_scale")
    return out


def dwconv(x: Act, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, k: int, stride: int, act: int) -> Act:
    assert x.coff == 0 and x.cstride == x.C
    pad = k // 2
    Ho = (x.H + 2 * pad - k) // stride + 1
    Wo = (x.W + 2 * pad - k) // stride + 1
    out = Act.new(x.N, Ho, Wo, x.C, x.dtype, x.t.device, zero=False)
    L.check(L.lib().hiseg_dwconv_fwd(hdtype(x.dtype), x.ptr(), x.N, x.H, x.W, x.C, k, stride, w.data_ptr(),
                                     scale.data_ptr(), shift.data_ptr(), act, out.ptr(), Ho, Wo, L.stream_ptr()),
            "dwconv")
    return out


def dwconv_se_gate(x: Act, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, k: int, stride: int, act: int,
                   w1, b1, w2, b2, se_act: int):
    """Depthwise conv + folded BN + act with the SqueezeExcite pool fused into it; returns (h, gate [N, C])."""
    assert x.coff == 0 and x.cstride == x.C
    pad = k // 2
    Ho = (x.H + 2 * pad - k) // stride + 1
    Wo = (x.W + 2 * pad - k) // stride + 1
    lib = L.lib()
    out = Act.new(x.N, Ho, Wo, x.C, x.dtype, x.t.device, zero=False)
    tiles = lib.hiseg_dw_gap_parts(hdtype(x.dtype), x.N, Ho, Wo, x.C, k, stride)
    partial = torch.empty(x.N * tiles * x.C, dtype=torch.float32, device=x.t.device)
    L.check(lib.hiseg_dwconv_gap_fwd(hdtype(x.dtype), x.ptr(), x.N, x.H, x.W, x.C, k, stride, w.data_ptr(),
                                     scale.data_ptr(), shift.data_ptr(), act, out.ptr(), Ho, Wo, partial.data_ptr(),
                                     L.stream_ptr()), "dwconv_gap")
    gate = torch.empty(x.N, x.C, dtype=torch.float32, device=x.t.device)
    L.check(lib.hiseg_se_gate_partials_fwd(partial.data_ptr(), tiles, x.N, Ho * Wo, x.C, w1.data_ptr(), _ptr(b1),
                                           w1.shape[0], w2.data_ptr(), _ptr(b2), se_act, gate.data_ptr(),
                                           L.stream_ptr()), "se_gate_partials")
    return out, gate


def image_max(x: torch.Tensor) -> torch.Tensor:
    """The device-side maximum of a contiguous f32 batch (hiseg_image_max_fwd's encoded buffer): the /255 flag of
    normalize_input, read by the kernel that normalises."""
    maxbuf = torch.empty(1, dtype=torch.float32, device=x.device)
    L.check(L.lib().hiseg_image_max_fwd(x.data_ptr(), x.numel(), maxbuf.data_ptr(), L.stream_ptr()), "image_max")
    return maxbuf


@dataclass
class RawImages:
    """The f32 NCHW image batch standing in for its normalised NHWC activation: the stem conv normalises it while it
    stages its halo (stem_raw), so that activation is never stored.  ``plan``: that conv; ``maxbuf``: image_max of
    the batch."""
    plan: ConvPlan
    t: torch.Tensor
    mean: torch.Tensor
    std: torch.Tensor
    maxbuf: torch.Tensor
    dtype: torch.dtype

    @property
    def N(self) -> int:
        return self.t.shape[0]

    @property
    def H(self) -> int:
        return self.t.shape[2]

    @property
    def W(self) -> int:
        return self.t.shape[3]


def input_norm(images: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, dtype: torch.dtype,
               stem: Optional[ConvPlan] = None):
    """normalize_input (hierarchical_segmentation_unet.py:1885-1890) with a device-side max flag.  ``stem``: the
    plan of the one conv that reads the result; where the library normalises inside that layer
    (stem_raw_ok) the images come back as :class:`RawImages` for stem_raw and no normalised copy is written; an
    :class:`Act` otherwise.  The maximum is a reduction over the whole batch and is launched first either way."""
    _require_gpu(images)
    raw_ok = stem is not None and stem_raw_ok(stem, images, dtype)
    x = images.contiguous().float()
    B, C, H, W = x.shape
    maxbuf = image_max(x)
    if raw_ok:
        return RawImages(stem, x, mean, std, maxbuf, dtype)
    out = Act.new(B, H, W, C, dtype, x.device, zero=False)
    L.check(L.lib().hiseg_input_norm_fwd(hdtype(dtype), x.data_ptr(), B, C, H, W, maxbuf.data_ptr(), mean.data_ptr(),
                                         std.data_ptr(), out.ptr(), out.cstride, L.stream_ptr()), "input_norm")
    return out


def _stem_raw_desc(p: ConvPlan, images: torch.Tensor, mean, std, maxbuf, out: Optional[Act]):
    """The Conv2dDesc of the stem conv reading raw images (hiseg_conv2d_desc.raw_src).  Source A is described as the
    8-channel NHWC view the images stand for and is not read."""
    B, _, H, W = images.shape
    d = L.Conv2dDesc()
    d.dtype = d.out_dtype = L.HISEG_BF16
    d.N, d.H, d.W = B, H, W
    d.Ho = (H + 2 * p.pad - p.kh) // p.stride + 1
    d.Wo = (W + 2 * p.pad - p.kw) // p.stride + 1
    d.KH, d.KW, d.stride, d.pad = p.kh, p.kw, p.stride, p.pad
    d.a_cstride, d.a_coff, d.Ca, d.a_up = p.ca, 0, p.ca, 1
    d.weight, d.Cout, d.Cout_pad, d.K_pad = p.weight, p.gemm_cols, p.cout_pad, p.k_pad
    d.scale, d.shift, d.act, d.act_beta = p.scale, p.shift, int(p.act), L.act_beta(p.act)
    if out is not None:
        d.out, d.o_cstride, d.o_coff = out, out.cstride, out.coff
    else:
        d.out, d.o_cstride, d.o_coff = p.weight, round_up(p.cout, 8), 0   # (a plan: any aligned address)
    d.raw_src, d.raw_mean, d.raw_std, d.raw_max = images, mean, std, maxbuf
    return d


def stem_raw_ok(p: ConvPlan, images: torch.Tensor, dtype: torch.dtype) -> bool:
    """Whether the library runs this stem conv straight from ``images`` (planning only, no launch): bf16 compute,
    contiguous f32 [B, 3, H, W] on the GPU, a single-source 3x3 stride-2 layer, every operand under 2 GiB
    (hiseg_conv2d_fused_ok).  A launch hook that wants every layer as a plain conv (RECORD) gets the two passes."""
    if RECORD is not None or dtype != torch.bfloat16 or images.dim() != 4 or images.shape[1] != 3 or \
            images.dtype != torch.float32 or not images.is_cuda or not images.is_contiguous():
        return False
    if p.convT or (p.kh, p.kw, p.stride, p.pad) != (3, 3, 2, 1) or p.cb or p.weight.dtype != torch.bfloat16:
        return False
    # (the tables' addresses: the plan looks at their alignment only)
    d = _stem_raw_desc(p, images, p.scale, p.scale, p.scale, None)
    return bool(L.lib().hiseg_conv2d_fused_ok(ctypes.byref(d)))


def stem_raw(raw: RawImages) -> Act:
    """The stem conv on raw images (input_norm asked stem_raw_ok): the bits of conv2d(plan, input_norm(images)),
    recorded as path ("stem_raw", 1)."""
    p, x = raw.plan, raw.t
    out = Act.new(raw.N, (raw.H - 1) // 2 + 1, (raw.W - 1) // 2 + 1, p.cout, raw.dtype, x.device)
    d = _stem_raw_desc(p, x, raw.mean, raw.std, raw.maxbuf, out)
    if GATE is not None:   # (far below GATE.min_flops: a light launch, as the plain stem conv is)
        GATE.light()
    L.check(L.lib().hiseg_conv2d_fwd(ctypes.byref(d), L.stream_ptr()), "stem_raw")
    return out


def hier_combine(low: torch.Tensor, N: int, h: int, w: int, tfeat: Optional[Act], ut_w, ut_scale, ut_shift, ut_act,
                 u1_w, u1_b, t_w, t_b, want_aux: bool, per_sample: bool = False, tn2: Optional[torch.Tensor] = None):
    """Fused upsample_bg_fg + target 1x1 + hierarchical combine; ``per_sample``: ut_scale/ut_shift are the
    [N][32] LayerNorm2d tables of hiseg_ubf_ln_tables.  ``tn2`` (f32 [N*2h*2w, 2], conv2d's Head2.out): the target
    1x1 was applied by the conv that produced tfeat; tfeat / t_w / t_b are then not read."""
    dev = low.device
    logits = torch.empty(N, 3, 2 * h, 2 * w, dtype=torch.float32, device=dev)
    bgfg = torch.empty(N, 2, 2 * h, 2 * w, dtype=torch.float32, device=dev) if want_aux else None
    tn = torch.empty(N, 2, 2 * h, 2 * w, dtype=torch.float32, device=dev) if want_aux else None
    if tn2 is not None:
        assert tn2.dtype == torch.float32 and tn2.is_contiguous() and tn2.numel() == N * 4 * h * w * 2
        L.check(L.lib().hiseg_hier_combine_tn_fwd(low.data_ptr(), N, h, w, tn2.data_ptr(), ut_w.data_ptr(),
                                                  ut_scale.data_ptr(), ut_shift.data_ptr(), int(ut_act),
                                                  L.act_beta(ut_act), int(per_sample), u1_w.data_ptr(), u1_b.data_ptr(),
                                                  logits.data_ptr(), _ptr(bgfg), _ptr(tn), L.stream_ptr()),
                "hier_combine_tn")
        return logits, bgfg, tn
    assert tfeat.coff == 0 and tfeat.cstride == tfeat.C and (tfeat.H, tfeat.W) == (2 * h, 2 * w)
    L.check(L.lib().hiseg_hier_combine_fwd(hdtype(tfeat.dtype), low.data_ptr(), N, h, w, tfeat.ptr(), tfeat.C,
                                           ut_w.data_ptr(), ut_scale.data_ptr(), ut_shift.data_ptr(), int(ut_act),
                                           L.act_beta(ut_act), int(per_sample), u1_w.data_ptr(), u1_b.data_ptr(), t_w.data_ptr(), t_b.data_ptr(),
                                           logits.data_ptr(), _ptr(bgfg), _ptr(tn), L.stream_ptr()), "hier_combine")
    return logits, bgfg, tn


def hier_combine_resize(low: torch.Tensor, N: int, h: int, w: int, tn2: torch.Tensor, ut_w, ut_scale, ut_shift, ut_act,
                        u1_w, u1_b, mh: int, mw: int, want_aux: bool, per_sample: bool = False):
    """hier_combine at a mask size (mh, mw) other than (2h, 2w): upsample_bg_fg, the bilinear resize of its two
    logits and of the target logits ``tn2`` (f32 [N*2h*2w, 2]) to the mask size, the softmax and the combine in one
    launch (hiseg_hier_combine_resize).  Returns logits [N,3,mh,mw] and, with ``want_aux``, the resized bg/fg and
    target logits [N,2,mh,mw]."""
    _require_gpu(low, tn2)
    dev = low.device
    assert tn2.dtype == torch.float32 and tn2.is_contiguous() and tn2.numel() == N * 4 * h * w * 2
    logits = torch.empty(N, 3, mh, mw, dtype=torch.float32, device=dev)
    bgfg = torch.empty(N, 2, mh, mw, dtype=torch.float32, device=dev) if want_aux else None
    tn = torch.empty(N, 2, mh, mw, dtype=torch.float32, device=dev) if want_aux else None
    L.check(L.lib().hiseg_hier_combine_resize(low.data_ptr(), N, h, w, tn2.data_ptr(), ut_w.data_ptr(),
                                              ut_scale.data_ptr(), ut_shift.data_ptr(), int(ut_act),
                                              L.act_beta(ut_act), int(per_sample), u1_w.data_ptr(), u1_b.data_ptr(),
                                              int(mh), int(mw), logits.data_ptr(), _ptr(bgfg), _ptr(tn),
                                              L.stream_ptr()), "hier_combine_resize")
    return logits, bgfg, tn


def layernorm2d(z: Act, weight: torch.Tensor, bias: torch.Tensor, eps: float, act: int,
                residual: Optional[Act] = None, out: Optional[Act] = None) -> Act:
    """LayerNorm2d (model.py:18-38) of a conv output z, then (+ residual) and the activation:
    per-sample statistics over (C, H, W) (hiseg_ln_fwd_stats) and one apply pass with the folded
    per-sample tables (hiseg_bn_apply, per_sample = 1).  weight / bias: f32 [C]."""
    lib = L.lib()
    dev = z.t.device
    N, HW, C = z.N, z.H * z.W, z.C
    ws = torch.empty(int(lib.hiseg_ln_ws(N, HW, C)), dtype=torch.float32, device=dev)
    mean = torch.empty(N, dtype=torch.float32, device=dev)
    invstd = torch.empty_like(mean)
    scale = torch.empty(N * C, dtype=torch.float32, device=dev)
    shift = torch.empty_like(scale)
    L.check(lib.hiseg_ln_fwd_stats(hdtype(z.dtype), z.ptr(), N, HW, C, z.cstride, z.coff, weight.data_ptr(),
                                   bias.data_ptr(), float(eps), ws.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                   scale.data_ptr(), shift.data_ptr(), L.stream_ptr()), "ln_fwd_stats")
    y = out if out is not None else Act.new(N, z.H, z.W, C, z.dtype, dev, cpad=z.cstride)
    d = L.BnApplyDesc()
    d.dtype, d.P, d.HW, d.C = hdtype(z.dtype), N * HW, HW, C
    d.z, d.z_cstride, d.z_coff = z, z.cstride, z.coff
    d.scale, d.shift, d.per_sample = scale, shift, 1
    if residual is not None:
        d.residual, d.r_cstride, d.r_coff = residual, residual.cstride, residual.coff
    d.act, d.act_beta = int(act), L.act_beta(act)
    d.y, d.y_cstride, d.y_coff = y, y.cstride, y.coff
    L.check(lib.hiseg_bn_apply(ctypes.byref(d), L.stream_ptr()), "ln_apply")
    return y


def instance_masks(logits: torch.Tensor, dilation: int = 0) -> torch.Tensor:
    N, _, mh, mw = logits.shape
    out = torch.empty(N, 1, mh, mw, dtype=torch.float32, device=logits.device)
    L.check(L.lib().hiseg_instance_masks_fwd(logits.contiguous().data_ptr(), N, mh, mw, int(dilation), out.data_ptr(),
                                             L.stream_ptr()), "instance_masks")
    return out


def binary_masks(u: torch.Tensor, oc_w: torch.Tensor, oc_b: torch.Tensor) -> torch.Tensor:
    B, _, H, W = u.shape
    out = torch.empty(B, 1, H, W, dtype=torch.float32, device=u.device)
    L.check(L.lib().hiseg_binary_masks_fwd(L.HISEG_F32, u.data_ptr(), 1, B, H, W, oc_w.data_ptr(), oc_b.data_ptr(),
                                           out.data_ptr(), L.stream_ptr()), "binary_masks")
    return out


# ---- mask post-processing (include/hiseg_post.h): f32 planes [..., H, W], any leading dimensions


def _post_planes(x: torch.Tensor, what: str):
    _require_gpu(x)
    if x.dim() < 2:
        raise ValueError(f"{what}: expected [..., H, W] planes, got shape {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    H, W = x.shape[-2:]
    return x, (x.numel() // (H * W) if H * W else 0), H, W


def _post_chunks(iterations: int, H: int, W: int, radius: int, force_tiled: bool):
    """Iterations per launch: one launch in the LDS-resident form, at most a 32-pixel halo per launch in the tiled
    form (the launches compose to the same bits)."""
    if iterations < 1:
        raise ValueError(f"iterations must be >= 1, got {iterations}")
    cap = L.lib().hiseg_post_max_iterations(H, W, radius, int(force_tiled))
    out = []
    while iterations > 0:
        out.append(min(iterations, cap))
        iterations -= out[-1]
    return out


def edge_smooth(x: torch.Tensor, threshold: float = 0.5, blur_strength: float = 3.0, iterations: int = 1, *,
                binarize_input: bool = False, _force_tiled: bool = False) -> torch.Tensor:
    """BinaryMaskEdgeSmoothing applied `iterations` times to every H x W plane of x; f32 in, f32 0/1 out."""
    x, NC, H, W = _post_planes(x, "edge_smooth")
    for n in _post_chunks(iterations, H, W, 1, _force_tiled):
        out = torch.empty_like(x)
        L.check(L.lib().hiseg_edge_smooth_fwd(x.data_ptr(), out.data_ptr(), NC, H, W, threshold, blur_strength, n,
                                              int(binarize_input), int(_force_tiled), L.stream_ptr()), "edge_smooth")
        x, binarize_input = out, False
    return x


def class_edge_smooth(scores: torch.Tensor, threshold: float = 0.5, blur_strength: float = 3.0, iterations: int = 1,
                      *, _force_tiled: bool = False) -> torch.Tensor:
    """[B,3,H,W] scores -> [B,3,H,W]: the masks argmax == c, each smoothed `iterations` times."""
    if scores.dim() != 4 or scores.shape[1] != 3:
        raise ValueError(f"class_edge_smooth: expected [B,3,H,W] scores, got shape {tuple(scores.shape)}")
    x, _, H, W = _post_planes(scores, "class_edge_smooth")
    chunks = _post_chunks(iterations, H, W, 1, _force_tiled)
    out = torch.empty_like(x)
    L.check(L.lib().hiseg_class_edge_smooth_fwd(x.data_ptr(), out.data_ptr(), x.shape[0], H, W, threshold,
                                                blur_strength, chunks[0], int(_force_tiled), L.stream_ptr()),
            "class_edge_smooth")
    rest = iterations - chunks[0]
    return edge_smooth(out, threshold, blur_strength, rest, _force_tiled=_force_tiled) if rest else out


def var_gated_blur(x: torch.Tensor, kernel_size: int, sigma_spatial: float, gain: float, iterations: int, *,
                   clamp_input: bool = False, threshold: Optional[float] = None,
                   _force_tiled: bool = False) -> torch.Tensor:
    """x <- w*f + (1-w)*x, f = G*x, w = exp(-max(G*x^2 - f^2, 0) * gain), `iterations` times; `threshold` set:
    the result is (x > threshold) as 0/1."""
    x, NC, H, W = _post_planes(x, "var_gated_blur")
    chunks = _post_chunks(iterations, H, W, max(kernel_size // 2, 1), _force_tiled)
    for i, n in enumerate(chunks):
        last = i == len(chunks) - 1
        out = torch.empty_like(x)
        L.check(L.lib().hiseg_var_gated_blur_fwd(
            x.data_ptr(), out.data_ptr(), NC, H, W, kernel_size, sigma_spatial, gain, int(clamp_input and i == 0),
            int(last and threshold is not None), threshold if threshold is not None else 0.0, n, int(_force_tiled),
            L.stream_ptr()), "var_gated_blur")
        x = out
    return x


def morph_bilateral(x: torch.Tensor, kernel_size: int = 5, sigma: float = 1.0, morph_size: int = 3, *,
                    _force_tiled: bool = False) -> torch.Tensor:
    """MorphologicalBilateralFilter on every plane: clamp, open, Gaussian, close, > 0.5."""
    x, NC, H, W = _post_planes(x, "morph_bilateral")
    out = torch.empty_like(x)
    L.check(L.lib().hiseg_morph_bilateral_fwd(x.data_ptr(), out.data_ptr(), NC, H, W, kernel_size, sigma, morph_size,
                                              int(_force_tiled), L.stream_ptr()), "morph_bilateral")
    return out


def bilateral(x: torch.Tensor, kernel_size: int = 5, sigma_spatial: float = 1.0,
              sigma_range: float = 0.1) -> torch.Tensor:
    """The true bilateral filter with reflect padding on every plane."""
    x, NC, H, W = _post_planes(x, "bilateral")
    out = torch.empty_like(x)
    L.check(L.lib().hiseg_bilateral_fwd(x.data_ptr(), out.data_ptr(), NC, H, W, kernel_size, sigma_spatial,
                                        sigma_range, L.stream_ptr()), "bilateral")
    return out


def guided_filter(x: torch.Tensor, guide: Optional[torch.Tensor] = None, radius: int = 2, eps: float = 0.01,
                  force_tiled: bool = False) -> torch.Tensor:
    """EdgePreservingFilter: [B,Cx,H,W] x guided by [B,Cg,H,W] (None: by itself) -> f32 [B,max(Cx,Cg),H,W]; the
    channels broadcast as in x * guide."""
    _require_gpu(x, guide)
    for t, what in ((x, "x"), (guide, "guide")):
        if t is not None and t.dim() != 4:
            raise ValueError(f"guided_filter: expected a (B, C, H, W) {what}, got shape {tuple(t.shape)}")
    B, Cx, H, W = x.shape
    Cg = Cx
    if guide is not None:
        Cg = guide.shape[1]
        if (guide.shape[0], *guide.shape[2:]) != (B, H, W) or not (Cx == Cg or Cx == 1 or Cg == 1):
            raise ValueError(f"guided_filter: x {tuple(x.shape)} and guide {tuple(guide.shape)} do not broadcast "
                             "over the channels")
        guide = guide.to(torch.float32).contiguous()
    x = x.to(torch.float32).contiguous()
    out = torch.empty(B, max(Cx, Cg), H, W, dtype=torch.float32, device=x.device)
    L.check(L.lib().hiseg_guided_filter_fwd(x.data_ptr(), _ptr(guide), out.data_ptr(), B, Cx, Cg, H, W, radius, eps,
                                            int(force_tiled), L.stream_ptr()), "guided_filter")
    return out


# The directional, adaptive and optimized edge-smoothing filters: stencils of radius 2.  `return_soft` adds the f32
# blend of the last iteration before its threshold.


def _variant_planes(x: torch.Tensor, what: str, dtypes=(torch.float32,)):
    _require_gpu(x)
    if x.dim() < 2:
        raise ValueError(f"{what}: expected [..., H, W] planes, got shape {tuple(x.shape)}")
    if x.dtype not in dtypes:
        raise ValueError(f"{what}: expected planes of {' or '.join(str(d) for d in dtypes)}, got {x.dtype}")
    x = x.contiguous()
    H, W = x.shape[-2:]
    return x, (x.numel() // (H * W) if H * W else 0), H, W


def _variant_run(x, H, W, iterations, return_soft, force_tiled, launch, out_dtype=None):
    """`launch(x, out, soft_ptr, n)` once per chunk of iterations; the soft blend comes from the last chunk."""
    chunks = _post_chunks(iterations, H, W, 2, force_tiled)
    soft = None
    for i, n in enumerate(chunks):
        out = torch.empty_like(x, dtype=out_dtype)
        if return_soft and i == len(chunks) - 1:
            soft = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        launch(x, out, _ptr(soft), n)
        x = out
    return (x, soft) if return_soft else x


def dir_edge_smooth(x: torch.Tensor, iterations: int = 1, *, return_soft: bool = False, _force_tiled: bool = False):
    """DirectionalEdgeSmoothing applied `iterations` times to every H x W plane of x; f32 in, f32 0/1 out."""
    x, NC, H, W = _variant_planes(x, "dir_edge_smooth")

    def launch(src, out, soft, n):
        L.check(L.lib().hiseg_dir_edge_smooth_fwd(src.data_ptr(), out.data_ptr(), soft, NC, H, W, n,
                                                  int(_force_tiled), L.stream_ptr()), "dir_edge_smooth")
    return _variant_run(x, H, W, iterations, return_soft, _force_tiled, launch)


def adaptive_edge_smooth(x: torch.Tensor, blur_strength: torch.Tensor, edge_sensitivity: torch.Tensor,
                         final_threshold: torch.Tensor, iterations: int = 1, *, return_soft: bool = False,
                         _force_tiled: bool = False):
    """AdaptiveEdgeSmoothing applied `iterations` times.  The parameters are f32 tensors on x's device with one
    element (every plane), one per plane, or -- for a [B,C,H,W] x -- one per image as the reference's [B,1]; they
    are read by the kernel only."""
    x, NC, H, W = _variant_planes(x, "adaptive_edge_smooth")
    params = []
    for name, p in (("blur_strength", blur_strength), ("edge_sensitivity", edge_sensitivity),
                    ("final_threshold", final_threshold)):
        if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
            raise ValueError(f"adaptive_edge_smooth: {name} must be a float32 tensor, got "
                             f"{p.dtype if isinstance(p, torch.Tensor) else type(p).__name__}")
        _require_gpu(p)
        if p.device != x.device:
            raise ValueError(f"adaptive_edge_smooth: {name} is on {p.device}, the planes on {x.device}")
        params.append(p)
    if all(p.numel() == 1 for p in params):
        stride = 0
        params = [p.contiguous() for p in params]
    else:
        stride = 1
        for i, p in enumerate(params):
            if p.numel() == 1:
                p = p.reshape(1).expand(NC)
            elif x.dim() == 4 and p.numel() == x.shape[0] and p.numel() != NC:
                p = p.reshape(-1, 1).expand(-1, x.shape[1])
            elif p.numel() != NC:
                raise ValueError(f"adaptive_edge_smooth: a parameter of {p.numel()} elements for {NC} planes "
                                 f"(shape {tuple(x.shape)})")
            params[i] = p.contiguous()
    bs, es, ft = params

    def launch(src, out, soft, n):
        L.check(L.lib().hiseg_adaptive_edge_smooth_fwd(src.data_ptr(), out.data_ptr(), soft, NC, H, W, bs.data_ptr(),
                                                       es.data_ptr(), ft.data_ptr(), stride, n, int(_force_tiled),
                                                       L.stream_ptr()), "adaptive_edge_smooth")
    return _variant_run(x, H, W, iterations, return_soft, _force_tiled, launch)


def opt_edge_smooth(x: torch.Tensor, iterations: int = 1, *, to_fp16: bool = False, return_soft: bool = False,
                    _force_tiled: bool = False):
    """OptimizedEdgeSmoothing applied `iterations` times: f32 planes in and out, or f16 planes in and out (f32
    arithmetic on the f16 values).  `to_fp16` on f32 planes: the kernel rounds them to f16 while it reads them and
    writes f16 planes -- the bits of opt_edge_smooth(x.half()) without the cast pass."""
    x, NC, H, W = _variant_planes(x, "opt_edge_smooth", (torch.float32, torch.float16))

    def launch(src, out, soft, n):
        dtype = (L.HISEG_POST_F16 if src.dtype == torch.float16 else
                 L.HISEG_POST_F32_TO_F16 if out.dtype == torch.float16 else L.HISEG_POST_F32)
        L.check(L.lib().hiseg_opt_edge_smooth_fwd(dtype, src.data_ptr(), out.data_ptr(), soft, NC, H, W, n,
                                                  int(_force_tiled), L.stream_ptr()), "opt_edge_smooth")
    return _variant_run(x, H, W, iterations, return_soft, _force_tiled, launch,
                        out_dtype=torch.float16 if to_fp16 else None)


# ---- boundary refinement stage (include/hiseg_refine.h): f32 NCHW logits [N,3,H,W]


def _refine_logits(x: torch.Tensor, what: str):
    _require_gpu(x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{what}: expected [N,3,H,W] logits, got shape {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    N, _, H, W = x.shape
    return x, N, H, W


@dataclass
class EdgeMap:
    """What hiseg_edge_map_fwd leaves for the blend and the backward."""
    x: torch.Tensor                 # the logits [N,3,H,W] f32
    e_raw: torch.Tensor             # [N,H,W]
    mnmx: torch.Tensor              # [2], device
    x_cl: Optional[Act]             # channel-last copy of x in the compute dtype
    probs: Optional[torch.Tensor]   # softmax(x, 1), kept for the backward


def edge_map(x: torch.Tensor, cl_dtype: Optional[torch.dtype] = None, want_probs: bool = False) -> EdgeMap:
    """detect_edges up to the raw edge strength and its batch-global min / max (refinement.py:98-123)."""
    x, N, H, W = _refine_logits(x, "edge_map")
    lib, dev = L.lib(), x.device
    e = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    mnmx = torch.empty(2, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.hiseg_edge_map_ws(N, H, W)), dtype=torch.float32, device=dev)
    probs = torch.empty_like(x) if want_probs else None
    cl = Act.new(N, H, W, 3, cl_dtype, dev, zero=False) if cl_dtype is not None else None
    L.check(lib.hiseg_edge_map_fwd(x.data_ptr(), N, H, W, e.data_ptr(), mnmx.data_ptr(), _ptr(probs),
                                   cl.ptr() if cl is not None else None,
                                   hdtype(cl_dtype) if cl is not None else 0, cl.cstride if cl is not None else 0,
                                   ws.data_ptr(), L.stream_ptr()), "edge_map_fwd")
    return EdgeMap(x, e, mnmx, cl, probs)


def boundary_blend(em: EdgeMap, R: Act, blend: torch.Tensor, want_edges: bool = False):
    """x + blend * R * E (refinement.py:124-147); R: f32 channel-last [N,H,W,3(+pad)], blend: f32 device scalar.
    Returns (out, E or None)."""
    N, _, H, W = em.x.shape
    assert R.dtype == torch.float32 and R.coff == 0 and (R.N, R.H, R.W, R.C) == (N, H, W, 3)
    out = torch.empty_like(em.x)
    E = torch.empty(N, 1, H, W, dtype=torch.float32, device=em.x.device) if want_edges else None
    L.check(L.lib().hiseg_boundary_blend_fwd(em.x.data_ptr(), R.ptr(), R.cstride, em.e_raw.data_ptr(),
                                             em.mnmx.data_ptr(), blend.data_ptr(), N, H, W, out.data_ptr(), _ptr(E),
                                             L.stream_ptr()), "boundary_blend_fwd")
    return out, E


def pack_refine_conv2(w2: torch.Tensor, device) -> torch.Tensor:
    """conv2's weights [32,32,3,3] as bf16 MFMA A-operand fragments [tap][tile][lane][8] (include/hiseg_refine.h):
    element j of lane l of tile t is w2[16 t + (l & 15)][8 (l >> 4) + j][ky][kx]."""
    assert tuple(w2.shape) == (32, 32, 3, 3)
    w = w2.detach().to(device=device, dtype=torch.float32).permute(2, 3, 0, 1).reshape(9, 2, 16, 4, 8)
    return w.permute(0, 1, 3, 2, 4).contiguous().to(torch.bfloat16).reshape(9, 2, 64, 8)


FUSED_REFINE_CALLS = [0]   # launches of the fused kernel (tests: the path taken)


def boundary_refine_fused(em: EdgeMap, blend, w1, s1, t1, w2_frag, s2, t2, w3, b3) -> torch.Tensor:
    """The stage after the edge map in one kernel (eval BatchNorm folded, ReLU, bf16 intermediates)."""
    N, _, H, W = em.x.shape
    out = torch.empty_like(em.x)
    L.check(L.lib().hiseg_boundary_refine_fused(
        em.x.data_ptr(), N, H, W, em.e_raw.data_ptr(), em.mnmx.data_ptr(), blend.data_ptr(), w1.data_ptr(),
        s1.data_ptr(), t1.data_ptr(), w2_frag.data_ptr(), s2.data_ptr(), t2.data_ptr(), w3.data_ptr(), b3.data_ptr(),
        out.data_ptr(), L.stream_ptr()), "boundary_refine_fused")
    FUSED_REFINE_CALLS[0] += 1
    return out


# ------------------------------------------------------- UNet-guided direct 3-class head (include/hiseg_guided_head.h)
def _mask_planes(mask: torch.Tensor):
    """The raw foreground-logit planes of a contiguous f32 [N,C,h,w] map's LAST channel: (first plane, floats
    between two ROIs' planes)."""
    assert mask.dtype == torch.float32 and mask.is_contiguous() and mask.dim() == 4
    return mask[:, mask.shape[1] - 1], mask.shape[1] * mask.shape[2] * mask.shape[3]


def guided_prep(mask: torch.Tensor, dtype: torch.dtype, out: Optional[Act] = None, want_fg_prob: bool = False,
                want_factor: bool = False):
    """One pass over the mask logits (f32 [N,1 or 2,h,w], the foreground channel last): p = sigmoid(m) as a
    one-channel activation in the compute dtype (``out``: a one-channel slice of a wider buffer to write it into),
    optionally p f32 [N,1,h,w] and the guidance factor 0.5 + 0.5 p f32 [N*h*w]."""
    _require_gpu(mask)
    N, _, h, w = mask.shape
    plane, stride = _mask_planes(mask)
    if out is None:
        out = Act.new(N, h, w, 1, dtype, mask.device, zero=False)
    assert out.dtype == dtype and (out.N, out.H, out.W, out.C) == (N, h, w, 1)
    d = L.GuidedPrepDesc()
    d.mask, d.mask_stride, d.N, d.h, d.w, d.dtype = plane, stride, N, h, w, hdtype(dtype)
    d.fgp_c, d.fgp_cstride, d.fgp_coff = out, out.cstride, out.coff
    fg = torch.empty(N, 1, h, w, dtype=torch.float32, device=mask.device) if want_fg_prob else None
    factor = torch.empty(N * h * w, dtype=torch.float32, device=mask.device) if want_factor else None
    d.fg_prob, d.factor = fg, factor
    if N:
        L.check(L.lib().hiseg_guided_prep_fwd(ctypes.byref(d), L.stream_ptr()), "guided_prep")
    return out, fg, factor


def pack_guided_attn(w1: torch.Tensor, dtype: torch.dtype, device):
    """attention_module.0's weight [64, C, 1, 1] -> (W1 transposed f32 [C, 64], the bf16 MFMA A-operand fragments
    [tile][kstep][lane][8] of include/hiseg_guided_head.h, or None where the matrix-core form does not apply)."""
    hid, C = w1.shape[:2]
    w = w1.detach().to(device=device, dtype=torch.float32).reshape(hid, C)
    frag = None
    if dtype == torch.bfloat16 and hid == 64 and C == 256:
        v = w.reshape(4, 16, C // 32, 4, 8)                  # tile, row, kstep, lane group, element
        frag = v.permute(0, 2, 3, 1, 4).contiguous().to(torch.bfloat16).reshape(-1)   # tile, kstep, (lg, row), element
    return w.t().contiguous(), frag


def guided_attn(x: Act, w1t: torch.Tensor, b1, w2, b2, act: int, factor: torch.Tensor, want_att: bool = False,
                w1_frag: Optional[torch.Tensor] = None):
    """sigmoid(w2 . act(W1 x + b1) + b2) per pixel -> (gate = att * factor f32 [P], att f32 [P] or None)."""
    assert x.coff == 0 and x.cstride == x.C
    P = x.N * x.H * x.W
    assert factor.dtype == torch.float32 and factor.numel() == P and tuple(w1t.shape) == (x.C, w2.numel())
    gate = torch.empty(P, dtype=torch.float32, device=x.t.device)
    att = torch.empty(P, dtype=torch.float32, device=x.t.device) if want_att else None
    d = L.GuidedAttnDesc()
    d.dtype, d.x, d.P, d.C, d.hidden = hdtype(x.dtype), x, P, x.C, w2.numel()
    d.w1t, d.b1, d.w2, d.b2 = w1t, b1, w2, b2
    d.act, d.act_beta = int(act), L.act_beta(act)
    d.factor, d.att, d.gate = factor, att, gate
    d.w1_frag = w1_frag if x.dtype == torch.bfloat16 else None
    if P:
        L.check(L.lib().hiseg_guided_attn_fwd(ctypes.byref(d), L.stream_ptr()), "guided_attn")
    return gate, att


def guided_finish(z: Act, w3: torch.Tensor, b3: torch.Tensor, mh: int, mw: int, mask: Optional[torch.Tensor] = None,
                  want_aux: bool = False, want_fg_prob: bool = True):
    """final_classifier.3 (1x1 -> 3) on z, the bilinear resize to (mh, mw) and the aux tensors in one kernel.
    Returns (logits [N,3,mh,mw], aux dict): with ``want_aux`` bg_fg_logits, target_nontarget_logits,
    pretrained_bg_fg_mask and (``want_fg_prob``) fg_prob from the resized mask logits (f32 [N,1 or 2,h,w])."""
    assert z.coff == 0 and z.cstride == z.C and tuple(w3.shape) == (3, z.C)
    dev = z.t.device
    N = z.N
    d = L.GuidedFinishDesc()
    d.dtype, d.z, d.N, d.h, d.w, d.C = hdtype(z.dtype), z, N, z.H, z.W, z.C
    d.w3, d.b3, d.mh, d.mw = w3, b3, int(mh), int(mw)
    logits = torch.empty(N, 3, mh, mw, dtype=torch.float32, device=dev)
    d.logits = logits
    aux = {}
    if want_aux:
        d.mask, d.mask_stride = _mask_planes(mask)
        aux["bg_fg_logits"] = torch.empty(N, 2, mh, mw, dtype=torch.float32, device=dev)
        aux["target_nontarget_logits"] = torch.empty(N, 2, mh, mw, dtype=torch.float32, device=dev)
        aux["pretrained_bg_fg_mask"] = torch.empty(N, 1, mh, mw, dtype=torch.float32, device=dev)
        if want_fg_prob:
            aux["fg_prob"] = torch.empty(N, 1, mh, mw, dtype=torch.float32, device=dev)
            d.fg_prob = aux["fg_prob"]
        d.bg_fg_logits, d.tn_logits, d.mask_out = (aux["bg_fg_logits"], aux["target_nontarget_logits"],
                                                   aux["pretrained_bg_fg_mask"])
    if N:
        L.check(L.lib().hiseg_guided_finish_fwd(ctypes.byref(d), L.stream_ptr()), "guided_finish")
    return logits, aux


# ------------------------------------------------------------------ distance transform (include/hiseg_distance.h)
_DIST_TABLES = {}


def _distance_table(width: int, device) -> torch.Tensor:
    """(1 - sqrt(d2) / width) for d2 in [0, width^2), evaluated on the host in double as the reference evaluates it
    (distance_aware_loss.py:172-174); uploaded once per (width, device)."""
    key = (int(width), str(device))
    t = _DIST_TABLES.get(key)
    if t is None:
        d = torch.sqrt(torch.arange(width * width, dtype=torch.float64))
        t = _DIST_TABLES[key] = (1.0 - d / width).to(device)
    return t


def _distance_targets(mask: torch.Tensor, what: str):
    _require_gpu(mask)
    if mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3:
        raise ValueError(f"{what}: expected a class mask [H,W] or [N,H,W], got shape {tuple(mask.shape)}")
    return mask.to(torch.int64).contiguous()


def boundary_distance(mask: torch.Tensor, max_distance: float = 10.0, *, force_tiled: bool = False,
                      return_d2: bool = False):
    """DistanceTransform.compute_boundary_distance (distance_aware_loss.py:13-50) for class masks [H,W] or [N,H,W]
    with values 0, 1, 2: the exact Euclidean distance to the nearest boundary site clipped to ``max_distance``, as a
    float64 tensor of the mask's shape (``return_d2``: also the int32 squared distance, capped).  The site rule --
    per sample -- and the result for a mask without sites are those of the reference (include/hiseg_distance.h).
    ``max_distance >= max(H, W)`` gives the unclipped transform."""
    squeeze = mask.dim() == 2
    t = _distance_targets(mask, "boundary_distance")
    N, H, W = t.shape
    if not max_distance > 0:
        raise ValueError(f"boundary_distance: max_distance {max_distance}")
    import math
    radius = min(int(math.ceil(max_distance)), max(H, W))
    d2cap = min((radius + 1) ** 2, 2 ** 30) if radius < max(H, W) else 2 ** 30
    lib = L.lib()
    d2 = torch.empty(N, H, W, dtype=torch.int32, device=t.device)
    ws = torch.empty(int(lib.hiseg_distance_ws(N, H, W)), dtype=torch.float32, device=t.device)
    L.check(lib.hiseg_distance_transform(t.data_ptr(), N, H, W, radius, d2cap, int(force_tiled), d2.data_ptr(),
                                         ws.data_ptr(), L.stream_ptr()), "distance_transform")
    dist = torch.sqrt(d2.to(torch.float64)).clamp_(max=float(max_distance))
    if squeeze:
        dist, d2 = dist[0], d2[0]
    return (dist, d2) if return_d2 else dist


def boundary_weight_map(mask: torch.Tensor, boundary_width: int = 5, boundary_weight: float = 2.0,
                        instance_sep_weight: float = 3.0, instance_distances: Optional[torch.Tensor] = None,
                        instance_present: Optional[torch.Tensor] = None, *,
                        dev_weights: Optional[torch.Tensor] = None, force_tiled: bool = False):
    """BoundaryWeightGenerator.generate_weights (distance_aware_loss.py:147-185) for class masks [N,H,W] (or [H,W]).
    Returns (weights f32, d2 int32) of the mask's shape: d2 is the squared distance to the nearest boundary site
    capped at boundary_width^2.  ``instance_distances`` f32 [N,H,W] with ``instance_present`` uint8 [N] (all present
    when None) multiplies the weight by instance_sep_weight where the map is < 50.  ``dev_weights``: device float
    [2] read in place of the two weight arguments (AdaptiveBoundaryLoss)."""
    squeeze = mask.dim() == 2
    t = _distance_targets(mask, "boundary_weight_map")
    N, H, W = t.shape
    width = int(boundary_width)
    if width < 1:
        raise ValueError(f"boundary_weight_map: boundary_width {boundary_width}")
    lib, dev = L.lib(), t.device
    inst = pres = None
    if instance_distances is not None:
        _require_gpu(instance_distances, instance_present)
        inst = instance_distances.to(torch.float32).reshape(N, H, W).contiguous()
        pres = (torch.ones(N, dtype=torch.uint8, device=dev) if instance_present is None
                else instance_present.to(torch.uint8).reshape(N).contiguous())
    if dev_weights is not None:
        _require_gpu(dev_weights)
        assert dev_weights.dtype == torch.float32 and dev_weights.numel() == 2 and dev_weights.is_contiguous()
    d2 = torch.empty(N, H, W, dtype=torch.int32, device=dev)
    w = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.hiseg_distance_ws(N, H, W)), dtype=torch.float32, device=dev)
    table = _distance_table(width, dev)
    L.check(lib.hiseg_distance_weight_map(t.data_ptr(), N, H, W, width, table.data_ptr(), float(boundary_weight),
                                          float(instance_sep_weight), _ptr(dev_weights), _ptr(inst), _ptr(pres),
                                          int(force_tiled), d2.data_ptr(), w.data_ptr(), ws.data_ptr(),
                                          L.stream_ptr()), "distance_weight_map")
    if squeeze:
        w, d2 = w[0], d2[0]
    return w, d2


# ------------------------------------------------------------ full-frame instance composition (include/hiseg_compose.h)
def _roi_bits(src: torch.Tensor, channels: int, what: str):
    _require_gpu(src)
    if src.dim() != 4 or src.shape[1] != channels:
        raise ValueError(f"{what}: expected [N,{channels},mh,mw], got shape {tuple(src.shape)}")
    src = src.to(torch.float32).contiguous()
    N, _, mh, mw = src.shape
    wpr = L.lib().hiseg_compose_words_per_row(mw)
    bits = torch.empty(N, mh, wpr, dtype=torch.int32, device=src.device)
    score = torch.empty(N, dtype=torch.float32, device=src.device)
    count = torch.empty(N, dtype=torch.int32, device=src.device)
    return src, N, mh, mw, bits, score, count


def roi_mask_classify(logits: torch.Tensor, score_threshold: float = 0.5):
    """Logits f32 [N,3,mh,mw] -> (bits int32 [N,mh,(mw+31)//32], score f32 [N], count int32 [N]): the target mask
    (first-maximum argmax == 1 and softmax maximum > score_threshold) bit-packed, its mean confidence and its size."""
    x, N, mh, mw, bits, score, count = _roi_bits(logits, 3, "roi_mask_classify")
    L.check(L.lib().hiseg_roi_mask_classify_fwd(_ptr(x) if N else None, N, mh, mw, float(score_threshold),
                                                bits.data_ptr(), score.data_ptr(), count.data_ptr(), L.stream_ptr()),
            "roi_mask_classify")
    return bits, score, count


def roi_mask_pack(masks: torch.Tensor):
    """instance_masks f32 [N,1,mh,mw] -> (bits, score, count) as roi_mask_classify: set where > 0.5, score 1 where
    any pixel is set, else 0."""
    x, N, mh, mw, bits, score, count = _roi_bits(masks, 1, "roi_mask_pack")
    L.check(L.lib().hiseg_roi_mask_pack_fwd(_ptr(x) if N else None, N, mh, mw, bits.data_ptr(), score.data_ptr(),
                                            count.data_ptr(), L.stream_ptr()), "roi_mask_pack")
    return bits, score, count


def compose_instance_map(bits: torch.Tensor, score: torch.Tensor, rois: torch.Tensor, frame_size, mask_width: int):
    """Packed masks, scores and rois f32 [N,5] -> label int32 [B,H,W] for frame_size = (B, H, W): 0 is background,
    k + 1 means ROI k owns the pixel (the highest ROI index of the frame whose nearest-resized mask is set there)."""
    _require_gpu(bits, score, rois)
    B, H, W = (int(v) for v in frame_size)
    if bits.dim() != 3 or bits.dtype != torch.int32:
        raise ValueError(f"compose_instance_map: expected int32 bits [N,mh,words], got {bits.dtype} "
                         f"{tuple(bits.shape)}")
    N, mh, wpr = bits.shape
    mw = int(mask_width)
    if wpr != L.lib().hiseg_compose_words_per_row(mw):
        raise ValueError(f"compose_instance_map: {wpr} words per row do not hold a mask {mw} wide")
    if tuple(rois.shape) != (N, 5) or tuple(score.shape) != (N,):
        raise ValueError(f"compose_instance_map: {N} masks, rois {tuple(rois.shape)}, score {tuple(score.shape)}")
    bits, score = bits.contiguous(), score.to(torch.float32).contiguous()
    rois = rois.to(torch.float32).contiguous()
    label = torch.empty(B, H, W, dtype=torch.int32, device=bits.device)
    L.check(L.lib().hiseg_instance_map_fwd(_ptr(bits) if N else None, _ptr(score) if N else None,
                                           _ptr(rois) if N else None, N, mh, mw, B, H, W, label.data_ptr(),
                                           L.stream_ptr()), "instance_map")
    return label


def instance_overlay(label: torch.Tensor, image: torch.Tensor, colors: torch.Tensor, alpha: float = 0.5):
    """label int32 [B,H,W], image uint8 [B,H,W,3], colors uint8 [N,3] -> uint8 [B,H,W,3]: cv2.addWeighted(image,
    1 - alpha, colour of the owner (0 where there is none), alpha, 0)."""
    _require_gpu(label, image, colors)
    if label.dim() != 3 or label.dtype != torch.int32:
        raise ValueError(f"instance_overlay: expected an int32 label map [B,H,W], got {label.dtype} "
                         f"{tuple(label.shape)}")
    B, H, W = label.shape
    if tuple(image.shape) != (B, H, W, 3) or image.dtype != torch.uint8:
        raise ValueError(f"instance_overlay: expected a uint8 image {(B, H, W, 3)}, got {image.dtype} "
                         f"{tuple(image.shape)}")
    if colors.dim() != 2 or colors.shape[1] != 3 or colors.dtype != torch.uint8:
        raise ValueError(f"instance_overlay: expected uint8 colors [N,3], got {colors.dtype} {tuple(colors.shape)}")
    label, image, colors = label.contiguous(), image.contiguous(), colors.contiguous()
    if label.data_ptr() % 16:    # a view into a larger buffer: the kernel reads labels four to a 16-byte load
        label = label.clone()
    if image.data_ptr() % 4:
        image = image.clone()
    N = colors.shape[0]
    out = torch.empty_like(image)
    L.check(L.lib().hiseg_instance_overlay_fwd(label.data_ptr(), image.data_ptr(), _ptr(colors) if N else None, N, B,
                                               H, W, float(alpha), out.data_ptr(), L.stream_ptr()), "instance_overlay")
    return out
