"""Execution of the RGB hierarchical path on libhiseg kernels.

The modules in :mod:`hiseg.model` / :mod:`hiseg.layers` / :mod:`hiseg.effunet` only hold
parameters.  This module walks them in the reference's forward order and issues one
libhiseg call per fused layer:

* every Conv2d(+BatchNorm2d eval)(+activation)(+residual add)(+gate multiply) is ONE
  implicit-GEMM launch (hiseg_conv2d_fwd) with BN/bias folded into a per-channel affine;
* concatenations (feature_combiner input, EnhancedUNet / smp decoder skips) never exist in
  memory: the conv loader reads its K range from two sources (and upsamples source A ×2 for
  the smp decoder);
* the trainable 1→2 output_conv of the pretrained-UNet wrapper is fused into the RoIAlign
  gather, the whole upsample_bg_fg branch into the hierarchical combine kernel, the target
  branch's last 1×1 into the epilogue of the conv before it (or the combine kernel where that
  conv has no such form) and its spatial-attention multiply into the ConvTranspose's loader.

Packed weights ("plans") are cached per model, compute dtype and device and rebuilt when
any parameter or buffer changes (tensor version counters).  Activations are NHWC.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .effunet import DepthwiseSeparableConv, InvertedResidual
from .layers import LayerNorm2d, Swish
from .ops import Act, round_up

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU = L.ACT_NONE, L.ACT_RELU, L.ACT_SIGMOID, L.ACT_SILU
ACT_GELU, ACT_SWISH = L.ACT_GELU, L.ACT_SWISH


# ------------------------------------------------------------------------------------ plans
def act_code(m: nn.Module) -> int:
    """The hiseg activation code of an activation module (advanced/activation_utils.py:71-101).
    Swish(beta != 1) returns an L.ActCode carrying beta."""
    if isinstance(m, nn.ReLU):
        return ACT_RELU
    if isinstance(m, nn.SiLU):
        return ACT_SILU
    if isinstance(m, Swish):
        return ACT_SILU if float(m.beta) == 1.0 else L.ActCode(ACT_SWISH, float(m.beta))
    if isinstance(m, nn.GELU):
        if getattr(m, "approximate", "none") != "none":
            raise NotImplementedError("tanh-approximate GELU is not in the reference's activation factory")
        return ACT_GELU
    if isinstance(m, nn.Sigmoid):
        return ACT_SIGMOID
    if isinstance(m, nn.Identity):
        return ACT_NONE
    raise NotImplementedError(f"activation {type(m).__name__} is not in the reference's activation factory")


def _bn(m: Optional[nn.Module]):
    if m is None:
        return None
    if isinstance(m, nn.BatchNorm2d):
        if m.training:
            raise NotImplementedError("batch-statistics BatchNorm (train mode) is not on the hiseg inference path")
        return m
    if isinstance(m, LayerNorm2d):
        raise AssertionError("LayerNorm2d has per-sample statistics and cannot be folded into a conv plan (use cna)")
    raise NotImplementedError(f"normalisation {type(m).__name__}")


def _signature(tensors):
    return tuple((t.data_ptr(), t._version) for t in tensors if t is not None)


def _bn_tensors(bn):
    if bn is None:
        return ()
    return (getattr(bn, "weight", None), getattr(bn, "bias", None), getattr(bn, "running_mean", None),
            getattr(bn, "running_var", None))


class Ctx:
    """Per-forward context: compute dtype, device and the model's plan cache.

    Every plan records the (storage, version) of the tensors it was packed from and is rebuilt only when one
    of them changed -- so a training step that updates some parameters (or train-mode BN running statistics)
    re-packs just those layers, not the whole model (the frozen encoder of the distillation student, the
    teacher)."""

    def __init__(self, root: nn.Module, dtype: torch.dtype, device: torch.device):
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"hiseg compute dtype must be float32 or bfloat16, got {dtype}")
        self.dtype, self.device = dtype, device
        cache = root.__dict__.get("_hiseg_plans")
        if cache is None or cache["dtype"] != dtype or cache["device"] != device:
            cache = {"dtype": dtype, "device": device, "plans": {}}
            root.__dict__["_hiseg_plans"] = cache
        self.plans: Dict = cache["plans"]

    def _get(self, key, build, deps=()):
        sig = _signature(deps)
        ent = self.plans.get(key)
        if ent is None or ent[0] != sig:
            ent = (sig, build())
            self.plans[key] = ent
        return ent[1]

    def conv(self, conv: nn.Conv2d, bn=None, act: int = ACT_NONE, split=None) -> ops.ConvPlan:
        def build():
            assert conv.groups == 1 and conv.dilation in ((1, 1), 1)
            assert conv.kernel_size[0] == conv.kernel_size[1] and conv.stride[0] == conv.stride[1]
            return ops.pack_conv(conv.weight, conv.bias, _bn(bn), act, self.dtype, self.device,
                                 stride=conv.stride[0], pad=conv.padding[0], split=split)
        return self._get(("conv", id(conv), act, split), build, (conv.weight, conv.bias) + _bn_tensors(bn))

    def convT(self, conv: nn.ConvTranspose2d, bn=None, act: int = ACT_NONE) -> ops.ConvPlan:
        def build():
            assert conv.kernel_size == (2, 2) and conv.stride == (2, 2) and conv.padding == (0, 0)
            return ops.pack_convT2x2(conv.weight, conv.bias, _bn(bn), act, self.dtype, self.device)
        return self._get(("convT", id(conv), act), build, (conv.weight, conv.bias) + _bn_tensors(bn))

    def f32(self, t: torch.Tensor, shape=None) -> torch.Tensor:
        def build():
            v = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
            return v.view(shape) if shape is not None else v
        return self._get(("f32", id(t), shape), build, (t,))

    def affine(self, key, cout, bias, bn):
        def build():
            s, h = ops.fold_affine(cout, bias, _bn(bn), self.device)
            return s.contiguous(), h.contiguous()
        return self._get(("aff", key), build, (bias,) + _bn_tensors(bn))

    def dw(self, conv: nn.Conv2d, bn):
        def build():
            c, _, k, _ = conv.weight.shape
            w = conv.weight.detach().float().to(self.device).view(c, k * k).t().contiguous()
            s, h = ops.fold_affine(c, conv.bias, _bn(bn), self.device)
            return w, s.contiguous(), h.contiguous(), k, conv.stride[0]
        return self._get(("dw", id(conv)), build, (conv.weight, conv.bias) + _bn_tensors(bn))


def cna(E: Ctx, conv: nn.Module, norm: Optional[nn.Module], act: int, x: Act, xb: Optional[Act] = None, *,
        split=None, residual: Optional[Act] = None, out: Optional[Act] = None, convT: bool = False) -> Act:
    """conv -> norm -> (+ residual) -> act.  Eval BatchNorm (or no norm) folds into the conv launch;
    LayerNorm2d (model.py:18-38) needs the conv output's per-sample statistics first: raw conv (+ bias),
    then ops.layernorm2d (statistics + one apply pass with residual and activation)."""
    if isinstance(norm, LayerNorm2d):
        plan = E.convT(conv, None, ACT_NONE) if convT else E.conv(conv, None, ACT_NONE, split=split)
        z = ops.conv2d(plan, x, xb)
        C = z.C
        return ops.layernorm2d(z, E.f32(norm.weight, (C,)), E.f32(norm.bias, (C,)), norm.eps, act,
                               residual=residual, out=out)
    plan = E.convT(conv, norm, act) if convT else E.conv(conv, norm, act, split=split)
    return ops.conv2d(plan, x, xb, residual=residual, out=out)


def _check_input(x: torch.Tensor, what: str):
    if not x.is_cuda:
        raise RuntimeError(f"{what}: hiseg runs on the GPU only (got a CPU tensor); there is no CPU fallback")


# ------------------------------------------------------------------------------------ blocks
# residual_block takes the one-launch form of a 64-channel block (ops.resblock) where the library has it; False runs
# every block as two launches (the tests' bit-for-bit comparison; not a setting of the product)
RESBLOCK_FUSED = True
# unet_logit_iter hands the raw images to the EfficientNet stem where the library normalises inside that layer
# (ops.stem_raw); False runs input_norm + stem (the tests' bit-for-bit comparison; not a setting of the product)
STEM_RAW = True


def _block_acts(blk: nn.Module) -> Tuple[int, int]:
    return (act_code(blk.activation1 if hasattr(blk, "activation1") else blk.activation),
            act_code(blk.activation2 if hasattr(blk, "activation2") else blk.activation))


def gated_block_ok(E: Ctx, blk: nn.Module, x: Act, gate: torch.Tensor, head2: ops.Head2) -> bool:
    """Whether both convs of a ResidualBlock whose input is x * gate[image][channel] (and whose output feeds only
    ``head2``) apply the gate where they read x -- conv1 in its loader, conv2 on its residual.  All or nothing: if
    either conv lacks the form the gated tensor has to exist anyway."""
    if isinstance(blk.norm1, LayerNorm2d) or isinstance(blk.norm2, LayerNorm2d) or x.dtype != torch.bfloat16:
        return False
    a1, a2 = _block_acts(blk)
    p1, p2 = E.conv(blk.conv1, blk.norm1, a1), E.conv(blk.conv2, blk.norm2, a2)
    if p1.cout != x.C or p2.cout != x.C:   # (conv2's input is conv1's output: x stands in for its shape below)
        return False
    return ops._fused_ok(p1, x, None, None, None, None, None, None, x.dtype, 1, a_gate=gate) and \
        ops._fused_ok(p2, x, None, x, None, None, None, head2, x.dtype, 1, res_gate=gate)


def residual_block(E: Ctx, blk: nn.Module, x: Act, out: Optional[Act] = None,
                   head2: Optional[ops.Head2] = None, in_gate: Optional[torch.Tensor] = None) -> Optional[Act]:
    """ResidualBlock (refinement.py:31-55 / unet.py:35-58): one launch for the 64-channel bf16 form
    (ops.resblock), else two fused launches.  ``head2``: a 1x1 -> 2 that alone
    consumes the block's output (ops.Head2); returns None when conv2's epilogue applied it.  ``in_gate`` (f32
    [N, C]): the block's input is x * in_gate[image][channel], applied by both convs as they read x (the caller
    checked gated_block_ok)."""
    a1, a2 = _block_acts(blk)
    if RESBLOCK_FUSED and in_gate is None and head2 is None and out is None and x.C == 64 and \
            x.dtype == torch.bfloat16 and not isinstance(blk.norm1, LayerNorm2d) and \
            not isinstance(blk.norm2, LayerNorm2d):
        # the 64-channel blocks: one launch, the intermediate stays on the compute unit (the same bits)
        y = ops.resblock(E.conv(blk.conv1, blk.norm1, a1), E.conv(blk.conv2, blk.norm2, a2), x)
        if y is not None:
            return y
    if in_gate is not None:
        h = ops.conv2d(E.conv(blk.conv1, blk.norm1, a1), x, a_gate=in_gate)
        return ops.conv2d(E.conv(blk.conv2, blk.norm2, a2), h, residual=x, res_gate=in_gate, head2=head2)
    h = cna(E, blk.conv1, blk.norm1, a1, x)
    if head2 is not None and out is None and not isinstance(blk.norm2, LayerNorm2d):
        return ops.conv2d(E.conv(blk.conv2, blk.norm2, a2), h, residual=x, head2=head2)
    return cna(E, blk.conv2, blk.norm2, a2, h, residual=x, out=out)


def rgb_feature_extractor(E: Ctx, seq: nn.Sequential, x: Act, out: Optional[Act] = None) -> Act:
    """hierarchical_segmentation_rgb.py:657-673.  ``out``: where the last layer writes."""
    h = cna(E, seq[0], seq[1], act_code(seq[2]), x)
    h = residual_block(E, seq[3], h)
    h = cna(E, seq[4], seq[5], act_code(seq[6]), h)
    h = residual_block(E, seq[7], h)
    h = cna(E, seq[8], seq[9], act_code(seq[10]), h)
    h = residual_block(E, seq[11], h)
    return cna(E, seq[12], seq[13], act_code(seq[14]), h, out=out)


def rgb_extractor_plain(E: Ctx, seq: nn.Sequential, x: Act) -> Act:
    """RGBFeatureExtractor.features (hierarchical_segmentation_rgb.py:253-281): conv + norm + act per layer, a
    residual block after every layer but the first."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        x = cna(E, mods[i], mods[i + 1], act_code(mods[i + 2]), x)
        i += 3
        if i < len(mods) and not isinstance(mods[i], nn.Conv2d):
            x = residual_block(E, mods[i], x)
            i += 1
    return x


def enhanced_unet(E: Ctx, u: nn.Module, x: Act) -> Tuple[Act, Act]:
    """EnhancedUNet.forward (hierarchical_segmentation_unet.py:375-417).

    Returns the 2-channel logits twice: f32 [N,h,w,2] (combine input) and compute-dtype
    channel-padded (fg_gate input), both written by the same final launch.
    """
    d = u.depth
    if x.H % (1 << (d - 1)) or x.W % (1 << (d - 1)):
        raise NotImplementedError(
            f"ROI size {x.H}x{x.W} is not divisible by 2^{d - 1}: the reference's bilinear resize of the up-conv "
            "output (unet.py:408) is then not the identity; not supported on the hiseg path")
    feats = []
    for i in range(d):
        enc = u.encoders[i]
        if i == 0:
            x = cna(E, enc[0], enc[1], act_code(enc[2]), x)
            x = residual_block(E, enc[3], x)
            x = residual_block(E, enc[4], x)
        else:
            x = residual_block(E, enc[0], x)
            x = residual_block(E, enc[1], x)
            x = cna(E, enc[2], enc[3], act_code(enc[4]), x)
        feats.append(x)
        if i < d - 1:
            x = ops.maxpool2x2(x)
    b = u.bottleneck
    a = residual_block(E, b[0], x)
    a = residual_block(E, b[1], a)
    a = cna(E, b[2], b[3], act_code(b[4]), a)
    att = ops.conv2d(E.conv(b[5], None, ACT_SIGMOID), a)
    x = ops.conv2d(E.conv(u.bottleneck_conv), x, mul=att)
    for i in range(d - 1):
        up = ops.conv2d(E.convT(u.upconvs[i]), x)
        skip = feats[d - 2 - i]
        dec = u.decoders[i]
        x = cna(E, dec[0], dec[1], act_code(dec[2]), up, skip, split=(up.C, skip.C))
        x = residual_block(E, dec[3], x)
        x = residual_block(E, dec[4], x)
    f = u.final
    h = cna(E, f[0], f[1], act_code(f[2]), x)
    low = Act.new(h.N, h.H, h.W, 2, torch.float32, E.device, cpad=2, zero=False)
    low_t = Act.new(h.N, h.H, h.W, 2, E.dtype, E.device)
    ops.conv2d(E.conv(f[3]), h, out=low, out2=low_t)
    return low, low_t


def hier_head(E: Ctx, head: nn.Module, feat: Act, aux: str) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """RefinedHierarchicalSegmentationHead.forward (refinement.py:734-804) over
    ExtendedHierarchicalSegmentationHeadUNetV2.forward (:550-606).  A HierarchicalSegmentationHeadUNetV2 (unet.py
    :775-845, the plain RGB model's head without a refinement flag) is the same walk with no refiner and no aux
    branch, and its aux dict has no ``shared_features``."""
    bh = getattr(head, "base_head", head)
    plain = bh is head
    sf = bh.shared_features
    s = cna(E, sf[0], sf[1], act_code(sf[2]), feat)
    s = residual_block(E, sf[4], s)
    s = residual_block(E, sf[6], s)
    low, low_t = enhanced_unet(E, bh.bg_vs_fg_unet, s)
    fg = bh.fg_gate
    g = cna(E, fg[0], None, act_code(fg[1]), low_t)
    g = cna(E, fg[3], None, act_code(fg[4]), g)
    gated = ops.conv2d(E.conv(fg[5], None, ACT_SIGMOID), g, mul=s)
    tb = bh.target_vs_nontarget_branch
    if bh.use_attention_module:
        t = residual_block(E, tb[0], gated)
        if isinstance(tb[4], LayerNorm2d):
            t = ops.attn_spatial(t, E.f32(tb[1].conv.weight))
            t = cna(E, tb[3], tb[4], act_code(tb[5]), t, convT=True)
        else:   # the attention multiply rides in the ConvTranspose's loader (ops.conv2d px_scale)
            att = ops.attn_map(t, E.f32(tb[1].conv.weight))
            t = ops.conv2d(E.convT(tb[3], tb[4], act_code(tb[5])), t, px_scale=att)
        ca = tb[6]
        gate = ops.se_gate(t, E.f32(ca.fc1.weight, (ca.fc1.out_channels, ca.fc1.in_channels)), None,
                           E.f32(ca.fc2.weight, (ca.fc2.out_channels, ca.fc2.in_channels)), None,
                           act_code(ca.activation))
        blk, last = tb[8], tb[9]
    else:
        t = residual_block(E, tb[0], gated)
        t = cna(E, tb[2], tb[3], act_code(tb[4]), t, convT=True)
        blk, last = tb[6], tb[7]
        gate = None
    # the branch's last residual block feeds only its last 1x1 (-> 2), which rides in conv2's epilogue where the
    # layer has that form (ops.Head2): t is then None and h2.out the two target logits per pixel
    h2 = ops.Head2(E.f32(last.weight, (2, last.in_channels)), E.f32(last.bias))
    # the channel-attention multiply (attention_modules.py:64) rides in the two convs that alone read its result
    # where both have that form; otherwise the gated tensor is written by its own pass
    if gate is not None and not gated_block_ok(E, blk, t, gate, h2):
        t, gate = ops.channel_scale(t, gate), None
    tH, tW = t.H, t.W
    t = residual_block(E, blk, t, head2=h2, in_gate=gate)
    mh, mw = bh.mask_height, bh.mask_width
    assert (tH, tW) == (2 * low.H, 2 * low.W)
    up = bh.upsample_bg_fg
    per_sample = isinstance(up[1], LayerNorm2d)
    if per_sample:   # LayerNorm2d over the ConvTranspose output: per-ROI tables [N][32]
        ut_s = torch.empty(low.N * 32, dtype=torch.float32, device=E.device)
        ut_h = torch.empty_like(ut_s)
        L.check(L.lib().hiseg_ubf_ln_tables(low.t.data_ptr(), low.N, low.H, low.W, E.f32(up[0].weight).data_ptr(),
                                            E.f32(up[0].bias).data_ptr(), E.f32(up[1].weight, (32,)).data_ptr(),
                                            E.f32(up[1].bias, (32,)).data_ptr(), float(up[1].eps), 1, None, None,
                                            ut_s.data_ptr(), ut_h.data_ptr(), L.stream_ptr()), "ubf_ln_tables")
    else:
        ut_s, ut_h = E.affine(("ut", id(up[0])), up[0].out_channels, up[0].bias, up[1])
    want = aux == "full"
    if (mh, mw) == (tH, tW):
        logits, bgfg, tn = ops.hier_combine(
            low.t, low.N, low.H, low.W, t, E.f32(up[0].weight), ut_s, ut_h, act_code(up[2]),
            E.f32(up[3].weight, (2, up[3].in_channels)), E.f32(up[3].bias),
            h2.w, h2.b, want, per_sample=per_sample, tn2=h2.out)
    else:   # the reference resizes both branches from 2 x ROI to the mask size, then combines (refinement.py:559-596)
        tn2 = h2.out
        if t is not None:   # the branch's last conv had no Head2 epilogue: its 1x1 first, two f32 logits per pixel
            tq = Act.new(t.N, tH, tW, 2, torch.float32, E.device, cpad=2, zero=False)
            ops.conv2d(E.conv(last), t, out=tq)
            tn2 = tq.t
        logits, bgfg, tn = ops.hier_combine_resize(
            low.t, low.N, low.H, low.W, tn2, E.f32(up[0].weight), ut_s, ut_h, act_code(up[2]),
            E.f32(up[3].weight, (2, up[3].in_channels)), E.f32(up[3].bias), mh, mw, want, per_sample=per_sample)
    if not plain and head.use_boundary_refinement:   # refines the returned masks only; the aux tensors stay (refinement.py:767-769)
        logits = boundary_refine(E, head.boundary_refiner, logits)
    auxd: Dict[str, torch.Tensor] = {}
    if not want:
        return logits, auxd
    fg_att = ops.conv2d(E.conv(fg[5], None, ACT_SIGMOID), g)
    auxd.update({
        "bg_fg_logits": bgfg, "bg_fg_logits_low": low.to_nchw(), "target_nontarget_logits": tn,
        "fg_attention": fg_att.to_nchw(),
    })
    if plain:
        return logits, auxd
    auxd["shared_features"] = s.to_nchw()
    lib = L.lib()
    if head.use_contour_detection:
        cb = head.contour_branch.contour_branch
        c = cna(E, cb[0], cb[1], act_code(cb[2]), s)
        c = cna(E, cb[3], cb[4], act_code(cb[5]), c)
        cm = Act.new(c.N, c.H, c.W, 1, torch.float32, E.device, cpad=1, zero=False)
        ops.conv2d(E.conv(cb[6], None, ACT_SIGMOID), c, out=cm)
        auxd["contours"] = _resize(cm.t.view(c.N, 1, c.H, c.W), mh, mw, lib)
    if head.use_distance_transform:
        dd = head.distance_decoder
        dh = dd.distance_head
        dx = cna(E, dh[0], dh[1], act_code(dh[2]), s)
        dx = residual_block(E, dh[3], dx)
        dm = Act.new(dx.N, dx.H, dx.W, 1, torch.float32, E.device, cpad=1, zero=False)
        ops.conv2d(E.conv(dh[4]), dx, out=dm)
        dmap = dm.t.view(dx.N, 1, dx.H, dx.W)
        dmask = torch.empty_like(dmap)
        L.check(lib.hiseg_distance_mask_fwd(dmap.data_ptr(), dmap.numel(), E.f32(dd.threshold).data_ptr(),
                                            dmask.data_ptr(), L.stream_ptr()), "distance_mask")
        auxd["distance_mask"] = _resize(dmask, mh, mw, lib)
        auxd["distance_map"] = _resize(dmap, mh, mw, lib)
    return logits, auxd


# A/B switches of the guided head's fused forms (tests, tools/guided_head_bench.py): False takes the explicit
# fall-back -- a materialised 257-channel input_adjust input / a pixel_scale pass before final_classifier.0.
GUIDED_FUSE_SRC_B = True
GUIDED_FUSE_PX_SCALE = True


def guided_head(E: Ctx, head: nn.Module, feats: Act, mask: torch.Tensor, aux: str, feats_into=None):
    """PretrainedUNetGuidedSegmentationHead.forward (rgb.py:123-218), eval mode.  ``mask``: f32 [N, 1 or 2, h, w],
    the raw foreground logit in its last channel, at the features' size.  ``feats_into``: the explicit fall-back of
    the source-B form -- a callable taking the 256-channel slice of the 257-channel buffer and writing the features
    there (``feats`` is then None)."""
    if head.training:
        raise NotImplementedError("PretrainedUNetGuidedSegmentationHead is inference only on the hiseg path; "
                                  "call .eval()")
    want = aux == "full"
    att_on = head.use_attention_module
    N, _, h, w = mask.shape
    mh, mw = head.mask_height, head.mask_width
    same = (mh, mw) == (h, w)
    ia = head.input_adjust
    cin = ia.in_channels - 1
    if feats_into is None:   # fg_prob is loader source B of input_adjust: the 257-channel tensor never exists
        assert (feats.N, feats.H, feats.W, feats.C) == (N, h, w, cin), "features and mask sizes differ"
        fgp, fg_low, factor = ops.guided_prep(mask, E.dtype, want_fg_prob=want and same, want_factor=att_on)
        x = ops.conv2d(E.conv(ia, split=(cin, 1)), feats, fgp)
    else:
        comb = Act.new(N, h, w, cin + 1, E.dtype, E.device, zero=False)
        feats_into(comb.slice(0, cin))
        _, fg_low, factor = ops.guided_prep(mask, E.dtype, out=comb.slice(cin, 1), want_fg_prob=want and same,
                                            want_factor=att_on)
        x = ops.conv2d(E.conv(ia), comb)
    fp = head.feature_processor
    y = cna(E, fp[0], fp[1], act_code(fp[2]), x)
    y = residual_block(E, fp[4], y)
    y = residual_block(E, fp[6], y)
    fc = head.final_classifier
    att = None
    if att_on:
        am = head.attention_module
        if am[0].out_channels != 64 or am[0].in_channels != y.C:
            raise NotImplementedError(f"the guided head's attention kernel is built for 64 hidden units "
                                      f"(mid_channels 256), got {am[0].out_channels}")
        w1t, frag = E._get(("guided_attn", id(am[0])), lambda: ops.pack_guided_attn(am[0].weight, E.dtype, E.device),
                           (am[0].weight,))
        gate, att = ops.guided_attn(y, w1t, E.f32(am[0].bias), E.f32(am[2].weight, (64,)), E.f32(am[2].bias),
                                    act_code(am[1]), factor, want_att=want, w1_frag=frag)
        if isinstance(fc[1], LayerNorm2d) or not GUIDED_FUSE_PX_SCALE:
            z = cna(E, fc[0], fc[1], act_code(fc[2]), ops.pixel_scale(y, gate))
        else:   # the gate multiply rides in final_classifier.0's loader where the layer has that form
            z = ops.conv2d(E.conv(fc[0], fc[1], act_code(fc[2])), y, px_scale=gate)
    else:
        z = cna(E, fc[0], fc[1], act_code(fc[2]), y)
    logits, auxd = ops.guided_finish(z, E.f32(fc[3].weight, (3, fc[3].in_channels)), E.f32(fc[3].bias), mh, mw,
                                     mask=mask, want_aux=want, want_fg_prob=not same)
    if not want:
        return logits, {}
    if same:   # nothing is resized: fg_prob is the ROI-size one (rgb.py:143, :187-194)
        auxd["fg_prob"] = fg_low
    auxd["attention"] = att.view(N, 1, h, w) if att is not None else None
    return logits, auxd


def refine_fused_eligible(mod: nn.Module, dtype: torch.dtype) -> bool:
    """Whether the fused inference kernel of include/hiseg_refine.h covers this module: bf16 compute dtype, eval
    mode, both norms BatchNorm (folded), both activations ReLU, 3 -> 32 -> 32 -> 3 channels with biases."""
    import os
    ec = mod.edge_conv
    return (dtype == torch.bfloat16 and not mod.training and os.environ.get("HISEG_REFINE_FUSED", "1") != "0"
            and isinstance(ec[1], nn.BatchNorm2d) and isinstance(ec[4], nn.BatchNorm2d)
            and isinstance(ec[2], nn.ReLU) and isinstance(ec[5], nn.ReLU)
            and tuple(ec[0].weight.shape) == (32, 3, 3, 3) and tuple(ec[3].weight.shape) == (32, 32, 3, 3)
            and tuple(ec[6].weight.shape) == (3, 32, 1, 1) and ec[6].bias is not None)


def boundary_refine(E: Ctx, mod: nn.Module, logits: torch.Tensor, want_edges: bool = False):
    """BoundaryRefinementModule.forward (refinement.py:131-149), eval mode.  The common case -- bf16 compute dtype,
    both norms BatchNorm, ReLU, 32 edge channels -- is the edge pass plus ONE fused kernel (refine_fused_eligible;
    HISEG_REFINE_FUSED=0 turns it off for A/B timing).  Anything else: the edge pass also writes the channel-last
    copy of the logits the convs read; conv + norm + act launches as everywhere (cna), the last 1x1 into an f32
    buffer; one blend pass.  ``want_edges``: also return the normalised edge map [N,1,H,W] (conv chain only)."""
    if mod.training:
        raise NotImplementedError("hiseg executes the inference (eval-mode) forward; call .eval()")
    ec = mod.edge_conv
    if not want_edges and refine_fused_eligible(mod, E.dtype):
        em = ops.edge_map(logits)
        s1, t1 = E.affine(("refine1", id(ec[0])), 32, ec[0].bias, ec[1])
        s2, t2 = E.affine(("refine2", id(ec[3])), 32, ec[3].bias, ec[4])
        w2f = E._get(("refine_w2", id(ec[3])), lambda: ops.pack_refine_conv2(ec[3].weight, E.device),
                     (ec[3].weight,))
        return ops.boundary_refine_fused(em, E.f32(mod.blend_weight, (1,)), E.f32(ec[0].weight, (32, 27)), s1, t1,
                                         w2f, s2, t2, E.f32(ec[6].weight, (3, 32)), E.f32(ec[6].bias))
    em = ops.edge_map(logits, cl_dtype=E.dtype)
    h = cna(E, ec[0], ec[1], act_code(ec[2]), em.x_cl)
    h = cna(E, ec[3], ec[4], act_code(ec[5]), h)
    R = Act.new(h.N, h.H, h.W, 3, torch.float32, E.device)
    ops.conv2d(E.conv(ec[6]), h, out=R)
    out, edges = ops.boundary_blend(em, R, E.f32(mod.blend_weight, (1,)), want_edges)
    return (out, edges) if want_edges else out


def _resize(x: torch.Tensor, H: int, W: int, lib) -> torch.Tensor:
    N, C, h, w = x.shape
    if (h, w) == (H, W):
        return x
    out = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    L.check(lib.hiseg_resize_bilinear_fwd(x.data_ptr(), N * C, h, w, out.data_ptr(), H, W, L.stream_ptr()),
            "resize_bilinear")
    return out


# ------------------------------------------------------------------------------------ full-image UNet
def _se(E: Ctx, se: nn.Module, h: Act) -> torch.Tensor:
    rd, c = se.conv_reduce.out_channels, se.conv_reduce.in_channels
    return ops.se_gate(h, E.f32(se.conv_reduce.weight, (rd, c)), E.f32(se.conv_reduce.bias),
                       E.f32(se.conv_expand.weight, (c, rd)), E.f32(se.conv_expand.bias), ACT_SILU)


def _dw(E: Ctx, conv: nn.Conv2d, bn, x: Act, act: int) -> Act:
    w, s, h, k, stride = E.dw(conv, bn)
    return ops.dwconv(x, w, s, h, k, stride, act)


def _dw_se(E: Ctx, conv: nn.Conv2d, bn, se: nn.Module, x: Act) -> Tuple[Act, torch.Tensor]:
    """conv_dw + BN + SiLU with the SE global pool fused into it, then the SE MLP -> gate [N, C]."""
    w, s, h, k, stride = E.dw(conv, bn)
    rd, c = se.conv_reduce.out_channels, se.conv_reduce.in_channels
    return ops.dwconv_se_gate(x, w, s, h, k, stride, ACT_SILU, E.f32(se.conv_reduce.weight, (rd, c)),
                              E.f32(se.conv_reduce.bias), E.f32(se.conv_expand.weight, (c, rd)),
                              E.f32(se.conv_expand.bias), ACT_SILU)


def mbconv(E: Ctx, blk: nn.Module, x: Act, out_cpad: Optional[int] = None) -> Act:
    """timm DepthwiseSeparableConv / InvertedResidual (eval): the SE pool is fused into the depthwise conv,
    the SE gate is applied inside the projection conv's loader (in_scale), the skip add in its epilogue.
    ``out_cpad``: channel stride of the block output (zero pad channels)."""
    if isinstance(blk, DepthwiseSeparableConv):
        h, g = _dw_se(E, blk.conv_dw, blk.bn1, blk.se, x)
        return ops.conv2d(E.conv(blk.conv_pw, blk.bn2), h, in_scale=g, residual=x if blk.has_skip else None,
                          out_cpad=out_cpad)
    if isinstance(blk, InvertedResidual):
        h = ops.conv2d(E.conv(blk.conv_pw, blk.bn1, ACT_SILU), x)
        h, g = _dw_se(E, blk.conv_dw, blk.bn2, blk.se, h)
        return ops.conv2d(E.conv(blk.conv_pwl, blk.bn3), h, in_scale=g, residual=x if blk.has_skip else None,
                          out_cpad=out_cpad)
    raise TypeError(type(blk))


def _block_out_channels(blk: nn.Module) -> int:
    return (blk.conv_pw if isinstance(blk, DepthwiseSeparableConv) else blk.conv_pwl).out_channels


def _drain(gen):
    """Run a forward generator (below) to its end and return its value."""
    while True:
        try:
            next(gen)
        except StopIteration as e:
            return e.value


def unet_logit(E: Ctx, pre: nn.Module, images: torch.Tensor) -> torch.Tensor:
    """PreTrainedPeopleSegmentationUNet.forward (unet.py:1901-1916): normalise, smp.Unet -> u [B,1,H,W] f32."""
    return _drain(unet_logit_iter(E, pre, images))


def unet_logit_iter(E: Ctx, pre: nn.Module, images: torch.Tensor):
    """unet_logit as a generator: yields after each encoder block / decoder block (the serving schedule's chunks,
    hiseg.model.StreamPipelinedExport(gate=True)), returns u."""
    B, _, H, W = images.shape
    if H % 32 or W % 32:
        raise NotImplementedError(f"image size {H}x{W} must be a multiple of 32 for the EfficientNet-UNet")
    return (yield from effunet_forward_iter(E, pre.model, unet_input(E, pre, images)))


def unet_input(E: Ctx, pre: nn.Module, images: torch.Tensor):
    """normalize_input for the smp.Unet.  The stem conv is the normalised images' only reader: where the library
    has that form it normalises as it stages them, and this returns ops.RawImages (the maximum launched, no
    normalised copy written) for effunet_stem; the normalised NHWC Act otherwise."""
    enc = pre.model.encoder
    stem = E.conv(enc.conv_stem, enc.bn1, ACT_SILU) if STEM_RAW else None
    return ops.input_norm(images, E.f32(pre.norm_mean, (3,)), E.f32(pre.norm_std, (3,)), E.dtype, stem=stem)


def effunet_stem(E: Ctx, enc: nn.Module, x) -> Act:
    """conv_stem + bn1 + SiLU on unet_input's result (an Act, or ops.RawImages: one launch normalises and convolves)."""
    if isinstance(x, ops.RawImages):
        return ops.stem_raw(x)
    return ops.conv2d(E.conv(enc.conv_stem, enc.bn1, ACT_SILU), x)


def effunet_forward(E: Ctx, net: nn.Module, x: Act) -> torch.Tensor:
    """smp.Unet('timm-efficientnet-bX') forward (eval) on an NHWC input -> logits [B,1,H,W] f32."""
    return _drain(effunet_forward_iter(E, net, x))


def effunet_forward_iter(E: Ctx, net: nn.Module, x):
    """effunet_forward as a generator: yields after the stem, each MBConv block and each decoder block.  ``x``: the
    normalised NHWC input, or ops.RawImages (unet_input: the stem normalises)."""
    B, H, W = x.N, x.H, x.W
    enc = net.encoder
    x = effunet_stem(E, enc, x)
    feats = [x]
    yield
    for si, stage in enumerate(enc.blocks):
        for bi, blk in enumerate(stage):
            # the skip features of decoder blocks 0-2 (stage 2 / 3 / 5 outputs: 24 / 40 / 112 channels for B0-B1,
            # 48 / 80 / 224 for B7) are stored with a 64-multiple channel stride, zero pad channels, so those
            # blocks' conv1 (upsampled x ++ skip) takes the halo-tiled kernels instead of the generic one; the next
            # stage reads the padded map through its channel stride
            cpad = None
            if E.dtype == torch.bfloat16 and si + 1 in (2, 3, 5) and bi == len(stage) - 1:
                c = _block_out_channels(blk)
                cpad = round_up(c, 64) if c % 64 else None
            x = mbconv(E, blk, x, out_cpad=cpad)
            yield
        if si + 1 in (2, 3, 5, 7):
            feats.append(x)
    skips = feats[-2::-1]
    x = feats[-1]
    for i, blk in enumerate(net.decoder.blocks):
        skip = skips[i] if i < len(skips) else None
        split = (x.C, skip.C, skip.cstride) if skip is not None else None
        x = ops.conv2d(E.conv(blk.conv1[0], blk.conv1[1], ACT_RELU, split=split), x, skip, a_up=2)
        x = ops.conv2d(E.conv(blk.conv2[0], blk.conv2[1], ACT_RELU), x)
        yield
    u = Act.new(B, H, W, 1, torch.float32, E.device, cpad=1, zero=False)
    ops.conv2d(E.conv(net.segmentation_head[0]), x, out=u)
    return u.t.view(B, 1, H, W)


# ------------------------------------------------------------------------------------ entry points
def _root_dtype(m: nn.Module) -> torch.dtype:
    return getattr(m, "hiseg_dtype", torch.float32)


def unet_logits_nchw(pre: nn.Module, x: torch.Tensor) -> torch.Tensor:
    _check_input(x, "PreTrainedPeopleSegmentationUNet")
    E = Ctx(pre, _root_dtype(pre), x.device)
    return unet_logit(E, pre, x)


def _output_conv(E: Ctx, oc: nn.Conv2d, u: torch.Tensor) -> torch.Tensor:
    B, _, H, W = u.shape
    out = torch.empty(B, 2, H, W, dtype=torch.float32, device=u.device)
    L.check(L.lib().hiseg_output_conv_fwd(u.data_ptr(), B, H, W, E.f32(oc.weight, (2,)).data_ptr(),
                                          E.f32(oc.bias).data_ptr(), out.data_ptr(), L.stream_ptr()), "output_conv")
    return out


def unet_two_channel_nchw(wrapper: nn.Module, x: torch.Tensor) -> torch.Tensor:
    _check_input(x, "PreTrainedPeopleSegmentationUNetWrapper")
    E = Ctx(wrapper, _root_dtype(wrapper), x.device)
    return _output_conv(E, wrapper.output_conv, unet_logit(E, wrapper.model, x))


def roi_align_nchw(m: nn.Module, feat: torch.Tensor, rois: torch.Tensor, oh, ow) -> torch.Tensor:
    _check_input(feat, "DynamicRoIAlign")
    oh = int(oh.item()) if torch.is_tensor(oh) else int(oh[0] if isinstance(oh, (list, tuple)) else oh)
    ow = int(ow.item()) if torch.is_tensor(ow) else int(ow[0] if isinstance(ow, (list, tuple)) else ow)
    feat = feat.contiguous().float()
    out = torch.empty(rois.shape[0], feat.shape[1], oh, ow, dtype=torch.float32, device=feat.device)
    ops.roi_align(feat, rois.to(feat.device), oh, ow, m.spatial_scale_h, m.spatial_scale_w, m.aligned,
                  nchw_out=out)
    return out


def rgb_model_forward(model: nn.Module, images: torch.Tensor, rois: torch.Tensor, aux: str = "full",
                      unet_logit_override: Optional[torch.Tensor] = None):
    """HierarchicalRGBSegmentationModelWithFullImagePretrainedUNet.forward (rgb.py:729-774).

    ``unet_logit_override`` (tests only) substitutes the smp.Unet output u [B,1,H,W], the way the
    golden vectors were produced from the reference.
    """
    _check_input(images, "HierarchicalRGBSegmentationModelWithFullImagePretrainedUNet")
    if model.training:
        raise NotImplementedError("hiseg executes the inference (eval-mode) forward; call model.eval()")
    dev = images.device
    E = Ctx(model, _root_dtype(model), dev)
    images = images.contiguous().float()
    rois = rois.to(device=dev, dtype=torch.float32).contiguous()
    N = rois.shape[0]
    rh, rw = model.roi_size
    wrapper = model.pretrained_unet
    if unet_logit_override is not None:
        u = unet_logit_override.to(device=dev, dtype=torch.float32).contiguous()
    else:
        u = unet_logit(E, wrapper.model, images)
    oc = wrapper.output_conv
    ma, mr = model.roi_align_mask, model.roi_align_rgb
    guided = not hasattr(model, "feature_combiner")   # rgb.py:758-765: the guided head takes features and masks
    rf = None
    if guided:   # the guidance is read in f32 whatever the compute dtype: its aux tensors saturate (rgb.py:196-202)
        rf = torch.empty(N, 2, rh, rw, dtype=torch.float32, device=dev)
        ops.roi_align(u, rois, rh, rw, ma.spatial_scale_h, ma.spatial_scale_w, ma.aligned, nchw_out=rf,
                      aff_w=E.f32(oc.weight, (2,)), aff_b=E.f32(oc.bias))
    else:
        roi_logits = Act.new(N, rh, rw, 2, E.dtype, dev, zero=False)
        ops.roi_align(u, rois, rh, rw, ma.spatial_scale_h, ma.spatial_scale_w, ma.aligned, out=roi_logits,
                      aff_w=E.f32(oc.weight, (2,)), aff_b=E.f32(oc.bias), zero_to=roi_logits.cstride)
    rgb = Act.new(N, rh, rw, 3, E.dtype, dev, zero=False)
    ops.roi_align(images, rois, rh, rw, mr.spatial_scale_h, mr.spatial_scale_w, mr.aligned, out=rgb,
                  zero_to=rgb.cstride)
    if guided and not GUIDED_FUSE_SRC_B:
        logits, auxd = guided_head(E, model.segmentation_head, None, rf, aux, feats_into=lambda dst: (
            rgb_feature_extractor(E, model.rgb_feature_extractor, rgb, out=dst)))
    elif guided:
        feats = rgb_feature_extractor(E, model.rgb_feature_extractor, rgb)
        logits, auxd = guided_head(E, model.segmentation_head, feats, rf, aux)
    else:
        feats = rgb_feature_extractor(E, model.rgb_feature_extractor, rgb)
        comb = ops.conv2d(E.conv(model.feature_combiner, split=(feats.C, 2)), feats, roi_logits)
        logits, auxd = hier_head(E, model.segmentation_head, comb, aux)
    if aux == "full":
        auxd["full_image_logits"] = _output_conv(E, oc, u)
        if rf is None:
            rf = torch.empty(N, 2, rh, rw, dtype=torch.float32, device=dev)
            ops.roi_align(u, rois, rh, rw, ma.spatial_scale_h, ma.spatial_scale_w, ma.aligned, nchw_out=rf,
                          aff_w=E.f32(oc.weight, (2,)), aff_b=E.f32(oc.bias))
        auxd["roi_features"] = rf
        rp = torch.empty(N, 3, rh, rw, dtype=torch.float32, device=dev)
        ops.roi_align(images, rois, rh, rw, mr.spatial_scale_h, mr.spatial_scale_w, mr.aligned, nchw_out=rp)
        auxd["roi_patches"] = rp
    else:
        auxd["unet_logit"] = u
    return logits, auxd


def rgb_plain_forward(model: nn.Module, images: torch.Tensor, rois: torch.Tensor, aux: str = "full"):
    """HierarchicalRGBSegmentationModel.forward (hierarchical_segmentation_rgb.py:410-439): RoIAlign (aligned=False)
    of the images, RGBFeatureExtractor, hierarchical head.  ``aux`` "full" adds ``roi_patches``, the RoIAligned RGB
    as f32 NCHW."""
    _check_input(images, "HierarchicalRGBSegmentationModel")
    if model.training:
        raise NotImplementedError("hiseg executes the inference (eval-mode) forward; call model.eval()")
    dev = images.device
    E = Ctx(model, _root_dtype(model), dev)
    images = images.contiguous().float()
    rois = rois.to(device=dev, dtype=torch.float32).contiguous()
    N = rois.shape[0]
    rh, rw = model.roi_height, model.roi_width
    ra = model.roi_align
    rgb = Act.new(N, rh, rw, 3, E.dtype, dev, zero=False)
    ops.roi_align(images, rois, rh, rw, ra.spatial_scale_h, ra.spatial_scale_w, ra.aligned, out=rgb,
                  zero_to=rgb.cstride)
    feats = rgb_extractor_plain(E, model.rgb_extractor.features, rgb)
    logits, auxd = hier_head(E, model.segmentation_head, feats, aux)
    if aux == "full":
        rp = torch.empty(N, 3, rh, rw, dtype=torch.float32, device=dev)
        ops.roi_align(images, rois, rh, rw, ra.spatial_scale_h, ra.spatial_scale_w, ra.aligned, nchw_out=rp)
        auxd["roi_patches"] = rp
    return logits, auxd


def export_forward(model: nn.Module, images: torch.Tensor, rois: torch.Tensor, dilation: int = 0):
    """Exported contract: (instance_masks [N,1,mh,mw], binary_masks [B,1,H,W])."""
    logits, auxd = rgb_model_forward(model, images, rois, aux="none")
    E = Ctx(model, _root_dtype(model), images.device)
    oc = model.pretrained_unet.output_conv
    inst = ops.instance_masks(logits, dilation)
    binary = ops.binary_masks(auxd["unet_logit"], E.f32(oc.weight, (2,)), E.f32(oc.bias))
    return inst, binary


def export_unet_phase(model: nn.Module, images: torch.Tensor):
    """First half of the exported contract: full-image UNet logit u and binary_masks."""
    return _drain(export_unet_phase_iter(model, images))


def export_unet_phase_iter(model: nn.Module, images: torch.Tensor):
    """export_unet_phase as a generator (yields between UNet blocks), returns (u, binary_masks)."""
    _check_input(images, "RGBHierarchicalExportWrapper")
    E = Ctx(model, _root_dtype(model), images.device)
    u = yield from unet_logit_iter(E, model.pretrained_unet.model, images.contiguous().float())
    oc = model.pretrained_unet.output_conv
    return u, ops.binary_masks(u, E.f32(oc.weight, (2,)), E.f32(oc.bias))


def export_head_phase(model: nn.Module, images: torch.Tensor, rois: torch.Tensor, u: torch.Tensor, dilation: int = 0):
    """Second half: RoIAlign + ROI head from u -> instance_masks."""
    logits, _ = rgb_model_forward(model, images, rois, aux="none", unet_logit_override=u)
    return ops.instance_masks(logits, dilation)


# ------------------------------------------------------------------------------------ sub-module forwards (NCHW f32)
def _root_for(m: nn.Module):
    return m


def residual_block_nchw(blk: nn.Module, x: torch.Tensor) -> torch.Tensor:
    _check_input(x, "ResidualBlock")
    E = Ctx(blk, _root_dtype(blk), x.device)
    return residual_block(E, blk, Act.from_nchw(x, E.dtype)).to_nchw()


def enhanced_unet_nchw(u: nn.Module, x: torch.Tensor) -> torch.Tensor:
    _check_input(x, "EnhancedUNet")
    E = Ctx(u, _root_dtype(u), x.device)
    low, _ = enhanced_unet(E, u, Act.from_nchw(x, E.dtype))
    return low.to_nchw()


def boundary_refine_nchw(mod: nn.Module, x: torch.Tensor, want_edges: bool = False):
    _check_input(x, "BoundaryRefinementModule")
    E = Ctx(mod, _root_dtype(mod), x.device)
    return boundary_refine(E, mod, x, want_edges)


def guided_head_nchw(head: nn.Module, features: torch.Tensor, bg_fg_mask: torch.Tensor):
    _check_input(features, "PretrainedUNetGuidedSegmentationHead")
    _check_input(bg_fg_mask, "PretrainedUNetGuidedSegmentationHead")
    if bg_fg_mask.dim() != 4 or bg_fg_mask.shape[1] not in (1, 2) or bg_fg_mask.shape[0] != features.shape[0]:
        raise ValueError(f"bg_fg_mask: expected [N, 1 or 2, h, w], got shape {tuple(bg_fg_mask.shape)}")
    if tuple(bg_fg_mask.shape[2:]) != tuple(features.shape[2:]):
        raise NotImplementedError(
            f"bg_fg_mask {tuple(bg_fg_mask.shape[2:])} and features {tuple(features.shape[2:])} differ in size: the "
            "resize of fg_prob to the feature size (rgb.py:147-153) is not on the hiseg path (the model aligns both "
            "to the ROI size)")
    E = Ctx(head, _root_dtype(head), features.device)
    mask = bg_fg_mask.to(torch.float32).contiguous()
    if GUIDED_FUSE_SRC_B:
        return guided_head(E, head, Act.from_nchw(features, E.dtype), mask, "full")
    x = features.contiguous().float()

    def into(dst: Act):
        N, C, H, W = x.shape
        L.check(L.lib().hiseg_nchw_to_nhwc_fwd(ops.hdtype(E.dtype), x.data_ptr(), N, C, H, W, dst.ptr(), dst.cstride,
                                               L.stream_ptr()), "nchw_to_nhwc")
    return guided_head(E, head, None, mask, "full", feats_into=into)


def head_nchw(head: nn.Module, x: torch.Tensor):
    _check_input(x, type(head).__name__)
    E = Ctx(head, _root_dtype(head), x.device)
    return hier_head(E, head, Act.from_nchw(x, E.dtype), "full")
