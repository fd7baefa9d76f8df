"""hiseg_hier_combine_resize on its own against a float64 restatement.

The oracle builds upsample_bg_fg (ConvTranspose2d 2 -> 32 k2 s2, the folded norm affine or per-ROI LayerNorm tables,
the activation, the 1x1 32 -> 2) in torch double, applies F.interpolate (bilinear, align_corners=False) in double to
its two logits and to the two target logits, then the softmax and the combine of
advanced/hierarchical_segmentation_refinement.py:593-596.  Bar: the project's f32 bar, 1e-4 * max(1, |ref|max) per
tensor (tests/test_gpu_parity.py).  Outputs are prefilled with NaN, so a pixel the kernel does not write fails.
"""
import pytest
import torch
import torch.nn.functional as F

import filler

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32_TOL = 1e-4
SHAPES = [(2, 1, 1, 1, 1), (2, 2, 3, 2, 3), (1, 3, 5, 7, 4), (2, 4, 4, 5, 7), (2, 7, 9, 20, 25),
          (3, 20, 18, 47, 33)]   # (N, h, w, mh, mw); the last spans several workgroups


def _case(N, h, w, per_sample, seed=600):
    r = lambda k, shape: torch.from_numpy(filler.normal(seed + k, shape))   # noqa: E731
    u = lambda k, shape, a: torch.from_numpy(filler.uniform(seed + k, shape, -a, a))   # noqa: E731
    rows = N if per_sample else 1
    return dict(low=r(1, (N, h, w, 2)) * 2.0, tn2=r(2, (N * 4 * h * w, 2)) * 2.0, ut_w=u(3, (2, 32, 2, 2), 0.7),
                scale=1.0 + u(4, (rows, 32), 0.3), shift=u(5, (rows, 32), 0.3), u1_w=u(6, (2, 32), 0.3),
                u1_b=u(7, (2,), 0.1))


def oracle(c, act, mh, mw):
    d = {k: v.double() for k, v in c.items()}
    N, h, w, _ = d["low"].shape
    z = F.conv_transpose2d(d["low"].permute(0, 3, 1, 2), d["ut_w"], None, stride=2)
    z = z * d["scale"].view(-1, 32, 1, 1) + d["shift"].view(-1, 32, 1, 1)
    z = torch.relu(z) if act == "relu" else F.silu(z)
    b = F.conv2d(z, d["u1_w"].view(2, 32, 1, 1), d["u1_b"])
    t = d["tn2"].view(N, 2 * h, 2 * w, 2).permute(0, 3, 1, 2)
    if (mh, mw) != (2 * h, 2 * w):
        b = F.interpolate(b, size=(mh, mw), mode="bilinear", align_corners=False)
        t = F.interpolate(t, size=(mh, mw), mode="bilinear", align_corners=False)
    p = torch.softmax(b, 1)[:, 1]
    logits = torch.stack([b[:, 0], b[:, 1] + t[:, 0] * p, b[:, 1] + t[:, 1] * p], 1)
    return logits, b, t.contiguous()


def _launch(d, act, per_sample, mh, mw, outs):
    from hiseg import _lib as L
    N, h, w, _ = d["low"].shape
    code = L.ACT_RELU if act == "relu" else L.ACT_SILU
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    L.check(L.lib().hiseg_hier_combine_resize(
        ptr(d["low"]), N, h, w, ptr(d["tn2"]), ptr(d["ut_w"]), ptr(d["scale"]), ptr(d["shift"]), int(code),
        L.act_beta(code), int(per_sample), ptr(d["u1_w"]), ptr(d["u1_b"]), mh, mw, *[ptr(o) for o in outs],
        L.stream_ptr()), "hier_combine_resize")


def _bar(ref):
    return F32_TOL * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("aux", [True, False])
@pytest.mark.parametrize("act", ["relu", "silu"])
@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_%dx%d_to_%dx%d" % s)
def test_matches_the_float64_oracle(shape, per_sample, act, aux):
    N, h, w, mh, mw = shape
    c = _case(N, h, w, per_sample)
    refs = oracle(c, act, mh, mw)
    d = {k: v.to(DEV).contiguous() for k, v in c.items()}
    nan = lambda ch: torch.full((N, ch, mh, mw), float("nan"), device=DEV)   # noqa: E731
    outs = [nan(3), nan(2) if aux else None, nan(2) if aux else None]
    _launch(d, act, per_sample, mh, mw, outs)
    torch.cuda.synchronize()
    figs = []
    for name, got, ref in zip(("logits", "bg_fg_logits", "target_nontarget_logits"), outs, refs):
        if got is None:
            continue
        assert torch.isfinite(got).all(), name
        figs.append((name, (got.double().cpu() - ref).abs().max().item(), _bar(ref)))
    print(f"hier_combine_resize {shape} ps={per_sample} {act}: " + ", ".join(f"{n} {e:.2e}/{b:.2e}" for n, e, b in figs))
    for n, e, b in figs:
        assert e < b, (n, e, b)
    first = [o.clone() for o in outs if o is not None]
    _launch(d, act, per_sample, mh, mw, outs)   # a second call into the same buffers: the same bits
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, [o for o in outs if o is not None]))


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("shape", [(2, 4, 4), (3, 20, 18)], ids=lambda s: "N%d_%dx%d" % s)
def test_at_twice_the_roi_it_agrees_with_hier_combine(shape, per_sample):
    """The engine never sends (2h, 2w) to the new kernel; there it must still say what hiseg_hier_combine says."""
    from hiseg import _lib as L, ops
    N, h, w = shape
    c = _case(N, h, w, per_sample, seed=700)
    d = {k: v.to(DEV).contiguous() for k, v in c.items()}
    ref = ops.hier_combine(d["low"], N, h, w, None, d["ut_w"], d["scale"], d["shift"], L.ACT_RELU, d["u1_w"], d["u1_b"],
                           None, None, True, per_sample=per_sample, tn2=d["tn2"])
    got = ops.hier_combine_resize(d["low"], N, h, w, d["tn2"], d["ut_w"], d["scale"], d["shift"], L.ACT_RELU, d["u1_w"],
                                  d["u1_b"], 2 * h, 2 * w, True, per_sample=per_sample)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert (a.double() - b.double()).abs().max().item() < _bar(b)
    assert torch.equal(got[2], d["tn2"].view(N, 2 * h, 2 * w, 2).permute(0, 3, 1, 2))   # weights 1 and 0: a copy


def test_out_of_range_arguments_are_refused():
    from hiseg import _lib as L
    c = {k: v.to(DEV).contiguous() for k, v in _case(1, 32, 32, False).items()}
    out = torch.full((1, 3, 8, 8), float("nan"), device=DEV)
    with pytest.raises(L.HisegError, match="source window"):
        _launch(c, "relu", False, 8, 8, [out, None, None])   # an eighth of the 64 x 64 grid: the window passes the LDS
    with pytest.raises(L.HisegError, match="bad shape"):
        _launch(c, "relu", False, 0, 8, [out, None, None])
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert L.lib().hiseg_last_error_string()
