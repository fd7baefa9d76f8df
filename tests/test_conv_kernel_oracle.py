"""tests/conv_kernel_oracle.py against torch's own float64 operators, and the premise of tier A of
tests/test_gpu_conv_kernels.py for every one of its cases (no GPU)."""
import pytest
import torch
import torch.nn.functional as F

import conv_kernel_oracle as O


def torch_ref(c, t, dt):
    """The same operation through F.interpolate / F.conv2d / F.conv_transpose2d in float64."""
    a = t["xa"]
    if c["a_up"] > 1:
        a = F.interpolate(a, scale_factor=c["a_up"], mode="nearest")
    if t["gate"] is not None:
        a = (a.float() * t["gate"].float()[:, :, None, None]).to(O.DTYPES[dt]).double()
    x = a if t["xb"] is None else torch.cat([a, t["xb"]], 1)
    if c["convT"]:
        z = F.conv_transpose2d(x, t["w"], stride=2)
    else:
        z = F.conv2d(x, t["w"], stride=c["stride"], padding=c["pad"])
    z = z * t["scale"][None, :, None, None] + t["shift"][None, :, None, None]
    if t["residual"] is not None:
        z = z + t["residual"]
    act = c["act"]
    v = z if act == 0 else F.relu(z) if act == 1 else torch.sigmoid(z) if act == 2 else z * torch.sigmoid(c["beta"] * z)
    return v if t["mul"] is None else v * t["mul"]


FORMS = {
    "plain_3x3": dict(Ca=5, Cout=7, H=6, W=5),
    "stride2": dict(Ca=8, Cout=6, H=9, W=11, stride=2, act=1),
    "stride2_even": dict(Ca=8, Cout=6, H=8, W=8, stride=2, act=1),
    "pad0_3x3": dict(Ca=4, Cout=3, H=6, W=7, pad=0),
    "k5": dict(Ca=4, Cout=3, H=6, W=7, k=5, pad=2),
    "1x1": dict(Ca=16, Cout=1, H=3, W=4, k=1, pad=0),
    "up2_two_sources_res_mul": dict(Ca=8, Cb=5, Cout=6, H=6, W=4, a_up=2, residual=True, mul=True, act=1),
    "gate_1x1": dict(N=3, Ca=8, Cout=5, H=3, W=4, k=1, pad=0, gate=True),
    "gate_3x3_two_sources": dict(Ca=8, Cb=8, Cout=5, H=3, W=4, gate=True, residual=True),
    "convT": dict(N=3, Ca=8, Cout=4, H=3, W=5, k=1, pad=0, convT=True, act=1, residual=True),
    "sigmoid": dict(Ca=8, Cout=4, H=3, W=5, act=2, mul=True),
    "silu": dict(Ca=8, Cout=4, H=3, W=5, act=3),
    "swish": dict(Ca=8, Cout=4, H=3, W=5, act=5, beta=1.5, residual=True),
}


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("name", list(FORMS))
def test_oracle_agrees_with_torch(name, tier, dt):
    case = FORMS[name]
    if tier == "A" and case.get("act", 0) > 1:
        pytest.skip("tier A inputs go with exact activations only")
    c, t = O.make_inputs(case, tier, dt)
    r = O.run(c, t, dt)
    ref = torch_ref(c, t, dt)
    assert r["v"].shape == ref.shape
    assert (r["v"] - ref).abs().max() <= 1e-12 * max(1.0, ref.abs().max().item())
    assert r["out"].dtype == O.DTYPES[dt] and torch.equal(r["out"], r["v"].float().to(O.DTYPES[dt]))
    assert bool((r["S"] >= r["pre"].abs() - 1e-9).all())   # the absolute-value pipeline dominates the pre-activation
    for k in ("xa", "xb", "w", "residual", "mul"):          # inputs are values of the compute dtype
        if t[k] is not None:
            assert torch.equal(t[k].to(O.DTYPES[dt]).double(), t[k]), k


def test_upsample_and_pixel_shuffle_index_maps():
    x = torch.arange(2 * 3 * 2 * 3, dtype=torch.float64).view(2, 3, 2, 3)
    assert torch.equal(O.upsample_nearest(x, 2), F.interpolate(x, scale_factor=2, mode="nearest"))
    w = torch.arange(3 * 2 * 4, dtype=torch.float64).view(3, 2, 2, 2)
    assert torch.equal(O._gemm(x, w, 1, 0, True), F.conv_transpose2d(x, w, stride=2))


def tier_a_cases():
    """Every (case, compute dtype, output dtype) tests/test_gpu_conv_kernels.py runs in tier A, from that module's
    own tables and case builders (a case edited there is proved here as it then stands)."""
    import test_gpu_conv_kernels as G
    seen = {}

    def add(case, dts=("bf16",)):
        case = dict(case)
        f32o = case.pop("f32_out", False)
        if case.get("act", 0) > 1:
            return
        for dt in dts:
            seen.setdefault((tuple(sorted(case.items())), dt, "f32" if f32o else dt), (case, dt, "f32" if f32o else dt))

    for case, _ in G.GENERIC.values():
        add(case, ("f32", "bf16"))
    for case, _ in G.SPLITK.values():
        add(case)
    for table in (G.FAST, G.WIDE, G.PW, G.SMALL, G.ROWS):
        for case in table.values():
            add(case)
    for name in G.HALO:
        for variant in G.HALO_CMUL:
            add(G.halo_case(name, variant))
    for cout in G.HALO_PARTIAL_COUTS:
        for case in G.halo_partial_cases(cout):
            add(case)
    for case in G.STATS.values():
        add(case)
    add(G.PW_GATE_RANGES)
    add(G.SMALL_GATE_TWO_SOURCES)
    for H, W in G.SMALL_S2_SIZES:
        add(G.small_s2_case(H, W, O.ACT_RELU))
    for case, _, dt in G.AUTO.values():
        add(case, (dt,))
    for case, _ in G.DECLINES.values():
        add(case)
    return list(seen.values())


TIER_A = tier_a_cases()


@pytest.mark.parametrize("i", range(len(TIER_A)))
def test_tier_a_premise(i):
    """Float32 evaluation equals float64 exactly and S < 2^22 (< 2^24): with every term a multiple of 1/4 (a gate of
    1/2 times a scale of 1/2) no larger than S, every partial sum in any order is a float32 value.  It holds by
    construction -- S <= |x| |w| K |scale| + |shift| + |residual| <= 16 K + 5 with K <= 2^17 -- which the bound on S
    computed here from the inputs' ranges, not their values, asserts as well."""
    case, dt, out_dt = TIER_A[i]
    c, t = O.make_inputs(case, "A", dt)
    r64 = O.run(c, t, dt, out_dt)
    r32 = O.run(c, t, dt, out_dt, compute=torch.float32)
    assert torch.equal(r32["v"].double(), r64["v"]) and torch.equal(r32["pre"].double(), r64["pre"])
    assert torch.equal(r32["out"], r64["out"]) and torch.equal(r32["out2"], r64["out2"])
    K = c["Ca"] if c["convT"] else c["k"] * c["k"] * (c["Ca"] + c["Cb"])
    worst = 2 * (2 * max(O.TIER_A_GATES) if c["gate"] else 2) * K * 2 + 3 + 2   # |x| |w| K |scale| + |shift| + |res|
    assert r64["S"].max() <= worst < 2 ** 22
    assert torch.equal(r64["v"] * 4, (r64["v"] * 4).round())   # multiples of 1/4
