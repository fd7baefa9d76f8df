"""tests/wgrad_oracle.py against float64 autograd (no GPU), and the exactness premise of tier A for every case of
tests/test_gpu_wgrad_kernels.py, proved from the shapes alone."""
import pytest
import torch
import torch.nn.functional as F

import conv_kernel_oracle as O
import test_gpu_wgrad_kernels as G
import wgrad_oracle as W

CASES = {
    "3x3_two_sources_pads": dict(N=2, Ca=5, Cb=3, Cout=6, H=7, W=9),
    "3x3_stride2": dict(N=2, Ca=4, Cout=5, H=9, W=8, stride=2),
    "1x1": dict(N=3, Ca=7, Cout=4, H=5, W=6, k=1, pad=0),
    "5x5_pad1": dict(N=1, Ca=3, Cout=2, H=8, W=9, k=5, pad=1),
    "up2_two_sources": dict(N=2, Ca=4, Cb=5, Cout=3, H=6, W=8, a_up=2),
    "convT": dict(N=2, Ca=5, Cout=3, H=4, W=5, k=1, pad=0, convT=True),
    "halo_shape": dict(N=3, Ca=8, Cout=8, H=9, W=17),
}


def autograd(c, xa, xb, dy, bias):
    """(gw, gb, X) by float64 autograd of F.conv2d / F.conv_transpose2d; the nearest upsampling by indexing."""
    X = O.gather_input(xa, xb, c["a_up"], None, "bf16")
    if c["convT"]:
        w = torch.zeros(c["Ca"], c["Cout"], 2, 2, dtype=torch.float64, requires_grad=True)
    else:
        w = torch.zeros(c["Cout"], c["Ca"] + c["Cb"], c["k"], c["k"], dtype=torch.float64, requires_grad=True)
    b = torch.zeros(c["Cout"], dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose2d(X, w, b, stride=2) if c["convT"] else F.conv2d(X, w, b, stride=c["stride"], padding=c["pad"])
    (y * dy).sum().backward()
    return w.grad, (b.grad if bias else None), X


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_reduced_partials_are_autograd(name, bias, dt):
    c, xa, xb, dy = W.make_inputs(CASES[name], "B", dt)
    gw, gb, X = autograd(c, xa, xb, dy, bias)
    g = W.geometry(c, dt, bias)
    nblocks = (g["M"] + g["PB"] - 1) // g["PB"]
    m = W.wgrad_map(c, dt, bias)
    partitions = [(1, nblocks, None), (nblocks, 1, None), ((nblocks + 1) // 2, 2, None)]
    if name == "halo_shape":
        partitions += [(s, 0, W.halo_partition(c["N"], c["H"], c["W"], s)) for s in (1, 5, 12, 13)]
    for splits, bps, part in partitions:
        ws = W.partials(c, X, dy, bias, splits, bps, dt, partition=part)
        assert ws.shape == (splits, g["cols"], g["Ktot"] + int(bias))
        rw, rb = W.reduce(ws, m)
        assert rw.shape == gw.shape and (rw - gw).abs().max() <= 1e-12 * gw.abs().max()
        if bias:
            assert (rb - gb).abs().max() <= 1e-12 * gb.abs().max()
    old = (torch.ones_like(gw), torch.ones_like(gb) if bias else None)
    aw, ab = W.reduce(ws, m, old)
    assert torch.equal(aw, rw + 1) and (not bias or torch.equal(ab, rb + 1))
    s = W.S(c, X, dy, bias, dt)
    assert bool((W.partials(c, X, dy, bias, 1, nblocks, dt)[0].abs() <= s).all())


def pack_entry(c, dt, mode):
    g = W.geometry(c, dt, False)
    k = 2 if c["convT"] else c["k"]
    cop = W.rup(c["Cout"], W.CHUNK[dt])
    cinp = g["ca"] + g["cb"]
    e = dict(Cout=c["Cout"], Cin_real=c["Ca"] + c["Cb"], KH=k, KW=k, ca=g["ca"], ca_real=c["Ca"], cb=g["cb"],
             cb_real=c["Cb"], cop=cop, mode=mode)
    if mode in (0, 2):
        e["rows"], e["K_pad"] = W.rup(g["cols"], 16), W.rup(g["Ktot"], 64)
    else:
        e["rows"], e["K_pad"] = W.rup(cinp, 16), W.rup(k * k * cop, 64)
    e["total"] = e["rows"] * e["K_pad"]
    shape = (c["Ca"], c["Cout"], 2, 2) if c["convT"] else (c["Cout"], c["Ca"] + c["Cb"], k, k)
    e["src"] = torch.randn(*shape, generator=O.gen(3), dtype=torch.float64)
    return e, g


@pytest.mark.parametrize("name", ["3x3_two_sources_pads", "1x1", "5x5_pad1", "convT"])
def test_forward_packs_are_the_forward_gemm(name):
    """Modes 0 and 2: im2col(X) times the packed matrix is F.conv2d / F.conv_transpose2d, pads zero."""
    c, xa, xb, dy = W.make_inputs(CASES[name], "B", "bf16")
    e, g = pack_entry(c, "bf16", 2 if c["convT"] else 0)
    P = W.pack(e).view(e["rows"], e["K_pad"])
    assert bool((P[g["cols"]:] == 0).all()) and bool((P[:, g["Ktot"]:] == 0).all())
    X = O.gather_input(xa, xb, 1, None, "bf16")
    y = W.im2col(c, X, "bf16") @ P[:g["cols"], :g["Ktot"]].t()                 # [M][GEMM columns]
    if c["convT"]:
        ref = W.dy_matrix(c, F.conv_transpose2d(X, e["src"], stride=2), "bf16")
    else:
        ref = F.conv2d(X, e["src"], padding=c["pad"]).permute(0, 2, 3, 1).reshape(g["M"], g["cols"])
    assert (y - ref).abs().max() <= 1e-12 * ref.abs().max()


@pytest.mark.parametrize("name", ["3x3_two_sources_pads", "1x1", "convT"])
def test_dgrad_packs_give_autograd_dx(name):
    """Modes 1 and 3: a float64 forward conv of dy with the packed matrix -- pad KH - 1 - pad (conv), 2x2 stride 2
    (ConvTranspose), as train_engine.conv_bwd launches it -- is autograd's dx."""
    c, xa, xb, dy = W.make_inputs(CASES[name], "B", "bf16")
    e, g = pack_entry(c, "bf16", 3 if c["convT"] else 1)
    P = W.pack(e).view(e["rows"], e["K_pad"])
    X = O.gather_input(xa, xb, 1, None, "bf16").requires_grad_(True)
    y = F.conv_transpose2d(X, e["src"], stride=2) if c["convT"] else F.conv2d(X, e["src"], padding=c["pad"])
    (y * dy).sum().backward()
    k, cop, cinp = e["KH"], e["cop"], g["ca"] + g["cb"]
    assert bool((P[:, k * k * cop:] == 0).all()) and bool((P[cinp:] == 0).all())
    wk = P[:cinp, :k * k * cop].reshape(cinp, k, k, cop).permute(0, 3, 1, 2)       # [cp_in][co][ky'][kx']
    dyp = torch.zeros(dy.shape[0], cop, *dy.shape[2:], dtype=torch.float64)
    dyp[:, :c["Cout"]] = dy
    dx = O._taps(dyp, wk, 2, 0) if c["convT"] else O._taps(dyp, wk, 1, k - 1 - c["pad"])
    ref = torch.zeros_like(dx)
    ref[:, :c["Ca"]] = X.grad[:, :c["Ca"]]
    ref[:, g["ca"]:g["ca"] + c["Cb"]] = X.grad[:, c["Ca"]:]
    assert (dx - ref).abs().max() <= 1e-12 * ref.abs().max()


@pytest.mark.parametrize("mode", [0, 1])
def test_fragment_order_is_frag_pack(mode):
    from hiseg import ops
    e = dict(Cout=32, Cin_real=120, KH=3, KW=3, ca=64, ca_real=60, cb=64, cb_real=60, cop=64, mode=mode)
    e["rows"], e["K_pad"] = (32, 9 * 128) if mode == 0 else (128, 9 * 64)
    e["total"] = e["rows"] * e["K_pad"]
    e["src"] = torch.randn(32, 120, 3, 3, generator=O.gen(4), dtype=torch.float64)
    row_major = W.pack(e).view(e["rows"], e["K_pad"])
    frag = W.pack(dict(e, mode=mode | W.PACK_FRAG))
    assert torch.equal(frag, ops.frag_pack(row_major, 9, 128 if mode == 0 else 64))


def test_bias_pack():
    e = dict(Cout=6, Cin_real=4, KH=2, KW=2, ca=8, ca_real=4, cb=0, cb_real=0, cop=8, mode=W.PACK_BIAS, rows=1,
             K_pad=24, total=24, src=torch.arange(6.0))
    assert torch.equal(W.pack(e), torch.arange(6.0).double().repeat(4))


# ------------------------------------------------------------------------------------------- the tier A premise
@pytest.mark.parametrize("tab,name,case,dt", G.all_wgrad_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_tier_a_premise_of_every_gpu_case(tab, name, case, dt):
    """|x|, |dy| <= 2 (make_inputs): every partial sum of a weight-gradient element, in any order and over any subset
    of the M pixels, is an integer of magnitude <= 4 M (the bias column: 2 M; the ConvTranspose bias, summed over four
    columns by the reducer: 16 M with the factor below).  4 M < 2^22 makes each exactly representable in f32, and the
    reducer's accumulate onto |old| <= 3 stays below 2^23.  The operands themselves are exact in bf16."""
    bias = case.get("bias", False)
    g = W.geometry(case, dt, bias)
    bound = W.tier_a_bound(case, dt, bias)
    assert bound == 4 * g["M"] * (4 if g["convT"] and bias else 1)
    assert 4 * g["M"] < 2 ** 22 and bound + 3 < 2 ** 23
    c, xa, xb, dy = W.make_inputs({k: v for k, v in case.items() if k not in ("bias", "a_view", "dy_view")}, "A", dt)
    for t in (xa, xb, dy):
        if t is not None:
            assert t.abs().max() <= 2 and torch.equal(t, t.round()) and torch.equal(t.to(O.DTYPES[dt]).double(), t)
    # the launch constraints the entry point checks (wgrad_geometry): channel chunks of the dtype
    assert g["cols"] % W.CHUNK[dt] == 0 and (not g["convT"] or c["Cout"] % W.CHUNK[dt] == 0)


def test_tier_a_premise_of_the_reducer_cases():
    """Synthetic partials are integers of magnitude <= REDUCE_ABS over at most max(splits) planes (times 4 for the
    ConvTranspose bias), accumulated onto |old| <= REDUCE_OLD: below 2^23, every sum exact in f32 in any order."""
    smax = max(G.QUAD_SPLITS + G.TAPS_SPLITS)
    assert 4 * smax * G.REDUCE_ABS + G.REDUCE_OLD < 2 ** 23
    # the split counts pin the reducers' switches: the quad kernel's `sp += 32` wrap and the tap-major block shapes
    assert min(G.QUAD_SPLITS) == 1 and any(32 < s <= 64 for s in G.QUAD_SPLITS) and max(G.QUAD_SPLITS) > 64
    assert {64, 65} <= set(G.TAPS_SPLITS) and max(G.TAPS_SPLITS) > 128
    m = G.TAPS_MAP
    items = m["Cout"] * m["ca"] // 4
    assert items % 16 and items % 64 and m["ca"] == m["ca_real"] and m["cb"] == 0
    q = G.QUAD_MAP
    assert q["ca_real"] < q["ca"] and q["cb_real"] < q["cb"]
    assert (q["Cout"] * ((9 * (q["ca"] + q["cb"]) + 1 + 3) // 4)) % 64
