"""The two ends of the training step on their own against the float64 oracles of tests/loss_optim_oracle.py: every entry
point of csrc/train_loss.hip and csrc/optim.hip, called through hiseg._lib.

Inputs are rounded to f32 before either side sees them and nothing is excluded from a comparison.  Every output buffer
is filled with SENTINEL first and carries a guard tail that must be unchanged bit for bit afterwards (the loss workspace
too: the elements beyond hiseg_loss_ws(N, H, W); nothing here reads the workspace's contents).
tests/test_loss_optim_oracle.py proves on the CPU that the oracles are right and that every case table below keeps its
margins (LOSS_CASES is the list of all loss inputs used here).

Bounds.  The project's rule: |k - ref| <= 4 max(e32) + c * 2^-23 * M, e32 the distance of the oracle's float32
evaluation from its float64 evaluation (u = 2^-24 is the f32 unit round-off, 2^-23 = 2 u).

  gradients   element-wise: c = 4, M = max|ref|.
  loss sums   The main pass splits a plane of H W pixels into 16 ranges, a block of 256 threads each, so one thread adds
              m = ceil(ceil(H W / 16) / 256) terms and the block's tree has 8 levels: a term passes m + 8 f32 additions,
              each with relative error u on a partial sum <= M = sum |term|.  A term itself is built by at most R = 18
              rounded operations (the consistency term: softmax of three logits, a sigmoid, two additions and a square;
              a cross entropy takes 9 to 12) and the result is rounded once: c = (m + 8 + 18 + 1) / 2.  The rows are
              summed in double.  For a cross entropy lse - logit the operands cancel, so |term| is taken as
              |lse| + |logit| (times the class weight); for the contour term as max(x, 0) + |x t| + log1p(exp(-|x|)).
  outputs     bg/fg = S0 / S1 with S1 the sum of the class weights: c 2^-23 (M0 / S1 + |bg/fg|); target/non-target,
              final, consistency, boundary, contour, distance: c 2^-23 M / normaliser; dice of one ROI with
              q = (2 I + 1e-6) / D moves by (2 B_I + q (B_P + B_T)) / D, B_x = c 2^-23 x, averaged over the ROIs;
              the totals are the weighted sums of these.  Every output adds 2^-23 |ref| for its final cast.  Accuracy
              and IoU are quotients of exact counts and a clamped term is exactly 10: compared with float(ref)
              exactly.  The four class-weight outputs are casts of the double state: 2^-23 |ref|.
  norm        hiseg_grad_norm_partials: one thread adds ceil(n / 262144) squares, the tree has 8 levels, a square is
              one rounding and the partial one: c = (ceil(n / 262144) + 8 + 2) / 2, M = sum g^2; compared as the
              float64 sum of the 1024 partials.
  state       double arithmetic: 1e-12 relative; calls and tn_initialised exact.

hiseg_adamw_step_segmented's clipped g, m, v and norm_out are compared bit for bit with the oracle's float32
evaluation (the norm taken from the kernel's own partials, summed in float64 in index order); p under the element-wise
rule, because the bias corrections pass through a device pow.  That comparison found m one rounding apart in about a
tenth of the elements (test_adamw_segmented, every case, and the finite step of test_adamw_skip fail on the parent
commit): adamw_seg_kernel spelt its arithmetic with __fmul_rn / __fadd_rn / __fsub_rn, which the compiler treats as
plain operators, and it fused the lerp's product into the add (v_fmac_f32) or subtract (v_fma_f32) that consumes it.
The kernel now rounds each operation on its own (mul_r / add_r / sub_r in csrc/optim.hip), as its comment says.

Worst observed ratio of kernel error over bound per kernel (profiles/loss_optim_kernel_errors.txt, MI355X):

  kernel              ratio
  adamw_guarded       0.115
  adamw_segmented_p   0.112   p only; clipped g, m, v, norm_out are bit for bit
  adamw_step          0.115
  grad_norm_partials  0.175   per block and in total
  loss_dbgfg          0.327   worst with bg_weight = 0: only the small consistency gradient is left
  loss_dcont          0.137
  loss_ddist          0.060
  loss_dpred          0.188
  loss_dtn            0.127
  loss_out            0.134   the 16 outputs (accuracy, IoU and clamped terms compared exactly)
  (No ratio is above 0.5: the sum bounds are worst-case accumulation bounds, random data stays far below them.)

Entry point -> tests:
  hiseg_loss_state_init            test_loss_state_sequence
  hiseg_loss_ws                    every loss test (the workspace holds exactly that many elements before its guard)
  hiseg_loss_fwd                   test_loss_general, test_loss_grad_out_and_null_pointers, test_loss_target_maps,
                                   test_loss_geometry, test_loss_clamps, test_loss_class_weight_clamps,
                                   test_loss_state_sequence, test_loss_ties, test_loss_deterministic,
                                   test_loss_rejections
  hiseg_loss_fwd_begin / _fwd_end  test_loss_external_counts (also: hiseg_loss_fwd == _begin + _end bit for bit)
  hiseg_loss_bwd                   the same tests as hiseg_loss_fwd
  hiseg_grad_norm_partials         test_grad_norm_partials, and before every optimiser step below
  hiseg_adamw_step_segmented       test_adamw_segmented, test_adamw_skip, test_optim_rejections
  hiseg_adamw_step_segmented_dev   test_adamw_segmented_dev_and_graph
  hiseg_adamw_step_guarded         test_adamw_guarded_and_plain, test_adamw_guarded_skip
  hiseg_adamw_step                 test_adamw_guarded_and_plain
"""
import functools
import os

import numpy as np
import pytest
import torch

import filler
import loss_optim_oracle as O
from hiseg import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.5
GUARD = 64
BAD_ARG = -1
U23 = 2.0 ** -23
R_TERM = 18
RATIOS = {}
F32, F64 = np.float32, np.float64


def lib():
    return L.lib()


def stream():
    return L.stream_ptr()


def ok(status, what):
    L.check(status, what)
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    out = os.environ.get("HISEG_LOSS_OPTIM_KERNEL_ERRORS")
    if out:
        with open(out, "w") as f:
            f.write("# worst |kernel - float64 oracle| / bound per kernel (tests/test_gpu_loss_optim_kernels.py)\n")
            for kern, r in sorted(RATIOS.items()):
                f.write(f"{kern:24s} {r:.3f}\n")


def record(kernel, what, err, bound):
    err, bound = np.asarray(err, dtype=F64), np.broadcast_to(np.asarray(bound, dtype=F64), np.shape(err))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.where(err == 0, 0.0, err / bound).max())
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
    print(f"{kernel} {what}: max err {err.max():.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{kernel} {what}: error / bound = {ratio:.3f} (max err {err.max():.3e})"


def check_ew(kernel, what, k, r64, r32):
    """The element-wise rule: 4 max(e32) + 4 * 2^-23 max|ref|."""
    k, r64, r32 = np.asarray(k, F64).reshape(r64.shape), np.asarray(r64, F64), np.asarray(r32, F64)
    record(kernel, what, np.abs(k - r64), 4 * np.abs(r32 - r64).max() + 4 * U23 * np.abs(r64).max())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == F32 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Buf:
    """n values of a dtype on the device (the sentinel if vals is None) followed by a guard tail."""

    def __init__(self, vals=None, n=None, dtype=torch.float32, sentinel=SENTINEL):
        if vals is not None:
            vals = torch.as_tensor(np.ascontiguousarray(vals)).reshape(-1).to(dtype)
            n = vals.numel()
        flat = torch.full((n + GUARD,), sentinel, dtype=dtype)
        if vals is not None:
            flat[:n] = vals
        self.n, self.sentinel, self.t = n, sentinel, flat.to(DEV)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, *shape):
        a = self.t[:self.n].cpu().numpy()
        return a.reshape(*shape) if shape else a

    def assert_tail(self, written=None):
        tail = self.t[self.n if written is None else written:]
        assert torch.equal(tail, torch.full_like(tail, self.sentinel)), "wrote past the documented extent"


def ptr(b):
    return None if b is None else b.ptr


# =========================================================================================== loss: case tables
def _f32(a):
    return np.ascontiguousarray(a, dtype=F32)


def labels(kind, seed, N, H, W):
    rng = np.random.default_rng(seed)
    if kind == "ellipse":
        return filler.ellipse_targets(seed, N, H, W)
    if kind == "random":          # patches of random labels: every class and many boundaries at tiny sizes
        return rng.integers(0, 3, size=(N, H, W)).astype(np.int64)
    if kind == "bg":
        return np.zeros((N, H, W), np.int64)
    if kind == "fg_only":
        return np.maximum(filler.ellipse_targets(seed, N, H, W), 1)
    if kind == "one_fg":          # a single foreground pixel (class 1)
        t = np.zeros((N, H, W), np.int64)
        t[0, H // 2, W // 2] = 1
        return t
    if kind == "all_fg":          # classes 1 and 2 only
        return 1 + (rng.random((N, H, W)) < 0.3).astype(np.int64)
    if kind == "one_nt":          # all class 1 but a single class-2 pixel
        t = np.ones((N, H, W), np.int64)
        t[0, 1, 1] = 2
        return t
    raise KeyError(kind)


def make_case(kind, seed, N, H, W, ties=False, dist_mode="random"):
    """Loss inputs as f32 arrays.  Promised margins: no bg/fg logit difference within 2^-6 of zero (apart from the
    exact ties placed with ties=True); every dist - target exactly 0 or at least 2^-10 in size."""
    rng = np.random.default_rng(seed + 1000)
    tg = labels(kind, seed, N, H, W)
    pred = _f32(2.0 * rng.standard_normal((N, 3, H, W)))
    bgfg = _f32(2.0 * rng.standard_normal((N, 2, H, W)))
    tn = _f32(2.0 * rng.standard_normal((N, 2, H, W)))
    cont = _f32(rng.standard_normal((N, 1, H, W)))
    dist = _f32(rng.uniform(size=(N, 1, H, W)))
    near = np.abs(bgfg[:, 1].astype(F64) - bgfg[:, 0]) < 2.0 ** -5
    bgfg[:, 1][near] = bgfg[:, 0][near] + F32(0.25)
    dtg = O.distance_target(tg, F32)
    if dist_mode == "target":
        dist = dtg[:, None].copy()
    close = np.abs(dist[:, 0].astype(F64) - dtg) < 2.0 ** -9
    if dist_mode != "target":
        dist[:, 0][close] = dtg[close] + F32(2.0 ** -4)
    if ties:
        flat = rng.permutation(N * H * W)[:max(2, N * H * W // 16)]
        n, y, x = np.unravel_index(flat, (N, H, W))
        bgfg[n, 1, y, x] = bgfg[n, 0, y, x]                      # exact bg/fg ties: argmax takes index 0
        pred[n, 1, y, x] = pred[n, 0, y, x] = np.maximum(pred[n, 0, y, x], pred[n, 2, y, x]) + F32(0.5)   # equal top logits
        n2, y2, x2 = np.unravel_index(rng.permutation(N * H * W)[:max(2, N * H * W // 8)], (N, H, W))
        dist[n2, 0, y2, x2] = dtg[n2, y2, x2]                    # dist == target exactly
    return dict(pred=pred, bgfg=bgfg, tn=tn, cont=cont, dist=dist, tg=tg, name=f"{kind}-{seed}-{N}x{H}x{W}",
                ties=ties)


def clamp_case(which):
    """One batch whose boundary / contour / distance term lands above 11 (the others stay below 9)."""
    c = make_case("ellipse", 61, 2, 12, 16)
    tg = c["tg"]
    if which == "ba":       # the true class 20 below the others: cross entropy ~ 20 at every pixel
        oh = np.stack([tg == 0, tg == 1, tg == 2], 1)
        c["pred"] = _f32(np.where(oh, -20.0, 0.0) + 0.125 * c["pred"])
    elif which == "contour":  # logit -30 on the contour, +30 off it: binary cross entropy 30 at every pixel
        c["cont"] = _f32(np.where(O.contour_target(tg, 3) > 0, -30.0, 30.0))[:, None]
    elif which == "dist":
        c["dist"] = _f32(np.full_like(c["dist"], 20.0))
    c["name"] = f"clamp-{which}"
    return c


BASE_W = ("bg_weight", "fg_weight", "consistency_weight", "dice_weight", "ce_weight")


def general_cfgs():
    cf = [("all", O.make_cfg(contour_ks=5)), ("static", O.make_cfg(contour_ks=5, use_dynamic_weights=0))]
    for k in ("use_boundary_aware", "use_contour", "use_distance"):
        cf.append((f"{k}=0", O.make_cfg(contour_ks=5, **{k: 0})))
    for k in BASE_W:
        cf.append((f"{k}=0", O.make_cfg(contour_ks=5, **{k: 0.0})))
    for ks in (1, 3, 5, 7, 11):
        cf.append((f"ks={ks}", O.make_cfg(contour_ks=ks)))
    return cf


@functools.lru_cache(maxsize=None)
def general_case():
    return make_case("ellipse", 7, 3, 24, 32)


# (name, N, H, W, label kind): the smallest shapes that reach each path of the launch geometry
GEOMETRY = [("tiny", 1, 3, 5, "random"),          # a plane of fewer than 16 pixels: empty splits
            ("rows80", 5, 4, 4, "random"),        # 80 and 112 partial rows: both tails of the finalize loops
            ("rows112", 7, 4, 4, "random"),
            ("n257", 257, 4, 4, "random"),        # the strided per-ROI dice loop
            ("n300", 300, 4, 4, "random"),
            ("stride", 5, 128, 112, "ellipse"),   # 71 680 pixels: loss_targets_kernel's loop runs twice
            ("cap", 17, 256, 256, "ellipse")]     # 1 114 112 pixels: the 4096-block cap of the element-wise kernels
GEOMETRY_KS = {"cap": 11, "stride": 7}


@functools.lru_cache(maxsize=None)
def geometry_case(name):
    _, N, H, W, kind = next(g for g in GEOMETRY if g[0] == name)
    return make_case(kind, 40 + N, N, H, W)


# (name, label kind, N, H, W): target mixes that push each class weight to a clamp
WEIGHT_CLAMPS = [("one_fg", "one_fg", 1, 8, 8), ("all_fg", "all_fg", 1, 8, 8), ("one_nt", "one_nt", 1, 8, 8)]
# (name, N, H, W, ks): target maps through the public surface
MAP_CASES = [("ellipse", 3, 24, 32, 1), ("ellipse", 3, 24, 32, 3), ("ellipse", 3, 24, 32, 11), ("random", 2, 4, 5, 11),
             ("random", 2, 1, 9, 3), ("random", 2, 9, 1, 3), ("random", 1, 1, 1, 3)]
STATE_SEQS = {"ellipse_first": ("ellipse", "bg", "ellipse", "fg_only"), "bg_first": ("bg", "ellipse", "bg", "all_fg")}


def state_case(kind, i):
    return make_case(kind, 80 + i, 2, 16, 12)


def loss_cases():
    """Every (name, cfg, case) the loss tests below evaluate: the CPU test checks margins and map equality on these."""
    out = [(f"general/{n}", cfg, general_case()) for n, cfg in general_cfgs()]
    out += [(f"geometry/{g[0]}", O.make_cfg(contour_ks=GEOMETRY_KS.get(g[0], 3)), geometry_case(g[0])) for g in GEOMETRY]
    out += [(f"clamp/{w}", O.make_cfg(contour_ks=3), clamp_case(w)) for w in ("ba", "contour", "dist")]
    out += [("clamp/none", O.make_cfg(contour_ks=3), make_case("ellipse", 61, 2, 12, 16))]
    out += [(f"weights/{n}", O.make_cfg(contour_ks=3), make_case(kind, 70, N, H, W)) for n, kind, N, H, W in WEIGHT_CLAMPS]
    out += [(f"maps/{k}-{N}x{H}x{W}-ks{ks}", O.make_cfg(contour_ks=ks), make_case(k, 90, N, H, W))
            for k, N, H, W, ks in MAP_CASES]
    for sname, seq in STATE_SEQS.items():
        out += [(f"state/{sname}/{i}", O.make_cfg(contour_ks=3), state_case(k, i)) for i, k in enumerate(seq)]
    out += [("ties", O.make_cfg(contour_ks=3), make_case("ellipse", 33, 2, 12, 20, ties=True))]
    out += [("counts/local", O.make_cfg(contour_ks=3), make_case("ellipse", 21, 2, 16, 12)),
            ("counts/other", O.make_cfg(contour_ks=3), make_case("fg_only", 22, 2, 16, 12))]
    return out


LOSS_CASES = loss_cases


# =========================================================================================== loss: harness
def cfg_struct(cfg):
    c = L.LossCfg()
    for k in O.CFG_FLOATS + O.CFG_INTS:
        setattr(c, k, cfg[k])
    return c


GRADS = ("pred", "bgfg", "tn", "cont", "dist")


class LossRun:
    """One hiseg_loss_fwd (or _begin + _end) and hiseg_loss_bwd on fresh sentinel-filled buffers."""

    def __init__(self, cfg, case, state=None, grad_out=None, null=(), two_phase=False, counts_in=None,
                 want_counts=False, backward=True):
        N, _, H, W = case["pred"].shape
        self.N, self.H, self.W = N, H, W
        cs = cfg_struct(cfg)
        dev = {k: (None if k in null else torch.from_numpy(case[k]).to(DEV)) for k in GRADS}
        tg = torch.from_numpy(case["tg"]).to(DEV)
        nws = int(lib().hiseg_loss_ws(N, H, W))
        self.ws = Buf(n=nws)
        assert self.ws.ptr % 8 == 0
        self.out = Buf(n=O.NOUT)
        if state is None:
            self.state = Buf(n=8, dtype=torch.float64)
            ok(lib().hiseg_loss_state_init(self.state.ptr, stream()), "loss_state_init")
        else:
            self.state = state
        p = lambda k: None if dev[k] is None else dev[k].data_ptr()
        self.counts = Buf(n=4, dtype=torch.float64) if want_counts else None
        if two_phase:
            ok(lib().hiseg_loss_fwd_begin(cs, N, H, W, tg.data_ptr(), self.ws.ptr, ptr(self.counts), stream()),
               "loss_fwd_begin")
            cin = None if counts_in is None else Buf(counts_in, dtype=torch.float64)
            ok(lib().hiseg_loss_fwd_end(cs, N, H, W, p("pred"), p("bgfg"), p("tn"), p("cont"), p("dist"),
                                        tg.data_ptr(), ptr(cin), self.state.ptr, self.ws.ptr, self.out.ptr, stream()),
               "loss_fwd_end")
        else:
            ok(lib().hiseg_loss_fwd(cs, N, H, W, p("pred"), p("bgfg"), p("tn"), p("cont"), p("dist"), tg.data_ptr(),
                                    self.state.ptr, self.ws.ptr, self.out.ptr, stream()), "loss_fwd")
        self.grads = {}
        if backward:
            self.go = None if grad_out is None else Buf(np.array([grad_out], F32))
            self.gbuf = {k: (None if ("d" + k) in null else Buf(n=case[k].size)) for k in GRADS}
            g = self.gbuf
            ok(lib().hiseg_loss_bwd(cs, N, H, W, p("pred"), p("bgfg"), p("tn"), p("cont"), p("dist"), tg.data_ptr(),
                                    self.ws.ptr, ptr(self.go), ptr(g["pred"]), ptr(g["bgfg"]), ptr(g["tn"]),
                                    ptr(g["cont"]), ptr(g["dist"]), stream()), "loss_bwd")
            for k, b in g.items():
                if b is not None:
                    b.assert_tail()
                    self.grads[k] = b.get(*case[k].shape)
            if self.go is not None:
                self.go.assert_tail()
        for b in (self.ws, self.out, self.state, self.counts):
            if b is not None:
                b.assert_tail()
        for k in GRADS:          # the inputs are read-only
            if dev[k] is not None:
                assert same_bits(dev[k].cpu().numpy(), case[k]), k
        assert np.array_equal(tg.cpu().numpy(), case["tg"])
        self.o = self.out.get()
        self.st = self.state.get()


def scalar_bounds(cfg, N, H, W, o64, o32, X):
    """Bound of each of the 16 outputs (module docstring) and the value to compare with."""
    P = N * H * W
    m = -(-(-(-(H * W) // 16)) // 256)
    cu = (m + 8 + R_TERM + 1) / 2 * U23
    T = X["terms"]
    cast = U23 * np.abs(o64)
    B = np.zeros(O.NOUT)
    exact = np.zeros(O.NOUT, bool)
    sw, fgl = float(X["sw"]), max(float(X["counts"][1]), 1.0)
    B[1] = cu * (T["mag_bf"].sum() / sw + abs(o64[1]))
    B[2] = cu * T["mag_tn"].sum() / fgl
    B[3] = cu * T["mag_fin"].sum() / P
    B[4] = cu * T["term_cons"].sum() / P
    B[5] = ((2 * cu * X["I"] + X["q"] * cu * (X["Ps"] + X["Ts"])) / X["D"]).mean()
    for i, key, mag in ((6, "ba", "mag_ba"), (7, "contour", "mag_ct"), (8, "dist", "term_d")):
        if key in X["raw"]:
            if X["raw"][key] > O.CLAMP:
                exact[i] = True
            else:
                B[i] = cu * T[mag].sum() / P
    base = (("bg_weight", 1), ("fg_weight", 2), ("ce_weight", 3), ("dice_weight", 5), ("consistency_weight", 4))
    refine = (("boundary_aware_weight", 6), ("contour_weight", 7), ("distance_weight", 8))
    B[15] = sum(abs(cfg[k]) * (B[i] + cast[i]) for k, i in base)
    B[0] = B[15] + sum(abs(cfg[k]) * (B[i] + cast[i]) for k, i in refine)
    exact[9] = exact[10] = True
    bound = np.where(exact, 0.0, 4 * np.abs(o32.astype(F64) - o64) + B + cast)
    ref = np.where(exact, o64.astype(F32).astype(F64), o64)
    return ref, bound


def oracle(cfg, case, state=None, counts=None, grad_out=1.0):
    st = O.state_init() if state is None else state
    a = (cfg, case["pred"], case["bgfg"], case["tn"], case["cont"], case["dist"], case["tg"], st)
    return O.loss_eval(*a, counts=counts, grad_out=grad_out), O.loss_eval(*a, counts=counts, grad_out=grad_out, dt=F32)


def check_loss(run, cfg, case, what, state=None, counts=None, grad_out=1.0, kernel="loss_out"):
    (o64, g64, st64, X), (o32, g32, _, _) = oracle(cfg, case, state, counts, grad_out)
    ref, bound = scalar_bounds(cfg, run.N, run.H, run.W, o64, o32, X)
    record(kernel, what, np.abs(run.o.astype(F64) - ref), bound)
    for k, g in run.grads.items():
        check_ew("loss_d" + k, what, g, g64[k], g32[k])
    assert run.st[4] == st64[4] and run.st[7] == st64[7], "tn_initialised / calls"
    np.testing.assert_allclose(run.st, st64, rtol=1e-12, atol=0, err_msg="EMA state")
    return o64, g64, st64, X


# =========================================================================================== loss: tests
@pytest.mark.parametrize("name", [n for n, _ in general_cfgs()])
def test_loss_general(name):
    """N = 3, 24 x 32, ellipse targets, over the configuration matrix: outputs and all five gradients."""
    cfg = dict(general_cfgs())[name]
    case = general_case()
    run = LossRun(cfg, case)
    check_loss(run, cfg, case, name)


def test_loss_deterministic():
    cfg, case = O.make_cfg(contour_ks=5), general_case()
    a, b = LossRun(cfg, case), LossRun(cfg, case)
    assert same_bits(a.o, b.o) and same_bits(a.st, b.st)
    for k in GRADS:
        assert same_bits(a.grads[k], b.grads[k]), k


def test_loss_grad_out_and_null_pointers():
    """grad_out 0.375, -2 and null (= 1); each gradient pointer null in turn leaves the others bit-identical; cont and
    dist null with their terms off: dcont / ddist, if passed, are all zero."""
    cfg, case = O.make_cfg(contour_ks=5), general_case()
    full = LossRun(cfg, case)
    check_loss(full, cfg, case, "grad_out null")
    for go in (0.375, -2.0, 1.0):
        r = LossRun(cfg, case, grad_out=go)
        check_loss(r, cfg, case, f"grad_out {go}", grad_out=go)
        assert same_bits(r.o, full.o)
        if go == 1.0:
            for k in GRADS:
                assert same_bits(r.grads[k], full.grads[k]), k
    for k in GRADS:
        r = LossRun(cfg, case, null=("d" + k,))
        assert set(r.grads) == set(GRADS) - {k}
        for j in r.grads:
            assert same_bits(r.grads[j], full.grads[j]), (k, j)
    off = O.make_cfg(contour_ks=5, use_contour=0, use_distance=0)
    r = LossRun(off, case, null=("cont", "dist"))
    case_off = dict(case, cont=None, dist=None)
    check_loss(LossRun(off, case), off, case, "terms off, pointers given")
    (o64, g64, _, X), (o32, _, _, _) = oracle(off, case_off)
    ref, bound = scalar_bounds(off, r.N, r.H, r.W, o64, o32, X)
    record("loss_out", "cont / dist null", np.abs(r.o.astype(F64) - ref), bound)
    assert not r.grads["cont"].any() and not r.grads["dist"].any()
    r2 = LossRun(off, case, null=("cont", "dist", "dcont", "ddist"))
    for j in ("pred", "bgfg", "tn"):
        assert same_bits(r2.grads[j], r.grads[j]), j


def only(weight, **kw):
    """A configuration with every weight 0 but one."""
    z = {k: 0.0 for k in O.CFG_FLOATS if k != "target_weight"}
    z.update(use_boundary_aware=0, use_contour=0, use_distance=0, use_dynamic_weights=0)
    z.update(kw)
    z[weight] = 0.5
    return O.make_cfg(**z)


@pytest.mark.parametrize("kind,N,H,W,ks", MAP_CASES)
def test_loss_target_maps(kind, N, H, W, ks):
    """The three target maps recovered through the public surface must equal the oracle's exactly: the boundary weight
    as dpred of a boundary-only run over dpred of a cross-entropy-only run, the dilated contour target as the sign of
    dcont at cont = 0, the distance target by placing dist on the oracle's map (gradient exactly 0) and 2^-10 either side of it."""
    case = make_case(kind, 90, N, H, W)
    tg = case["tg"]
    ba = LossRun(only("boundary_aware_weight", use_boundary_aware=1), case).grads["pred"].astype(F64)
    ce = LossRun(only("ce_weight"), case).grads["pred"].astype(F64)
    assert (ce != 0).all()
    bw = O.boundary_weight(tg)
    assert np.array_equal(ba / ce, np.broadcast_to(bw[:, None], ba.shape)), "boundary weight map"
    cfg_c = only("contour_weight", use_contour=1, contour_ks=ks)
    dc = LossRun(cfg_c, dict(case, cont=np.zeros_like(case["cont"]))).grads["cont"][:, 0]
    assert (dc != 0).all()
    assert np.array_equal((dc < 0).astype(F64), O.contour_target(tg, ks)), "dilated contour target"
    cfg_d = only("distance_weight", use_distance=1)
    dtg = O.distance_target(tg, F32)
    assert np.array_equal(dtg.astype(F64), O.distance_target(tg, F64))
    zero = dict(case, dist=np.zeros_like(case["dist"]))
    check_loss(LossRun(cfg_d, zero), cfg_d, zero, f"distance loss at dist = 0 {kind} {N}x{H}x{W}")
    step = F32(2.0 ** -10)
    for place, sign in ((dtg, 0.0), (dtg + step, 1.0), (dtg - step, -1.0)):
        assert np.array_equal(place.astype(F64), dtg.astype(F64) + sign * 2.0 ** -10)      # placed exactly
        dd = LossRun(cfg_d, dict(case, dist=_f32(place[:, None]))).grads["dist"]
        assert np.array_equal(np.sign(dd), np.full_like(dd, sign)), f"distance target map ({sign:+.0f})"


@pytest.mark.parametrize("name", [g[0] for g in GEOMETRY])
def test_loss_geometry(name):
    cfg = O.make_cfg(contour_ks=GEOMETRY_KS.get(name, 3))
    case = geometry_case(name)
    check_loss(LossRun(cfg, case), cfg, case, name)


@pytest.mark.parametrize("which", ["ba", "contour", "dist"])
def test_loss_clamps(which):
    """A term above 11 is reported as exactly 10 and contributes exactly nothing to the gradients; below 9 it is
    unclamped (clamp/none, which test_loss_general's cases are too)."""
    cfg = O.make_cfg(contour_ks=3)
    case = clamp_case(which)
    run = LossRun(cfg, case)
    o64, _, _, X = check_loss(run, cfg, case, f"clamp {which}")
    idx, flag = {"ba": (6, "use_boundary_aware"), "contour": (7, "use_contour"), "dist": (8, "use_distance")}[which]
    assert X["raw"][which] > 11 and run.o[idx] == 10.0
    off = LossRun(O.make_cfg(contour_ks=3, **{flag: 0}), case)
    if which == "ba":
        assert same_bits(run.grads["pred"], off.grads["pred"])
    else:
        assert not run.grads["cont" if which == "contour" else "dist"].any()
    base = make_case("ellipse", 61, 2, 12, 16)
    o64, _, _, X = check_loss(LossRun(cfg, base), cfg, base, "clamp none")
    assert all(v < 9 for v in X["raw"].values())


@pytest.mark.parametrize("name,kind,N,H,W", WEIGHT_CLAMPS)
def test_loss_class_weight_clamps(name, kind, N, H, W):
    """A single foreground pixel, all foreground, a single class-2 pixel: the 0.5 and 3.0 clamps of the class weights."""
    cfg = O.make_cfg(contour_ks=3)
    case = make_case(kind, 70, N, H, W)
    _, _, _, X = check_loss(LossRun(cfg, case), cfg, case, name)
    assert any(r > 3.0 for r in X["raw_weights"]), X["raw_weights"]


@pytest.mark.parametrize("seq", list(STATE_SEQS))
def test_loss_state_sequence(seq):
    """Four consecutive calls on one state; all eight state values after each.  bg_first reaches the first-call branch
    of the target/non-target EMA after a call without foreground."""
    cfg = O.make_cfg(contour_ks=3)
    state = Buf(n=8, dtype=torch.float64)
    ok(lib().hiseg_loss_state_init(state.ptr, stream()), "loss_state_init")
    assert np.array_equal(state.get(), O.state_init())
    state.assert_tail()
    st = O.state_init()
    for i, kind in enumerate(STATE_SEQS[seq]):
        case = state_case(kind, i)
        run = LossRun(cfg, case, state=state)
        _, _, st, _ = check_loss(run, cfg, case, f"{seq} call {i} ({kind})", state=st)
        assert st[7] == i + 1


def test_loss_external_counts():
    """_begin reports this batch's counts exactly; _end's weights follow the counts it is given (a two-rank sum), the
    target/non-target normalisation this batch's own foreground count; hiseg_loss_fwd == _begin + _end(null)."""
    cfg = O.make_cfg(contour_ks=3)
    case, other = make_case("ellipse", 21, 2, 16, 12), make_case("fg_only", 22, 2, 16, 12)
    local = O.class_counts(case["tg"])
    total = local + O.class_counts(other["tg"])
    assert total[1] != local[1]
    run = LossRun(cfg, case, two_phase=True, counts_in=total, want_counts=True)
    assert np.array_equal(run.counts.get(), local)
    o64, _, _, _ = check_loss(run, cfg, case, "external counts", counts=total)
    (own, _, _, _), _ = oracle(cfg, case)
    assert abs(o64[2] - own[2]) > 1e-3 * abs(own[2]), "the case does not tell the two counts apart"
    one = LossRun(cfg, case)
    two = LossRun(cfg, case, two_phase=True)
    assert same_bits(one.o, two.o) and same_bits(one.st, two.st)
    for k in GRADS:
        assert same_bits(one.grads[k], two.grads[k]), k


def test_loss_ties():
    """Exact bg/fg ties and equal top logits: accuracy and IoU equal the oracle's counts (scalar_bounds compares them
    exactly); dist == target exactly: the gradient there is 0."""
    cfg = O.make_cfg(contour_ks=3)
    case = make_case("ellipse", 33, 2, 12, 20, ties=True)
    run = LossRun(cfg, case)
    _, g64, _, X = check_loss(run, cfg, case, "ties")
    tie = case["bgfg"][:, 0] == case["bgfg"][:, 1]
    assert tie.sum() >= 2 and (tie & (case["tg"] > 0)).any() and (tie & (case["tg"] == 0)).any()
    at = X["terms"]["r"] == 0
    assert at.sum() >= 2 and not run.grads["dist"][:, 0][at].any() and (run.grads["dist"][:, 0][~at] != 0).all()


def test_loss_rejections():
    """HISEG_ERR_BAD_ARG, nothing launched: out, workspace and state keep the sentinel."""
    case = make_case("ellipse", 7, 2, 8, 8)
    N, _, H, W = case["pred"].shape
    dev = {k: torch.from_numpy(case[k]).to(DEV) for k in GRADS}
    tg = torch.from_numpy(case["tg"]).to(DEV)
    ws, out, state = Buf(n=int(lib().hiseg_loss_ws(N, H, W)) + 2), Buf(n=O.NOUT), Buf(n=8, dtype=torch.float64)

    def call(cfg, n=N, cont=True, dist=True, ws_off=0):
        p = lambda k: dev[k].data_ptr()
        st = lib().hiseg_loss_fwd(cfg_struct(cfg), n, H, W, p("pred"), p("bgfg"), p("tn"), p("cont") if cont else None,
                                  p("dist") if dist else None, tg.data_ptr(), state.ptr, ws.ptr + 4 * ws_off, out.ptr,
                                  stream())
        torch.cuda.synchronize()
        assert st == BAD_ARG, st
        for b in (ws, out, state):
            b.assert_tail(0)

    call(O.make_cfg(), cont=False)
    call(O.make_cfg(), dist=False)
    call(O.make_cfg(), ws_off=1)
    call(O.make_cfg(), n=0)
    st = lib().hiseg_loss_fwd_begin(cfg_struct(O.make_cfg()), N, H, W, tg.data_ptr(), ws.ptr + 4, None, stream())
    torch.cuda.synchronize()
    assert st == BAD_ARG
    ws.assert_tail(0)


# =========================================================================================== optimiser
OPT_N = [1, 255, 262144 + 777, 3 * 262144 + 5]
H_ = O.hyper()
STEP_CHOICES = [0, 1, 9, 999, 100000]


def opt_inputs(n, seed):
    rng = np.random.default_rng(seed)
    p = _f32(rng.standard_normal(n))
    g = _f32(0.1 * rng.standard_normal(n))
    m = _f32(0.05 * rng.standard_normal(n))
    v = _f32(0.01 * rng.random(n) + 1e-4)
    return p, g, m, v


def seg_table(kind, n, seed=0):
    """seg_start[nseg + 1]: 1 segment; 8 at boundaries that are no multiple of 256; 256 with empty and 1-element
    segments, a boundary inside a wavefront (37) and one at n - 1."""
    rng = np.random.default_rng(seed + n)
    if kind == 1:
        return np.array([0, n], np.int64)
    if kind == 8:
        b = rng.integers(0, n + 1, 7)
        b = np.where((b % 256 == 0) & (b > 0) & (b < n), b + 3, b)
    else:
        b = np.concatenate([[0, 1, 37, 37, 38, n - 1, n - 1], rng.integers(0, n + 1, 248)])
    b = np.sort(np.clip(b, 0, n))
    return np.concatenate([[0], b, [n]]).astype(np.int64)


def seg_steps(nseg, seed=0):
    return np.random.default_rng(seed + nseg).choice(STEP_CHOICES, nseg).astype(np.int32)


class OptRun:
    """p, g, m, v, partial, norm_out, steps[2][nseg], skipped on the device, each with a guard tail."""

    def __init__(self, p, g, m, v, seg_start=None, steps=None, parity=0, skipped=3):
        self.n = p.size
        self.p, self.g, self.m, self.v = Buf(p), Buf(g), Buf(m), Buf(v)
        self.partial, self.norm = Buf(n=O.OPT_BLOCKS), Buf(n=1)
        self.parity = parity
        self.nseg = 1 if seg_start is None else len(seg_start) - 1
        self.seg = Buf(np.array([0, self.n], np.int64) if seg_start is None else seg_start, dtype=torch.int64,
                       sentinel=-5)
        st = np.full((2, self.nseg), -5, np.int32)
        st[parity] = 0 if steps is None else steps
        self.steps = Buf(st, dtype=torch.int32, sentinel=-5)
        self.skipped = Buf(np.array([skipped], np.int32), dtype=torch.int32, sentinel=-5)

    def partials(self):
        ok(lib().hiseg_grad_norm_partials(self.g.ptr, self.n, self.partial.ptr, stream()), "grad_norm_partials")
        self.partial.assert_tail()
        return self.partial.get().astype(F64)

    def segmented(self, h, max_norm, dev=None, sync=True):
        a = (self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.n)
        b = (self.partial.ptr, float(max_norm), self.norm.ptr, self.seg.ptr, self.nseg, self.steps.ptr, self.parity,
             self.skipped.ptr, stream())
        if dev is None:
            st = lib().hiseg_adamw_step_segmented(*a, h["lr"], h["b1"], h["b2"], h["omb1"], h["omb2"], h["decay"],
                                                  h["eps"], *b)
        else:
            st = lib().hiseg_adamw_step_segmented_dev(*a, dev.data_ptr(), h["b1"], h["b2"], h["omb1"], h["omb2"],
                                                      h["eps"], *b)
        L.check(st, "adamw_step_segmented")
        if sync:
            torch.cuda.synchronize()

    def guarded(self, h, max_norm):
        ok(lib().hiseg_adamw_step_guarded(self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.n, h["lr"], h["b1"],
                                          h["b2"], h["eps"], h["wd"], self.partial.ptr, float(max_norm), self.norm.ptr,
                                          self.steps.ptr, self.parity, self.skipped.ptr, stream()), "adamw_guarded")

    def plain(self, h, bc1, bc2, max_norm, with_partial=True):
        ok(lib().hiseg_adamw_step(self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.n, h["lr"], h["b1"], h["b2"],
                                  h["eps"], h["wd"], bc1, bc2, self.partial.ptr if with_partial else None,
                                  float(max_norm), self.norm.ptr, stream()), "adamw_step")

    def arrays(self):
        return self.p.get(), self.g.get(), self.m.get(), self.v.get()

    def assert_tails(self):
        for b in (self.p, self.g, self.m, self.v, self.partial, self.norm, self.seg, self.steps, self.skipped):
            b.assert_tail()


@pytest.mark.parametrize("n", OPT_N)
def test_grad_norm_partials(n):
    """The float64 sum of the 1024 partials against the float64 sum of squares; a block without elements writes 0."""
    _, g, _, _ = opt_inputs(n, n)
    r = OptRun(g, g, g, g)
    part = r.partials()
    ref = O.grad_norm_partials_ref(g)
    empty = np.arange(O.OPT_BLOCKS) >= -(-n // 256)
    assert not part[empty].any() and (n >= 262144 or empty.any())
    c = (-(-n // 262144) + 8 + 2) / 2
    g32 = g * g
    e32 = abs(float(g32.sum(dtype=F32)) - ref.sum())
    record("grad_norm_partials", f"n={n}", np.abs(part.sum() - ref.sum()), 4 * e32 + c * U23 * ref.sum())
    record("grad_norm_partials", f"n={n} per block", np.abs(part - ref), c * U23 * ref + 1e-300)


def run_segmented(n, kind, clip, parity, seed=0):
    p, g, m, v = opt_inputs(n, seed + n)
    seg, steps = seg_table(kind, n), None
    steps = seg_steps(len(seg) - 1, seed)
    r = OptRun(p, g, m, v, seg, steps, parity)
    part = r.partials()
    norm = O.norm_from_partials(part)
    max_norm = {"off": 0.0, "inactive": 4.0 * float(norm) + 1.0, "active": 0.25 * float(norm)}[clip]
    r.segmented(H_, max_norm)
    r.assert_tails()
    kp, kg, km, kv = r.arrays()
    p32, g32, m32, v32, s2, sk = O.adamw_segmented(p, g, m, v, H_, norm, max_norm, seg, steps, F32)
    p64, *_ = O.adamw_segmented(p, g, m, v, H_, norm, max_norm, seg, steps, F64)
    what = f"n={n} nseg={kind} clip={clip} parity={parity}"
    assert same_bits(r.norm.get(), np.array([norm], F32)), "norm_out"
    if clip != "active":
        assert same_bits(kg, g), "g changed without an active clip"
    assert same_bits(kg, g32), "clipped g"
    assert same_bits(km, m32), "m"
    assert same_bits(kv, v32), "v"
    check_ew("adamw_segmented_p", what, kp, p64, p32)
    st = r.steps.get(2, len(steps))
    assert np.array_equal(st[0], steps + 1) and np.array_equal(st[1], steps + 1), "both parity slots hold t + 1"
    assert r.skipped.get()[0] == 3
    return r


@pytest.mark.parametrize("n", OPT_N)
@pytest.mark.parametrize("kind", [1, 8, 256])
def test_adamw_segmented(n, kind):
    for clip, parity in (("off", 0), ("inactive", 1), ("active", 0), ("active", 1)):
        run_segmented(n, kind, clip, parity)


def test_adamw_segmented_dev_and_graph():
    """[lr, 1 - lr wd] in a device buffer: bit-identical to the scalar-argument call; one captured step replayed three
    times with the buffer updated in between equals three eager steps bit for bit."""
    n = OPT_N[2]
    p, g, m, v = opt_inputs(n, 5)
    seg, steps = seg_table(8, n), seg_steps(8, 1)
    a, b = OptRun(p, g, m, v, seg, steps), OptRun(p, g, m, v, seg, steps)
    hyp = torch.tensor([H_["lr"], H_["decay"]], dtype=torch.float32, device=DEV)
    a.partials(), b.partials()
    a.segmented(H_, 1.0)
    b.segmented(H_, 1.0, dev=hyp)
    for x, y in zip(a.arrays() + (a.steps.get(), a.norm.get()), b.arrays() + (b.steps.get(), b.norm.get())):
        assert same_bits(x, y)
    sched = [O.hyper(lr=lr) for lr in (1e-3, 7e-4, 2e-4)]
    eager, graphed = OptRun(p, g, m, v, seg, steps), OptRun(p, g, m, v, seg, steps)

    def step(r, sync):
        L.check(lib().hiseg_grad_norm_partials(r.g.ptr, r.n, r.partial.ptr, stream()), "grad_norm_partials")
        r.segmented(H_, 1.0, dev=hyp, sync=sync)

    for h in sched:
        hyp.copy_(torch.tensor([h["lr"], h["decay"]], dtype=torch.float32))
        step(eager, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(graphed, False)
    for h in sched:
        hyp.copy_(torch.tensor([h["lr"], h["decay"]], dtype=torch.float32))
        graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager.arrays() + (eager.steps.get(),), graphed.arrays() + (graphed.steps.get(),)):
        assert same_bits(x, y)
    assert np.array_equal(eager.steps.get(2, 8)[0], steps + 3)
    graphed.assert_tails()
    # the eager steps against the oracle, so that "equal" is not "equally wrong"
    q = (p, g, m, v, steps)
    for h in sched:
        norm = O.norm_from_partials(O.grad_norm_partials_ref(q[1]))
        q64 = O.adamw_segmented(*q[:4], h, norm, 1.0, seg, q[4], F64)
        q = O.adamw_segmented(*q[:4], h, norm, 1.0, seg, q[4], F32)[:5]
    check_ew("adamw_segmented_p", "three scheduled steps", eager.p.get(), q64[0], q[0])


def skip_cases(n):
    out = []
    for bad in (np.nan, np.inf):
        out += [(f"{bad}@0", {0: bad}), (f"{bad}@n-1", {n - 1: bad})]
        i = 1023 * 256 + 5                # an index only block 1023 reads
        if i < n:
            out.append((f"{bad}@block1023", {i: bad}))
    out.append(("overflow", "overflow"))
    return out


@pytest.mark.parametrize("n", OPT_N)
def test_adamw_skip(n):
    """A non-finite norm: p, g, m, v and the step counts unchanged bit for bit, skipped + 1, norm_out non-finite, and
    the next finite step is the oracle's step t + 1."""
    p, g, m, v = opt_inputs(n, 11 + n)
    seg, steps = seg_table(8, n), seg_steps(8, 2)
    for name, bad in skip_cases(n):
        gb = g.copy()
        if bad == "overflow":             # all finite, the sum of squares overflows f32
            gb[:] = np.where(np.arange(n) % 2 == 0, 2e19, -2e19).astype(F32)
            assert np.isfinite(gb).all()
        else:
            for i, val in bad.items():
                gb[i] = val
        r = OptRun(p, gb, m, v, seg, steps, parity=1)
        r.partials()
        r.segmented(H_, 1.0)
        r.assert_tails()
        for x, y in zip(r.arrays(), (p, gb, m, v)):
            assert same_bits(x, y), name
        st = r.steps.get(2, 8)
        assert np.array_equal(st[0], steps) and np.array_equal(st[1], steps), name
        assert r.skipped.get()[0] == 4 and not np.isfinite(r.norm.get()[0]), name
        r.g.t[:n] = torch.from_numpy(g).to(DEV)
        part = r.partials()
        norm = O.norm_from_partials(part)
        r.segmented(H_, 1.0)
        p32, g32, m32, v32, s2, _ = O.adamw_segmented(p, g, m, v, H_, norm, 1.0, seg, steps, F32)
        p64, *_ = O.adamw_segmented(p, g, m, v, H_, norm, 1.0, seg, steps, F64)
        kp, kg, km, kv = r.arrays()
        assert same_bits(km, m32) and same_bits(kv, v32) and same_bits(kg, g32), name
        check_ew("adamw_segmented_p", f"n={n} after skip {name}", kp, p64, p32)
        assert np.array_equal(r.steps.get(2, 8), np.stack([steps + 1, steps + 1])) and r.skipped.get()[0] == 4


@pytest.mark.parametrize("n", OPT_N)
@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_adamw_guarded_and_plain(n, clip):
    p, g, m, v = opt_inputs(n, 21 + n)
    for t0, parity in ((0, 0), (9, 1)):
        r = OptRun(p, g, m, v, steps=np.array([t0], np.int32), parity=parity)
        norm = O.norm_from_partials(r.partials())
        r.guarded(H_, clip)
        r.assert_tails()
        ref64 = O.adamw_guarded(p, g, m, v, H_, norm, clip, t0, F64)
        ref32 = O.adamw_guarded(p, g, m, v, H_, norm, clip, t0, F32)
        for name, k, a, b in zip("pgmv", r.arrays(), ref64, ref32):
            check_ew("adamw_guarded", f"{name} n={n} clip={clip} t={t0}", k, a, b)
        assert same_bits(r.norm.get(), np.array([norm], F32))
        assert r.steps.get().tolist() == [t0 + 1, t0 + 1] and r.skipped.get()[0] == 3
        # hiseg_adamw_step with the bias corrections as f32 arguments, with and without the partials
        bc1, bc2 = float(F32(1 - H_["b1"] ** (t0 + 1))), float(F32(1 - H_["b2"] ** (t0 + 1)))
        for with_partial in (True, False):
            r = OptRun(p, g, m, v)
            r.partials()
            r.plain(H_, bc1, bc2, clip, with_partial)
            r.assert_tails()
            nrm = norm if with_partial else None
            ref64 = O.adamw_plain(p, g, m, v, H_, bc1, bc2, nrm, clip, F64)
            ref32 = O.adamw_plain(p, g, m, v, H_, bc1, bc2, nrm, clip, F32)
            for name, k, a, b in zip("pgmv", r.arrays(), ref64, ref32):
                check_ew("adamw_step", f"{name} n={n} clip={clip} t={t0} partial={with_partial}", k, a, b)
            if with_partial:
                assert same_bits(r.norm.get(), np.array([norm], F32))
            else:
                r.norm.assert_tail(0)


@pytest.mark.parametrize("n", [255, OPT_N[2]])
def test_adamw_guarded_skip(n):
    p, g, m, v = opt_inputs(n, 31 + n)
    gb = g.copy()
    gb[n - 1] = np.nan
    r = OptRun(p, gb, m, v, steps=np.array([9], np.int32), parity=1)
    r.partials()
    r.guarded(H_, 1.0)
    r.assert_tails()
    for x, y in zip(r.arrays(), (p, gb, m, v)):
        assert same_bits(x, y)
    assert r.steps.get().tolist() == [9, 9] and r.skipped.get()[0] == 4 and not np.isfinite(r.norm.get()[0])


def test_optim_rejections():
    """nseg 0 or 257, parity 2, n = 0, a null pointer: an error, nothing written."""
    n = 300
    p, g, m, v = opt_inputs(n, 3)
    r = OptRun(p, g, m, v, seg_table(8, n), seg_steps(8))
    part = r.partials()
    before = [b.t.clone() for b in (r.p, r.g, r.m, r.v, r.norm, r.steps, r.skipped)]

    def call(nseg=8, parity=0, nn=n, pp=r.p.ptr, dev=None):
        a = (pp, r.g.ptr, r.m.ptr, r.v.ptr, nn)
        b = (r.partial.ptr, 1.0, r.norm.ptr, r.seg.ptr, nseg, r.steps.ptr, parity, r.skipped.ptr, stream())
        if dev is None:
            st = lib().hiseg_adamw_step_segmented(*a, H_["lr"], H_["b1"], H_["b2"], H_["omb1"], H_["omb2"],
                                                  H_["decay"], H_["eps"], *b)
        else:
            st = lib().hiseg_adamw_step_segmented_dev(*a, dev, H_["b1"], H_["b2"], H_["omb1"], H_["omb2"], H_["eps"],
                                                      *b)
        torch.cuda.synchronize()
        assert st != 0
        for x, y in zip(before, (r.p, r.g, r.m, r.v, r.norm, r.steps, r.skipped)):
            assert torch.equal(x, y.t)

    hyp = torch.tensor([H_["lr"], H_["decay"]], dtype=torch.float32, device=DEV)
    for dev in (None, hyp.data_ptr()):
        for kw in (dict(nseg=0), dict(nseg=257), dict(parity=2), dict(nn=0), dict(pp=None)):
            call(dev=dev, **kw)
    for kw in (dict(parity=2), dict(nn=0), dict(pp=None)):
        st = lib().hiseg_adamw_step_guarded(kw.get("pp", r.p.ptr), r.g.ptr, r.m.ptr, r.v.ptr, kw.get("nn", n),
                                            H_["lr"], H_["b1"], H_["b2"], H_["eps"], H_["wd"], r.partial.ptr, 1.0,
                                            r.norm.ptr, r.steps.ptr, kw.get("parity", 0), r.skipped.ptr, stream())
        assert st != 0
    assert lib().hiseg_grad_norm_partials(r.g.ptr, 0, r.partial.ptr, stream()) != 0
    assert lib().hiseg_grad_norm_partials(None, n, r.partial.ptr, stream()) != 0
    assert lib().hiseg_adamw_step(r.p.ptr, r.g.ptr, r.m.ptr, r.v.ptr, 0, H_["lr"], H_["b1"], H_["b2"], H_["eps"],
                                  H_["wd"], 0.1, 0.001, None, 0.0, None, stream()) != 0
    torch.cuda.synchronize()
    for x, y in zip(before, (r.p, r.g, r.m, r.v, r.norm, r.steps, r.skipped)):
        assert torch.equal(x, y.t)
    assert np.array_equal(r.partial.get().astype(F64), part)
