"""Each train-mode BatchNorm entry point on its own against the float64 oracle of tests/bn_kernel_oracle.py:
hiseg_bn_stats, hiseg_bn_finalize, hiseg_bn_finalize_n, hiseg_bn_apply, hiseg_bn_bwd, called through hiseg._lib with
hiseg._lib.bn_last_path() asserted after every launch.

Inputs are rounded to the compute dtype before either side sees them and nothing is excluded from a comparison.
Every activation view has cstride > C and a non-zero coff, is filled with SENTINEL first and carries a guard tail;
after each launch everything but the live channels must still hold the sentinel bit for bit, and so must the rows of
`partial` beyond the split count of the case.

Exact cases (test_apply_exact, test_constant_channel, test_bwd_exact) use small integers and powers of two, so
every f32 intermediate of the header's formulas is exact and the kernel must equal float64, rounded once to the output
dtype, bit for bit.  tests/test_bn_kernel_oracle.py proves that premise on the CPU from the case tables below.

Bounded cases.  Element-wise outputs (y, dz, dres) follow the rule of tests/test_gpu_train_kernels.py, with e32 the
distance of the float32 evaluation of the oracle from its float64 evaluation:

  f32 output                       |k - ref| <= 4 max(e32) + 4 * 2^-23 max|ref|
  bf16 output written once         2^-8 |ref| + the f32 rule
  bf16 output with accumulate      2^-7 max(|old|, |ref|) + the f32 rule

Per-channel statistics are f32 accumulations over pixels; their bound is 4 max(e32) + k * 2^-23 * M with k and M from
the inputs and the launch geometry alone (u = 2^-24 is the f32 unit round-off, 2^-23 = 2 u):

  geometry    S = clamp(P // 32, 1, 1024) splits of pps = ceil(P / S) pixels; a block is CT channel lanes x R = 256 // CT
              pixel rows (CT = min(C / chunk, 256) on the chunk path, min(C, 256) on the scalar one), so one thread
              accumulates m = ceil(pps / R) pixels and L = min(R, pps) rows hold data.  The rows are merged by a tree
              (depth = ceil(log2 L)) on the chunk path and by one thread walking them (depth = L - 1) on the scalar
              one.  The S splits are merged in double; that and the final cast cost one u of the result.
  sums        (dbeta = sum g, dgamma = sum g xhat, the premerge's group sums): a value passes m + depth additions,
              each relative error u on a partial sum <= M = max_c sum_p |term|; a term itself carries up to three
              roundings (xhat's subtraction and product, g xhat), and the result one.  k = (m + depth + 4) / 2.
  mean        Z = max|z|.  The n-th Welford update computes d = x - mean (error <= 2 Z u), d / n (two roundings of a
              value <= 2 Z / n, and d's error over n) and the addition (<= Z u): (1 + 6 / n) Z u, over n = 1..m at
              most (m + 6 (1 + ln m)) Z u.  A Chan merge level computes d, nb / nt, their product and the addition:
              <= 6 Z u.  Sub-means are averaged with weights <= 1, so errors of different threads do not add.
              k_mean = (m + 6 (1 + ln m) + 6 depth + 1) / 2, M = Z.
  M2          every term d (x - mean') or d^2 na nb / nt is at most (2 Z)^2, so M = P (2 Z)^2.  Three roundings per
              term and m + depth additions give (m + depth + 3) u M; an error delta <= k_mean 2 u Z in the running
              mean changes the terms by 2 delta sum |d| <= 2 k_mean u M.  k_M2 = (m + depth + 3) / 2 + k_mean.
  derived     var = M2 / n; invstd = (var + eps)^-1/2 moves by invstd^3 / 2 per unit of var; scale = gamma invstd,
              shift = beta - mean gamma invstd, rm' and rv' follow by the product rule from the bounds of mean and var
              with the reference's own magnitudes, plus one 2^-23 of the result for the final cast.
  dconv_bias  = k (s1 - P (s1 / P) - s3 (s2 / P)) is analytically near zero, so it is bounded by the rounding of its
              three terms: |gamma invstd| (2 B_s1 + |s3| B_s2 / P + |s2| B_s3 / P), B_x the sum bounds above (the
              kernel forms the expression in double from the f32 sums).

Worst observed ratio of kernel error over bound per kernel and dtype (profiles/bn_kernel_errors.txt):

  kernel            f32     bf16
  bn_stats          0.007   0.008     mean and M2 of the float64 merge of the kernel's own split rows, chunk kernel
  bn_stats_scalar   0.001   0.001     the same of the scalar kernel (its bound carries the row walk: depth = L - 1)
  bn_finalize       0.086   0.092     mean, invstd, scale, shift, rm, rv
  bn_finalize_n     0.141   -         group rows and outputs at explicit split counts
  bn_apply          0.157   0.995
  bn_bwd            0.239   0.995     dz, dres
  bn_bwd_params     0.112   0.094     dgamma, dbeta, dconv_bias
  (MI355X.  A bf16 output written once sits near 1.0 by construction, as in tests/test_gpu_train_kernels.py.  The
  statistics bounds are worst-case accumulation bounds, so random data stays far below them; no f32 ratio is above 0.5.)

HISEG_BN_U=2 against U = 1 is compared bit for bit (bn_apply; bn_bwd's dz, dres and parameter gradients).  The
comparison found the f32 backward's dz one rounding apart for sigmoid / SiLU / GELU / Swish: the U = 1 instance fused
g's last multiply into g - sum(g)/P, the U = 2 instance, whose g is computed in its load loop, could not.  g's
products are now rounded explicitly (mul_rounded in csrc/bn_train.hip), so every instance builds dz from the g that
dres stores.
"""
import math
import os
import re

import pytest
import torch

import bn_kernel_oracle as B
from hiseg import _lib as L
from hiseg import train_engine as TE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
HD = {"f32": L.HISEG_F32, "bf16": L.HISEG_BF16}
CHUNK = {"f32": 4, "bf16": 8}
SENTINEL = -7.5          # exact in bf16
GUARD = 64
EPS, MOM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))
MOM32 = float(torch.tensor(MOM, dtype=torch.float32))
BAD_ARG = -1
KPRE = 64                # csrc/bn_train.hip, constexpr int KPRE: given split rows are summed in groups of KPRE above 4 KPRE
RATIOS = {}
NONE, RELU, SIGMOID, SILU, GELU, SWISH = range(6)

# view layouts: (cstride - C, coff, base offset in elements).  "vec" keeps every 16-byte chunk aligned; the others
# break one condition of the chunk path each.
LAYOUTS = {"vec": (16, 8, 0), "coff1": (16, 1, 0), "base1": (16, 8, 1), "tight": (1, 1, 0)}


def lib():
    return L.lib()


def stream():
    return L.stream_ptr()


def ok(status, what):
    L.check(status, what)
    torch.cuda.synchronize()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, dt, *shape, scale=1.0, shift=0.0):
    """float64 values that are exactly representable in the compute dtype."""
    return (scale * torch.randn(*shape, generator=g, dtype=torch.float64) + shift).to(DTYPES[dt]).double()


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def pick(g, choices, *shape):
    c = torch.tensor(choices, dtype=torch.float64)
    return c[torch.randint(0, len(choices), shape, generator=g)]


def chan_table(g, N, C):
    m = torch.rand(N, C, generator=g, dtype=torch.float64) + 0.5
    m[torch.rand(N, C, generator=g) < 0.3] = 0.0
    m[0, 0], m[N - 1, C - 1] = 0.0, 1.0 / 0.7
    return m.float().double()


class View:
    """[P][cstride] activations with channels [coff, coff + C) live, the sentinel everywhere else, a guard tail after
    the last row and, for layout "base1", a base pointer one element past the allocation's aligned start."""

    def __init__(self, vals, dt, layout="vec", P=None, C=None):
        if vals is not None:
            P, C = vals.shape
        pad, coff, base = LAYOUTS[layout]
        self.P, self.C, self.cstride, self.coff = P, C, C + pad, coff
        buf = torch.full((P, self.cstride), SENTINEL, dtype=torch.float64)
        if vals is not None:
            buf[:, coff:coff + C] = vals
        flat = torch.full((base + P * self.cstride + GUARD,), SENTINEL, dtype=torch.float64)
        flat[base:base + P * self.cstride] = buf.reshape(-1)
        self.flat = flat.to(DTYPES[dt]).to(DEV)
        self.t = self.flat[base:]                      # data_ptr() advanced by `base` elements
        self.base = base
        self.before = self.flat.clone()

    def body(self, flat):
        return flat[self.base:self.base + self.P * self.cstride].view(self.P, self.cstride)

    def live(self):
        return self.body(self.flat)[:, self.coff:self.coff + self.C].double().cpu()

    def assert_rest_untouched(self):
        a, b = self.flat.clone(), self.before.clone()
        self.body(a)[:, self.coff:self.coff + self.C] = 0
        self.body(b)[:, self.coff:self.coff + self.C] = 0
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "a dead channel or the guard tail was written"

    def assert_unchanged(self):
        assert torch.equal(self.flat.view(torch.uint8), self.before.view(torch.uint8))


class F32:
    """n f32 values (`fill`, the sentinel by default, if vals is None) followed by a guard tail of the sentinel."""

    def __init__(self, vals=None, n=None, fill=SENTINEL):
        n = vals.numel() if vals is not None else n
        flat = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32)
        flat[:n] = fill
        if vals is not None:
            flat[:n] = vals.reshape(-1).float()
        self.n, self.t = n, flat.to(DEV)

    def get(self, *shape):
        return self.t[:self.n].double().cpu().reshape(*shape) if shape else self.t[:self.n].double().cpu()

    def assert_written(self, floats):
        """A buffer filled with NaN: exactly its first `floats` values were written."""
        live = ~torch.isnan(self.t[:self.n])
        assert int(live.sum()) == floats and bool(live[:floats].all()), (int(live.sum()), floats)

    def assert_tail(self, written=None):
        w = self.n if written is None else written
        tail = self.t[w:]
        assert torch.equal(tail, torch.full_like(tail, SENTINEL)), "wrote past the documented extent"


def f32ptr(x):
    return None if x is None else x.t.data_ptr()


def splits_of(P):
    return max(1, min(1024, P // 32))


def path(**want):
    got = L.bn_last_path()
    assert got is not None
    for k, v in want.items():
        assert got[k] == v, (k, got)
    return got


def is_vec(dt, C, *views):
    v = CHUNK[dt]
    return C % v == 0 and all(w is None or (w.cstride % v == 0 and w.coff % v == 0 and w.base == 0) for w in views)


def record(kernel, dt, what, err, bound):
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
    key = (kernel, dt)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{kernel} {dt} {what}: max err {err.max().item():.3e} ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{kernel} {dt} {what}: error / bound = {ratio:.3f} (max err {err.max().item():.3e})"


def check_ew(kernel, dt, what, k, r64, r32, mode="f32", old=None):
    """The element-wise rule of the module docstring."""
    k, r64, r32 = k.double().reshape(r64.shape), r64.double(), r32.double()
    base = 4 * (r32 - r64).abs().max() + 4 * 2.0 ** -23 * r64.abs().max()
    if mode == "f32":
        bound = base.expand_as(r64)
    elif mode == "once":
        bound = 2.0 ** -8 * r64.abs() + base
    else:
        bound = 2.0 ** -7 * torch.maximum(old.double().reshape(r64.shape).abs(), r64.abs()) + base
    record(kernel, dt, what, (k - r64).abs(), bound)


def check_stat(kernel, dt, what, k, r64, r32, slack):
    """A per-channel statistic: 4 max(e32) + slack, slack = k * 2^-23 * M built by the caller from the inputs."""
    k, r64, r32 = k.double().reshape(r64.shape), r64.double(), r32.double()
    bound = 4 * (r32 - r64).abs().max() + slack
    record(kernel, dt, what, (k - r64).abs(), bound if torch.is_tensor(bound) else torch.tensor(bound))


def out_mode(dt, acc=False):
    return "f32" if dt == "f32" else ("acc" if acc else "once")


def both(fn, *args, **kw):
    def cast(a, dtype):
        if isinstance(a, torch.Tensor) and a.is_floating_point():
            return a.to(dtype)
        return a
    r64 = fn(*[cast(a, torch.float64) for a in args], **{k: cast(v, torch.float64) for k, v in kw.items()})
    r32 = fn(*[cast(a, torch.float32) for a in args], **{k: cast(v, torch.float32) for k, v in kw.items()})
    return r64, r32


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    out = os.environ.get("HISEG_BN_KERNEL_ERRORS")
    if out:
        with open(out, "w") as f:
            f.write("# worst |kernel - float64 oracle| / bound per kernel and dtype (tests/test_gpu_bn_kernels.py)\n")
            for (kern, dt), r in sorted(RATIOS.items()):
                f.write(f"{kern:28s} {dt:5s} {r:.3f}\n")


# ------------------------------------------------------------------------------------------- geometry and bounds
def geometry(dt, C, P, vec):
    S = splits_of(P)
    pps = -(-P // S)
    CT = min(C // CHUNK[dt], 256) if vec else min(C, 256)
    R = 256 // CT
    m = -(-pps // R)
    rows = min(R, pps)
    depth = math.ceil(math.log2(rows)) if vec else rows - 1
    return S, m, depth


def k_sum(m, depth):
    return (m + depth + 4) / 2


def k_mean(m, depth):
    return (m + 6 * (1 + math.log(m)) + 6 * depth + 1) / 2


def k_m2(m, depth):
    return (m + depth + 3) / 2 + k_mean(m, depth)


U23 = 2.0 ** -23


def stat_slacks(z, P, gamma, beta, rm, rv, m, depth):
    """Slack of each finalize output from the mean / M2 slacks by the product rule (module docstring, 'derived')."""
    Z = z.abs().max().item()
    n, mean, m2 = B.bn_stats(z)
    mean_r, inv, scale, shift, rm2, rv2 = B.bn_finalize(n, mean, m2, gamma, beta, EPS32, MOM32, rm, rv, P)
    s_mean = k_mean(m, depth) * U23 * Z
    s_m2 = k_m2(m, depth) * U23 * P * (2 * Z) ** 2
    s_var = s_m2 / P
    s_inv = 0.5 * inv ** 3 * s_var + U23 * inv
    g = torch.ones_like(mean) if gamma is None else gamma.abs()
    s_scale = g * s_inv + U23 * scale.abs()
    s_shift = g * (inv * s_mean + mean.abs() * s_inv) + U23 * shift.abs()
    s_rm = MOM32 * s_mean + U23 * rm2.abs()
    s_rv = MOM32 * s_var * (P / (P - 1) if P > 1 else 1.0) + U23 * rv2.abs()
    return dict(mean=s_mean, m2=s_m2, invstd=s_inv, scale=s_scale, shift=s_shift, rm=s_rm, rv=s_rv)


# ------------------------------------------------------------------------------------------- stats + finalize
def run_stats(dt, z, layout="vec"):
    """hiseg_bn_stats on z: (partial rows [S][3][C] as float64, the F32 buffer, whether the chunk path ran)."""
    P, C = z.shape
    vz = View(z, dt, layout)
    part = F32(n=(splits_of(P) + 2) * 3 * C)     # two spare rows and the guard tail must stay untouched
    ok(lib().hiseg_bn_stats(HD[dt], vz.t.data_ptr(), P, C, vz.cstride, vz.coff, part.t.data_ptr(), stream()),
       "bn_stats")
    vec = is_vec(dt, C, vz)
    path(entry="stats", vec=vec)
    vz.assert_unchanged()
    S = splits_of(P)
    part.assert_tail(S * 3 * C)          # exactly clamp(P // 32, 1, 1024) rows are written
    rows = part.get()[:S * 3 * C].reshape(S, 3, C)
    assert not (rows == SENTINEL).all(dim=1).any(), "a split row was not written"
    assert torch.equal(rows[:, 0].sum(0), torch.full((C,), float(P), dtype=torch.float64)), "n does not sum to P"
    return rows, part, vec


def run_finalize(part, C, P, gamma, beta, rm, rv):
    outs = {k: F32(n=C) for k in ("mean", "invstd", "scale", "shift")}
    frm, frv = (None if rm is None else F32(rm)), (None if rv is None else F32(rv))
    fg, fb = (None if gamma is None else F32(gamma)), (None if beta is None else F32(beta))
    ok(lib().hiseg_bn_finalize(part.t.data_ptr(), C, P, f32ptr(fg), f32ptr(fb), EPS, MOM, f32ptr(frm), f32ptr(frv),
                               outs["mean"].t.data_ptr(), outs["invstd"].t.data_ptr(), outs["scale"].t.data_ptr(),
                               outs["shift"].t.data_ptr(), stream()), "bn_finalize")
    for o in list(outs.values()) + [x for x in (frm, frv) if x is not None]:
        o.assert_tail()
    res = {k: v.get() for k, v in outs.items()}
    res["rm"], res["rv"] = (None if frm is None else frm.get()), (None if frv is None else frv.get())
    return res


def finalize_refs(z, P, gamma, beta, rm, rv):
    def f(z, gamma, beta, rm, rv):
        n, mean, m2 = B.bn_stats(z)
        return (m2,) + tuple(B.bn_finalize(n, mean, m2, gamma, beta, EPS32, MOM32, rm, rv, P))
    return both(f, z, gamma, beta, rm, rv)


def check_stats_and_finalize(dt, z, layout="vec", gamma=True, beta=True, fin_par=None, seed=0):
    P, C = z.shape
    g = gen(1000 + seed)
    gam = rnd(g, "f32", C, scale=0.3, shift=1.0) if gamma else None
    bet = rnd(g, "f32", C, scale=0.5) if beta else None
    rm, rv = rnd(g, "f32", C, scale=0.5), rnd(g, "f32", C, scale=0.1, shift=1.0).abs()
    rows, part, vec = run_stats(dt, z, layout)
    S, m, depth = geometry(dt, C, P, vec)
    sl = stat_slacks(z, P, gam, bet, rm, rv, m, depth)
    r64, r32 = finalize_refs(z, P, gam, bet, rm, rv)
    tag = f"P={P} C={C} {layout}"
    # the float64 merge of the kernel's own split rows
    _, k_mean_, k_m2_ = B.merge(rows)
    kern = "bn_stats" if vec else "bn_stats_scalar"
    check_stat(kern, dt, f"mean {tag}", k_mean_, r64[1], r32[1], sl["mean"])
    check_stat(kern, dt, f"M2 {tag}", k_m2_, r64[0], r32[0], sl["m2"])
    res = run_finalize(part, C, P, gam, bet, rm, rv)
    want_par = (S > 256) if fin_par is None else fin_par
    path(entry="finalize", par=want_par, premerge=False)
    for i, name in enumerate(("mean", "invstd", "scale", "shift", "rm", "rv"), start=1):
        check_stat("bn_finalize", dt, f"{name} {tag}", res[name], r64[i], r32[i], sl[name])
    return S


SPLIT_P = [1, 31, 33, 64, 8223, 8224, 32768, 32785]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("P", SPLIT_P)
def test_split_count(dt, P):
    """The split count is clamp(P // 32, 1, 1024): exactly that many rows of `partial` are written, n sums to P, and
    the finalize kernel changes from rows to par above 256 splits (P = 8223 / 8224).  P = 1: the biased variance."""
    z = rnd(gen(P), dt, P, 8, scale=1.3, shift=0.4)
    S = check_stats_and_finalize(dt, z, gamma=(P != 33), beta=(P != 64), seed=P)     # also gamma / beta == NULL
    assert S == max(1, min(1024, P // 32))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("P", [2048, 8224])
@pytest.mark.parametrize("fin", ["0", "1"])
def test_finalize_kernel_forced(dt, P, fin, monkeypatch):
    """HISEG_BN_FIN = 0 (par) and 1 (rows) at a split count where the default would take the other: same bound."""
    monkeypatch.setenv("HISEG_BN_FIN", fin)
    z = rnd(gen(P + 7), dt, P, 8, scale=1.3, shift=-0.7)
    check_stats_and_finalize(dt, z, fin_par=(fin == "0"), seed=P + 7)


# (C, layout): the scalar statistics kernel forced by the channel count, by coff and by the base pointer
SCALAR_STATS = [(6, "vec"), (16, "coff1"), (16, "base1")]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("C,layout", SCALAR_STATS)
@pytest.mark.parametrize("P", [100, 2051])
def test_stats_scalar(dt, C, layout, P):
    """bn_stats_kernel on ordinary data: its Welford update, the one-thread walk over the pixel rows and the Chan cross
    term, against float64 with the scalar geometry of the bounds (depth = rows - 1).  P = 100: three splits, one pixel
    per thread and dead rows; P = 2051: 64 splits of 32 or 33 pixels, so with C = 6 (R = 42) only the first rows of a
    block carry two pixels and with C = 16 (R = 16) every row carries two or three."""
    z = rnd(gen(P + C), dt, P, C, scale=1.3, shift=0.4)
    rows, _, vec = run_stats(dt, z, layout)
    assert not vec
    check_stats_and_finalize(dt, z, layout, seed=P + C)


# ------------------------------------------------------------------------------------------- constant channel (exact)
CONST_V = 2.5
CONST_CASES = [("f32", 8, 100, "vec"), ("bf16", 8, 100, "vec"), ("f32", 6, 100, "vec"), ("bf16", 16, 8224, "coff1"),
               ("f32", 8, 8224, "vec")]


@pytest.mark.parametrize("dt,C,P,layout", CONST_CASES)
def test_constant_channel(dt, C, P, layout):
    """Channel 2 holds CONST_V at every pixel: each split row has mean == v and M2 == 0 exactly, n sums to P,
    invstd == float(1 / sqrt(double(eps))), scale / shift are the header's fold in double, rv' == (1 - momentum) rv."""
    g = gen(77)
    z = rnd(g, dt, P, C, scale=1.3, shift=0.4)
    z[:, 2] = CONST_V
    rows, part, _ = run_stats(dt, z, layout)
    c = rows[:, :, 2]
    live = c[:, 0] > 0
    assert live.all() and c[:, 0].sum() == P
    assert torch.equal(c[:, 1], torch.full_like(c[:, 1], CONST_V)), "mean of a constant channel"
    assert torch.equal(c[:, 2], torch.zeros_like(c[:, 2])), "M2 of a constant channel is not exactly 0"
    gam, bet = rnd(g, "f32", C, shift=1.0), rnd(g, "f32", C)
    rm, rv = rnd(g, "f32", C), rnd(g, "f32", C).abs() + 0.5
    res = run_finalize(part, C, P, gam, bet, rm, rv)
    path(entry="finalize", par=splits_of(P) > 256)
    inv = 1.0 / math.sqrt(EPS32)
    f = lambda x: float(torch.tensor(x, dtype=torch.float64).float())
    assert res["mean"][2].item() == CONST_V
    assert res["invstd"][2].item() == f(inv)
    assert res["scale"][2].item() == f(gam[2].item() * inv)
    assert res["shift"][2].item() == f(bet[2].item() - CONST_V * gam[2].item() * inv)
    assert res["rv"][2].item() == f((1.0 - MOM32) * rv[2].item())


# ------------------------------------------------------------------------------------------- apply
def apply_desc(dt, P, HW, C, vz, scale, shift, vres, act, beta, mul, vy, per_sample):
    d = L.BnApplyDesc()
    d.dtype, d.P, d.HW, d.C = HD[dt], P, HW, C
    d.z, d.z_cstride, d.z_coff = vz.t, vz.cstride, vz.coff
    d.scale, d.shift = scale.t, shift.t
    if vres is not None:
        d.residual, d.r_cstride, d.r_coff = vres.t, vres.cstride, vres.coff
    d.act, d.act_beta, d.per_sample = act, beta, per_sample
    if mul is not None:
        d.chan_mul = mul.t
    d.y, d.y_cstride, d.y_coff = vy.t, vy.cstride, vy.coff
    return d


def run_apply(dt, HW, z, scale, shift, res, act, beta, mul, per_sample, layout="vec", res_layout=None, u2=None,
              monkeypatch=None):
    """hiseg_bn_apply -> (live y as float64, vec?).  u2: also run under HISEG_BN_U=2 and require identical bits."""
    P, C = z.shape
    vz, vy = View(z, dt, layout), View(None, dt, layout, P, C)
    vres = None if res is None else View(res, dt, res_layout or layout)
    fs, fh = F32(scale), F32(shift)
    fm = None if mul is None else F32(mul)
    d = apply_desc(dt, P, HW, C, vz, fs, fh, vres, act, beta, fm, vy, per_sample)
    ok(lib().hiseg_bn_apply(d, stream()), "bn_apply")
    vec = is_vec(dt, C, vz, vy, vres)
    path(entry="apply", vec=vec, u2=False)
    vy.assert_rest_untouched()
    if u2:
        vy2 = View(None, dt, layout, P, C)
        d.y = vy2.t
        monkeypatch.setenv("HISEG_BN_U", "2")
        ok(lib().hiseg_bn_apply(d, stream()), "bn_apply U=2")
        monkeypatch.delenv("HISEG_BN_U")
        path(entry="apply", vec=vec, u2=vec)
        assert torch.equal(vy2.flat.view(torch.uint8), vy.flat.view(torch.uint8)), "HISEG_BN_U=2 changed bits"
    return vy.live(), vec


# (dtype, C, layout, per_sample): the chunk and the scalar kernel, each with [C] and per-sample [N][C] tables
APPLY_EXACT = [(dt, C, "vec", ps) for dt in DTYPES for C in (16, 6) for ps in (0, 1)]
N_EX, HW_EX = 3, 7


def apply_exact_inputs(dt, C, per_sample):
    g = gen(300 + C + per_sample)
    P = N_EX * HW_EX
    rows = N_EX if per_sample else 1
    z, res = ints(g, -8, 8, P, C), ints(g, -8, 8, P, C)
    scale = pick(g, [-2, -1, -0.5, 0.5, 1, 2], rows, C)
    shift = ints(g, -4, 3, rows, C) + 0.5
    mul = pick(g, [0.0, 2.0], N_EX, C)
    if not per_sample:
        scale, shift = scale[0], shift[0]
    return z, res, scale, shift, mul


@pytest.mark.parametrize("dt,C,layout,per_sample", APPLY_EXACT)
def test_apply_exact(dt, C, layout, per_sample):
    z, res, scale, shift, mul = apply_exact_inputs(dt, C, per_sample)
    for act in (NONE, RELU):
        for r, m in ((None, None), (res, mul), (res, None), (None, mul)):
            y, vec = run_apply(dt, HW_EX, z, scale, shift, r, act, 1.0, m, per_sample, layout)
            assert vec == (C == 16)
            ref = B.bn_apply(z, scale, shift, r, act, 1.0, m, HW_EX, per_sample)
            assert torch.equal(y, ref.to(DTYPES[dt]).double()), f"act={act} residual={r is not None} mul={m is not None}"


ACTS = [(NONE, 1.0), (RELU, 1.0), (SIGMOID, 1.0), (SILU, 1.0), (GELU, 1.0), (SWISH, 1.5)]
# (C, layout, residual layout): chunk path; scalar by C, by coff, by base pointer, by a misaligned residual alone
APPLY_FORMS = [(16, "vec", None), (6, "vec", None), (16, "coff1", None), (16, "base1", None), (16, "vec", "base1")]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("C,layout,res_layout", APPLY_FORMS)
@pytest.mark.parametrize("per_sample", [0, 1])
def test_apply(dt, C, layout, res_layout, per_sample, monkeypatch):
    """Every activation, with and without residual and chan_mul, [C] and per-sample tables, N = 3 images of HW = 37
    pixels (no multiple of a block's rows).  The scalar kernel is forced in four ways."""
    N, HW = 3, 37
    P = N * HW
    g = gen(400 + C)
    z, res = rnd(g, dt, P, C, scale=1.5), rnd(g, dt, P, C)
    rows = (N, C) if per_sample else (C,)
    scale, shift = rnd(g, "f32", *rows, scale=0.5, shift=1.0), rnd(g, "f32", *rows, scale=0.5)
    mul = chan_table(g, N, C)
    for act, beta in ACTS:
        for r, m in ((res, mul), (None, None)) if res_layout is None else ((res, mul),):
            y, vec = run_apply(dt, HW, z, scale, shift, r, act, beta, m, per_sample, layout, res_layout, u2=True,
                               monkeypatch=monkeypatch)
            assert vec == (C == 16 and layout == "vec" and res_layout is None)
            r64, r32 = both(B.bn_apply, z, scale, shift, r, act, beta, m, HW, per_sample)
            check_ew("bn_apply", dt, f"act={act} C={C} {layout}/{res_layout} ps={per_sample}", y, r64, r32,
                     out_mode(dt))


@pytest.mark.parametrize("dt", list(DTYPES))
def test_apply_scalar_grid_stride(dt):
    """The scalar kernel's grid is capped (ew_blocks in csrc/train_norm.h, read from the source: blocks of 256
    elements): with one pixel more than cap * 256 / C the first threads take a second iteration.  C = 7 in rows of 8
    keeps the largest buffer near 10 MB."""
    src = open(os.path.join(os.path.dirname(L.__file__), "..", "csrc", "train_norm.h")).read()
    m = re.search(r"inline unsigned ew_blocks\(long long n\) \{.*?b > (\d+) \? (\d+) :", src, flags=re.S)
    assert m and m.group(1) == m.group(2), "ew_blocks no longer has the form this test reads its cap from"
    cap = int(m.group(1))
    C = 7
    HW = cap * 256 // C + 1
    g = gen(5)
    z = rnd(g, dt, HW, C)
    scale, shift = rnd(g, "f32", C, shift=1.0), rnd(g, "f32", C)
    assert HW * C > cap * 256 and (HW - 1) * C <= cap * 256
    y, vec = run_apply(dt, HW, z, scale, shift, None, RELU, 1.0, None, 0, layout="tight")
    assert not vec
    r64, r32 = both(B.bn_apply, z, scale, shift, None, RELU, 1.0, None, HW, 0)
    check_ew("bn_apply", dt, "grid stride", y, r64, r32, out_mode(dt))


# ------------------------------------------------------------------------------------------- backward
def bwd_desc(dt, P, HW, C, v, tabs, act, beta, acc_params, acc_dres, partial, partial_splits=0):
    d = L.BnBwdDesc()
    d.dtype, d.P, d.HW, d.C = HD[dt], P, HW, C
    for name, pre in (("dy", "dy"), ("y", "y"), ("z", "z"), ("dz", "dz"), ("dres", "dres"), ("residual", "r")):
        w = v.get(name)
        if w is not None:
            setattr(d, name, w.t)
            setattr(d, pre + "_cstride", w.cstride)
            setattr(d, pre + "_coff", w.coff)
    for name in ("chan_mul", "mean", "invstd", "gamma", "beta", "fwd_scale", "fwd_shift", "dgamma", "dbeta",
                 "dconv_bias"):
        if tabs.get(name) is not None:
            setattr(d, name, tabs[name].t)
    d.partial = partial.t
    d.act, d.act_beta, d.accumulate_params, d.dres_accumulate = act, beta, acc_params, acc_dres
    d.partial_splits = partial_splits
    return d


MODE_OF = {"none": "none", "y": "y", "fold": "pre"}


def expected_mode(act, src):
    if src == "pre":
        return "relu_pre" if act == RELU else "pre"
    return MODE_OF[src]


def make_bwd_inputs(dt, N, HW, C, act, beta, fwd, with_res, with_mul, with_gamma, with_beta, seed):
    """Random backward inputs.  For ReLU the pre-activation (and so the stored y) is moved at least 2^-6 from zero, in
    float64 after rounding, by nudging z."""
    g = gen(seed)
    P = N * HW
    z = rnd(g, dt, P, C, scale=1.3, shift=0.3)
    res = rnd(g, dt, P, C) if with_res else None
    gam = rnd(g, "f32", C, scale=0.25, shift=1.0) * pick(g, [-1.0, 1.0], C) if with_gamma else None
    bet = rnd(g, "f32", C, scale=0.5) if with_beta else None
    mul = chan_table(g, N, C) if with_mul else None

    def tables(z):
        n, mean, m2 = B.bn_stats(z)
        mean, inv, scale, shift, _, _ = B.bn_finalize(n, mean, m2, gam, bet, EPS32, MOM32, None, None, P)
        return [t.float().double() for t in (mean, inv, scale, shift)]

    mean, inv, scale, shift = tables(z)
    if act == RELU:   # the tables stay fixed while z moves: they are inputs of the backward, not recomputed
        for _ in range(4):
            pre = z * scale + shift + (res if with_res else 0)
            bad = pre.abs() < 2.0 ** -6
            if not bad.any():
                break
            tgt = torch.where(pre >= 0, 1.0, -1.0) * 2.0 ** -3
            z = torch.where(bad, (tgt - shift - (res if with_res else 0)) / scale, z).to(DTYPES[dt]).double()
        pre = z * scale + shift + (res if with_res else 0)
        assert pre.abs().min() >= 2.0 ** -6 and (pre > 0).any() and (pre < 0).any()
    dy = rnd(g, dt, P, C)
    y = B.bn_apply(z, scale, shift, res, act, beta, mul, HW, 0).to(DTYPES[dt]).double()
    return dict(z=z, dy=dy, y=y, res=res, gamma=gam, beta=bet, mul=mul, mean=mean, invstd=inv,
                fwd_scale=scale if fwd else None, fwd_shift=shift if fwd else None)


def run_bwd(dt, N, HW, C, act, beta, inp, want_dres, acc_dres, acc_params, layout="vec", dres_layout=None,
            exact=False, u2=False, monkeypatch=None, tag=""):
    P = N * HW
    g = gen(9)
    old_dres = rnd(g, dt, P, C) if not exact else ints(g, -3, 3, P, C)
    old = {k: (rnd(g, "f32", C) if not exact else ints(g, -5, 5, C)) for k in ("dgamma", "dbeta", "dconv_bias")}

    def views():
        v = dict(dy=View(inp["dy"], dt, layout), z=View(inp["z"], dt, layout), dz=View(None, dt, layout, P, C))
        src = B.deriv_source(act, inp["fwd_scale"] is not None, inp["res"] is not None, want_dres)
        if src == "y":
            v["y"] = View(inp["y"], dt, layout)
        if inp["res"] is not None:
            v["residual"] = View(inp["res"], dt, layout)
        if want_dres:
            v["dres"] = View(old_dres, dt, dres_layout or layout)
        return v, src

    def launch(v):
        tabs = {k: (None if inp.get(src_k) is None else F32(inp[src_k])) for k, src_k in
                (("chan_mul", "mul"), ("mean", "mean"), ("invstd", "invstd"), ("gamma", "gamma"), ("beta", "beta"),
                 ("fwd_scale", "fwd_scale"), ("fwd_shift", "fwd_shift"))}
        for k in old:
            tabs[k] = F32(old[k])
        S = splits_of(P)
        part = F32(n=(S + 1) * 3 * C)
        d = bwd_desc(dt, P, HW, C, v, tabs, act, beta, acc_params, acc_dres, part)
        ok(lib().hiseg_bn_bwd(d, stream()), "bn_bwd")
        part.assert_tail()
        for k in old:
            tabs[k].assert_tail()
        return tabs

    v, src = views()
    tabs = launch(v)
    vec = is_vec(dt, C, *v.values())
    path(entry="bwd", vec=vec, mode=expected_mode(act, src), reduce=True, premerge=False, par=True, u2=False)
    for name in ("dy", "z", "y", "residual"):
        if name in v:
            v[name].assert_unchanged()
    v["dz"].assert_rest_untouched()
    if want_dres:
        v["dres"].assert_rest_untouched()
    if u2:
        v2, _ = views()
        monkeypatch.setenv("HISEG_BN_U", "2")
        tabs2 = launch(v2)
        monkeypatch.delenv("HISEG_BN_U")
        path(entry="bwd", vec=vec, u2=vec)
        for name in ("dz", "dres"):
            if name in v:
                assert torch.equal(v2[name].flat.view(torch.uint8), v[name].flat.view(torch.uint8)), name
        for k in old:
            assert torch.equal(tabs2[k].t, tabs[k].t), k

    args = (inp["dy"], inp["z"], inp["mean"], inp["invstd"], inp["gamma"], inp["beta"], act, beta, inp["mul"], HW)
    kw = dict(y=inp["y"] if src == "y" else None, fwd_scale=inp["fwd_scale"], fwd_shift=inp["fwd_shift"],
              residual=inp["res"], wants_dres=want_dres)
    r64, r32 = both(B.bn_bwd, *args, **kw)
    names = ("dz", "dres", "dgamma", "dbeta", "dconv_bias")
    r64, r32 = dict(zip(names, r64)), dict(zip(names, r32))
    if acc_dres:
        r64["dres"], r32["dres"] = r64["dres"] + old_dres, r32["dres"] + old_dres.float()
    if acc_params:
        for k in old:
            r64[k], r32[k] = r64[k] + old[k], r32[k] + old[k].float()
    got = dict(dz=v["dz"].live(), dres=v["dres"].live() if want_dres else None,
               **{k: tabs[k].get() for k in old})
    if exact:
        assert torch.equal(got["dz"], r64["dz"].to(DTYPES[dt]).double()), "dz"
        if want_dres:
            assert torch.equal(got["dres"], r64["dres"].to(DTYPES[dt]).double()), "dres"
        for k in old:
            assert torch.equal(got[k], r64[k].float().double()), k
        return vec
    check_ew("bn_bwd", dt, f"dz {tag}", got["dz"], r64["dz"], r32["dz"], out_mode(dt))
    if want_dres:
        check_ew("bn_bwd", dt, f"dres {tag}", got["dres"], r64["dres"], r32["dres"], out_mode(dt, acc_dres), old_dres)
    # parameter gradients: the sum bounds of the module docstring
    _, m, depth = geometry(dt, C, P, vec)
    g64, xh = B.bn_g(*args, **kw)
    ks = k_sum(m, depth) * U23
    b1, b2, b3 = ks * g64.abs().sum(0), ks * (g64 * xh).abs().sum(0), ks * xh.abs().sum(0)
    accs = {k: (U23 * r64[k].abs() if acc_params else 0.0) for k in old}
    check_stat("bn_bwd_params", dt, f"dbeta {tag}", got["dbeta"], r64["dbeta"], r32["dbeta"], b1 + accs["dbeta"])
    check_stat("bn_bwd_params", dt, f"dgamma {tag}", got["dgamma"], r64["dgamma"], r32["dgamma"], b2 + accs["dgamma"])
    kk = inp["invstd"] * (1.0 if inp["gamma"] is None else inp["gamma"].abs())
    s1, s2, s3 = g64.sum(0), (g64 * xh).sum(0), xh.sum(0)
    bcb = kk * (2 * b1 + s3.abs() * b2 / P + s2.abs() * b3 / P) + U23 * r64["dconv_bias"].abs()
    check_stat("bn_bwd_params", dt, f"dconv_bias {tag}", got["dconv_bias"], r64["dconv_bias"], r32["dconv_bias"], bcb)
    return vec


# exact backward: (act, fwd tables, residual, dres): modes none, y (ReLU) and relu_pre without and with a residual
BWD_EXACT_MODES = [(NONE, False, False, False), (NONE, False, False, True), (RELU, False, False, True),
                   (RELU, False, False, False), (RELU, True, False, False), (RELU, True, True, True)]
BWD_EXACT = [(dt, C) for dt in DTYPES for C in (16, 6)]
N_BX, HW_BX = 2, 32          # P = 64: a power of two, two splits


def bwd_exact_inputs(C, act, fwd, with_res):
    g = gen(600 + C + act + 2 * fwd + 4 * with_res)
    P = N_BX * HW_BX
    z, dy = ints(g, -4, 4, P, C), ints(g, -2, 2, P, C)
    res = ints(g, -3, 3, P, C) if with_res else None
    mean, inv = ints(g, -2, 2, C), pick(g, [0.5, 1.0, 2.0], C)
    gam = pick(g, [-2, -1, -0.5, 0.5, 1, 2], C)
    mul = pick(g, [0.0, 2.0], N_BX, C)
    fs, fh = pick(g, [-1.0, 1.0, 2.0], C), ints(g, -3, 2, C) + 0.5     # integer + half: never zero
    y = ints(g, -3, 3, P, C)
    return dict(z=z, dy=dy, y=y, res=res, gamma=gam, beta=None, mul=mul, mean=mean, invstd=inv,
                fwd_scale=fs if fwd else None, fwd_shift=fh if fwd else None)


@pytest.mark.parametrize("dt,C", BWD_EXACT)
@pytest.mark.parametrize("act,fwd,with_res,want_dres", BWD_EXACT_MODES)
def test_bwd_exact(dt, C, act, fwd, with_res, want_dres):
    inp = bwd_exact_inputs(C, act, fwd, with_res)
    for acc in (0, 1):
        vec = run_bwd(dt, N_BX, HW_BX, C, act, 1.0, inp, want_dres, acc, acc, exact=True)
        assert vec == (C == 16)


# (act, beta, fwd tables, residual, dres): every reachable way of taking act'(.)
BWD_MODES = [
    (NONE, 1.0, False, False, False), (NONE, 1.0, False, False, True),
    (RELU, 1.0, False, False, False), (RELU, 1.0, False, False, True),      # from y
    # sigmoid: always from y, the tables are ignored.  With chan_mul the stored y is sigmoid(.) * chan_mul and the header's
    # y (1 - y) is taken of that scaled y: kernel and oracle follow the header here, autograd would not (the CPU test
    # skips that combination); the engine never puts a Dropout2d mask behind a sigmoid BatchNorm.
    (SIGMOID, 1.0, False, False, False), (SIGMOID, 1.0, True, False, True),
    (RELU, 1.0, True, False, False),                                       # mask recomputed, no dres
    (RELU, 1.0, True, False, True),                                        # tables, dres, no residual: back to y
    (RELU, 1.0, True, True, True),                                         # after a residual add
    (SILU, 1.0, False, False, False), (SILU, 1.0, True, False, False), (SILU, 1.0, True, True, True),
    (GELU, 1.0, True, False, False), (GELU, 1.0, True, True, True),
    (SWISH, 1.5, True, False, False), (SWISH, 1.5, True, True, True),
]
# (C, layout, dres layout): chunk path; scalar by C, coff, base pointer and a misaligned dres alone
BWD_FORMS = [(16, "vec", None), (6, "vec", None), (16, "coff1", None), (16, "base1", None), (16, "vec", "base1")]


BWD_PARAMS = [f + m for f in BWD_FORMS for m in BWD_MODES if f[2] is None or m[4]]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("C,layout,dres_layout,act,beta,fwd,with_res,want_dres", BWD_PARAMS)
def test_bwd(dt, C, layout, dres_layout, act, beta, fwd, with_res, want_dres, monkeypatch):
    N, HW = 3, 37
    plain = (act + C // 2 + fwd) % 2 == 0    # alternate: all of chan_mul / gamma / beta present, or none of them
    inp = make_bwd_inputs(dt, N, HW, C, act, beta, fwd, with_res, not plain, not plain, not plain, 700 + act)
    for acc in (0, 1):
        vec = run_bwd(dt, N, HW, C, act, beta, inp, want_dres, acc, acc, layout, dres_layout, u2=(acc == 0),
                      monkeypatch=monkeypatch, tag=f"act={act} fwd={fwd} res={with_res} C={C} {layout}/{dres_layout}")
        assert vec == (C == 16 and layout == "vec" and dres_layout is None)


def test_bwd_argument_checks():
    """GELU without the forward's tables, a smooth activation with dres but no residual, an activation without y:
    HISEG_ERR_BAD_ARG, nothing launched (the recorded path and every buffer stay as they were)."""
    dt, N, HW, C = "f32", 2, 16, 8
    P = N * HW
    run_stats(dt, rnd(gen(1), dt, P, C))
    before = L.bn_last_path()
    assert before["entry"] == "stats"
    inp = make_bwd_inputs(dt, N, HW, C, SILU, 1.0, True, False, False, True, True, 1)
    for act, fwd, want_dres, give_y in ((GELU, False, False, True), (SWISH, False, False, True),
                                        (SILU, True, True, True), (GELU, True, True, True),
                                        (RELU, False, False, False), (SIGMOID, False, False, False)):
        v = dict(dy=View(inp["dy"], dt), z=View(inp["z"], dt), dz=View(None, dt, "vec", P, C))
        if give_y:
            v["y"] = View(inp["y"], dt)
        if want_dres:
            v["dres"] = View(inp["dy"], dt)
        tabs = {k: F32(inp[k]) for k in ("mean", "invstd", "gamma", "beta")}
        if fwd:
            tabs["fwd_scale"], tabs["fwd_shift"] = F32(inp["fwd_scale"]), F32(inp["fwd_shift"])
        part = F32(n=2 * 3 * C)
        st = lib().hiseg_bn_bwd(bwd_desc(dt, P, HW, C, v, tabs, act, 1.0, 0, 0, part), stream())
        torch.cuda.synchronize()
        assert st == BAD_ARG, (act, fwd, want_dres, give_y, st)
        assert L.bn_last_path() == before
        for w in v.values():
            w.assert_unchanged()
        part.assert_tail(0)


# ------------------------------------------------------------------------------------------- row trees, channel blocks
# (dtype, C, P): R = 42 and 85 (no power of two: dead rows), a second channel block with one live chunk, and R = 1 with
# more pixels than the 2048-block grid cap (the element-wise loops stride; under U = 2 the last p0 + stride >= P)
TREE_CASES = [("f32", 24, 100), ("bf16", 24, 100), ("f32", 1028, 70), ("bf16", 2056, 70), ("bf16", 2048, 2051)]


@pytest.mark.parametrize("dt,C,P", TREE_CASES)
def test_row_trees_and_channel_blocks(dt, C, P, monkeypatch):
    g = gen(C + P)
    z = rnd(g, dt, P, C, scale=1.3, shift=0.4)
    check_stats_and_finalize(dt, z, seed=C)
    scale, shift = rnd(g, "f32", C, scale=0.3, shift=1.0), rnd(g, "f32", C, scale=0.5)
    res = rnd(g, dt, P, C)
    y, vec = run_apply(dt, P, z, scale, shift, res, SILU, 1.0, None, 0, u2=True, monkeypatch=monkeypatch)
    assert vec
    check_ew("bn_apply", dt, f"C={C} P={P}", y, *both(B.bn_apply, z, scale, shift, res, SILU, 1.0, None, P, 0),
             out_mode(dt))
    inp = make_bwd_inputs(dt, 1, P, C, RELU, 1.0, True, True, False, True, True, C)
    assert run_bwd(dt, 1, P, C, RELU, 1.0, inp, True, 0, 0, u2=True, monkeypatch=monkeypatch, tag=f"C={C} P={P}")


# ------------------------------------------------------------------------------------------- explicit split counts
def synthetic_stat_partials(g, S, C, P):
    """[S][3][C] (n, mean, M2) of S pixel ranges of random data, some empty, rounded to f32."""
    z = 1.3 * torch.randn(P, C, generator=g, dtype=torch.float64) + 0.4
    cuts = torch.sort(torch.randint(0, P + 1, (S - 1,), generator=g)).values.tolist()
    cuts = [0] + cuts + [P]
    rows = torch.zeros(S, 3, C, dtype=torch.float64)
    for s in range(S):
        seg = z[cuts[s]:cuts[s + 1]]
        if len(seg):
            n, mean, m2 = B.bn_stats(seg)
            rows[s, 0], rows[s, 1], rows[s, 2] = n, mean, m2
    return rows.float().double(), z.abs().max().item()


@pytest.mark.parametrize("S", [40, 300])
def test_finalize_n_scratch_contract(S):
    """More than 256 splits are pre-merged in groups of 64 in place: row 64 g holds group g's merge afterwards.  The
    merges run in double, so the slack is the casts: 2 * 2^-23 of Z (mean), of P (2 Z)^2 (M2)."""
    C, P = 24, 5000
    g = gen(S)
    rows, Z = synthetic_stat_partials(g, S, C, P)
    part = F32(rows)
    gam, bet = rnd(g, "f32", C, shift=1.0), rnd(g, "f32", C)
    rm, rv = rnd(g, "f32", C), rnd(g, "f32", C).abs() + 0.5
    outs = {k: F32(n=C) for k in ("mean", "invstd", "scale", "shift")}
    frm, frv, fg, fb = F32(rm), F32(rv), F32(gam), F32(bet)
    ok(lib().hiseg_bn_finalize_n(part.t.data_ptr(), S, C, P, fg.t.data_ptr(), fb.t.data_ptr(), EPS, MOM,
                                 frm.t.data_ptr(), frv.t.data_ptr(), outs["mean"].t.data_ptr(),
                                 outs["invstd"].t.data_ptr(), outs["scale"].t.data_ptr(), outs["shift"].t.data_ptr(),
                                 stream()), "bn_finalize_n")
    path(entry="finalize", premerge=S > 256, par=False)
    part.assert_tail()
    for o in list(outs.values()) + [frm, frv]:
        o.assert_tail()
    s_mean, s_m2 = 2 * U23 * Z, 2 * U23 * P * (2 * Z) ** 2
    after = part.get(S, 3, C)
    if S > 256:
        for grp in range(-(-S // 64)):
            n, mean, m2 = B.merge(rows[64 * grp:64 * (grp + 1)])
            assert torch.equal(after[64 * grp, 0], n)
            check_stat("bn_finalize_n", "f32", f"group {grp} mean", after[64 * grp, 1], mean, mean, s_mean)
            check_stat("bn_finalize_n", "f32", f"group {grp} M2", after[64 * grp, 2], m2, m2, s_m2)
    else:
        assert torch.equal(after, rows), "partials were modified at a split count without a pre-merge"
    n, mean, m2 = B.merge(rows)
    assert n[0].item() == P
    r = B.bn_finalize(n, mean, m2, gam, bet, EPS32, MOM32, rm, rv, P)
    # twice the casts: the group rows are rounded to f32 before the final merge
    s_var = 2 * s_m2 / P
    s_inv = 0.5 * r[1] ** 3 * s_var + U23 * r[1]
    slack = dict(mean=2 * s_mean, invstd=s_inv, scale=gam.abs() * s_inv + U23 * r[2].abs(),
                 shift=gam.abs() * (r[1] * 2 * s_mean + r[0].abs() * s_inv) + U23 * r[3].abs(),
                 rm=MOM32 * 2 * s_mean + U23 * r[4].abs(), rv=MOM32 * s_var * P / (P - 1) + U23 * r[5].abs())
    got = {k: v.get() for k, v in outs.items()}
    got["rm"], got["rv"] = frm.get(), frv.get()
    for i, name in enumerate(("mean", "invstd", "scale", "shift", "rm", "rv")):
        check_stat("bn_finalize_n", "f32", f"{name} S={S}", got[name], r[i], r[i], slack[name])


BWD_GIVEN_C = 16


def bwd_given_partials(dt, S, floats, fill):
    """hiseg_bn_bwd on S split rows written by the test into a `partial` of `floats` values (`fill` elsewhere), checked
    against float64; returns the buffer."""
    N, HW, C = 3, 37, BWD_GIVEN_C
    P = N * HW
    inp = make_bwd_inputs(dt, N, HW, C, RELU, 1.0, True, True, True, True, True, 900 + S)
    args = (inp["dy"], inp["z"], inp["mean"], inp["invstd"], inp["gamma"], inp["beta"], RELU, 1.0, inp["mul"], HW)
    kw = dict(fwd_scale=inp["fwd_scale"], fwd_shift=inp["fwd_shift"], residual=inp["res"], wants_dres=True)
    g64, xh = B.bn_g(*args, **kw)
    rows = torch.zeros(S, 3, C, dtype=torch.float64)
    for p in range(P):                       # pixel p belongs to split p % S; splits >= P stay empty
        rows[p % S, 0] += g64[p]
        rows[p % S, 1] += g64[p] * xh[p]
        rows[p % S, 2] += xh[p]
    rows = rows.float().double()
    part = F32(n=floats, fill=fill)
    part.t[:S * 3 * C] = rows.reshape(-1).float().to(DEV)
    v = dict(dy=View(inp["dy"], dt), z=View(inp["z"], dt), dz=View(None, dt, "vec", P, C),
             residual=View(inp["res"], dt), dres=View(None, dt, "vec", P, C))
    tabs = {k: F32(inp[s]) for k, s in (("chan_mul", "mul"), ("mean", "mean"), ("invstd", "invstd"),
                                        ("gamma", "gamma"), ("beta", "beta"), ("fwd_scale", "fwd_scale"),
                                        ("fwd_shift", "fwd_shift"))}
    for k in ("dgamma", "dbeta", "dconv_bias"):
        tabs[k] = F32(n=C)
    ok(lib().hiseg_bn_bwd(bwd_desc(dt, P, HW, C, v, tabs, RELU, 1.0, 0, 0, part, S), stream()), "bn_bwd")
    path(entry="bwd", vec=True, mode="relu_pre", reduce=False, premerge=S > 256, par=True)
    part.assert_tail()
    assert torch.equal(part.get()[:S * 3 * C].reshape(S, 3, C), rows), "the given partials were modified"
    v["dz"].assert_rest_untouched()
    v["dres"].assert_rest_untouched()

    def ref(g, xh, rows, inv, gam):
        s = rows.sum(0)
        dz = B.bn_bwd_from_sums(g, xh, s[0], s[1], inv, gam, P)
        k = gam * inv
        return dz, s[1], s[0], k * (s[0] - P * (s[0] / P) - s[2] * (s[1] / P))
    r64, r32 = both(ref, g64, xh, rows, inp["invstd"], inp["gamma"])
    tag = f"S={S}"
    check_ew("bn_bwd", dt, f"dz {tag}", v["dz"].live(), r64[0], r32[0], out_mode(dt))
    check_ew("bn_bwd", dt, f"dres {tag}", v["dres"].live(), g64, g64.float(), out_mode(dt))
    ks = (U23 if S <= 256 else (16 + 2 + 4) / 2 * U23)
    b = ks * rows.abs().sum(0)
    check_stat("bn_bwd_params", dt, f"dgamma {tag}", tabs["dgamma"].get(), r64[1], r32[1], b[1])
    check_stat("bn_bwd_params", dt, f"dbeta {tag}", tabs["dbeta"].get(), r64[2], r32[2], b[0])
    kk = (inp["gamma"] * inp["invstd"]).abs()
    s = rows.sum(0).abs()
    check_stat("bn_bwd_params", dt, f"dconv_bias {tag}", tabs["dconv_bias"].get(), r64[3], r32[3],
               kk * (2 * b[0] + s[2] * b[1] / P + s[1] * b[2] / P) + U23 * r64[3].abs())
    for k in ("dgamma", "dbeta", "dconv_bias"):
        tabs[k].assert_tail()
    return part


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("S", [40, 300])
def test_bwd_partial_splits(dt, S):
    """partial_splits > 0: `partial` already holds [S][3][C] sums of (g, g xhat, xhat), here summed by the test from
    the oracle's per-pixel terms and rounded to f32; the reduction pass is skipped and above 256 splits the groups of
    64 are summed first (f32: 16 sequential additions and a two-level tree, k = (16 + 2 + 4) / 2 on sum |rows|).  The
    workspace is exactly (S + ceil(S / 64) + 1) * 3 * C floats."""
    bwd_given_partials(dt, S, (S + -(-S // 64) + 1) * 3 * BWD_GIVEN_C, SENTINEL)


# ------------------------------------------------------------------------------------------- partial buffer sizes
# hiseg.train_engine sizes every `partial` it allocates with bn_stats_partial_floats / bn_bwd_partial_floats; the
# kernels' write extent follows from the split count, KPRE and the 4 KPRE threshold in csrc/bn_train.hip.  Buffers of
# exactly those sizes, filled with NaN, with the sentinel guard behind them.
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("S", [4 * KPRE, 4 * KPRE + 1])
def test_bwd_partial_splits_threshold(dt, S):
    """The last split count without a pre-merge and the first with one (G = 5 groups), the buffer sized as the engine
    sizes the data-gradient epilogue's: the given rows, without a pre-merge one coefficient row, with one G group rows
    and the coefficient row after them are all that is written, and the guard holds (bwd_given_partials)."""
    G = -(-S // KPRE) if S > 4 * KPRE else 0
    assert G == (5 if S == 4 * KPRE + 1 else 0)
    part = bwd_given_partials(dt, S, TE.bn_bwd_partial_floats(BWD_GIVEN_C, S), float("nan"))
    part.assert_written((S + G + 1) * 3 * BWD_GIVEN_C)


# one split; hiseg_bn_partials() splits, the cap; 33 splits of 32 or 33 pixels
EXTENT_P = [31, 32 * 1024, 33 * 32 + 5]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("C", [8, 6])
@pytest.mark.parametrize("P", EXTENT_P)
def test_partial_buffer_extent(dt, C, P):
    """hiseg_bn_stats writes exactly S * 3 * C floats of a bn_stats_partial_floats(C) buffer and hiseg_bn_bwd
    (S + 1) * 3 * C of a bn_bwd_partial_floats(C) one (S rows of sums, one of coefficients), S = P // 32 clamped to
    [1, hiseg_bn_partials()]; the guards hold and no output is NaN.  C = 8: the chunk kernels, C = 6: the scalar ones."""
    cap = lib().hiseg_bn_partials()
    assert EXTENT_P[1] == 32 * cap
    S = max(1, min(cap, P // 32))
    vec = C == 8
    inp = make_bwd_inputs(dt, 1, P, C, NONE, 1.0, False, False, False, True, True, 1200 + C)
    v = dict(dy=View(inp["dy"], dt), z=View(inp["z"], dt), dz=View(None, dt, "vec", P, C))
    part = F32(n=TE.bn_stats_partial_floats(C), fill=float("nan"))
    ok(lib().hiseg_bn_stats(HD[dt], v["z"].t.data_ptr(), P, C, v["z"].cstride, v["z"].coff, part.t.data_ptr(),
                            stream()), "bn_stats")
    path(entry="stats", vec=vec)
    part.assert_tail()
    part.assert_written(S * 3 * C)
    assert part.get()[:S * 3 * C].reshape(S, 3, C)[:, 0].sum(0).eq(P).all(), "n does not sum to P"

    part = F32(n=TE.bn_bwd_partial_floats(C), fill=float("nan"))
    tabs = {k: F32(inp[k]) for k in ("mean", "invstd", "gamma", "beta")}
    for k in ("dgamma", "dbeta", "dconv_bias"):
        tabs[k] = F32(n=C)
    ok(lib().hiseg_bn_bwd(bwd_desc(dt, P, P, C, v, tabs, NONE, 1.0, 0, 0, part), stream()), "bn_bwd")
    path(entry="bwd", vec=vec, mode="none", reduce=True, premerge=False, par=True, u2=False)
    part.assert_tail()
    part.assert_written((S + 1) * 3 * C)
    v["dz"].assert_rest_untouched()
    assert not torch.isnan(v["dz"].live()).any()
    for k in ("dgamma", "dbeta", "dconv_bias"):
        tabs[k].assert_tail()
        assert not torch.isnan(tabs[k].get()).any(), k
