"""tests/loss_optim_oracle.py is right, and the premises of tests/test_gpu_loss_optim_kernels.py hold, on the CPU:

  * the float64 loss oracle against the reference's own recorded results (tests/golden/train_loss.npz, cases a to e
    with the three consecutive calls of case a) at the tolerances of tests/test_oracle_train.py, and against
    oracle/train.py's torch restatement at float64 on configurations the golden lacks;
  * its float32 and float64 evaluations of the boundary, contour and distance target maps agree bit for bit on every
    case table of the GPU file;
  * every case table keeps its promised margins (nothing is excluded from any comparison there);
  * the optimiser oracle against torch.optim.AdamW: float64 against float64, and the float32 evaluation against
    torch.optim.AdamW(foreach=True) in float32 on the CPU.  Observed: m and v do not match bit for bit, because
    torch's CPU lerp and addcmul fuse a multiply-add that the order in adamw_seg_kernel's comment rounds twice
    (test_adamw_oracle_matches_torch records the figures); they and the parameters stay within the f32 rule.
"""
import numpy as np
import pytest
import torch

import loss_optim_oracle as O
import test_gpu_loss_optim_kernels as G
from helpers import load
from oracle import train as T
from test_oracle_train import loss_inputs, loss_targets

pytestmark = []          # (the imported module's gpu mark does not apply here)
F32, F64 = np.float32, np.float64
GRADS = ("pred", "bgfg", "tn", "cont", "dist")


# ------------------------------------------------------------------------------------------- loss: recorded reference
def golden_cfg(H, W, c_w=0.1, base_res=64 * 48):
    """The reference's resolution-adjusted contour weight and dilation kernel (oracle/train.py)."""
    wgt = max(0.001, min(c_w * float(np.sqrt(base_res / (H * W))), 0.5))
    ew = max(1, int(np.sqrt(H * W / 3072) * 1.5))
    return O.make_cfg(contour_weight=wgt, contour_ks=2 * ew - 1 if ew > 1 else 1)


DICT_TO_OUT = {"bg_fg_loss": 1, "target_nontarget_loss": 2, "final_loss": 3, "consistency_loss": 4, "total_loss": 15,
               "ce_loss": 3, "dice_loss": 5, "aux_fg_bg_loss": 1, "aux_fg_accuracy": 9, "aux_fg_iou": 10,
               "bg_weight": 11, "fg_weight": 12, "target_weight": 13, "nontarget_weight": 14, "boundary_aware": 6,
               "contour": 7, "distance_transform": 8}


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_loss_oracle_matches_recorded_reference(case):
    g = load("train_loss")
    keys = [str(k) for k in g["dict_keys"]]
    names = sorted({k.split("_")[0] for k in g.files if k.endswith("_meta")})
    state = O.state_init()
    for key in [n for n in names if n[0] == case]:
        seed, n, mh, mw = (int(v) for v in g[f"{key}_meta"])
        ins = [t.numpy().astype(F32) for t in loss_inputs(seed, n, mh, mw)]
        tg = loss_targets(str(g[f"{key}_kind"]), seed, n, mh, mw).numpy()
        cfg = golden_cfg(mh, mw)
        out, grads, state, _ = O.loss_eval(cfg, *ins, tg, state)
        ref_loss = float(g[f"{key}_loss"])
        assert abs(out[0] - ref_loss) < 1e-5 * max(1.0, abs(ref_loss)), key
        for k, rv in zip(keys, g[f"{key}_dict"]):
            if np.isnan(rv):
                continue
            got = cfg["contour_weight"] if k == "contour_weight" else out[DICT_TO_OUT[k]]
            assert got == pytest.approx(float(rv), rel=1e-5, abs=1e-6), (key, k)
        for nm in GRADS:
            ref = g[f"{key}_grad_{nm}"]
            if ref.size == 0:
                assert not grads[nm].any(), (key, nm)
                continue
            assert np.abs(grads[nm] - ref).max() <= 1e-6 + 1e-4 * np.abs(ref).max(), (key, nm)


# ------------------------------------------------------------------------------------------- loss: torch restatement
def torch_loss(cfg, case, H, W, grad_out=1.0):
    """oracle/train.py's RefinedHierarchicalLoss at float64 with the cfg's weights; its contour dilation follows the
    image size, so contour_targets is evaluated with the cfg's kernel here."""
    fn = T.RefinedHierarchicalLoss(bg_weight=cfg["bg_weight"], fg_weight=cfg["fg_weight"],
                                   target_weight=cfg["target_weight"], consistency_weight=cfg["consistency_weight"],
                                   use_dynamic_weights=bool(cfg["use_dynamic_weights"]), dice_weight=cfg["dice_weight"],
                                   ce_weight=cfg["ce_weight"], boundary_aware_weight=cfg["boundary_aware_weight"],
                                   contour_loss_weight=cfg["contour_weight"],
                                   distance_loss_weight=cfg["distance_weight"],
                                   use_boundary_aware_loss=bool(cfg["use_boundary_aware"]),
                                   use_contour_detection=bool(cfg["use_contour"]),
                                   use_distance_transform=bool(cfg["use_distance"]), base_mask_size=(H, W))
    ins = {k: torch.from_numpy(case[k]).double().requires_grad_(True) for k in GRADS}
    tg = torch.from_numpy(case["tg"])
    aux = {"bg_fg_logits": ins["bgfg"], "target_nontarget_logits": ins["tn"], "contours": ins["cont"],
           "distance_map": ins["dist"]}
    ks = cfg["contour_ks"]
    old = T.contour_targets

    def contour_targets(masks):
        t = (masks == 1).double()[:, None]
        dy = torch.nn.functional.pad((t[:, :, 1:] - t[:, :, :-1]).abs(), (0, 0, 0, 1), mode="replicate")
        dx = torch.nn.functional.pad((t[:, :, :, 1:] - t[:, :, :, :-1]).abs(), (0, 1, 0, 0), mode="replicate")
        c = torch.max(dy, dx)
        if ks > 1:
            c = (torch.nn.functional.conv2d(c, torch.ones(1, 1, ks, ks, dtype=torch.float64) / (ks * ks),
                                            padding=ks // 2) > 0.1).double()
        return c

    T.contour_targets = contour_targets
    try:
        loss, d = fn(ins["pred"], tg, aux)
    finally:
        T.contour_targets = old
    (grad_out * loss).backward()
    return loss.item(), d, {k: (np.zeros_like(case[k], F64) if v.grad is None else v.grad.numpy()) for k, v in ins.items()}


TORCH_CFGS = [("static", dict(use_dynamic_weights=0)), ("no_ba", dict(use_boundary_aware=0)),
              ("no_contour", dict(use_contour=0)), ("no_dist", dict(use_distance=0)), ("ks3", dict(contour_ks=3)),
              ("ks7", dict(contour_ks=7)), ("no_dice", dict(dice_weight=0.0)), ("go", dict())]


@pytest.mark.parametrize("name,kw", TORCH_CFGS)
def test_loss_oracle_matches_torch_restatement(name, kw):
    case = G.make_case("ellipse", 17, 2, 20, 14)
    cfg = O.make_cfg(**dict(dict(contour_ks=5), **kw))
    go = -0.75 if name == "go" else 1.0
    out, grads, _, _ = O.loss_eval(cfg, *(case[k] for k in GRADS), case["tg"], O.state_init(), grad_out=go)
    loss, d, tgrads = torch_loss(cfg, case, 20, 14, go)
    assert out[0] == pytest.approx(loss, rel=1e-12)
    pairs = {k: i for k, i in DICT_TO_OUT.items() if k in d}
    for k, i in pairs.items():
        # the torch restatement keeps its class weights and counts in f32 tensors
        assert out[i] == pytest.approx(d[k], rel=1e-6 if "weight" in k or k.startswith("aux_fg") else 1e-11), k
    for k in GRADS:
        assert np.abs(grads[k] - tgrads[k]).max() <= 1e-12 * max(1.0, np.abs(tgrads[k]).max()), k


# ------------------------------------------------------------------------------------------- loss: premises
ALL_CASES = G.LOSS_CASES()


@pytest.mark.parametrize("name", [c[0] for c in ALL_CASES])
def test_loss_case_premises(name):
    """Target maps bit-identical in f32 and f64, and the promised margins, on one case table of the GPU file."""
    _, cfg, case = next(c for c in ALL_CASES if c[0] == name)
    tg, ks = case["tg"], cfg["contour_ks"]
    for fn in (O.boundary_weight, O.contour_raw, lambda t, d: O.contour_target(t, ks, d), O.distance_target):
        a32, a64 = fn(tg, F32), fn(tg, F64)
        assert a32.dtype == F32 and np.array_equal(a32.astype(F64), a64)
    assert set(np.unique(tg)) <= {0, 1, 2}
    for k in GRADS:
        assert case[k].dtype == F32 and np.isfinite(case[k]).all()
    diff = case["bgfg"][:, 1].astype(F64) - case["bgfg"][:, 0]
    tie = diff == 0
    assert (np.abs(diff)[~tie] >= 2.0 ** -6).all()
    assert tie.any() == case["ties"], "exact ties only where they are placed on purpose"
    r = case["dist"][:, 0].astype(F64) - O.distance_target(tg)
    assert ((r == 0) | (np.abs(r) >= 2.0 ** -10)).all()
    _, _, _, X = O.loss_eval(cfg, *(case[k] for k in GRADS), tg, O.state_init())
    for k, v in X["raw"].items():
        assert v < 9 or v > 11, (k, v)
    for w in X["raw_weights"]:
        for edge in (0.5, 3.0):
            # exactly on the edge the clamp changes nothing; otherwise 1 % away from it, or far beyond
            assert w == edge or abs(w / edge - 1) >= 0.01, (w, edge)


def test_loss_cases_cover_the_issue():
    names = [c[0] for c in ALL_CASES]
    assert len(set(names)) == len(names)
    raw = {}
    for n, cfg, case in ALL_CASES:
        if n.startswith(("clamp/", "weights/", "state/")):
            raw[n] = O.loss_eval(cfg, *(case[k] for k in GRADS), case["tg"], O.state_init())[3]
    assert raw["clamp/ba"]["raw"]["ba"] > 11 and raw["clamp/contour"]["raw"]["contour"] > 11
    assert raw["clamp/dist"]["raw"]["dist"] > 11 and all(v < 9 for v in raw["clamp/none"]["raw"].values())
    w = {n: raw[f"weights/{n}"]["raw_weights"] for n in ("one_fg", "all_fg", "one_nt")}
    assert w["one_fg"][1] > 3.0 and w["one_fg"][2] == 0.5 and w["all_fg"][0] > 3.0 and w["one_nt"][3] > 3.0
    assert not raw["state/ellipse_first/1"]["active"] and raw["state/ellipse_first/2"]["active"]
    assert not raw["state/bg_first/0"]["active"] and raw["state/bg_first/1"]["active"]


# ------------------------------------------------------------------------------------------- optimiser
def test_seg_index():
    seg = np.array([0, 0, 1, 37, 37, 38, 99, 100], np.int64)
    sg = O.seg_index(seg, 100)
    for i in range(100):
        s = sg[i]
        assert seg[s] <= i < seg[s + 1]
    for kind in (1, 8, 256):
        for n in G.OPT_N:
            t = G.seg_table(kind, n)
            assert len(t) == kind + 1 and t[0] == 0 and t[-1] == n and (np.diff(t) >= 0).all()
            if kind == 8 and n > 1000:
                assert (t[1:-1] % 256 != 0).all()
            if kind == 256 and n > 1000:
                d = np.diff(t)
                assert (d == 0).any() and (d == 1).any() and 37 in t and n - 1 in t


def _torch_run(dtype, foreach, steps=6, join=3, max_norm=1.0):
    """Four parameters, one per segment; the last two join the optimiser at step `join` (a new optimiser with the old
    state transferred, as progressive unfreezing does).  Returns per-step flat (p, m, v) and the per-step gradients."""
    rng = np.random.default_rng(5)
    sizes = [7, 300, 1, 64]
    ps = [torch.from_numpy(rng.standard_normal(s).astype(F32)).to(dtype).requires_grad_(True) for s in sizes]
    grads = [[torch.from_numpy((0.3 * rng.standard_normal(s)).astype(F32)).to(dtype) for s in sizes]
             for _ in range(steps)]
    # python doubles, as the training script passes them; the kernels get hyper()'s f32 roundings of the same values
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, foreach=foreach)
    opt = torch.optim.AdamW(ps[:2], **kw)
    hist = []
    for s in range(steps):
        if s == join:
            old, opt = opt, torch.optim.AdamW(ps, **kw)
            for p in ps[:2]:
                opt.state[p] = old.state[p]
        live = ps if s >= join else ps[:2]
        for p, g in zip(ps, grads[s]):
            p.grad = g.clone() if any(p is q for q in live) else None
        norm = torch.nn.utils.clip_grad_norm_(live, max_norm)
        opt.step()
        flat = lambda f: np.concatenate([f(p).detach().numpy().astype(F64) for p in live])
        hist.append((flat(lambda p: p), flat(lambda p: opt.state[p]["exp_avg"]),
                     flat(lambda p: opt.state[p]["exp_avg_sq"]), float(norm)))
    return sizes, [p.detach() for p in ps], grads, hist


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_adamw_oracle_matches_torch(mode):
    dt, tdt = (F64, torch.float64) if mode == "f64" else (F32, torch.float32)
    rng = np.random.default_rng(5)
    sizes = [7, 300, 1, 64]
    p0 = [rng.standard_normal(s).astype(F32) for s in sizes]
    _, _, grads, hist = _torch_run(tdt, foreach=True)
    h = O.hyper(exact=(mode == "f64"))
    join, n2 = 3, sizes[0] + sizes[1]
    p = np.concatenate(p0).astype(dt)
    m, v = np.zeros_like(p), np.zeros_like(p)
    seg = np.array([0, sizes[0], n2, n2 + sizes[2], sum(sizes)], np.int64)
    steps = np.zeros(4, np.int64)
    for s in range(6):
        k = 4 if s >= join else 2
        n = int(seg[k])
        g = np.concatenate([t.numpy() for t in grads[s][:k]]).astype(dt)
        if mode == "f64":
            norm = np.sqrt((g * g).sum())
        else:   # torch's norm: the f32 2-norm of the per-tensor f32 norms
            norm = float(hist[s][3])
        out = O.adamw_segmented(p[:n], g, m[:n], v[:n], h, norm, 1.0, seg[:k + 1], steps[:k], dt)
        p[:n], m[:n], v[:n], steps[:k] = out[0], out[2], out[3], out[4]
        tp, tm, tv, tnorm = hist[s]
        assert float(norm) == pytest.approx(tnorm, rel=1e-6)
        if mode == "f64":
            for a, b in ((p[:n], tp), (m[:n], tm), (v[:n], tv)):
                assert np.abs(a - b).max() <= 1e-13 * max(1.0, np.abs(b).max())
        else:
            # Observed: not bit for bit.  torch's CPU lerp is one fused multiply-add, self + weight * diff rounded
            # once, where the kernel's comment (and this oracle) round the product first: m differs by one unit in
            # the last place in about a tenth of the elements; v differs likewise in about 0.2 % (addcmul's
            # vectorised value * g * g).  Each stays within one rounding per step of the largest element.
            for a, b, name in ((m[:n], tm, "m"), (v[:n], tv, "v")):
                assert np.abs(a - b).max() <= (s + 1) * 2.0 ** -23 * np.abs(b).max(), f"{name} at step {s}"
            assert np.abs(p[:n] - tp).max() <= 4 * 2.0 ** -23 * np.abs(tp).max()
    assert steps.tolist() == [6, 6, 3, 3]


def test_adamw_lerp_branches_and_skip():
    rng = np.random.default_rng(1)
    p, g, m, v = (rng.standard_normal(50).astype(F32) for _ in range(4))
    v = np.abs(v)
    seg, steps = np.array([0, 50]), np.array([4])
    for b1 in (0.9, 0.3):         # 1 - b1 < 0.5 and >= 0.5: both branches of torch.lerp's formula
        h = O.hyper(b1=b1)
        m32 = O.adamw_segmented(p, g, m, v, h, 1.0, 0.0, seg, steps, F32)[2]
        want = torch.lerp(torch.from_numpy(m).double(), torch.from_numpy(g).double(), h["omb1"]).numpy()
        assert np.abs(m32 - want).max() <= 2.0 ** -23 * np.abs(want).max()
        d = g - m                                   # the two branches, each operation rounded to f32
        own = m + F32(h["omb1"]) * d if h["omb1"] < 0.5 else g - d * (F32(1) - F32(h["omb1"]))
        assert np.array_equal(m32, own)
        m64 = O.adamw_segmented(p, g, m, v, h, 1.0, 0.0, seg, steps, F64)[2]
        assert np.abs(m64 - (h["b1"] * m.astype(F64) + h["omb1"] * g)).max() < 1e-7
    for bad in (np.nan, np.inf):
        out = O.adamw_segmented(p, g, m, v, O.hyper(), F32(bad), 1.0, seg, steps, F32)
        assert out[5] == 1 and out[4].tolist() == [4]
        for a, b in zip(out[:4], (p, g, m, v)):
            assert np.array_equal(a, b)
        out = O.adamw_guarded(p, g, m, v, O.hyper(), F32(bad), 1.0, 4, F32)
        assert out[5] == 1 and out[4] == 4 and np.array_equal(out[0], p)


def test_adamw_plain_and_guarded_match_segmented_in_float64():
    """The three restatements are one update rule: in float64 they agree to rounding."""
    rng = np.random.default_rng(2)
    p, g, m, v = (rng.standard_normal(300).astype(F32) for _ in range(4))
    v = np.abs(v)
    h = O.hyper()
    norm = O.norm_from_partials(O.grad_norm_partials_ref(g))
    assert float(norm) == pytest.approx(np.sqrt((g.astype(F64) ** 2).sum()), rel=1e-7)
    a = O.adamw_segmented(p, g, m, v, h, norm, 1.0, np.array([0, 300]), np.array([9]), F64)
    b = O.adamw_guarded(p, g, m, v, h, norm, 1.0, 9, F64)
    c = O.adamw_plain(p, g, m, v, h, 1 - h["b1"] ** 10, 1 - h["b2"] ** 10, norm, 1.0, F64)
    for x, y, z in zip(a[:4], b[:4], c):
        assert np.abs(x - y).max() < 1e-6 and np.abs(x - z).max() < 1e-6
    part = O.grad_norm_partials_ref(np.ones(262144 + 300, F32))
    assert part[0] == 512 and part[1] == 256 + 44 and part[2:].tolist() == [256.0] * 1022
