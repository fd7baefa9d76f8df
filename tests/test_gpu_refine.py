"""Boundary refinement stage and active-contour loss on the GPU against the reference's recorded results
(tests/golden/refine.npz, gen_refine_golden.py).

Bars.  Module tensors that pass through convs: 1e-4 relative to the tensor's largest magnitude (the project's
bar, tests/test_gpu_parity.py); loss scalars 1e-5 (tests/test_gpu_train.py).  bf16: the error against the f32
fixture is at most twice the reference's own CPU bf16-autocast error plus 1e-4.  The whole-model step compares
with the bars of test_train_step_f32_matches_oracle (the ~50-layer train-mode BatchNorm stack amplifies rounding:
logits 3e-3, loss 1e-4, loss-dict entries 1e-3, gradients by cosine)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import filler
from helpers import b0_kwargs, hiseg_kwargs, load

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["min", "odd", "big", "const", "flat"]


@pytest.fixture(scope="module")
def G():
    return load("refine")


def rel(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double().cpu(), torch.as_tensor(np.asarray(b)).double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _module(G, norm, dtype=torch.float32, act="relu"):
    import hiseg
    m = filler.fill_module(hiseg.BoundaryRefinementModule(3, 32, norm, 8, act, 1.0))
    with torch.no_grad():
        m.blend_weight.fill_(float(G["blend"]))
    return hiseg.set_compute_dtype(m, dtype).to(DEV)


@pytest.mark.parametrize("norm", ["batchnorm", "layernorm2d"])
@pytest.mark.parametrize("case", CASES)
def test_module_eval_f32(G, case, norm):
    from hiseg import engine
    tag = "bn" if norm == "batchnorm" else "ln"
    x = torch.from_numpy(G[f"{case}_x"]).to(DEV)
    m = _module(G, norm).eval()
    out, E = engine.boundary_refine_nchw(m, x, want_edges=True)
    assert torch.equal(m(x), out)
    ref = torch.from_numpy(G[f"{case}_{tag}_eval_out"])
    if case == "const":   # the E = 0 branch: exact
        assert torch.equal(out.cpu(), x.cpu()) and torch.equal(out.cpu(), ref) and float(E.abs().max()) == 0.0
        return
    e_err = rel(E.cpu(), G[f"{case}_E"])
    d_err = rel((out - x).cpu(), ref - x.cpu())
    print(f"refine eval f32 {case}/{tag}: E {e_err:.2e} delta {d_err:.2e}")
    assert e_err < 1e-4 and d_err < 1e-4


@pytest.mark.parametrize("case", CASES)
def test_module_train_f32(G, case):
    m = _module(G, "batchnorm").train()
    x = torch.from_numpy(G[f"{case}_x"]).to(DEV).requires_grad_(True)
    g = torch.from_numpy(G[f"{case}_g"]).to(DEV)
    out = m(x)
    (out * g).sum().backward()
    torch.cuda.synchronize()
    dx = x.grad.cpu()
    ref_dx = torch.from_numpy(G[f"{case}_dx"])
    if case == "const":
        assert torch.equal(out.detach().cpu(), x.detach().cpu()) and torch.equal(dx, g.cpu())
    elif case == "flat":   # the reference's NaN where dy = dx = 0 exactly, the bar elsewhere
        nan = torch.from_numpy(G["flat_dx_nan"])
        assert torch.equal(torch.isnan(dx), nan)
        dx = torch.where(nan, torch.zeros_like(dx), dx)
    errs = {"out": rel((out.detach() - x.detach()).cpu(), torch.from_numpy(G[f"{case}_bn_train_out"]) - x.detach().cpu())
            if case != "const" else 0.0, "dx": rel(dx, ref_dx)}
    params = dict(m.named_parameters())
    for n in G[f"{case}_grad_names"]:
        rg = G[f"{case}_grad_{n}"]
        mg = params[str(n)].grad.cpu()
        assert torch.isfinite(mg).all(), n
        if np.abs(rg).max() == 0.0:
            assert float(mg.abs().max()) == 0.0, n
            continue
        if str(n) in ("edge_conv.0.bias", "edge_conv.3.bias"):
            # a conv bias in front of a train-mode BatchNorm has an exactly zero gradient (the batch mean removes
            # it): the reference holds rounding noise there, so the 1e-4 bar is taken relative to the gradient
            # that flows through that node, the norm's own bias gradient (tests/test_gpu_train.py does the same)
            scale = np.abs(G[f"{case}_grad_edge_conv.{int(str(n).split('.')[1]) + 1}.bias"]).max()
            assert np.abs(rg).max() < 1e-4 * scale, n
            errs[str(n)] = float(mg.abs().max()) / scale
            continue
        errs[str(n)] = rel(mg, rg)
    for n, b in m.named_buffers():
        if "running_" in n:
            errs[n] = rel(b.cpu(), G[f"{case}_buf_{n}"])
    print(f"refine train f32 {case}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, bad


def test_module_train_is_bit_reproducible(G):
    outs = []
    for _ in range(2):
        m = _module(G, "batchnorm").train()
        x = torch.from_numpy(G["big_x"]).to(DEV).requires_grad_(True)
        (m(x) * torch.from_numpy(G["big_g"]).to(DEV)).sum().backward()
        outs.append(torch.cat([x.grad.reshape(-1)] + [p.grad.reshape(-1) for p in m.parameters()]).cpu())
    assert torch.equal(outs[0], outs[1])


def _bf16_err(G, case, tag, out, x):
    ref = torch.from_numpy(G[f"{case}_{tag}_eval_out"])
    err = ((out - x).cpu() - (ref - x.cpu())).abs().max().item()
    bar = 2.0 * float(G[f"{case}_{tag}_eval_bf16_err"]) + 1e-4
    return err, bar


@pytest.mark.parametrize("case", ["min", "odd", "big", "flat"])
def test_module_eval_bf16_fused(G, case):
    """bf16 + eval BatchNorm + ReLU is the fused kernel's case: it is the path taken (one launch counted, no conv
    launch recorded) and meets the bf16 bar.  `min` (2 x 3) sits inside one tile, `big` (40 x 36) spans 3 x 3 tiles
    and is no multiple of 16, `odd` is 9 x 7."""
    from hiseg import engine, ops
    x = torch.from_numpy(G[f"{case}_x"]).to(DEV)
    m = _module(G, "batchnorm", torch.bfloat16).eval()
    assert engine.refine_fused_eligible(m, torch.bfloat16)
    before = ops.FUSED_REFINE_CALLS[0]
    ops.RECORD = []
    try:
        out = m(x)
        convs = len(ops.RECORD)
    finally:
        ops.RECORD = None
    assert ops.FUSED_REFINE_CALLS[0] == before + 1 and convs == 0
    err, bar = _bf16_err(G, case, "bn", out, x)
    print(f"refine eval bf16 fused {case}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar


def test_module_eval_bf16_fused_constant_input_is_exact(G):
    x = torch.from_numpy(G["const_x"]).to(DEV)
    assert torch.equal(_module(G, "batchnorm", torch.bfloat16).eval()(x), x)


@pytest.mark.parametrize("norm,act,tag", [("batchnorm", "relu", "bn"), ("layernorm2d", "relu", "ln"),
                                          ("batchnorm", "silu", "bnsilu")])
@pytest.mark.parametrize("case", ["odd", "big"])
def test_module_eval_bf16_chain(G, case, norm, act, tag, monkeypatch):
    """The conv chain in bf16 (edge map, blend and the final 1x1's output stay f32): the fallback for modules the
    fused kernel does not cover (LayerNorm2d, SiLU -- not eligible, no fused launch) and, with the fused kernel
    switched off, for the one it does.  Same bar."""
    from hiseg import engine, ops
    x = torch.from_numpy(G[f"{case}_x"]).to(DEV)
    m = _module(G, norm, torch.bfloat16, act).eval()
    if tag == "bn":
        monkeypatch.setenv("HISEG_REFINE_FUSED", "0")
    assert not engine.refine_fused_eligible(m, torch.bfloat16)
    before = ops.FUSED_REFINE_CALLS[0]
    ops.RECORD = []
    try:
        out = m(x)
        convs = len(ops.RECORD)
    finally:
        ops.RECORD = None
    assert ops.FUSED_REFINE_CALLS[0] == before and convs == 3
    err, bar = _bf16_err(G, case, tag, out, x)
    print(f"refine eval bf16 chain {case}/{tag}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar


def test_module_silu_f32_matches_fixture(G):
    x = torch.from_numpy(G["odd_x"]).to(DEV)
    out = _module(G, "batchnorm", act="silu").eval()(x)
    err = rel((out - x).cpu(), torch.from_numpy(G["odd_bnsilu_eval_out"]) - x.cpu())
    print(f"refine eval f32 odd/bnsilu: delta {err:.2e}")
    assert err < 1e-4


@pytest.mark.parametrize("case", ["ac_small", "ac_odd", "ac_mask"])
def test_active_contour(G, case):
    """Value and gradient; ac_small (2x2) runs through the zero-curvature code."""
    import hiseg
    pred = torch.from_numpy(G[f"{case}_pred"]).to(DEV).requires_grad_(True)
    loss = hiseg.active_contour_term(pred)
    loss.backward()
    v_err = abs(float(loss) / float(G[f"{case}_loss"]) - 1.0)
    g_err = rel(pred.grad.cpu(), G[f"{case}_grad"])
    print(f"active contour {case}: value {v_err:.2e} grad {g_err:.2e}")
    assert v_err < 1e-5 and g_err < 1e-4
    pred2 = pred.detach().clone().requires_grad_(True)
    hiseg.active_contour_term(pred2).backward()
    assert torch.equal(pred.grad, pred2.grad)


# ------------------------------------------------------------------------------------------ whole model
def _model(G, dt, refine=True):
    import hiseg
    m = hiseg.create_rgb_hierarchical_model(**hiseg_kwargs(dict(b0_kwargs(), use_boundary_refinement=refine)))
    filler.fill_module(m)
    if refine:
        with torch.no_grad():
            m.segmentation_head.boundary_refiner.blend_weight.fill_(float(G["blend"]))
    for mod in m.modules():
        if isinstance(mod, (nn.Dropout, nn.Dropout2d)):
            mod.p = 0.0
    hiseg.set_compute_dtype(m, dt)
    for mm in (m.roi_align_mask, m.roi_align_rgb):
        mm.spatial_scale_h, mm.spatial_scale_w = 96, 128
    return m.to(DEV)


def _inputs():
    images = torch.from_numpy(filler.uniform(61, (2, 3, 96, 128))).to(DEV)
    u = torch.from_numpy(filler.normal(62, (2, 1, 96, 128)) * 2.0).to(DEV)
    rois = torch.tensor([[0, .10, .10, .40, .90], [1, .35, .15, .80, .95], [0, .55, .05, .95, .70]]).to(DEV)
    tgt = torch.from_numpy(filler.ellipse_targets(63, 3, 128, 96)).to(DEV)
    return images, u, rois, tgt


def _loss():
    import hiseg
    return hiseg.RefinedHierarchicalLoss(
        use_active_contour_loss=True, use_boundary_aware_loss=True, use_contour_detection=True,
        use_distance_transform=True, active_contour_weight=0.1, boundary_aware_weight=0.1, contour_loss_weight=0.1,
        distance_loss_weight=0.1)


def sample(t, k):
    f = t.detach().reshape(-1)
    return f[::max(1, f.numel() // k)][:k].clone()


def test_head_eval_forward_matches_fixture(G):
    from hiseg import engine
    images, u, rois, _ = _inputs()
    m = _model(G, torch.float32).eval()
    logits, aux = engine.rgb_model_forward(m, images, rois, "full", unet_logit_override=u)
    plain = _model(G, torch.float32, refine=False).eval()
    base, _ = engine.rgb_model_forward(plain, images, rois, "full", unet_logit_override=u)
    errs = (rel(sample(logits, 4096).cpu(), G["step_eval_logits"]), rel(sample(base, 4096).cpu(), G["step_eval_base_logits"]),
            rel(sample(aux["bg_fg_logits"], 4096).cpu(), G["step_eval_bgfg"]))
    print("refine head eval: logits %.2e base %.2e bgfg %.2e" % errs)
    assert max(errs) < 1e-4
    assert not torch.equal(logits, base)


def _train_step(G, m, loss_fn, images, u, rois, tgt):
    from hiseg import train_engine as TE
    logits, aux = TE.train_forward(m, images, rois, u_override=u)
    loss, d = loss_fn(logits, tgt, aux)
    loss.backward()
    return logits, loss, d, aux


def test_train_step_matches_fixture_and_is_reproducible(G):
    images, u, rois, tgt = _inputs()
    runs = []
    for _ in range(2):
        m = _model(G, torch.float32).train()
        logits, loss, d, aux = _train_step(G, m, _loss(), images, u, rois, tgt)
        grads = torch.cat([p.grad.reshape(-1) for p in m.parameters() if p.grad is not None])
        runs.append((logits.detach().clone(), loss.detach().clone(), grads.clone()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    l_err = rel(sample(logits, 4096).cpu(), G["step_logits"])
    print(f"refine step: logits {l_err:.2e} loss {float(loss):.6f} vs {float(G['step_loss']):.6f}")
    assert l_err < 3e-3
    for k, f in (("bg_fg_logits", "step_bgfg"), ("target_nontarget_logits", "step_tn"), ("contours", "step_contours")):
        a_err = rel(sample(aux[k], 4096).cpu(), G[f])   # the aux tensors are the base head's: same bar as the logits
        print(f"  aux {k}: {a_err:.2e}")
        assert a_err < 3e-3, k
    assert float(loss) == pytest.approx(float(G["step_loss"]), rel=1e-4)
    ref_d = dict(zip([str(k) for k in G["step_dict_keys"]], G["step_dict"]))
    for k in ("bg_fg_loss", "final_loss", "dice_loss", "active_contour", "boundary_aware", "contour",
              "distance_transform", "total_loss"):
        print(f"  {k}: {d[k]:.6f} vs {ref_d[k]:.6f}")
        assert d[k] == pytest.approx(ref_d[k], rel=1e-3), k
    params = dict(m.named_parameters())
    for n in G["step_grad_names"]:
        n = str(n)
        rg = torch.from_numpy(G[f"step_grad_{n}"]).double().reshape(-1)
        mg = params[n].grad.detach().cpu()
        if f"step_gradsq_{n}" in G.files:
            assert float((mg.double() ** 2).sum()) == pytest.approx(float(G[f"step_gradsq_{n}"]), rel=4e-2), n
            mg = sample(mg, 1024)
        mg = mg.double().reshape(-1)
        if rg.numel() == 1:   # a scalar's cosine is its sign: compare the value (the step's gradient-norm bar, 4e-2)
            print(f"  grad {n}: {float(mg):.6e} vs {float(rg):.6e}")
            assert float(mg) == pytest.approx(float(rg), rel=4e-2), n
            continue
        if n.endswith(".bias") and rg.norm() < 1e-4:   # a conv bias in front of train-mode BatchNorm: rounding noise
            assert mg.norm() < 1e-4, n                 # around an exactly zero gradient (test_train_step_f32_matches_oracle)
            continue
        cos = float((mg * rg).sum() / (mg.norm() * rg.norm()))
        print(f"  grad {n}: cos {cos:.5f} norm {float(mg.norm()):.4e} vs {float(rg.norm()):.4e}")
        assert cos > (0.95 if rg.numel() <= 4 else 0.99), (n, cos)
    br = m.segmentation_head.boundary_refiner
    for n, b in br.named_buffers():
        if "running_" in n:
            assert rel(b.cpu(), G[f"step_buf_{n}"]) < 1e-3, n
        elif n.endswith("num_batches_tracked"):
            assert int(b) == int(G[f"step_buf_{n}"])


def test_graphed_train_step_with_refiner_equals_eager(G):
    """One captured step replayed against eager steps from the same state (bf16, fused AdamW): the stage makes no
    host synchronisation, and the losses are identical bit for bit."""
    import hiseg
    images, u, rois, tgt = _inputs()
    runs = []
    for graphed in (False, True):
        m = _model(G, torch.bfloat16).train()
        loss_fn = _loss()
        st = {"opt": None}

        def step():
            logits, aux = m(images, rois)
            loss, _ = loss_fn(logits, tgt, aux)
            if st["opt"] is None:
                st["opt"] = hiseg.FusedAdamW(m, lr=5e-4, weight_decay=0.01, max_grad_norm=1.0)
            st["opt"].zero_grad()
            loss.backward()
            st["opt"].step()
            return loss

        run = hiseg.GraphedStep(step, lambda: st["opt"]) if graphed else step
        losses = [float(run().detach()) for _ in range(3)]
        torch.cuda.synchronize()
        runs.append((losses, torch.cat([p.detach().float().reshape(-1) for p in m.parameters()]).cpu()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    assert all(np.isfinite(v) for v in runs[0][0])


def test_export_masks_come_from_refined_logits(G):
    import hiseg
    from hiseg import engine
    images, _, rois, _ = _inputs()
    m = _model(G, torch.bfloat16).eval()
    logits, _ = m(images, rois)
    inst, binary = engine.export_forward(m, images, rois)
    assert torch.equal(inst[:, 0] > 0.5, logits.argmax(1) == 1)
    plain = _model(G, torch.bfloat16, refine=False).eval()
    inst0, binary0 = engine.export_forward(plain, images, rois)
    assert int((inst != inst0).sum()) >= 1 and torch.equal(binary, binary0)
    got = hiseg.StreamPipelinedExport(hiseg.RGBHierarchicalExportWrapper(m)).run([(images, rois)] * 3)
    torch.cuda.synchronize()
    assert len(got) == 3 and all(torch.equal(a, inst) and torch.equal(b, binary) for a, b in got)
