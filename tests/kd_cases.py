"""Cases of the knowledge-distillation fixtures (tests/golden/kd.npz), shared by the generator
(tests/golden/gen_kd_golden.py) and the tests: shapes, temperatures, the seeded inputs (not stored in the fixture)
and how each variant calls ``DistillationLoss``."""
import numpy as np

import filler

SHAPES = ((1, 1, 1), (2, 7, 5), (3, 12, 10), (3, 33, 29), (2, 128, 96))
TEMPS = (4.0, 1.0, 0.5)
ALPHA = 0.7
STUB = {"total_loss": 0.625, "ce_loss": 0.5, "dice_loss": 0.125}
VARIANTS = ("all", "taux_none", "no_s_bgfg", "no_t_bgfg", "no_s_tn", "no_t_tn", "nologits", "bare")
AUX = ("bg_fg_logits", "target_nontarget_logits")


def tag(shape):
    return "s%dx%dx%d" % shape


def ttag(t):
    return "T" + str(t).replace(".", "p")


def kd_inputs(shape):
    """Student and teacher (logits, bg_fg, target_nontarget) ~ 2 N(0,1), f32 numpy, seeded by the shape."""
    n, h, w = shape
    seed = 7000 + 97 * n + 13 * h + w
    ch = (3, 2, 2)
    s = [filler.normal(seed + i, (n, c, h, w)) * 2.0 for i, c in enumerate(ch)]
    t = [filler.normal(seed + 10 + i, (n, c, h, w)) * 2.0 for i, c in enumerate(ch)]
    return s, t


def kd_targets(shape):
    n, h, w = shape
    return filler.ellipse_targets(7100 + n + h + w, n, h, w)


def grad_pixels(hw):
    p = np.arange(hw)
    return p[(p % 8 == 0) | (p < 128) | (p >= hw - 128)]


def call(variant, loss_fn, s, t, target):
    """(total, dict, heads) of one variant; s, t: lists of leaf tensors."""
    saux = dict(zip(AUX, s[1:]))
    taux = dict(zip(AUX, t[1:]))
    heads = [True, True, True]
    if variant == "taux_none":
        total, d = loss_fn((s[0], saux), t[0], target)
        heads = [True, False, False]
    elif variant == "bare":
        total, d = loss_fn(s[0], (t[0], taux), target, aux_outputs=saux)
    else:
        if variant == "no_s_bgfg":
            del saux[AUX[0]]
            heads[1] = False
        elif variant == "no_t_bgfg":
            del taux[AUX[0]]
            heads[1] = False
        elif variant == "no_s_tn":
            del saux[AUX[1]]
            heads[2] = False
        elif variant == "no_t_tn":
            del taux[AUX[1]]
            heads[2] = False
        elif variant == "nologits":
            heads[0] = False
        total, d = loss_fn((s[0], saux), (t[0], taux), target)
    return total, d, heads
