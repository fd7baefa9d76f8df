"""Host side of the ROI-safe training augmentation (hiseg/augment.py) and self-checks of its numpy oracle
(tests/augment_oracle.py): table builders against spelled-out loops, the sampler's determinism and frequencies,
the packed struct's size.  No GPU."""
import math

import numpy as np
import pytest


def _f32(x):
    return np.float32(x)


def test_brightness_contrast_lut_matches_the_loop_and_saturates():
    from hiseg.augment import brightness_contrast_lut
    for alpha, beta in ((1.0, 0.0), (1.2, 0.1), (0.8, -0.2), (3.0, 0.5), (0.5, -0.9), (1.13, -0.07)):
        want = np.zeros(256, np.uint8)
        for i in range(256):
            v = _f32(_f32(i) * _f32(alpha)) + _f32(beta * 255)
            want[i] = int(min(max(float(v), 0.0), 255.0))        # clip, then truncate
        np.testing.assert_array_equal(brightness_contrast_lut(alpha, beta), want, err_msg=str((alpha, beta)))
    assert brightness_contrast_lut(3.0, 0.5)[200:].min() == 255      # saturates high
    assert brightness_contrast_lut(0.5, -0.9)[:200].max() == 0       # and low
    np.testing.assert_array_equal(brightness_contrast_lut(1.0, 0.0), np.arange(256))


def test_rgb_shift_and_hsv_shift_luts_match_the_loops():
    from hiseg.augment import hsv_shift_luts, rgb_shift_lut
    lut = rgb_shift_lut(15, -15, 0.5)
    for c, s in enumerate((15, -15, 0.5)):
        for i in range(256):
            assert lut[c, i] == int(min(max(i + s, 0), 255)), (c, i)
    for hue, sat, val in ((10, -20, 20), (-20, 30, -20), (0, 0, 0), (1, 0, 0), (-7.5, 12.25, -3.5)):
        t = hsv_shift_luts(hue, sat, val)
        assert t.shape == (3, 256) and t.dtype == np.uint8
        for i in range(180):
            assert t[0, i] == int(math.fmod(math.fmod(i + hue, 180) + 180, 180)), (hue, i)
        for i in range(256):
            assert t[1, i] == int(min(max(i + sat, 0), 255))
            assert t[2, i] == int(min(max(i + val, 0), 255))
    assert hsv_shift_luts(1, 0, 0)[0, 179] == 0                       # hue wraps 179 -> 0
    assert hsv_shift_luts(-1, 0, 0)[0, 0] == 179                      # and back, for a negative shift
    np.testing.assert_array_equal(hsv_shift_luts(0, 0, 0)[1], np.arange(256))


def test_gamma_lut():
    from hiseg.augment import gamma_lut
    np.testing.assert_array_equal(gamma_lut(1), np.arange(256))
    for gamma in (0.8, 1.2, 1.07):
        want = [int((i / 255.0) ** gamma * 255) for i in range(256)]
        np.testing.assert_array_equal(gamma_lut(gamma), want)


def test_compose_luts_equals_sequential_application():
    from hiseg.augment import brightness_contrast_lut, compose_luts, gamma_lut, rgb_shift_lut
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, size=(17, 23, 3), dtype=np.uint8)
    a, b = rgb_shift_lut(12, -9, 4), gamma_lut(0.9)
    ab = compose_luts(a, b)
    assert ab.shape == (3, 256)
    seq = np.stack([b[a[c][x[..., c]]] for c in range(3)], -1)
    np.testing.assert_array_equal(np.stack([ab[c][x[..., c]] for c in range(3)], -1), seq)
    p, q = brightness_contrast_lut(1.1, -0.05), gamma_lut(1.15)
    np.testing.assert_array_equal(compose_luts(p, q)[x], q[p[x]])


def test_gaussian_kernel_sums_to_one_and_is_symmetric():
    from hiseg.augment import gaussian_kernel
    for ks in (3, 5, 7):
        for sigma in (0.5, 1.3, 3.0):
            k = gaussian_kernel(ks, sigma)
            assert k.shape == (ks, ks) and k.dtype == np.float32
            assert abs(float(k.astype(np.float64).sum()) - 1.0) <= ks * ks * 2.0 ** -24   # each weight rounded once
            np.testing.assert_array_equal(k, k.T)
            np.testing.assert_array_equal(k, k[::-1, ::-1])
            assert k[ks // 2, ks // 2] == k.max()


def test_sampler_is_deterministic_per_seed():
    from hiseg.augment import RoiSafeAugmentation
    for policy in ("light", "heavy-subset"):
        a = RoiSafeAugmentation(policy, seed=11).sample(64)
        b = RoiSafeAugmentation(policy, seed=11).sample(64)
        c = RoiSafeAugmentation(policy, seed=12).sample(64)
        assert a.host.tobytes() == b.host.tobytes()
        assert a.host.tobytes() != c.host.tobytes()
        assert set(np.unique(a.host["ksize"])) <= ({0, 3, 5} if policy == "light" else {0, 3, 5, 7})
    with pytest.raises(ValueError):
        RoiSafeAugmentation("heavy")


def test_sampler_frequencies_within_four_sigma():
    from hiseg.augment import RoiSafeAugmentation
    n = 4000
    p = RoiSafeAugmentation("light", seed=5).sample(n)
    for name, got, want in (("flip", p.host["flip"].mean(), 0.5), ("colour", p.ran[:, 0].mean(), 0.8),
                            ("blur", p.ran[:, 2].mean(), 0.1)):
        assert abs(got - want) <= 4 * math.sqrt(want * (1 - want) / n), (name, got)
    assert (p.host["ksize"] > 0).mean() == p.ran[:, 2].mean()
    # within the colour group the two members are equally likely (the HSV member sets the hsv flag)
    hsv_share = p.host["hsv"].sum() / p.ran[:, 0].sum()
    assert abs(hsv_share - 0.5) <= 4 * math.sqrt(0.25 / p.ran[:, 0].sum())
    h = RoiSafeAugmentation("heavy-subset", seed=6).sample(n)
    for name, got, want in (("colour", h.ran[:, 0].mean(), 0.8), ("lighting", h.ran[:, 1].mean(), 0.5),
                            ("blur", h.ran[:, 2].mean(), 0.05)):
        assert abs(got - want) <= 4 * math.sqrt(want * (1 - want) / n), (name, got)


def test_packed_struct_size_matches_the_library():
    import ctypes
    from hiseg import _lib as L
    from hiseg.augment import SAMPLE_DTYPE, AugParams
    assert SAMPLE_DTYPE.itemsize == ctypes.sizeof(L.AugSample) == 16 + 6 * 256 + 49 * 4
    assert L.lib().hiseg_aug_struct_size() == SAMPLE_DTYPE.itemsize
    p = AugParams(2)
    p.validate()
    p.host["ksize"][1] = 4
    with pytest.raises(L.HisegError, match="ksize"):
        p.validate()
    with pytest.raises(ValueError):
        AugParams(1).set(0, kernel=np.ones((4, 4), np.float32))


# ---- oracle self-checks ---------------------------------------------------------------------------------------------

def _params(n):
    from hiseg.augment import AugParams
    return AugParams(n)


def test_oracle_identity_returns_the_output_table():
    import augment_oracle as AO
    from hiseg.augment import out_table
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(9, 13, 3), dtype=np.uint8)
    for mode in ("normalize", "div255"):
        tab = out_table(mode)
        np.testing.assert_array_equal(AO.augment(img, _params(1).host[0], tab), tab[img].transpose(2, 0, 1))
    np.testing.assert_array_equal(out_table("div255"), (np.arange(256).astype(np.float32) / 255.0).astype(np.float32))


def test_oracle_hsv_round_trip_with_identity_tables_is_close_to_identity():
    """RGB -> HSV -> RGB at 8 bits loses at most 5 code values: hue has 30 steps per sector, so the sector fraction
    is off by at most 1/60 and a channel V * (1 - S * f) by 255 / 60 = 4.25; S's own rounding (half a step of 1/255,
    times V * f <= 255) adds at most 0.5 and the final rounding 0.5 -- 5.25 in all, so an integer difference <= 5.
    A gross error in either restated direction (a wrong sector, a wrong table) would move pixels by far more."""
    import augment_oracle as AO
    from hiseg.augment import hsv_shift_luts
    v = np.arange(0, 256, 15, dtype=np.uint8)
    img = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(1, -1, 3)
    p = _params(1).set(0, hsv_luts=hsv_shift_luts(0, 0, 0))
    back = AO.colour(img, p.host[0])
    assert np.abs(back.astype(int) - img.astype(int)).max() <= 5
    grey = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, 2)
    np.testing.assert_array_equal(AO.colour(grey, p.host[0]), grey)


def test_oracle_flip_commutes_with_a_symmetric_filter_only():
    import augment_oracle as AO
    from hiseg.augment import gaussian_kernel, out_table
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(12, 17, 3), dtype=np.uint8)
    tab = out_table("normalize")
    g = gaussian_kernel(5, 1.1)
    a = AO.augment(img, _params(1).set(0, flip=True, kernel=g).host[0], tab)
    b = AO.augment(img, _params(1).set(0, flip=False, kernel=g).host[0], tab)[:, :, ::-1]
    np.testing.assert_array_equal(a, b)
    diag = np.eye(7, dtype=np.float32) / 7
    c = AO.augment(img, _params(1).set(0, flip=True, kernel=diag).host[0], tab)
    d = AO.augment(img, _params(1).set(0, flip=False, kernel=diag).host[0], tab)[:, :, ::-1]
    assert not np.array_equal(c, d)


def test_oracle_flipped_target_is_not_the_mirrored_target():
    """cv2's nearest map floors, so resizing the mirrored ROI crop is not mirroring the resized crop: for an
    odd-width ROI the two differ, i.e. these inputs can tell a correct flipped gather from a mirrored output."""
    import augment_oracle as AO
    rng = np.random.default_rng(3)
    m, boxes = AO.ellipses(rng, 3, 97, 131)
    image_size, mask_size = (320, 240), (56, 56)
    differs = 0
    for box in ((40, 30, 40 + 131, 200), (0, 10, 77, 150), (320 - 93, 5, 320, 231)):
        assert (box[2] - box[0]) % 2 == 1
        flipped, nbox = AO.flipped_target(m, 1, box, mask_size, image_size)
        plain = AO.unflipped_target(m, 1, box, mask_size, image_size)
        assert nbox == (320 - box[2], box[1], 320 - box[0], box[3])
        assert set(np.unique(flipped)) <= {0, 1, 2}
        differs += int(not np.array_equal(flipped, plain[:, ::-1]))
    assert differs >= 1
