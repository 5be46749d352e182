"""SIFT detection on the device against the NumPy contract (tests/_sift_numpy.py): the pyramid and the refined
keypoints bit for bit, orientations and descriptors under a bound measured on the CPU, run-to-run identity, and two
real frames through the two-view chain."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sift_numpy as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# a keypoint before orientation is left out of the orientation / descriptor comparison only when one of its peak
# decisions lies within DELTA of the histogram maximum (relative); the tolerances are FACTOR x the gap between the
# float64 and the float32 stand-in, measured on frame 1 (``gap`` below)
DELTA = 1e-3
FACTOR = 4.0


def frame(n):
    return np.load(os.path.join(GOLDEN, "g13_upenn_%d.npz" % n))["image"]


def texture(h, w, seed, channels=1):
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, size=(h // 4 + 2, w // 4 + 2, channels)).astype(np.float64)
    img = np.kron(small, np.ones((4, 4, 1)))[:h, :w]
    yy, xx = np.mgrid[0:h, 0:w]
    img = img * 0.6 + 80 * (np.sin(xx / 5.0) * np.cos(yy / 7.0))[..., None] + 50
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img[..., 0] if channels == 1 else img


@pytest.fixture(scope="session")
def ref1():
    return S.detect(frame(1))


@pytest.fixture(scope="session")
def gap(ref1):
    """Largest angle (degrees) and descriptor (counts) difference between the float64 and the float32 stand-in."""
    r32 = S.detect(frame(1), precise=False)
    a, d, _ = _compare(ref1, r32, np.inf, np.inf, ref1["ori_margin"])
    return a, d


def _key(r, i):
    return (r["x"][i].tobytes(), r["y"][i].tobytes(), r["size"][i].tobytes(), r["response"][i].tobytes(), int(r["octave"][i]))


def _compare(ref, got, angle_tol, desc_tol, margin):
    """Every final keypoint whose parent clears DELTA must appear on both sides with its angles and descriptor
    within the bounds.  Returns (largest angle gap, largest descriptor gap, excluded parents)."""
    def groups(r):
        g = {}
        for i in range(len(r["x"])):
            g.setdefault(_key(r, i), []).append(i)
        return g
    gr, gg = groups(ref), groups(got)
    excluded = set(int(p) for p in np.nonzero(margin < DELTA)[0])
    skip_keys = {_key(ref, i) for i in range(len(ref["x"])) if int(ref["parent"][i]) in excluded}
    amax = dmax = 0.0
    for k, idx in gr.items():
        if k in skip_keys:
            continue
        assert k in gg, "keypoint %r missing" % (k,)
        jdx = gg[k]
        assert len(idx) == len(jdx), (k, ref["angle"][idx], got["angle"][jdx])
        ia = sorted(idx, key=lambda i: ref["angle"][i])
        ja = sorted(jdx, key=lambda j: got["angle"][j])
        for i, j in zip(ia, ja):
            da = abs(float(ref["angle"][i]) - float(got["angle"][j]))
            da = min(da, 360.0 - da)
            dd = float(np.abs(ref["descriptors"][i] - got["descriptors"][j]).max())
            amax, dmax = max(amax, da), max(dmax, dd)
    extra = [k for k in gg if k not in gr and k not in skip_keys]
    assert len(extra) <= len(skip_keys), "device keypoints the stand-in does not have: %d" % len(extra)
    assert amax <= angle_tol and dmax <= desc_tol, (amax, angle_tol, dmax, desc_tol)
    return amax, dmax, excluded


def _pyramid_equal(hip, img, ref=None, **params):
    """Every Gaussian and DoG level of the device equals the stand-in's bit for bit, for any sfm_sift_params values.
    Returns (the device's refined list, the stand-in result, the device's final arrays with the pyramid kept)."""
    if ref is None:
        ref = S.detect(img, with_descriptors=False, **params)
    with hip.SiftResult(img, keep_pyramid=True, **params) as r:
        assert r.n_octaves == len(ref["gauss"])
        assert r.n_layers == params.get("n_octave_layers", 3)
        for o in range(r.n_octaves):
            assert len(ref["gauss"][o]) == r.n_layers + 3 and len(ref["dog"][o]) == r.n_layers + 2
            for i, lev in enumerate(ref["gauss"][o]):
                got = r.level(hip.SIFT_LEVEL_GAUSS, o, i)
                assert got.shape == lev.shape and np.array_equal(got.view(np.uint32), lev.view(np.uint32)), ("gauss", o, i)
            for i, lev in enumerate(ref["dog"][o]):
                got = r.level(hip.SIFT_LEVEL_DOG, o, i)
                assert got.shape == lev.shape and np.array_equal(got.view(np.uint32), lev.view(np.uint32)), ("dog", o, i)
        return r.pre(), ref, r.arrays()


def _refined_equal(pre, want):
    """The refined keypoints before orientation: the same count, x, y, response and octave bit for bit (compared as
    sorted lists), size within 1 float32 ulp (exp2 on both sides)."""
    assert len(pre["x"]) == len(want["x"])
    key = lambda d, size: sorted(zip(d["x"].view(np.uint32).tolist(), d["y"].view(np.uint32).tolist(),
                                     d["response"].view(np.uint32).tolist(), d["octave"].tolist(), size))
    a = key(pre, pre["size"].tolist())
    b = key(want, want["size"].tolist())
    assert [t[:4] for t in a] == [t[:4] for t in b]
    for (_, _, _, _, sa), (_, _, _, _, sb) in zip(a, b):
        assert abs(np.float32(sa) - np.float32(sb)) <= np.spacing(np.float32(sb))


@pytest.mark.parametrize("shape,channels,seed", [((64, 80), 1, 1), ((45, 67), 1, 2), ((57, 40), 3, 3), ((12, 30), 1, 4)])
def test_pyramid_bit_exact_synthetic(hip, shape, channels, seed):
    """Gray and BGR, even and odd sizes, and a 12-row image whose last octaves are narrower than the blur radius."""
    pre, ref, _ = _pyramid_equal(hip, texture(shape[0], shape[1], seed, channels))
    _refined_equal(pre, ref["pre"])


def test_pyramid_and_refined_keypoints_bit_exact_on_frame(hip, ref1):
    pre, _, _ = _pyramid_equal(hip, frame(1))
    _refined_equal(pre, ref1["pre"])


def test_blur_weights_equal_stand_in(hip):
    p = S.Params()
    for s in [S.base_sigma(p)] + S.level_sigmas(p)[1:]:
        assert np.array_equal(hip.sift_blur_kernel(s), S.gaussian_kernel(s))


def test_orientations_and_descriptors_within_measured_bound(hip, ref1, gap):
    ga, gd = gap
    angle_tol = FACTOR * max(ga, 1e-4)
    desc_tol = max(1.0, FACTOR * gd)
    got = hip.sift_detect(frame(1))
    _, _, excluded = _compare(ref1, got, angle_tol, desc_tol, ref1["ori_margin"])
    print("excluded %d of %d refined keypoints; gap angle %.3g deg, descriptor %.3g" % (len(excluded), len(ref1["pre"]["x"]), ga, gd))
    assert len(excluded) < 0.01 * len(ref1["pre"]["x"])
    assert np.all(got["descriptors"] == np.rint(got["descriptors"]))
    assert got["descriptors"].min() >= 0 and got["descriptors"].max() <= 255


def test_final_order_is_the_contract(hip):
    got = hip.sift_detect(frame(2))
    keep = S.sort_dedup(got["x"], got["y"], got["size"], got["angle"], got["response"], got["octave"])
    assert np.array_equal(keep, np.arange(len(got["x"])))


def test_run_to_run_and_two_streams_identical(hip):
    import torch
    img = frame(3)
    a = hip.sift_detect(img)
    b = hip.sift_detect(img)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = [None, None]

    def run(i):
        out[i] = hip.sift_detect(img, stream=streams[i].cuda_stream)
    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for r in out:
        for k in a:
            assert np.array_equal(a[k], r[k]), k


def test_tiny_images(hip):
    """Zero octaves and one-pixel rows, each through the whole per-case comparison of the path tests."""
    from _sift_cases import TINY_SHAPES, check_image, tiny_image
    for shape in TINY_SHAPES:
        check_image(hip, tiny_image(shape), label="tiny %dx%d" % shape)


def test_bad_input_raises(hip):
    with pytest.raises(ValueError):
        hip.sift_detect(np.zeros((10, 10), np.float32))
    with pytest.raises(ValueError):
        hip.sift_detect(np.zeros((10, 10, 4), np.uint8))
    with pytest.raises(ValueError):
        hip.sift_detect(np.zeros((0, 10), np.uint8))
    with pytest.raises(ValueError):
        hip.sift_detect(np.zeros((32, 32), np.uint8), n_octave_layers=0)


# ---- three real frames from pixels: two-view initialisation, PnP of frame 3, one bundle adjustment -------------------
# Bounds fixed from the CPU run of the same chain (tests/test_sift_host.py::test_three_frame_chain_on_cpu; stand-in,
# BFMatcher stand-in, the oracle's two-view functions and nonlinear PnP) before the device ran it.  Measured there:
# 60 % of the ratio-test pairs of frames 1-2 within 2 px of the recorded pose's epipolar lines (median 1.6 px); 89
# fundamental inliers; view-1 rotation 4.3 deg from the recorded one; frame 3: rotation 7.7 deg.  The CPU run's PnP
# inlier count (58 of 126) comes from a DLT RANSAC, not the reference's six-point RANSAC with its own inlier test, so it
# bounds nothing here; the device's count is reported, and a registration that failed would show in the rotation.
# The baseline direction is not bounded: the two-view chain puts it 65-78 deg off on the CPU too.
MIN_EPIPOLAR_SHARE = 0.5
MIN_FUND_INLIERS = 60
MAX_ROT_DEG = 10.0
MAX_PNP_ROT_DEG = 15.0


def test_three_real_frames_from_pixels(sfm, hip):
    import _sift_chain as C
    k = C.halved_k()
    out = C.process_three_on_device(sfm, [frame(1), frame(2), frame(3)], k)
    share, med = C.epipolar_fraction(out["pairs01"][0], out["pairs01"][1], k, 1)
    views = out["views"]
    rot1 = C.rot_angle_deg(views[1].rot, C.recorded(1)[0])
    base1 = C.dir_angle_deg(views[1].loc, C.recorded(1)[1])
    rot3 = C.rot_angle_deg(out["pnp_rot"], C.recorded(2)[0])
    print("epipolar share %.3f (median %.2f px), fundamental inliers %d, view-1 rotation %.2f deg (baseline %.1f deg), "
          "frame 3: %d PnP inliers of %d, rotation %.2f deg; BA over %d points: rmse %.3f -> %.3f px"
          % (share, med, out["fund_inliers"], rot1, base1, out["pnp_inliers"], out["pnp_points"], rot3, out["n_points"],
             out["rmse_before_ba"], out["rmse_after_ba"]))
    assert share >= MIN_EPIPOLAR_SHARE
    assert out["fund_inliers"] >= MIN_FUND_INLIERS
    assert rot1 <= MAX_ROT_DEG
    assert rot3 <= MAX_PNP_ROT_DEG
    assert np.isfinite(out["rmse_after_ba"]) and out["rmse_after_ba"] <= out["rmse_before_ba"] * 1.01
    assert all(isinstance(p, sfm.processors.HipKeyPoint) for p in views[0].key_pts[:10])
    assert views[0].key_descriptors.dtype == np.float32 and views[0].key_descriptors.shape[1] == 128
