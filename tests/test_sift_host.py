"""The SIFT contract (tests/_sift_numpy.py) on the CPU: what it finds on known images, its symmetry under rotation,
order / duplicates / octave packing, input validation, tiny images, the drop-in classes' signatures, and the two-view
chain from pixels that fixes the bounds of tests/test_gpu_sift.py."""
import inspect
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bfmatcher_numpy as BF  # noqa: E402
import _sift_numpy as S  # noqa: E402
import _sift_chain as C  # noqa: E402
from test_gpu_sift import (MAX_PNP_ROT_DEG, MAX_ROT_DEG, MIN_EPIPOLAR_SHARE, MIN_FUND_INLIERS,  # noqa: E402
                           frame, texture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def blob(sigma, n=96):
    yy, xx = np.mgrid[0:n, 0:n]
    c = (n - 1) / 2.0
    return np.clip(30 + 200 * np.exp(-((xx - c) ** 2 + (yy - c) ** 2) / (2 * sigma ** 2)), 0, 255).astype(np.uint8), c


def test_gaussian_blob_found_at_centre_with_size_proportional_to_sigma():
    sizes = []
    for sigma in (4.0, 8.0):
        img, c = blob(sigma)
        r = S.detect(img)
        d = np.hypot(r["x"] - c, r["y"] - c)
        i = int(np.argmin(d))
        assert d[i] < 0.5, d[i]
        sizes.append(r["size"][i] / sigma)
    # a blob of scale sigma peaks where the DoG scale is about sqrt(2) sigma; size = 2 x scale
    assert abs(sizes[0] / sizes[1] - 1) < 0.15, sizes
    assert 1.5 < sizes[0] < 5.0


def test_rot90_maps_keypoints_angles_and_descriptors():
    img = texture(64, 64, 11)
    a = S.detect(img)
    b = S.detect(np.ascontiguousarray(np.rot90(img)))
    # pixel centres sit at x + 0.25 in the x2 base grid, so the rotation maps (x, y) -> (y, W - 0.5 - x) and the angle
    # to angle - 90 (cv2 angles turn clockwise).  Only the first octave is symmetric: octave o > 0 keeps every other pixel from
    # index 0, which a flip of an even-sized axis moves to the odd pixels.
    w = img.shape[1]
    first = lambda r: (r["octave"] & 255) == 255
    ea = {}
    for x, y, s, an, d, f in zip(a["x"], a["y"], a["size"], a["angle"], a["descriptors"], first(a)):
        if f:
            ea.setdefault((float(y), float(w - 0.5 - x), float(s)), []).append((float(an), d))
    hit = 0
    worst = 0.0
    n_b = 0
    for x, y, s, an, d, f in zip(b["x"], b["y"], b["size"], b["angle"], b["descriptors"], first(b)):
        if not f:
            continue
        n_b += 1
        best = None
        for (kx, ky, ks), lst in ea.items():
            if not (abs(kx - x) < 1e-3 and abs(ky - y) < 1e-3 and abs(ks - s) < 1e-3):
                continue
            for kan, kd in lst:
                da = (an - (kan - 90.0)) % 360.0
                da = min(da, 360 - da)
                if best is None or da < best[0]:
                    best = (da, kd)
        if best is None:
            continue
        hit += 1
        assert best[0] < 1.0, best[0]              # a bin boundary crossed by the reordered blur sums moves a peak
        # not item 4's bound: the two pyramids differ in their last bits (the row pass runs along the other axis), and a
        # sample crossing a bin boundary moves a few counts; the largest difference measured here is 4, the bound is 3x that
        worst = max(worst, float(np.abs(best[1] - d).max()))
        assert np.abs(best[1] - d).max() <= 12
    print("rot90: %d of %d matched, largest descriptor difference %g" % (hit, n_b, worst))
    assert hit >= 0.9 * n_b and hit > 10, (hit, len(ea), n_b)


def test_sort_dedup_and_octave_packing():
    x = np.array([1, 1, 0, 1, 1], np.float32)
    y = np.array([2, 2, 5, 2, 1], np.float32)
    size = np.array([3, 4, 1, 3, 1], np.float32)
    ang = np.array([10, 10, 0, 10, 0], np.float32)
    resp = np.array([0.5, 0.1, 0.2, 0.9, 0.1], np.float32)
    octv = np.array([1, 1, 1, 2, 1], np.int32)
    keep = S.sort_dedup(x, y, size, ang, resp, octv)
    # (0,5) first; then (1,1); then (1,2) size 4 before size 3; of the two (1,2,3,10) the higher response stays
    assert keep.tolist() == [2, 4, 1, 3]
    packed = 0 + (2 << 8) + (200 << 16)
    fixed = (packed & ~255) | ((packed - 1) & 255)
    o, layer, scale = S.unpack_octave(np.array([fixed, packed + 3]))
    assert o.tolist() == [-1, 3] and layer.tolist() == [2, 2] and scale.tolist() == [2.0, 0.125]
    assert (fixed >> 16) & 255 == 200


@pytest.mark.parametrize("bad", [np.zeros((8, 8), np.float32), np.zeros((8, 8, 4), np.uint8), np.zeros((0, 8), np.uint8),
                                 np.zeros((8,), np.uint8), np.zeros((8, 8, 1), np.uint8)])
def test_input_validation(bad):
    with pytest.raises(ValueError):
        S.detect(bad)


def test_bgr_uses_the_fixed_point_rule():
    img = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8)
    g = S.to_gray(img)
    want = [(1868 * b + 9617 * gg + 4899 * r + 8192) >> 14 for b, gg, r in img[0].astype(int)]
    assert g[0].tolist() == [float(v) for v in want]


@pytest.mark.parametrize("shape", [(1, 1), (1, 30), (8, 8), (16, 16), (16, 9), (12, 40)])
def test_tiny_images_work(shape):
    img = texture(max(shape[0], 4), max(shape[1], 4), 5)[:shape[0], :shape[1]]
    r = S.detect(img)
    n_oct = S.octave_count(*shape)
    assert len(r["gauss"]) == max(n_oct, 0)
    if n_oct <= 0:
        assert len(r["x"]) == 0
    for o, lev in enumerate(r["gauss"]):                   # octaves narrower than the blur radius are well defined
        assert all(np.isfinite(g).all() for g in lev)
    assert r["descriptors"].shape == (len(r["x"]), 128)


def test_reflect101_repeats_until_in_range():
    assert S.reflect101(np.array([-1, -5, 3, 7, 12]), 3).tolist() == [1, 1, 1, 1, 0]
    assert S.reflect101(np.array([-4, 9]), 1).tolist() == [0, 0]


def test_view_dropins_keep_the_reference_signatures(sfm, tmp_path):
    api = json.load(open(os.path.join(GOLDEN, "g13_view_api.json")))
    proc = sfm.processors
    for ref_name, cls in (("View", proc.HipView), ("ViewProcessor", proc.HipViewProcessor)):
        for name, sig in api[ref_name]["methods"].items():
            assert hasattr(cls, name), (ref_name, name)
            assert str(inspect.signature(getattr(cls, name))) == sig, (ref_name, name)
    v = proc.HipView(np.zeros((2, 2), np.uint8), 0, np.eye(3), [proc.HipKeyPoint(1.5, 2.5, 3.0, 45.0, 0.1, 255)],
                     np.arange(128, dtype=np.float32)[None])
    assert sorted(vars(v)) == api["View"]["fields"]
    vp = proc.HipViewProcessor('sift')
    assert set(api["ViewProcessor"]["fields"]) - set(vars(vp)) == {"detector"}   # the cv2 detector object
    with pytest.raises(ValueError):
        proc.HipViewProcessor('orb')
    assert proc.HipKeyPoint().class_id == -1 and not hasattr(proc.HipKeyPoint(), "__dict__")
    path = str(tmp_path / "keys.pkl")
    v.write_keys(path)
    back = vp.generate_view(v.img, 0, np.eye(3), key_path=path)
    kp = back.key_pts[0]
    assert (kp.pt, kp.size, kp.angle, kp.response, kp.octave, kp.class_id) == ((1.5, 2.5), 3.0, 45.0, 0.1, 255, -1)
    assert np.array_equal(back.key_descriptors, v.key_descriptors)


def test_three_frame_chain_on_cpu(sfm, oracle):
    """Stand-in -> BFMatcher stand-in (knn 2, ratio 0.7) -> the oracle's two-view functions -> DLT PnP RANSAC and the
    oracle's nonlinear PnP for frame 3: the run that fixed the bounds of test_gpu_sift.py's three-frame test."""
    k = C.halved_k()
    r = [S.detect(frame(n)) for n in (1, 2, 3)]

    def ratio_pairs(a, b):
        knn = BF.BFMatcher(BF.NORM_L2).knnMatch(b["descriptors"], a["descriptors"], k=2)
        p = [(m[0].trainIdx, m[0].queryIdx) for m in knn if len(m) == 2 and m[0].distance / m[1].distance < 0.7]
        return np.array([q[0] for q in p]), np.array([q[1] for q in p])

    def hom(rr, i):
        return np.vstack((rr["x"][i], rr["y"][i], np.ones(len(i))))

    t0, q1 = ratio_pairs(r[0], r[1])
    left, right = hom(r[0], t0), hom(r[1], q1)
    share, med = C.epipolar_fraction(left, right, k, 1)
    random.seed(-1)
    samples = sfm.sampling.sample_indices(left.shape[1], 8, 300, as_array=True)
    inl, fund = oracle.determine_fundamental(left, right, samples, 1e-2)
    ra, rb, ca, cb = oracle.pose_candidates(oracle.essential_from_fundamental(fund, k, k))
    rs, cs = [ra, ra, rb, rb], [ca, cb, ca, cb]
    p0 = k @ np.hstack((np.eye(3), np.zeros((3, 1))))
    projs = [k @ np.hstack((q.T, -q.T @ c)) for q, c in zip(rs, cs)]
    tris = [C.dlt_triangulate(p0, p, left, right) for p in projs]
    best, valid = oracle.disambiguate(p0, projs, tris)
    rot1 = C.rot_angle_deg(rs[best], C.recorded(1)[0])
    valid = np.array(valid)
    pts = oracle.nonlinear_triangulate_vec(tris[best][:, valid], [p0, projs[best]], [left[:, valid], right[:, valid]], 0.5, 100)
    pt_of = {int(key): j for j, key in enumerate(t0[valid])}
    t2, q2 = ratio_pairs(r[0], r[2])
    sel = [(j, pt_of[int(key)]) for j, key in enumerate(t2) if int(key) in pt_of]
    uv = hom(r[2], q2[[s_[0] for s_ in sel]])
    xh = pts[:, [s_[1] for s_ in sel]]
    inl3, r3, c3 = C.dlt_pnp_ransac(uv, xh, k, np.random.default_rng(0))
    r3, c3 = oracle.nonlinear_pnp(uv[:, inl3], xh[:, inl3], k, r3, c3, 5, 300)
    rot3 = C.rot_angle_deg(r3, C.recorded(2)[0])
    print("CPU chain: epipolar share %.3f (median %.2f px), %d inliers, rotation %.2f deg (baseline %.1f deg); frame 3: "
          "%d PnP inliers of %d, rotation %.2f deg" % (share, med, len(inl), rot1, C.dir_angle_deg(cs[best], C.recorded(1)[1]),
                                                       len(inl3), uv.shape[1], rot3))
    assert share >= MIN_EPIPOLAR_SHARE
    assert len(inl) >= MIN_FUND_INLIERS
    assert rot1 <= MAX_ROT_DEG
    assert rot3 <= MAX_PNP_ROT_DEG
