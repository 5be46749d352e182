"""The case table of the SIFT path tests, shared by tests/test_gpu_sift_paths.py (device against the stand-in) and
tests/test_sift_paths_host.py (what the table claims about the stand-in), and the per-case comparison both the path
tests and test_gpu_sift.py::test_tiny_images run.  Test code only; the reference is tests/_sift_numpy.py, precise mode.

Every image is small: the stand-in takes a fraction of a second per case, and its results are computed once per
process (``reference``) and never modified."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sift_numpy as S  # noqa: E402
from test_gpu_sift import DELTA, FACTOR, _compare, _key, _pyramid_equal, _refined_equal, texture  # noqa: E402

TINY_SHAPES = ((1, 1), (1, 40), (8, 8), (16, 16), (16, 9))       # the shapes of test_gpu_sift.py::test_tiny_images
MAX_EXCLUDED_CASE = 0.05                                         # share of a case's refined keypoints left out
MAX_EXCLUDED_POOL = 0.02                                         # ... and of the whole table's


def tiny_image(shape):
    return texture(max(shape[0], 4), max(shape[1], 4), 7)[:shape[0], :shape[1]]


def _base():
    return texture(64, 80, 1)


def _rot(k):
    return lambda: np.ascontiguousarray(np.rot90(texture(64, 64, 11), k))


def _blob24():
    yy, xx = np.mgrid[0:24, 0:24]
    return np.clip(30 + 200 * np.exp(-((xx - 11.5) ** 2 + (yy - 11.5) ** 2) / (2 * 5.0 ** 2)), 0, 255).astype(np.uint8)


def _stripes():
    _, xx = np.mgrid[0:48, 0:48]
    return (((xx // 4) % 2) * 255).astype(np.uint8)


def _faint():
    return (128 + (texture(40, 40, 30) >= 128)).astype(np.uint8)


def _checker():
    yy, xx = np.mgrid[0:48, 0:48]
    return ((((xx // 8) + (yy // 8)) % 2) * 255).astype(np.uint8)


# name -> (image maker, parameters, group).  The group names the table row; caps and claims are stated per row.
_TABLE = [
    ("base", _base, {}, "shape"),
    ("odd", lambda: texture(45, 67, 2), {}, "shape"),
    ("bgr", lambda: texture(57, 40, 3, 3), {}, "shape"),
    ("wide", lambda: texture(20, 150, 6, 3), {}, "shape"),     # 2 w = 300 > 256: the second x-block of base / blur / down
    ("tall", lambda: texture(150, 20, 7), {}, "shape"),        # levels narrower than the blur radius, long column pass
    ("L1", _base, dict(n_octave_layers=1), "layers"),
    ("L2", _base, dict(n_octave_layers=2), "layers"),
    ("L5", _base, dict(n_octave_layers=5), "layers"),
    ("L16", _base, dict(n_octave_layers=16), "layers"),        # the ABI's upper bound
    ("s0.8", _base, dict(sigma=0.8), "sigma"),                 # max(s^2 - 1, 0.01): a 3-tap base blur
    ("s1.2", _base, dict(sigma=1.2), "sigma"),
    ("s2.4", _base, dict(sigma=2.4), "sigma"),
    ("c0", _base, dict(contrast_threshold=0.0), "thresholds"),
    ("c0.1e3", _base, dict(contrast_threshold=0.1, edge_threshold=3.0), "thresholds"),
    ("e100", _base, dict(edge_threshold=100.0), "thresholds"),
    ("rot0", _rot(0), {}, "rot"),
    ("rot1", _rot(1), {}, "rot"),
    ("rot2", _rot(2), {}, "rot"),
    ("rot3", _rot(3), {}, "rot"),
    ("flip", lambda: np.ascontiguousarray(texture(64, 64, 11)[:, ::-1]), {}, "rot"),
    ("blob24", _blob24, {}, "blob"),
    ("stripes", _stripes, {}, "ties"),
    ("checker", _checker, {}, "ties"),
    # two gray levels, 16 layers, no contrast threshold: DoG values a few float32 steps apart, so tied maxima and minima
    # survive refinement and refinement steps of exactly 0.5 occur in x, y and the layer (the < 0.5 tests)
    ("faint", _faint, dict(contrast_threshold=0.0, n_octave_layers=16), "ties"),
    ("flat128", lambda: np.full((40, 40), 128, np.uint8), {}, "flat"),
    ("flat0", lambda: np.zeros((40, 40), np.uint8), {}, "flat"),
] + [("tiny%dx%d" % s, functools.partial(tiny_image, s), {}, "tiny") for s in TINY_SHAPES]

CASES = [t[0] for t in _TABLE]
_BY_NAME = {t[0]: t for t in _TABLE}


def group(name):
    return _BY_NAME[name][3]


def params(name):
    return dict(_BY_NAME[name][2])


def image(name):
    return _BY_NAME[name][1]()


@functools.lru_cache(maxsize=None)
def _reference_of(img_bytes, shape, items):
    img = np.frombuffer(img_bytes, np.uint8).reshape(shape)
    prm = dict(items)
    ref = S.detect(img, precise=True, **prm)
    r32 = S.detect(img, precise=False, **prm)
    ga, gd, _ = _compare(ref, r32, np.inf, np.inf, ref["ori_margin"])
    return ref, (ga, gd)


def reference_for(img, **prm):
    """(stand-in result in precise mode, (angle gap in degrees, descriptor gap in counts) to the float32 stand-in) of
    any image; computed once per process and shared, so callers must not modify it."""
    img = np.ascontiguousarray(img)
    return _reference_of(img.tobytes(), img.shape, tuple(sorted(prm.items())))


def reference(name):
    return reference_for(image(name), **params(name))


def excluded(ref):
    """Refined keypoints the orientation / descriptor comparison leaves out: a peak decision within DELTA."""
    return int(np.count_nonzero(ref["ori_margin"] < DELTA))


def tolerances(gap):
    """This project's rule: FACTOR x the float64 / float32 stand-in gap, at least 1e-4 deg x FACTOR and 1 count."""
    return FACTOR * max(gap[0], 1e-4), max(1.0, FACTOR * gap[1])


def _identical_share(ref, got):
    """(matched final keypoints, those whose angle and whole descriptor are bit-identical)."""
    def ranked(r):
        g = {}
        for i in range(len(r["x"])):
            g.setdefault(_key(r, i), []).append(i)
        return {(k, n): i for k, idx in g.items() for n, i in enumerate(sorted(idx, key=lambda i: r["angle"][i]))}
    a, b = ranked(ref), ranked(got)
    both = [(a[k], b[k]) for k in a if k in b]
    same = sum(1 for i, j in both if ref["angle"][i].tobytes() == got["angle"][j].tobytes()
               and np.array_equal(ref["descriptors"][i], got["descriptors"][j]))
    return len(both), same


def check_image(hip, img, label="", **prm):
    """The whole per-case comparison of the device with the stand-in for one image and parameter set:
    1. every Gaussian and DoG level and the refined list bit for bit (size within 1 float32 ulp);
    2. orientations and descriptors within FACTOR x the case's own float64 / float32 stand-in gap;
    3. the final list: count, integer descriptors in [0, 255], the contract's order, keep_pyramid on = off;
    4. at most MAX_EXCLUDED_CASE of the refined keypoints left out of 2.
    Returns a dict of the figures it printed."""
    ref, gap = reference_for(img, **prm)
    pre, _, kept = _pyramid_equal(hip, img, ref=ref, **prm)
    _refined_equal(pre, ref["pre"])
    angle_tol, desc_tol = tolerances(gap)
    got = hip.sift_detect(img, **prm)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), kept[k].view(np.uint32)), "keep_pyramid changes %s" % k
    amax, dmax, excl = _compare(ref, got, angle_tol, desc_tol, ref["ori_margin"])
    n_pre = len(ref["pre"]["x"])
    assert len(excl) <= MAX_EXCLUDED_CASE * n_pre, (len(excl), n_pre)
    if not excl:
        assert len(got["x"]) == len(ref["x"])
    assert got["descriptors"].shape == (len(got["x"]), 128)
    assert np.all(got["descriptors"] == np.rint(got["descriptors"]))
    if len(got["x"]):
        assert got["descriptors"].min() >= 0 and got["descriptors"].max() <= 255
    keep = S.sort_dedup(got["x"], got["y"], got["size"], got["angle"], got["response"], got["octave"])
    assert np.array_equal(keep, np.arange(len(got["x"])))
    matched, same = _identical_share(ref, got)
    out = dict(refined=n_pre, final=len(got["x"]), excluded=len(excl), gap_angle=gap[0], gap_desc=gap[1], angle=amax,
               desc=dmax, matched=matched, identical=same)
    print("%s: %d refined / %d final, %d excluded; stand-in gap %.3g deg / %g counts (bounds %.3g / %g); device %.3g deg / "
          "%g counts; %d of %d angle + descriptor bit-identical"
          % (label, n_pre, len(got["x"]), len(excl), gap[0], gap[1], angle_tol, desc_tol, amax, dmax, same, matched))
    return out


def check_case(hip, name):
    return check_image(hip, image(name), label=name, **params(name))
