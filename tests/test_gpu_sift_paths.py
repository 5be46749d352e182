"""Every path of csrc/sfm_sift.hip against the NumPy contract (tests/_sift_numpy.py, precise mode) on small images:
the case table of tests/_sift_cases.py (shapes, BGR, multi-block rows, every sfm_sift_params field, rotations, a clamped
descriptor radius, exact ties, empty lists, zero octaves), the row stride, the C-ABI's error returns and the independence
of one call from the calls before it.  tests/test_sift_paths_host.py holds the table to what it claims on the CPU.

Per case (``_sift_cases.check_image``): pyramid and refined list bit for bit; orientations and descriptors within
FACTOR x that case's own gap between the float64 and the float32 stand-in; the final list's count, value range, order
and independence of keep_pyramid; at most 5 % of the refined keypoints excluded (a peak decision within DELTA).

Measured on MI355X (each test prints its figures): on all 31 cases every angle and descriptor of the 2 962 compared
keypoints is bit-identical to the stand-in's (0 deg / 0 counts against bounds of 4e-4 deg / 1 count, 4 counts on L2);
30 of 2 416 refined keypoints are excluded.  DESIGN.md section 13 lists the source mutations each case catches."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sift_numpy as S  # noqa: E402
import _sift_cases as T  # noqa: E402
from test_gpu_sift import DELTA, FACTOR, _compare, _pyramid_equal, frame, texture  # noqa: E402,F401

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "descriptors")
_seen = {}


@pytest.mark.parametrize("name", T.CASES)
def test_case_equals_the_stand_in(hip, name):
    _seen[name] = T.check_case(hip, name)


def test_exclusion_caps_over_the_table(hip):
    """At most 2 % of the table's refined keypoints are left out of the orientation / descriptor comparison (per case:
    5 %, asserted with each case).  Reports the share of compared keypoints that came out bit-identical."""
    refs = {name: T.reference(name)[0] for name in T.CASES}
    excl = sum(T.excluded(r) for r in refs.values())
    n = sum(len(r["pre"]["x"]) for r in refs.values())
    assert excl <= T.MAX_EXCLUDED_POOL * n, (excl, n)
    matched = sum(s["matched"] for s in _seen.values())
    same = sum(s["identical"] for s in _seen.values())
    print("pooled: %d of %d refined keypoints excluded; %d of %d compared final keypoints bit-identical in angle and "
          "descriptor over %d cases" % (excl, n, same, matched, len(_seen)))


# ---- the C ABI called directly ------------------------------------------------------------------------------------
def _raw_detect(hip, buf, h, w, ch, stride, prm=None):
    """sfm_sift_detect on a raw byte buffer.  Returns (status, a SiftResult around the handle or None)."""
    lib = hip.load()
    handle = ctypes.c_void_p()
    rc = lib.sfm_sift_detect(buf.ctypes.data_as(ctypes.c_void_p), h, w, ch, stride,
                             ctypes.byref(prm) if prm is not None else None, ctypes.byref(handle))
    if rc != hip.OK:
        assert not handle.value
        return rc, None
    r = object.__new__(hip.SiftResult)
    r._lib, r._h = lib, handle
    return rc, r


def _params(hip, **kw):
    v = dict(n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, keep_pyramid=0)
    v.update(kw)
    return hip.SiftParams(int(v["n_octave_layers"]), float(v["contrast_threshold"]), float(v["edge_threshold"]),
                          float(v["sigma"]), int(v["keep_pyramid"]), None)


@pytest.mark.parametrize("name", ["base", "bgr"])
def test_row_stride_with_padding(hip, name):
    """Rows 13 bytes apart from the pixels' end, the padding set to 255, the buffer ending with the last pixel: the
    result equals the contiguous call's bit for bit, so no kernel reads the padding and the upload is no longer than
    stride (h - 1) + w ch."""
    img = T.image(name)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else 3
    stride = w * ch + 13
    buf = np.full(stride * (h - 1) + w * ch, 255, np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf, shape=(h, w * ch), strides=(stride, 1))
    rows[:] = img.reshape(h, w * ch)
    assert buf[w * ch:stride].min() == 255 and buf.size == stride * (h - 1) + w * ch
    want = hip.sift_detect(img)
    rc, r = _raw_detect(hip, buf, h, w, ch, stride)
    assert rc == hip.OK
    with r:
        got = r.arrays()
    assert len(want["x"]) > 0
    for k in FIELDS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    rc, r = _raw_detect(hip, np.ascontiguousarray(img).reshape(-1), h, w, ch, w * ch - 1)
    assert rc == hip.E_SHAPE and r is None


def test_null_params_are_the_defaults(hip):
    img = T.image("odd")
    rc, r = _raw_detect(hip, img.reshape(-1), img.shape[0], img.shape[1], 1, img.shape[1])
    assert rc == hip.OK
    with r:
        got = r.arrays()
        assert r.n_layers == 3 and r.info(hip.SIFT_INFO_KEEPS_PYRAMID) == 0
    rc, r = _raw_detect(hip, img.reshape(-1), img.shape[0], img.shape[1], 1, img.shape[1], _params(hip))
    assert rc == hip.OK
    with r:
        want = r.arrays()
    assert len(want["x"]) == len(T.reference("odd")[0]["x"])
    for k in FIELDS:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k


def test_copy_level_and_info_error_returns(hip):
    lib = hip.load()
    img = T.image("odd")
    out = np.zeros((2 * img.shape[0], 2 * img.shape[1]), np.float32)
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    with hip.SiftResult(img) as r:                          # the pyramid was not kept
        assert lib.sfm_sift_result_copy_level(r._h, hip.SIFT_LEVEL_GAUSS, 0, 0, ptr) == hip.E_SHAPE
        assert "not kept" in hip.last_error()
    with hip.SiftResult(img, n_octave_layers=2, keep_pyramid=True) as r:
        L, n_oct = r.n_layers, r.n_octaves
        assert L == 2 and r.info(hip.SIFT_INFO_KEEPS_PYRAMID) == 1
        assert lib.sfm_sift_result_copy_level(r._h, hip.SIFT_LEVEL_GAUSS, 0, L + 2, ptr) == hip.OK
        assert lib.sfm_sift_result_copy_level(r._h, hip.SIFT_LEVEL_DOG, 0, L + 1, ptr) == hip.OK
        for kind, octave, level in ((hip.SIFT_LEVEL_GAUSS, 0, L + 3), (hip.SIFT_LEVEL_DOG, 0, L + 2),
                                    (hip.SIFT_LEVEL_GAUSS, n_oct, 0), (2, 0, 0), (hip.SIFT_LEVEL_GAUSS, -1, 0),
                                    (hip.SIFT_LEVEL_GAUSS, 0, -1)):
            out[:] = 7.0
            assert lib.sfm_sift_result_copy_level(r._h, kind, octave, level, ptr) == hip.E_SHAPE, (kind, octave, level)
            assert np.all(out == 7.0)
        value = ctypes.c_int64(-5)
        assert lib.sfm_sift_result_info(r._h, 99, ctypes.byref(value)) == hip.E_SHAPE and value.value == -5
        assert lib.sfm_sift_result_info(r._h, hip.SIFT_INFO_N, None) == hip.E_SHAPE
        hh, ww = ctypes.c_int(), ctypes.c_int()
        assert lib.sfm_sift_result_level_shape(r._h, n_oct, ctypes.byref(hh), ctypes.byref(ww)) == hip.E_SHAPE


def test_null_handle_is_refused_by_every_result_function(hip):
    lib = hip.load()
    value, hh, ww = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    out = np.zeros(4, np.float32)
    ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.sfm_sift_result_info(None, hip.SIFT_INFO_N, ctypes.byref(value)) == hip.E_HANDLE
    assert lib.sfm_sift_result_level_shape(None, 0, ctypes.byref(hh), ctypes.byref(ww)) == hip.E_HANDLE
    assert lib.sfm_sift_result_copy(None, ptr, None, None, None, None, None, None) == hip.E_HANDLE
    assert lib.sfm_sift_result_copy_pre(None, ptr, None, None, None, None) == hip.E_HANDLE
    assert lib.sfm_sift_result_copy_level(None, hip.SIFT_LEVEL_GAUSS, 0, 0, ptr) == hip.E_HANDLE
    assert lib.sfm_sift_result_destroy(None) == hip.E_HANDLE
    assert np.all(out == 0)


@pytest.mark.parametrize("bad", [dict(n_octave_layers=17), dict(n_octave_layers=0), dict(sigma=64.0), dict(sigma=0.0),
                                 dict(edge_threshold=0.0), dict(contrast_threshold=-0.01),
                                 dict(contrast_threshold=float("nan"))])
def test_bad_parameters_are_refused(hip, bad):
    img = T.image("odd")
    rc, r = _raw_detect(hip, img.reshape(-1), img.shape[0], img.shape[1], 1, img.shape[1], _params(hip, **bad))
    assert rc == hip.E_SHAPE and r is None
    with pytest.raises(ValueError):
        hip.sift_detect(img, **bad)


def test_oversized_shape_is_refused_before_any_read(hip):
    """sfm_sift_detect checks the shape before it touches the image (the checks precede the call of detect(), which
    holds the only upload), so a 16-byte buffer with a lying width is never read."""
    buf = np.zeros(16, np.uint8)
    for h, w, stride in ((1, 16385, 16385), (16385, 1, 1), (1, 16385, 1)):
        rc, r = _raw_detect(hip, buf, h, w, 1, stride)
        assert rc == hip.E_SHAPE and r is None
    rc, r = _raw_detect(hip, buf, 4, 4, 2, 8)
    assert rc == hip.E_SHAPE
    lib = hip.load()
    assert lib.sfm_sift_detect(None, 4, 4, 1, 4, None, ctypes.byref(ctypes.c_void_p())) == hip.E_SHAPE
    assert lib.sfm_sift_detect(buf.ctypes.data_as(ctypes.c_void_p), 4, 4, 1, 4, None, None) == hip.E_SHAPE


def test_blur_kernel_writes_no_more_than_capacity(hip):
    lib = hip.load()
    full = hip.sift_blur_kernel(1.6)
    assert len(full) == 15 and np.array_equal(full, S.gaussian_kernel(1.6))
    for capacity in (0, 3, -2):
        out = np.full(len(full), -1.0, np.float32)
        k = ctypes.c_int()
        assert lib.sfm_sift_blur_kernel(1.6, capacity, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(k)) == hip.OK
        n = max(capacity, 0)
        assert k.value == len(full) and np.array_equal(out[:n], full[:n]) and np.all(out[n:] == -1.0)
    k = ctypes.c_int(-1)
    assert lib.sfm_sift_blur_kernel(0.0, 0, None, ctypes.byref(k)) == hip.E_SHAPE
    assert lib.sfm_sift_blur_kernel(1.6, 0, None, None) == hip.E_SHAPE
    assert lib.sfm_sift_blur_kernel(1000.0, 0, None, ctypes.byref(k)) == hip.E_SHAPE     # more than 4 095 taps


def test_result_does_not_depend_on_the_calls_before_it(hip):
    """The scratch planes and the pyramid come from a pool: the base case after a wider image and after a 19-level
    pyramid equals the base case alone, and a pyramid that a result keeps is not touched by later calls."""
    base = T.image("base")
    alone = hip.sift_detect(base)
    assert len(alone["x"]) == len(T.reference("base")[0]["x"])
    hip.sift_detect(T.image("wide"))
    ref16 = T.reference("L16")[0]
    with hip.SiftResult(base, n_octave_layers=16, keep_pyramid=True) as r16:
        assert r16.n == len(ref16["x"])
        after = hip.sift_detect(base)
        hip.sift_detect(T.image("wide"))
        for o, i in ((0, 18), (1, 0), (r16.n_octaves - 1, 18)):
            got = r16.level(hip.SIFT_LEVEL_GAUSS, o, i)
            assert np.array_equal(got.view(np.uint32), ref16["gauss"][o][i].view(np.uint32)), (o, i)
        got = r16.level(hip.SIFT_LEVEL_DOG, 0, 17)
        assert np.array_equal(got.view(np.uint32), ref16["dog"][0][17].view(np.uint32))
    again = hip.sift_detect(base)
    for k in FIELDS:
        assert np.array_equal(alone[k].view(np.uint32), after[k].view(np.uint32)), k
        assert np.array_equal(alone[k].view(np.uint32), again[k].view(np.uint32)), k
