"""What the case table of the SIFT path tests (tests/_sift_cases.py) claims, checked on the stand-in alone, so that a
change to ``texture`` or to the stand-in cannot quietly empty a case of tests/test_gpu_sift_paths.py.  If a claim
fails, change the seed or the size of that case, not the claim."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sift_numpy as S  # noqa: E402
import _sift_cases as T  # noqa: E402
from test_gpu_sift import DELTA, FACTOR, texture  # noqa: E402


def _refined(name):
    return len(T.reference(name)[0]["pre"]["x"])


@pytest.mark.parametrize("name", T.CASES)
def test_case_finds_keypoints_and_stays_inside_the_exclusion_cap(name):
    ref, gap = T.reference(name)
    n, excl = _refined(name), T.excluded(ref)
    print("%s: %d refined / %d final, %d excluded, stand-in gap %.3g deg / %g counts" % (name, n, len(ref["x"]), excl, gap[0], gap[1]))
    if T.group(name) == "flat":
        assert n == 0 and len(ref["gauss"]) > 0            # octaves exist, no candidate: the n_pre == 0 branch
        assert len(ref["cand"]["o"]) == 0
    elif T.group(name) == "tiny":
        assert n > 0 or len(ref["x"]) == 0
    elif name == "stripes":
        # every row is the same, so every candidate ties with its vertical neighbours and dyy = 0 rejects it (det <= 0):
        # the image reaches the >= / <= ties and, provably, nothing after them; the row's other images do (below)
        assert n == 0 and len(ref["cand"]["o"]) > 0
    else:
        assert n > 0
    assert excl <= T.MAX_EXCLUDED_CASE * n
    angle_tol, desc_tol = T.tolerances(gap)
    assert angle_tol >= FACTOR * 1e-4 and desc_tol >= 1.0


def test_pooled_exclusion_cap():
    excl = sum(T.excluded(T.reference(name)[0]) for name in T.CASES)
    n = sum(_refined(name) for name in T.CASES)
    print("pooled: %d of %d refined keypoints excluded (DELTA %g)" % (excl, n, DELTA))
    assert excl <= T.MAX_EXCLUDED_POOL * n


def test_base_case_reaches_three_octaves_and_all_layers():
    pre = T.reference("base")[0]["pre"]
    assert len(pre["x"]) == 87 and len(T.reference("base")[0]["x"]) == 114
    assert sorted(set(pre["o"].tolist())) == [0, 1, 2] and sorted(set(pre["layer"].tolist())) == [1, 2, 3]


@pytest.mark.parametrize("name,layers", [("L1", 1), ("L2", 2), ("L5", 5)])
def test_layer_cases_reach_every_layer(name, layers):
    ref = T.reference(name)[0]
    assert sorted(set(ref["pre"]["layer"].tolist())) == list(range(1, layers + 1))
    assert all(len(g) == layers + 3 for g in ref["gauss"])


def test_l16_reaches_the_last_layer_and_sigma_cases_change_the_tap_counts():
    assert int(T.reference("L16")[0]["pre"]["layer"].max()) == 16
    taps = {s: len(S.gaussian_kernel(S.base_sigma(S.Params(sigma=s)))) for s in (0.8, 1.2, 1.6, 2.4)}
    assert taps[0.8] == 3                                   # the max(s^2 - 1, 0.01) clamp: sigma 0.1
    assert len(set(taps.values())) == 4
    assert _refined("s0.8") == 555
    for s in (0.8, 1.2, 2.4):                               # and every level's blur differs from the default's
        assert [len(S.gaussian_kernel(x)) for x in S.level_sigmas(S.Params(sigma=s))[1:]] != \
               [len(S.gaussian_kernel(x)) for x in S.level_sigmas(S.Params())[1:]]


def test_threshold_cases_change_what_is_kept():
    base = _refined("base")
    assert _refined("c0") > base and _refined("e100") > base and _refined("c0.1e3") < base
    for name in ("c0", "c0.1e3", "e100"):
        p = S.Params(**T.params(name))
        assert np.floor(0.5 * p.contrast / p.L * 255) == (0 if name == "c0" else 4 if name == "c0.1e3" else 1)


def test_wide_and_tall_reach_the_second_block_and_the_narrow_levels():
    wide, tall = T.image("wide"), T.image("tall")
    assert wide.ndim == 3 and 2 * wide.shape[1] > 256 and (2 * wide.shape[1] - 10 + 63) // 64 == 5
    ref = T.reference("tall")[0]
    radius = max(len(S.gaussian_kernel(s)) for s in S.level_sigmas(S.Params())[1:]) // 2
    narrow = [g[0].shape for g in ref["gauss"] if g[0].shape[1] <= radius]
    assert narrow and max(h for h, _ in narrow) > radius    # reflect101 folds more than once along x, rows stay long


@pytest.mark.parametrize("name", ["rot0", "rot1", "rot2", "rot3", "flip"])
def test_rotations_have_an_angle_at_the_wrap(name):
    ang = T.reference(name)[0]["angle"]
    assert np.count_nonzero((ang < 5) | (ang > 355)) >= 1


def test_descriptor_bin_cannot_reach_n():
    """``if (o0 >= n) o0 -= n`` of the descriptor cannot fire: the sample's angle is below 360 and the keypoint's is not
    negative, and the largest float32 below 360 times float32(8 / 360) is still below 8.  (``o0 < 0`` can.)"""
    top = np.nextafter(np.float32(360), np.float32(0))
    assert np.float32(top * np.float32(8 / 360.0)) < np.float32(8)
    assert np.floor(np.float32(top * np.float32(8 / 360.0))) == 7


def test_blob24_radius_is_clamped_to_the_diagonal():
    ref = T.reference("blob24")[0]
    assert len(ref["pre"]["x"]) == 1 and len(ref["x"]) == 4
    o, layer, scale = S.unpack_octave(ref["octave"])
    assert np.all(o + 1 == 2)                              # one pyramid octave (index 2) holds all four
    for k in range(len(ref["x"])):
        h, w = ref["gauss"][int(o[k]) + 1][int(layer[k])].shape
        scl = ref["size"][k] * scale[k] * np.float32(0.5)
        assert np.rint(3 * scl * np.sqrt(2.0) * 2.5) > np.floor(np.sqrt(w * w + h * h))


def test_tie_cases_have_exact_ties_and_survivors():
    for name in ("stripes", "faint"):
        assert np.count_nonzero(T.reference(name)[0]["cand"]["neighbour_margin"] == 0) > 0, name
    assert _refined("checker") > 0 and _refined("faint") > 0
    # in ``faint`` some tied candidates survive refinement: without the ties the refined list is shorter
    ref = T.reference("faint")[0]
    c = ref["cand"]
    strict = c["neighbour_margin"] > 0
    p = S.Params(**T.params("faint"))
    n = sum(len(S.refine(ref["dog"], p, o, c["layer"][strict & (c["o"] == o)], c["r"][strict & (c["o"] == o)],
                         c["c"][strict & (c["o"] == o)])["x"]) for o in np.unique(c["o"][strict]))
    assert n < len(ref["pre"]["x"])


def test_tiny_cases_include_zero_octaves():
    assert [S.octave_count(*s) <= 0 for s in T.TINY_SHAPES] == [True, True, False, False, False]
    assert texture(4, 4, 7).shape == (4, 4)
