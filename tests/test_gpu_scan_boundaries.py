"""The one-workgroup exclusive scan (csrc/sfm_scan.h: block_exclusive_scan) driven across its chunk border through every
public path that reaches it: the observation build (obs_scan_kernel), sfm_ba_append (ba_append_scan_kernel, the
two-sequence instance), sfm_ba_cull (ba_cull_scan_kernel) and sfm_pnp_ransac_finish (pnp_mask_scan_kernel).

Sizes: 1, 63, 64, 65 are the edges of a wave, 1023 and 1024 those of the 1024-element chunk, 1025 is the first carry with
a one-element tail, 2049 two carries.  The scan is integer arithmetic: every comparison is exact, against values computed
with NumPy.  Six or seven cameras and tracks of one to four observations keep every case well under a second.

The scene's camera-major list (ba_cam_list_ptr_scan_kernel) scans per camera; its single-chunk path is covered by the
"rows"-mode and refine_cameras tests, its multi-chunk path is the shared body exercised here."""
import ctypes

import numpy as np
import pytest

import _screen_reference as sr
from test_gpu_append import _subset
from test_gpu_track_observations import assert_same_list, bits, host_list, make_store, set_rows

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
CHUNK = 1024


def ragged_tracks(rng, n_cams, n_pts):
    """(counts (n_pts,), pt_ptr, cam_idx, pt_idx): every point seen by one to four cameras, sorted by (point, camera)."""
    counts = rng.integers(1, 5, n_pts)
    cams = [np.sort(rng.choice(n_cams, k, replace=False)) for k in counts]
    cam_idx = np.concatenate(cams).astype(np.int32) if n_pts else np.zeros(0, dtype=np.int32)
    pt_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return counts, pt_ptr, cam_idx, np.repeat(np.arange(n_pts), counts).astype(np.int32)


# ---- observation build ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_observation_build(sfm, hip, n):
    """Point p is key 1 + perm_v[p] of every view of its track (key 0 is never used: a point is visible through a key
    above 0 only) and nothing else is in the tables, so the list is known in closed form."""
    n_views = 6
    rng = np.random.default_rng(7000 + n)
    counts, pt_ptr, cam_idx, pt_idx = ragged_tracks(rng, n_views, n)
    store, _xy, norm = make_store(sfm, hip, rng, n_views, n + 1)
    with store:
        perms = [rng.permutation(n) for _ in range(n_views)]
        rows = [np.full(n + 1, -1, dtype=np.int32) for _ in range(n_views)]
        for v in range(n_views):
            seen = pt_idx[cam_idx == v]
            rows[v][1 + perms[v][seen]] = seen
        set_rows(store, rows)
        key_idx = np.array([1 + perms[v][p] for v, p in zip(cam_idx, pt_idx)], dtype=np.int32)
        uv = np.stack([norm[v][:, k] for v, k in zip(cam_idx, key_idx)], axis=1)
        assert store.build_observations(n_views, n) == int(counts.sum())
        got = store.observations()
        np.testing.assert_array_equal(got[0], np.concatenate(([0], np.cumsum(counts))))
        assert_same_list(got, (pt_ptr, cam_idx, key_idx, uv), "%d points" % n)
        assert_same_list(got, host_list(sfm, store, norm, n_views, n), "%d points, host path" % n)


# ---- append: two sequences in one pass --------------------------------------------------------------------------------
APPEND_CASES = [(n, "mixed") for n in SIZES] + [(2049, "no_new_below_border"), (2049, "no_new_above_border")]


@pytest.mark.parametrize("n,variant", APPEND_CASES)
def test_append_two_sequences(sfm, hip, n, variant):
    """A resident problem of six cameras and N = n - 7 points (none for n < 7) grows to seven cameras and n points; the
    new observations are those of the new points and those of camera 6 on old points.  The first scanned sequence is the
    merged track length, the second the number of new observations per point.  In the two variants the second sequence
    is all zeros on one side of index 1024 while the first is not: a carry that mixed the sequences would move every
    offset beyond the border."""
    rng = np.random.default_rng(8000 + n + len(variant))
    v0, v1, n0 = 6, 7, max(n - 7, 0)
    counts, pt_ptr, cam_idx, pt_idx = ragged_tracks(rng, v1, n)
    uv = rng.uniform(-0.5, 0.5, (2, cam_idx.shape[0]))
    if variant != "mixed":
        # camera 6 leaves the old points of one side; in "above" the seven new points come without observations
        side = pt_idx < CHUNK if variant == "no_new_below_border" else pt_idx >= CHUNK
        stay = ~(side & ((cam_idx == 6) | (pt_idx >= n0)))
        cam_idx, pt_idx, uv = cam_idx[stay], pt_idx[stay], uv[:, stay]
        counts = np.bincount(pt_idx, minlength=n)
        pt_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    sc = SimpleScene(cam_idx, pt_idx)
    keep, ptr0 = _subset(sc, v0, n0)
    new = rng.permutation(np.flatnonzero(~keep))
    n_new = np.bincount(pt_idx[new], minlength=n)                      # the second sequence
    if n > CHUNK + 1:
        low, high = n_new[:CHUNK].any(), n_new[CHUNK:].any()
        assert (low, high) == {"mixed": (True, True), "no_new_below_border": (False, True), "no_new_above_border": (True, False)}[variant]
        assert counts[:CHUNK].any() and counts[CHUNK:].any()                # the first sequence is on both sides
    cams = sfm.scenes.make_scene(v1, 8, 1.0, seed=3).cams_init
    pts = rng.uniform(-1.0, 1.0, (3, n))
    with hip.BaProblem(v0, ptr0, cam_idx[keep], uv[:, keep]) as prob:
        prob.set_state(cams[:v0], pts[:, :n0])
        prob.append(cams[v0:], pts[:, n0:], cam_idx[new], pt_idx[new], uv[:, new])
        assert (prob.info(hip.INFO_N_CAMS), prob.info(hip.INFO_N_PTS), prob.info(hip.INFO_N_OBS)) == (v1, n, cam_idx.shape[0])
        got = prob.structure()
        np.testing.assert_array_equal(got[0], np.concatenate(([0], np.cumsum(counts))))
        assert_same_list(got, (pt_ptr, cam_idx, uv), "%d points, %s" % (n, variant))


class SimpleScene:
    """The two fields test_gpu_append._subset reads."""

    def __init__(self, cam_idx, pt_idx):
        self.cam_idx, self.pt_idx = cam_idx, pt_idx


# ---- cull ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_cull(sfm, hip, n):
    """Seven cameras, n points with one to four observations each, at the true state.  A planted set of observations is
    moved by 100 px and the error threshold sits in the gap below them (threshold_in_gap), min_obs = 2: the planted
    observations drop, and with them every point left with fewer than two.  Planted by hand: the first observation of
    point 0, every observation of point 1023 (the last element of the first chunk gives its offset on unchanged and keeps
    nothing) and one of point 1024."""
    rng = np.random.default_rng(9000 + n)
    full = sfm.scenes.make_scene(7, n, 1.0, seed=90 + n % 11)
    counts, pt_ptr, cam_idx, pt_idx = ragged_tracks(rng, 7, n)
    if n == 1:
        counts, pt_ptr, cam_idx, pt_idx = np.array([4]), np.array([0, 4], dtype=np.int32), np.arange(4, dtype=np.int32), np.zeros(4, dtype=np.int32)
    m = cam_idx.shape[0]
    uv_pix = full.uv_pix[:, full.pt_ptr[pt_idx] + cam_idx].copy()     # full visibility: observation (p, c) is at pt_ptr[p] + c
    planted = rng.random(m) < 0.05
    planted[0] = True
    if n > CHUNK - 1:
        planted[pt_ptr[CHUNK - 1]:pt_ptr[CHUNK]] = True
    if n > CHUNK:
        planted[pt_ptr[CHUNK]] = True
    angle = rng.uniform(0.0, 2.0 * np.pi, m)
    uv_pix[:, planted] += 100.0 * np.vstack((np.cos(angle), np.sin(angle)))[:, planted]
    uvn = sfm.geometry.normalise_pixels(uv_pix, full.intrinsic)
    cams, pts = full.cams_true, full.pts_true
    base = sr.screen_reference(pt_ptr, cam_idx, uvn, cams, pts)
    t = sr.threshold_in_gap(base.err2, (m - int(planted.sum())) / max(m - 1, 1))
    want = sr.screen_reference(pt_ptr, cam_idx, uvn, cams, pts, t, 1.0, 2)
    assert np.array_equal((want.obs_flags & sr.OBS_HIGH_ERROR) != 0, planted)
    survivors = np.bincount(pt_idx[~planted], minlength=n)
    assert np.array_equal(want.keep, np.where(survivors >= 2, survivors, 0))
    if n > CHUNK:
        assert want.keep[CHUNK - 1] == 0 and (want.keep[:CHUNK] < counts[:CHUNK]).any() and (want.keep[CHUNK:] < counts[CHUNK:]).any()
    new_ptr, new_cam, new_uv = sr.compact(pt_ptr, cam_idx, uvn, want.obs_flags)
    np.testing.assert_array_equal(new_ptr, np.concatenate(([0], np.cumsum(want.keep))))
    with hip.BaProblem(7, pt_ptr, cam_idx, uvn) as prob:
        prob.set_state(cams, pts)
        got = prob.cull(t, 1.0, 2)
        assert np.array_equal(got.obs_flags, want.obs_flags) and np.array_equal(got.pt_flags, want.pt_flags)
        assert got.summary.tolist() == want.summary.tolist()
        assert got.summary[0] == m and got.summary[1] == int(want.keep.sum()) == prob.info(hip.INFO_N_OBS)
        assert_same_list(prob.structure(), (new_ptr, new_cam, new_uv), "%d points" % n)


# ---- PnP compaction -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [s for s in SIZES if s >= 6])
def test_pnp_compaction(sfm, hip, n):
    """A view of n points (six is the least the entry point accepts, so size 1 has no case here) at its true pose: a fifth
    of the keys are moved by 30 to 150 px per coordinate, the others carry 0.4 px of noise, the threshold is 8 px.  Keys
    1023 and 1024 are inliers, key 1025 is an outlier.  The mask and its count are exact; the refined pose is that of
    sfm_pnp_nonlinear on the columns the host compacts, bit for bit (as test_gpu_linear_and_incremental.py holds it)."""
    rng = np.random.default_rng(6000 + n)
    sc = sfm.scenes.make_scene(2, n, 1.0, seed=60 + n % 13, pixel_noise=0.4)
    K = sc.intrinsic
    uv = np.vstack((sc.uv_pix[:, sc.cam_idx == 1], np.ones((1, n))))
    bad = rng.random(n) < 0.2
    bad[:6] = False                                                    # the one sample below
    bad[[i for i in (CHUNK - 1, CHUNK) if i < n]] = False
    if n > CHUNK + 1:
        bad[CHUNK + 1] = True
    uv[0:2, bad] += rng.uniform(30, 150, (2, int(bad.sum()))) * rng.choice([-1, 1], (2, int(bad.sum())))
    x = np.vstack((sc.pts_true, np.ones((1, n))))
    rot = sfm.geometry.quaternion_to_rotation(sc.cams_true[1, 3:7])
    loc = sc.cams_true[1, 0:3]
    want_idx = np.flatnonzero(~bad)
    samples = np.arange(6, dtype=np.int32).reshape(1, 6)
    r_sep, c_sep = hip.pnp_nonlinear(uv[:, want_idx], x[:, want_idx], K, rot, loc, 5.0, 10)
    (handle, _n), *_ = hip.pnp_ransac_begin(uv, x, K, samples, 8.0)
    # sfm_pnp_ransac_finish itself, for the count the Python wrapper does not return
    mask = np.full(n, -1, dtype=np.int32)
    count = ctypes.c_int(-1)
    r_ses, c_ses = np.empty((3, 3)), np.empty(3)
    as_d = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))            # noqa: E731
    rot_c, loc_c = np.ascontiguousarray(rot, dtype=np.float64), np.ascontiguousarray(loc, dtype=np.float64)
    hip.check(hip.load().sfm_pnp_ransac_finish(handle, as_d(rot_c), as_d(loc_c), 8.0, 5.0, 10, hip.QUIRKS_REFERENCE,
                                                mask.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(count),
                                                as_d(r_ses), as_d(c_ses)))
    assert count.value == want_idx.shape[0]
    np.testing.assert_array_equal(mask, (~bad).astype(np.int32))
    assert np.array_equal(bits(r_ses), bits(r_sep)) and np.array_equal(bits(c_ses), bits(c_sep.reshape(3)))
