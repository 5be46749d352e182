"""The bundle adjustment's observation list built from the device-resident key tracks (csrc/sfm_track.hip:
sfm_obs_build; csrc/sfm_ba_host.hip: sfm_ba_create_from_tracks / sfm_ba_sync_tracks / sfm_ba_get_structure;
HipBaMixin.ba_device_tracks) against the host path that already exists (observations.build_observations + the gather
from the same normalised tables, sfm_ba_create, ObservationTracker).  The list is integers and copied coordinates: every
comparison of it is exact, u and v as bit patterns.  Solver states are held to the project's parity bound of 1e-9
relative (the resident BA is not bit-reproducible without SFM_OPT_DETERMINISTIC), a rebuild against a from-scratch solve
to 1e-12 as in test_gpu_linear_and_incremental.py.

1. quirk Q3 by hand;  2. sizes around a wave, a 1024-thread scan chunk and two chunks, n_pts below the largest id;
3. from_tracks / REUSE / GROWN / GROWN / REUSE / REPLACED on one problem;  4. the synced problem solves like a host-built
one;  5. the drop-in through a synthetic per-view loop, switch on and off;  6. the drop-in from pixels."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sift_chain as C  # noqa: E402

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def host_list(sfm, store, norm, n_views, n_pts):
    """(pt_ptr, cam_idx, key_idx, uv) of the host path on the rows the store holds and the same normalised tables."""
    rows = [store.row(v, v) for v in range(n_views)]
    pt_ptr, cam, _pt, key = sfm.observations.build_observations(rows, n_pts)
    uv = np.empty((2, cam.shape[0]))
    for c in range(n_views):
        sel = cam == c
        uv[:, sel] = norm[c][:, key[sel]]
    return pt_ptr, cam, key, uv


def assert_same_list(got, want, what):
    """(pt_ptr, cam_idx[, key_idx], uv): integers equal, u and v equal as bit patterns."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got[:-1], want[:-1])):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, i, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg="%s: integer array %d" % (what, i))
    assert got[-1].shape == want[-1].shape, (what, "uv")
    np.testing.assert_array_equal(bits(got[-1]), bits(want[-1]), err_msg="%s uv" % what)


def set_rows(store, rows):
    for v, row in enumerate(rows):
        store.update_usage(v, np.arange(row.shape[0]), row)


def make_store(sfm, hip, rng, n_views, n_keys):
    store = hip.TrackStore()
    xy = [rng.uniform(0, 1200, (n_keys, 2)).astype(np.float32).astype(np.float64) for _ in range(n_views)]
    norm = [sfm.geometry.normalise_pixels(a.T, sfm.scenes.UPENN_K) for a in xy]
    for v in range(n_views):
        assert store.add_view(xy[v]) == v
        store.set_normalised(v, norm[v])
    return store, xy, norm


# ---- 1 ----------------------------------------------------------------------------------------------------------
def test_q3_by_hand(sfm, hip):
    rng = np.random.default_rng(1)
    store, _xy, norm = make_store(sfm, hip, rng, 3, 8)
    with store:
        up = store.upload_bytes
        assert up == 3 * 8 * 16 * 2                                   # coordinates and normalised tables, 16 B per key each
        rows = [np.full(8, -1, dtype=np.int32) for _ in range(3)]
        rows[0][[0, 3, 6, 2]] = [0, 2, 2, 9]      # point 0 only at key 0: invisible; point 2 at keys 3 and 6: key 3; id 9 >= n_pts
        rows[1][[0, 5, 4]] = [1, 1, 3]            # point 1 at keys 0 and 5: visible THROUGH key 0
        rows[2][1] = 7                            # no usable entry in view 2; points 4 and 5 are seen by nobody
        set_rows(store, rows)
        down = store.download_bytes
        assert store.build_observations(3, 6) == 3
        assert store.download_bytes == down
        got = store.observations()
        assert got[0].tolist() == [0, 0, 1, 2, 3, 3, 3]
        assert got[1].tolist() == [1, 0, 1] and got[2].tolist() == [0, 3, 4]
        np.testing.assert_array_equal(bits(got[3]), bits(np.stack([norm[1][:, 0], norm[0][:, 3], norm[1][:, 4]], axis=1)))
        assert store.download_bytes - down == 4 * 7 + 3 * (4 + 4 + 16)
        assert_same_list(got, host_list(sfm, store, norm, 3, 6), "3 views, 6 points")
        # ids that were out of range become points: the prefix case the other way round
        assert store.build_observations(3, 10) == 5                    # 7 and 9 each have one key > 0; point 0 stays invisible
        got = store.observations()
        assert got[1].tolist() == [1, 0, 1, 2, 0] and got[2].tolist() == [0, 3, 4, 1, 2]
        assert_same_list(got, host_list(sfm, store, norm, 3, 10), "3 views, 10 points")
        # no point at all
        assert store.build_observations(3, 0) == 0
        got = store.observations()
        assert got[0].tolist() == [0] and got[1].size == 0 and got[2].size == 0 and got[3].shape == (2, 0)
        assert_same_list(got, host_list(sfm, store, norm, 3, 0), "no point")
        # one view
        assert store.build_observations(1, 6) == 1
        got = store.observations()
        assert got[0].tolist() == [0, 0, 0, 1, 1, 1, 1] and got[1].tolist() == [0] and got[2].tolist() == [3]
        assert_same_list(got, host_list(sfm, store, norm, 1, 6), "one view")
        with pytest.raises(ValueError):
            store.build_observations(4, 6)                             # more views than the store has
        with pytest.raises(ValueError):
            store.build_observations(3, -1)
        assert store.upload_bytes == up + 3 * 8 * 8                    # only the usage lists went up since


def test_build_needs_the_normalised_tables(sfm, hip):
    with hip.TrackStore() as store:
        store.add_view(np.zeros((4, 2)))
        with pytest.raises(ValueError, match="normalised"):
            store.build_observations(1, 3)
        with pytest.raises(ValueError):
            store.observations()                                       # no list yet
        with pytest.raises(ValueError):
            hip.BaProblem.from_tracks(store)
        with pytest.raises(ValueError):
            store.set_normalised(0, np.zeros((2, 5)))                  # 5 coordinates for 4 keys
        store.set_normalised(0, np.zeros((2, 4)))
        assert store.build_observations(1, 3) == 0
        # 2 x views x points ints of scratch: capped at 2^28
        with pytest.raises(ValueError, match="scratch"):
            store.build_observations(1, (1 << 27) + 1)


# ---- 2 ----------------------------------------------------------------------------------------------------------
N_PTS = (63, 64, 65, 1023, 1024, 1025, 2049)


@pytest.mark.parametrize("n_views", [2, 5])
@pytest.mark.parametrize("n_keys", [70, 1100])
def test_sizes_around_a_wave_and_a_scan_chunk(sfm, hip, n_keys, n_views):
    """Seeded self rows: ids drawn with repeats (a dense pool, so that min_key != max_key often) up to 2100, above every
    n_pts used -- each build is the prefix case of the incremental loop; a fifth unused.  Key 0 is one key per view: in
    the even views it shares its id with a later key (visible through key 0), in the odd ones its id is its own
    (invisible), and about 5 % of the other keys repeat key 0's id."""
    rng = np.random.default_rng(1000 * n_keys + n_views)
    store, _xy, norm = make_store(sfm, hip, rng, n_views, n_keys)
    with store:
        rows = []
        for v in range(n_views):
            row = np.where(rng.random(n_keys) < 0.5, rng.integers(0, max(n_keys // 3, 8), n_keys), rng.integers(0, 2100, n_keys))
            row[rng.random(n_keys) < 0.2] = -1
            if v % 2 == 0:
                row[0] = 40 + v
                row[1:][rng.random(n_keys - 1) < 0.05] = row[0]
            else:
                row[0] = 2000 + v
                row[1:][row[1:] == row[0]] = -1
            rows.append(row.astype(np.int32))
        rows[0][n_keys - 1] = 2099
        set_rows(store, rows)
        assert max(int(r.max()) for r in rows) >= max(N_PTS)
        seen = set()
        for n_pts in N_PTS:
            want = host_list(sfm, store, norm, n_views, n_pts)
            assert store.build_observations(n_views, n_pts) == want[1].shape[0]
            assert_same_list(store.observations(), want, "%d points" % n_pts)
            seen.add(want[1].shape[0])
            # key 0 really is exercised both ways
            for v in range(min(n_views, 2)):
                through0 = bool(np.any((want[1] == v) & (want[2] == 0)))
                assert through0 == (v % 2 == 0 and np.count_nonzero(rows[v] == rows[v][0]) > 1), (v, n_pts)
        assert len(seen) > 1
        # fewer views than the store has
        want = host_list(sfm, store, norm, n_views - 1, 1025)
        assert store.build_observations(n_views - 1, 1025) == want[1].shape[0]
        assert_same_list(store.observations(), want, "one view fewer")


# ---- 3, 4 -------------------------------------------------------------------------------------------------------
N_KEYS, N0, N1 = 40, 20, 25


class SyncCase:
    """Four views of a 25-point scene with full pixel data: key 0 is a dummy, key p + 1 the projection of point p, key
    26 + j the projection of point j moved by a fraction of a pixel (a second key for the point).  Which of them the
    views USE is decided by the tables."""

    def __init__(self, sfm, hip):
        self.sfm, self.hip = sfm, hip
        self.sc = sc = sfm.scenes.make_scene(4, N1, 1.0, seed=77, pixel_noise=0.3)
        self.xy, self.norm = [], []
        for v in range(4):
            pix = sc.uv_pix[:, sc.cam_idx == v].T                       # (25, 2), point order
            xy = np.vstack(([[-1.0, -1.0]], pix, pix[:N_KEYS - 26] + [0.5, -0.25])).astype(np.float32).astype(np.float64)
            self.xy.append(xy)
            self.norm.append(sfm.geometry.normalise_pixels(xy.T, sc.intrinsic))
        self.store = hip.TrackStore()
        for v in range(3):
            self.store.add_view(self.xy[v])
            self.store.set_normalised(v, self.norm[v])
            pts = np.array([p for p in range(N0) if (p + v) % 4 != 0])
            self.store.update_usage(v, pts + 1, pts)
        self.prob = None

    def close(self):
        if self.prob is not None:
            self.prob.close()
        self.store.close()

    def host(self, n_views, n_pts):
        return host_list(self.sfm, self.store, self.norm, n_views, n_pts)

    def host_problem(self, n_views, n_pts):
        pt_ptr, cam, _key, uv = self.host(n_views, n_pts)
        return self.hip.BaProblem(n_views, pt_ptr, cam, uv)

    def assert_structure(self, n_views, n_pts, what):
        pt_ptr, cam, _key, uv = self.host(n_views, n_pts)
        with self.hip.BaProblem(n_views, pt_ptr, cam, uv) as ref:
            want = ref.structure()
        assert_same_list(want, (pt_ptr, cam, uv), what + ": sfm_ba_get_structure of a host-built problem")
        assert_same_list(self.prob.structure(), want, what)
        assert (self.prob.info(self.hip.INFO_N_CAMS), self.prob.info(self.hip.INFO_N_PTS), self.prob.info(self.hip.INFO_N_OBS)) == (
            n_views, n_pts, cam.shape[0]), what
        assert (self.prob.n_cams, self.prob.n_pts, self.prob.n_obs) == (n_views, n_pts, cam.shape[0]), what

    def create(self):
        self.store.build_observations(3, N0)
        self.prob = self.hip.BaProblem.from_tracks(self.store)
        self.prob.set_state(self.sc.cams_init[:3], self.sc.pts_init[:, :N0])

    def grow(self):
        """A view, five points, new entries in old views' rows: for the new points and for an old point (a second key's
        pixel).  Returns (action, n_new_obs)."""
        st = self.store
        st.add_view(self.xy[3])
        st.set_normalised(3, self.norm[3])
        pts = np.array([p for p in range(N1) if p % 3 != 0])
        st.update_usage(3, pts + 1, pts)
        for v in range(3):
            st.update_usage(v, np.arange(N0, N1) + 1, np.arange(N0, N1))
        st.update_usage(0, [30], [4])                                   # point 4 was not seen by view 0 ((4 + 0) % 4 == 0)
        st.build_observations(4, N1)
        return self.prob.sync_tracks(st, self.sc.cams_init[3:4], self.sc.pts_init[:, N0:N1])


def test_sync_sequence_on_one_problem(sfm, hip):
    case = SyncCase(sfm, hip)
    try:
        st = case.store
        # from_tracks
        case.create()
        prob = case.prob
        assert prob.upload_bytes == 0 + 3 * 56 + N0 * 24                # the structure cost nothing; set_state is the caller's
        base = prob.upload_bytes
        case.assert_structure(3, N0, "from_tracks")
        # nothing changed
        st.build_observations(3, N0)
        assert prob.sync_tracks(st) == (hip.SYNC_REUSE, 0) and prob.upload_bytes == base
        # a view, points, entries in old rows
        m_old = prob.n_obs
        action, n_new = case.grow()
        assert action == hip.SYNC_GROWN
        assert n_new == case.host(4, N1)[1].shape[0] - m_old and n_new > 0
        assert prob.upload_bytes - base == 56 * 1 + 24 * (N1 - N0)
        case.assert_structure(4, N1, "grown")
        cams, pts = prob.get_state()                                    # old state kept, new state behind it
        np.testing.assert_array_equal(pts, case.sc.pts_init)
        np.testing.assert_array_equal(cams[:, 0:3], case.sc.cams_init[:, 0:3])
        base = prob.upload_bytes
        # only new entries for existing points in existing views
        st.update_usage(1, [29], [3])                                   # (3 + 1) % 4 == 0: view 1 did not see point 3
        st.update_usage(0, [27], [1])                                   # a SECOND key for a point view 0 sees at key 2: nothing new
        st.build_observations(4, N1)
        assert prob.sync_tracks(st) == (hip.SYNC_GROWN, 1) and prob.upload_bytes == base
        case.assert_structure(4, N1, "grown again")
        st.build_observations(4, N1)
        assert prob.sync_tracks(st) == (hip.SYNC_REUSE, 0) and prob.upload_bytes == base
        # fewer points or views than the problem holds
        st.build_observations(4, N1 - 1)
        assert prob.sync_tracks(st)[0] == hip.SYNC_REPLACED
        st.build_observations(3, N1)
        assert prob.sync_tracks(st)[0] == hip.SYNC_REPLACED

        want = prob.structure()
        state = prob.get_state()

        def assert_replaced_and_untouched(what, **kw):
            assert prob.sync_tracks(st, **kw) == (hip.SYNC_REPLACED, 0), what
            assert_same_list(prob.structure(), want, what)
            assert prob.info(hip.INFO_N_OBS) == want[1].shape[0] and prob.upload_bytes == base, what
            for g, w in zip(prob.get_state(), state):
                np.testing.assert_array_equal(g, w, err_msg=what)

        def assert_back():
            st.build_observations(4, N1)
            assert prob.sync_tracks(st) == (hip.SYNC_REUSE, 0)

        # an entry that gave an observation goes away: (5 + 2) % 4 != 0, view 2 sees point 5 at key 6
        st.update_usage(2, [6], [-1])
        assert st.build_observations(4, N1) == want[1].shape[0] - 1
        assert_replaced_and_untouched("an observation removed")
        # ... and comes back at another key, with another pixel
        st.update_usage(2, [31], [5])
        assert st.build_observations(4, N1) == want[1].shape[0]
        assert_replaced_and_untouched("an observation moved to another key")
        st.update_usage(2, [6, 31], [5, -1])
        assert_back()
        # another intrinsic matrix for one view: the same keys, other coordinates
        k2 = case.sc.intrinsic.copy()
        k2[0, 0] *= 1.01
        st.set_normalised(1, sfm.geometry.normalise_pixels(case.xy[1].T, k2))
        assert st.build_observations(4, N1) == want[1].shape[0]
        assert_replaced_and_untouched("a view's normalised table replaced")
        st.set_normalised(1, case.norm[1])
        assert_back()
        # counts that do not match the list
        assert_replaced_and_untouched("a camera too many", cams_new=case.sc.cams_init[3:4])
        assert_replaced_and_untouched("a point too many", pts_new=case.sc.pts_init[:, :1])
        assert_back()
    finally:
        case.close()


def test_synced_problem_solves_like_a_host_built_one(sfm, hip, capsys):
    case = SyncCase(sfm, hip)
    try:
        case.create()
        case.prob.iterate(5.0, 1)                                       # the resident state has moved before the scene grows
        assert case.grow()[0] == hip.SYNC_GROWN
        sc = case.sc
        with case.host_problem(4, N1) as ref:
            results = []
            for prob in (case.prob, ref):
                prob.set_cameras(sc.cams_init)
                prob.set_points(0, sc.pts_init)
                prob.iterate(5.0, 3)
                results.append(prob.get_state())
        d_cams, d_pts = rel(results[0][0], results[1][0]), rel(results[0][1], results[1][1])
        with capsys.disabled():
            print("\nsynced against host-built problem after 3 iterations: cameras %.3e, points %.3e (relative)" % (d_cams, d_pts))
        assert np.all(np.isfinite(results[0][0])) and rel(results[0][0], sc.cams_init) > 1e-6      # the solver moved
        assert d_cams < 1e-9 and d_pts < 1e-9
    finally:
        case.close()


def test_synced_handle_keeps_its_identity(sfm, hip):
    """One SYNC_GROWN step behind a handle with options set: it keeps its stream, its linearise timer goes on counting, and
    with the fixed summation order it ends on the bits of a host-built problem of the grown scene with the same options."""
    import torch

    def options(prob, stream):
        prob.set_option(hip.OPT_SCHUR, hip.SCHUR_MFMA)
        prob.set_option(hip.OPT_DETERMINISTIC, 1)
        prob.set_option(hip.OPT_TIMING, 1 << hip.K_LINEARIZE)
        prob.set_stream(stream.cuda_stream)

    case = SyncCase(sfm, hip)
    try:
        stream = torch.cuda.Stream()
        case.create()
        prob = case.prob
        options(prob, stream)
        prob.iterate(5.0, 2)
        assert case.grow()[0] == hip.SYNC_GROWN
        assert prob.info(hip.INFO_REDUCE_IN_SOLVE) == 0
        assert prob.stream_ptr() == stream.cuda_stream
        cams_b, pts_b = prob.get_state()
        launches = prob.kernel_time(hip.K_LINEARIZE)[1]
        assert launches > 0
        prob.iterate(5.0, 2)
        assert prob.kernel_time(hip.K_LINEARIZE)[1] > launches
        cams_c, pts_c = prob.get_state()
        with case.host_problem(4, N1) as fresh:
            options(fresh, stream)
            fresh.set_state(cams_b, pts_b)
            fresh.iterate(5.0, 2)
            cams_f, pts_f = fresh.get_state()
        np.testing.assert_array_equal(bits(cams_c), bits(cams_f))
        np.testing.assert_array_equal(bits(pts_c), bits(pts_f))
        assert not np.array_equal(cams_c, cams_b)
    finally:
        case.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------
class LoopView:
    def __init__(self, rot, loc, k, xy, key_pts, descriptors):
        self.rot, self.loc, self.k = rot, loc, k
        self.key_xy, self.key_pts, self.key_descriptors = xy, key_pts, descriptors

    def update_cam_pose(self, rot, loc):
        self.rot, self.loc = rot, loc


class Holder:
    pass


class Loop:
    """One processor fed view by view as in test_gpu_linear_and_incremental.py's loop, through HipDeviceKeyTracker: key 0
    is a dummy, key p + 1 observes point p, SPARE more keys at the end repeat the first points' pixels; every view so far
    observes every point known so far.  The descriptors are
    random (whatever the matcher writes goes into the rows BETWEEN views, which the bundle adjustment does not read)."""
    PER_VIEW = 75
    SPARE = 5

    def __init__(self, sfm, sc, device_tracks):
        P = sfm.processors
        self.sfm, self.sc = sfm, sc
        self.vp, self.tp = Holder(), Holder()
        self.vp.view_list, self.tp.tri_pts = [], np.zeros((4, 0))
        self.kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
        self.bp = P.HipBaProcessor(self.vp, self.kt, None, self.tp, None, iteration=3, damping_factor=5)
        self.bp.ba_verbose = False
        self.bp.ba_device_tracks = device_tracks
        self.rng = np.random.default_rng(5)

    def close(self):
        self.bp.ba_release()
        self.kt.kt_release()

    def add_view(self, c):
        sc, g = self.sc, self.sfm.geometry
        pix = sc.uv_pix[:, sc.cam_idx == c].T
        xy = np.vstack(([[-1.0, -1.0]], pix, pix[:self.SPARE])).astype(np.float32).astype(np.float64)
        rot = g.quaternion_to_rotation(sc.cams_init[c, 3:7] / np.linalg.norm(sc.cams_init[c, 3:7]))
        view = LoopView(rot, sc.cams_init[c, 0:3].reshape(3, 1).copy(), sc.intrinsic.copy(), xy,
                        [self.sfm.scenes.KeyPoint(x, y) for x, y in xy],
                        self.rng.integers(0, 256, (xy.shape[0], 128)).astype(np.uint8))
        self.kt.add_new_view(view, self.vp.view_list)
        self.vp.view_list.append(view)

    def register(self, c):
        """View c arrives with PER_VIEW new points; returns the new point count."""
        self.add_view(c)
        n_old = self.tp.tri_pts.shape[1]
        new = np.arange(n_old, n_old + self.PER_VIEW)
        self.tp.tri_pts = np.hstack((self.tp.tri_pts, np.vstack((self.sc.pts_init[:, new], np.ones((1, new.size))))))
        for v in range(c):
            self.kt.track_list[v].update_usage((new + 1)[np.newaxis, :], new[np.newaxis, :])
        every = np.arange(0, n_old + self.PER_VIEW)
        self.kt.track_list[c].update_usage((every + 1)[np.newaxis, :], every[np.newaxis, :])
        return new.size

    def ba(self):
        """(action, upload delta, download delta of the tracker during the call)."""
        up, down = self.bp.ba_upload_bytes, self.kt.kt_download_bytes
        self.bp._BaProcessor__execute_bundle_adjustment()
        return self.bp.ba_last_action, self.bp.ba_upload_bytes - up, self.kt.kt_download_bytes - down

    def state(self):
        return (np.stack([self.sfm.geometry.pack_camera(v.rot, v.loc) for v in self.vp.view_list]), self.tp.tri_pts[0:3].copy())

    def set_state(self, cams_views, pts):
        for v, (rot, loc) in zip(self.vp.view_list, cams_views):
            v.update_cam_pose(rot.copy(), loc.copy())
        self.tp.tri_pts[:] = pts


def test_dropin_per_view_loop_switch_on_and_off(sfm, hip, capsys):
    sc = sfm.scenes.make_scene(5, 300, 1.0, seed=52, pixel_noise=0.3)
    on, off = Loop(sfm, sc, True), Loop(sfm, sc, False)
    try:
        for run in (on, off):
            run.add_view(0)
        worst = 0.0
        for c in range(1, 5):
            n_new = [run.register(c) for run in (on, off)]
            assert n_new == [Loop.PER_VIEW] * 2
            (a_on, up_on, down_on), (a_off, up_off, _down_off) = on.ba(), off.ba()
            assert a_on == a_off == ("create" if c == 1 else "append"), (c, a_on, a_off)
            assert down_on == 0, c                                      # no table comes down
            if c > 1:
                n_obs_new = (c + 1) * (c * Loop.PER_VIEW) - c * ((c - 1) * Loop.PER_VIEW)
                assert up_on == 56 + 24 * n_new[0], c
                assert up_off == 56 + 24 * n_new[1] + 24 * n_obs_new, c
            d = [rel(a, b) for a, b in zip(on.state(), off.state())]
            worst = max(worst, *d)
            assert d[0] < 1e-9 and d[1] < 1e-9, (c, d)
        with capsys.disabled():
            print("\nper-view loop, switch on against off: largest relative difference of poses / points %.3e" % worst)
        assert on.kt._store.info(hip.TRACK_INFO_N_OBS) == 5 * 300
        # nothing new: the resident structure is used again, nothing goes up
        assert on.ba() == ("reuse", 0, 0)
        action, up, _down = off.ba()
        assert action == "reuse" and up == 0
        d = [rel(a, b) for a, b in zip(on.state(), off.state())]
        assert d[0] < 1e-9 and d[1] < 1e-9, d
        # an entry removed: both rebuild, and from the same host state they agree as a rebuild agrees with a from-scratch solve
        snap_views = [(v.rot.copy(), v.loc.copy()) for v in off.vp.view_list]
        snap_pts = off.tp.tri_pts.copy()
        on.set_state(snap_views, snap_pts)
        results = []
        for run in (on, off):
            run.kt.track_list[2].update_usage(np.array([[6]]), np.array([[-1]]))
            action, _up, down = run.ba()
            assert action == "create"
            if run is on:
                assert down == 0
            results.append(run.state())
        assert rel(results[0][0], results[1][0]) < 1e-12 and rel(results[0][1], results[1][1]) < 1e-12
        assert on.bp._hip_scene.prob.n_obs == off.bp._hip_scene.prob.n_obs == 5 * 300 - 1
        # ... and with a from-scratch solve on the host path
        off.set_state(snap_views, snap_pts)
        off.bp.ba_resident = False
        assert off.ba()[0] == "solve"
        ref = off.state()
        assert rel(results[0][0], ref[0]) < 1e-12 and rel(results[0][1], ref[1]) < 1e-12
    finally:
        on.close()
        off.close()


def test_dropin_device_compares_lists_where_the_host_diff_rebuilds(sfm, hip):
    """A second, later key for a point a view already observes leaves the list as it is: "reuse" with the switch on,
    "create" on the host path (ObservationTracker.diff is conservative) -- and the same structure either way."""
    sc = sfm.scenes.make_scene(3, 150, 1.0, seed=53, pixel_noise=0.3)
    on, off = Loop(sfm, sc, True), Loop(sfm, sc, False)
    try:
        for run in (on, off):
            run.add_view(0)
            for c in (1, 2):
                run.register(c)
            assert run.ba()[0] == "create"
            run.kt.track_list[1].update_usage(np.array([[152]]), np.array([[1]]))      # point 1 sits at key 2 already
        assert on.ba() == ("reuse", 0, 0)
        assert off.ba()[0] == "create"
        assert_same_list(on.bp._hip_scene.prob.structure(), off.bp._hip_scene.prob.structure(), "second key")
        # a host-side replacement of a table is not seen with the switch on
        picture = on.kt.track_list[0].table
        t = picture.copy()
        t[0, :] = -1
        on.kt.track_list[0].table = t
        assert on.ba() == ("reuse", 0, 0)
        on.kt.track_list[0].table = picture
        # another intrinsic matrix: the normalised table of that view goes up again and the problem is rebuilt
        for run in (on, off):
            k = run.vp.view_list[1].k.copy()
            k[0, 0] *= 1.001
            run.vp.view_list[1].k = k
        up = on.kt.kt_upload_bytes
        assert on.ba()[0] == "create" and off.ba()[0] == "create"
        assert on.kt.kt_upload_bytes - up == 16 * (1 + 150 + Loop.SPARE)
        assert_same_list(on.bp._hip_scene.prob.structure(), off.bp._hip_scene.prob.structure(), "new intrinsic matrix")
        # switching off afterwards rebuilds from the host tables instead of diffing against a picture that was not kept
        on.bp.ba_device_tracks = False
        assert on.ba()[0] == "create"
        assert_same_list(on.bp._hip_scene.prob.structure(), off.bp._hip_scene.prob.structure(), "switched off")
    finally:
        on.close()
        off.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------
def run_from_pixels(sfm, imgs, k, device_tracks, capsys):
    from test_gpu_process import recording_classes
    P = sfm.processors
    log = {}
    Ba, Epi, Cam = recording_classes(P, log)
    random.seed(99)
    cfg_kt = P.RansacConfig(1e-2, 0.99, 0.75, 8, 200)
    cfg_ep = P.RansacConfig(1e-2, 0.99, 0.75, 8, 300)
    cfg_cp = P.RansacConfig(8.0, 0.99, 0.75, 8, 300)
    vp = P.HipViewProcessor('sift')
    kt = P.HipDeviceKeyTracker('sift', False, True, False, cfg_kt)
    bp = Ba(vp, kt, Epi(cfg_ep), P.HipTriangulationProcessor(), Cam(cfg_cp, 5, 300))
    bp.ba_verbose = False
    bp.ba_device_tracks = device_tracks
    capsys.readouterr()
    try:
        for img in imgs:
            assert bp.process(img, k) is None
        capsys.readouterr()
        log["action"] = bp.ba_last_action
        log["tables"] = [np.array(t.table, copy=True) for t in kt.track_list]
        log["n_points"] = bp.tri_processor.tri_pts.shape[1]
        log["cams_after_ba"] = np.stack([sfm.geometry.pack_camera(v.rot, v.loc) for v in vp.view_list])
        log["structure"] = bp._hip_scene.prob.structure()
    finally:
        bp.ba_release()
        kt.kt_release()
    return log


def test_dropin_from_pixels_switch_on_and_off(sfm, hip, capsys):
    imgs, k = [C.fixture(n)["image"] for n in (1, 2, 3)], C.halved_k()
    on, off = run_from_pixels(sfm, imgs, k, True, capsys), run_from_pixels(sfm, imgs, k, False, capsys)
    assert on["action"] == off["action"] == "create"
    assert len(on["tables"]) == 3
    for v in range(3):
        np.testing.assert_array_equal(on["tables"][v], off["tables"][v], err_msg="table %d" % v)
    assert on["fund_inliers"] == off["fund_inliers"] and on["pnp_inlier_list"] == off["pnp_inlier_list"]
    assert on["pnp_points"] == off["pnp_points"] and on["n_points"] == off["n_points"]
    for key in ("rots_before_ba", "locs_before_ba", "pts_before_ba"):
        np.testing.assert_array_equal(np.array(on[key]), np.array(off[key]), err_msg=key)
    assert on["rmse_before_ba"] == off["rmse_before_ba"]
    assert_same_list(on["structure"], off["structure"], "structure from pixels")
    for run in (on, off):
        assert np.isfinite(run["rmse_after_ba"]) and run["rmse_after_ba"] <= 1.01 * run["rmse_before_ba"]
    d = rel(on["cams_after_ba"], off["cams_after_ba"])
    with capsys.disabled():
        print("\nfrom pixels, switch on against off: rmse %.4f -> %.4f / %.4f px, poses differ by %.3e (relative)"
              % (on["rmse_before_ba"], on["rmse_after_ba"], off["rmse_after_ba"], d))
    assert d < 1e-9
