"""The KeyTracker drop-in on the device reproduces the reference's tables (tests/golden/g12_keytracker_*.npz), Python's
RNG stream in the fundamental-inlier case, uploads a view's descriptors once, and feeds the BA drop-in."""
import hashlib
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("sift_knn", "sift_knn_fund", "sift_cross", "sift_match", "orb_knn")


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def views_of(sfm, g):
    nv = int(g["n_views"])
    return [View([sfm.scenes.KeyPoint(x, y) for x, y in g["pix_%d" % v]], g["desc_%d" % v]) for v in range(nv)]


def ransac_of(sfm, g):
    r = g["ransac"]
    return sfm.processors.RansacConfig(float(r[0]), float(r[1]), float(r[2]), int(r[3]), int(r[4]))


def run(kt, views, knn, fund, cfg):
    for v in range(len(views)):
        kt.add_new_view(views[v], views[:v], knn, fund, cfg)


class _StandInBase:
    """What the mixin needs of key_tracker.KeyTracker: its constructor state and add_new_view (key_tracker.py:71-126)."""

    def __init__(self, key_type, is_cross_check, is_knn_match, is_fund_inlier, ransac_config):
        self.key_type, self.is_cross_check = key_type, is_cross_check
        self.is_knn_match, self.is_fund_inlier, self.ransac_config = is_knn_match, is_fund_inlier, ransac_config
        self.track_list = []

    def add_new_view(self, new_view, views, is_knn_match=None, is_fund_inlier=None, ransac_config=None):
        if len(self.track_list) == 0:
            self.track_list.append(_Track(1, len(new_view.key_pts), 0))
        else:
            self._KeyTracker__extend_list(new_view, views, is_knn_match or self.is_knn_match,
                                          is_fund_inlier or self.is_fund_inlier, ransac_config or self.ransac_config)

    def _KeyTracker__extend_list(self, *a):
        raise AssertionError("the reference body ran")


class _Track:
    def __init__(self, rows, cols, idx):
        self.table = np.full((rows, cols), -1, dtype=int)
        self.idx, self.key_num = idx, cols

    def expand_table(self):
        self.table = np.append(self.table, np.full((1, self.key_num), -1, dtype=int), 0)


@pytest.mark.parametrize("standalone", (True, False))
@pytest.mark.parametrize("case", CASES)
def test_keytracker_reproduces_reference(hip, sfm, case, standalone):
    g = np.load(os.path.join(GOLDEN, "g12_keytracker_%s.npz" % case))
    cross, knn, fund = (bool(x) for x in g["flags"])
    views = views_of(sfm, g)
    cfg = ransac_of(sfm, g)                     # seeds Python's RNG with -1, as the reference's RansacConfig
    if standalone:
        kt = sfm.processors.HipKeyTracker(str(g["key_type"]), cross, knn, fund, cfg)
    else:
        cls = type("KeyTracker", (sfm.processors.HipKeyTrackerMixin, _StandInBase), {})
        kt = cls(str(g["key_type"]), cross, knn, fund, cfg)
    try:
        run(kt, views, knn, fund, cfg)
    finally:
        kt.kt_release()
    for v in range(len(views)):
        np.testing.assert_array_equal(kt.track_list[v].table, g["table_%d" % v], err_msg="%s view %d" % (case, v))
    if fund:
        assert hashlib.sha256(repr(random.getstate()).encode()).hexdigest() == str(g["rng_digest"])


def test_second_view_uploads_only_itself(hip, sfm):
    g = np.load(os.path.join(GOLDEN, "g12_keytracker_sift_knn.npz"))
    views = views_of(sfm, g)
    kt = sfm.processors.HipKeyTracker("sift", False, True, False, None)
    sizes = [v.key_descriptors.nbytes for v in views]
    kt.add_new_view(views[0], [], True)
    kt.add_new_view(views[1], views[:1], True)
    assert kt.kt_upload_bytes == sizes[0] + sizes[1]
    kt.add_new_view(views[2], views[:2], True)
    assert kt.kt_upload_bytes == sizes[0] + sizes[1] + sizes[2]
    views[0].key_descriptors = views[0].key_descriptors.copy()          # another object: uploaded again
    kt.add_new_view(views[3], views[:3], True)
    assert kt.kt_upload_bytes == sum(sizes[:4]) + sizes[0]
    kt.kt_release()


def test_new_view_without_keys(hip, sfm):
    g = np.load(os.path.join(GOLDEN, "g12_keytracker_sift_knn.npz"))
    views = views_of(sfm, g)[:2] + [View([], np.zeros((0, 128), dtype=np.uint8))]
    kt = sfm.processors.HipKeyTracker("sift", False, True, False, None)
    run(kt, views, True, False, None)
    assert kt.track_list[2].table.shape == (3, 0)
    assert (kt.track_list[0].table[2] == -1).all()
    kt.kt_release()


def test_ba_runs_on_hip_keytracker_tables(hip, sfm, capsys):
    dv = sfm.scenes.make_descriptor_views(n_views=4, n_pts=150, seed=21, n_distract=10, n_dup=0)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(4)]
    kt = sfm.processors.HipKeyTracker("sift", False, True, False, None)
    run(kt, views, True, False, None)
    kt.kt_release()
    # points observed by views 0 and 1 through the tracker's matches; their indices go into the self rows
    row = kt.track_list[0].table[1]
    k0 = np.flatnonzero(row > 0)
    k1 = row[k0]
    pid = dv.point[0][k0]
    good = (pid >= 0) & (pid == dv.point[1][k1])
    k0, k1, pid = k0[good], k1[good], pid[good]
    assert k0.shape[0] > 30
    n = k0.shape[0]
    kt.track_list[0].table[0, k0] = np.arange(n)
    kt.track_list[1].table[1, k1] = np.arange(n)
    rng = np.random.default_rng(1)
    from scipy.spatial.transform import Rotation
    pts = np.vstack((np.zeros((3, n)), np.ones((1, n))))
    true = dv.pts
    pts[0:3] = true[:, pid] + rng.normal(0, 0.02, (3, n))

    class PV:
        def __init__(self, rot, loc, keys):
            self.rot, self.loc, self.k, self.key_pts = rot, loc.reshape(3, 1), dv.intrinsic, keys

        def update_cam_pose(self, rot, loc):
            self.rot, self.loc = rot, loc
    pviews = [PV(dv.rots[v] @ Rotation.from_rotvec(rng.normal(0, 0.002, 3)).as_matrix(), dv.locs[v], views[v].key_pts)
              for v in range(2)]

    class VP:
        view_list = pviews

    class TP:
        tri_pts = pts
    kt.track_list = kt.track_list[:2]
    for t in kt.track_list:
        t.table = t.table[:2]
    ba = sfm.processors.HipBaProcessor(VP, kt, None, TP, None, iteration=3)
    before = pts[0:3].copy()
    ba._BaProcessor__execute_bundle_adjustment()
    capsys.readouterr()
    assert ba.ba_last_action in ("create", "solve")
    assert np.all(np.isfinite(pts)) and not np.array_equal(before, pts[0:3])
    assert np.abs(pts[0:3] - true[:, pid]).max() < 1.0
    ba.ba_release()
