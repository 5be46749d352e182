"""Host-side tests of the robust triangulation of ragged tracks (no GPU): the pair numbering of sfm_tri_ransac_pair
against the reference's, the argument checks of native.check_ransac, and the NumPy reference itself
(tests/_tri_ransac_reference.py) on the scenes of its generator -- what it finds and how many points are settled."""
import numpy as np
import pytest

import _tri_ransac_reference as rr


@pytest.fixture(scope="module")
def lib(sfm):
    import os
    if not os.path.exists(sfm.native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    sfm.native.load()
    return sfm.native


@pytest.mark.parametrize("n,max_hyp", [(2, 128), (3, 128), (16, 128), (17, 128), (363, 65536), (46341, 128), (46341, 65536)])
def test_pair_numbering_equals_the_reference(lib, n, max_hyp):
    total = n * (n - 1) // 2
    want_i, want_j = rr.hypothesis_pairs(n, max_hyp)
    count = min(total, max_hyp)
    assert want_i.shape[0] == count == rr.hypothesis_count(n, max_hyp)
    assert np.all(want_i < want_j) and want_j.max() <= n - 1
    got = np.array([lib.tri_ransac_pair(n, max_hyp, h) for h in range(count)])
    assert np.all(got[:, 0] == count)
    assert np.array_equal(got[:, 1], want_i) and np.array_equal(got[:, 2], want_j)
    assert lib.tri_ransac_pair(n, max_hyp, count) == (count, -1, -1) and lib.tri_ransac_pair(n, max_hyp, -1) == (count, -1, -1)


def test_pair_numbering_at_its_edges(lib):
    assert {n: rr.hypothesis_count(n) for n in (16, 17)} == {16: 120, 17: 128}             # 136 pairs are sampled
    assert 363 * 362 // 2 == 65703 and 46341 ** 2 > 2 ** 31 > 46340 ** 2                  # the sizes the issue names
    assert lib.tri_ransac_pair(0, 128, 0)[0] == 0 and lib.tri_ransac_pair(1, 128, 0)[0] == 0
    assert lib.tri_ransac_pair(17, 0, 0)[0] == 128                                          # max_hyp = 0 means 128
    assert lib.tri_ransac_pair(17, 65537, 0)[0] == 0 and lib.tri_ransac_pair(17, -1, 0)[0] == 0
    # all pairs, in order, exactly once
    seen = [lib.tri_ransac_pair(16, 128, h)[1:] for h in range(120)]
    assert seen == [(i, j) for i in range(16) for j in range(i + 1, 16)]
    # the last pair of the longest track a 32-bit CSR can hold
    n = 2 ** 31 - 1
    total = n * (n - 1) // 2
    k = 65535 * total // 65536
    count, i, j = lib.tri_ransac_pair(n, 65536, 65535)
    before = i * (2 * n - i - 1) // 2                                                      # pairs that precede row i
    assert count == 65536 and 0 <= i < j < n and before <= k < before + (n - 1 - i) and j == i + 1 + (k - before)


@pytest.mark.parametrize("bad", [
    dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(cos_min_angle=-1.5), dict(cos_min_angle=float("nan")),
    dict(max_hyp=-1), dict(max_hyp=65537), dict(max_hyp=1.5), dict(iters=-1), dict(lam=-0.5), dict(lam=float("nan")),
    dict(group=3), dict(group=2), dict(group=128), dict(group=True), dict(cam_scale=np.ones(3)),
    dict(cam_scale=np.array([1.0, np.inf, 1.0, 1.0]))])
def test_check_ransac_refuses_bad_arguments(sfm, bad):
    args = dict(max_err2=16.0, cos_min_angle=0.999, max_hyp=128, lam=0.5, iters=3, cam_scale=None, group=0)
    assert sfm.native.check_ransac(4, **args) == (16.0, 0.999, 128, 0.5, 3, None, 0)
    args.update(bad)
    with pytest.raises(ValueError):
        sfm.native.check_ransac(4, **args)


def test_check_ransac_accepts_the_edges(sfm):
    out = sfm.native.check_ransac(4, 0.0, 1.0, 0, 0.0, 0, np.ones(4), 64)
    assert out[:5] == (0.0, 1.0, 0, 0.0, 0) and out[6] == 64
    assert sfm.native.check_ransac(4, float("inf"), -1.0, 65536, 1e9, 100)[2] == 65536


@pytest.mark.parametrize("k", [0, 1, 2])
def test_reference_flags_exactly_the_displaced_observations(k, capsys):
    """On tracks with at least three clean observations the reference's mask is the clean set on >= 98 % of the tracks
    (the prototype measured 100 %; seeds in _tri_ransac_reference.PROTOTYPE_SCENES)."""
    sc, ref = rr.scene_and_reference("proto%d" % k)
    clean = ~sc.displaced
    enough = [p for p in range(sc.n_pts) if clean[sc.pt_ptr[p]:sc.pt_ptr[p + 1]].sum() >= 3]
    exact = sum(np.array_equal(ref.inlier[sc.pt_ptr[p]:sc.pt_ptr[p + 1]].astype(bool), clean[sc.pt_ptr[p]:sc.pt_ptr[p + 1]])
                for p in enough)
    with capsys.disabled():
        print("\nscene %d x %d: %d of %d tracks with >= 3 clean observations flagged exactly; summary %s"
              % (sc.n_views, sc.n_pts, exact, len(enough), ref.summary.tolist()))
    assert len(enough) > 150 and sc.displaced.sum() > 0.05 * sc.displaced.shape[0]
    assert exact >= 0.98 * len(enough)
    err = np.linalg.norm(ref.X[0:3, enough] - sc.pts_true[:, enough], axis=0)
    assert err.max() < 0.05                                   # 0.5 px at f = 800 and a depth of 6 is 4e-3 per observation
    if k == 2:
        assert (ref.status & rr.SAMPLED).any() and sc.lengths.max() >= 19


def test_settled_share_is_within_the_cap(capsys):
    total = unsettled = 0
    for name in ("proto0", "proto1", "proto2", "paths"):
        sc, ref = rr.scene_and_reference(name)
        total += sc.n_pts
        unsettled += int((~ref.settled).sum())
        assert (~ref.settled).sum() <= 0.02 * sc.n_pts, name
    with capsys.disabled():
        print("\n%d of %d tracks unsettled" % (unsettled, total))
    assert unsettled <= 0.02 * total


def test_reference_summary_and_untouched_points():
    sc, ref = rr.scene_and_reference("paths")
    assert sorted(set(sc.lengths.tolist()) & set(rr.PATHS_LENGTHS)) == sorted(rr.PATHS_LENGTHS) and sc.n_pts <= 400
    few = sc.lengths < 2
    assert np.all(ref.status[few] == rr.TOO_FEW) and np.all(ref.best_hyp[few] == -1) and not ref.n_inliers[few].any()
    assert np.array_equal(ref.X[:, few], np.tile([[0.0], [0.0], [0.0], [1.0]], (1, few.sum())))
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.n_pts
    assert ref.summary[4] == ref.inlier.sum() == ref.n_inliers.sum()
    solved = ref.best_hyp >= 0
    assert ref.summary[5] == sc.lengths[solved].sum() - ref.n_inliers[solved].sum()
    p = int(np.flatnonzero(sc.lengths == 3)[0])
    assert ref.inlier[sc.pt_ptr[p]:sc.pt_ptr[p + 1]].tolist() == [1, 0, 1]
    # the gate at -1 leaves no model; x_init then comes back as it went in
    x_init = np.vstack((sc.pts_true + 0.25, np.full((1, sc.n_pts), 2.0)))
    none = rr.solve_tracks(sc.pt_ptr, sc.cam_idx, sc.uv, sc.projs, sc.cam_scale, x_init, cos_min=-1.0)
    assert np.array_equal(none.X, x_init) and not none.inlier.any() and np.all(none.best_hyp == -1)
    assert np.all(none.status[~few] & rr.NO_MODEL) and none.summary[0] == 0
