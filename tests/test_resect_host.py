"""Host-side checks of the robust resection (no GPU): the numbering of the triples against Python integers, the argument
checks, and the NumPy reference of tests/_resect_reference.py on the scenes the GPU tests use -- it flags exactly the
displaced observations on the prototype scenes, and EVERY camera of every scene any test uses is settled, so the GPU tests
compare decisions exactly and leave nothing out."""
import itertools

import numpy as np
import pytest

import _resect_reference as rf


def _check_numbering(native, n, max_hyp, hs):
    ks = rf.triple_numbers(n, max_hyp)
    H = len(ks)
    assert H == rf.hypothesis_count(n, max_hyp)
    i, j, l = rf.triples_of(n, ks) if H else (np.zeros(0, dtype=np.int64),) * 3
    for h in hs:
        got = native.resect_triple(n, max_hyp, h)
        assert got == (H, int(i[h]), int(j[h]), int(l[h])), (n, max_hyp, h)
        assert 0 <= got[1] < got[2] < got[3] < n
    assert native.resect_triple(n, max_hyp, -1) == (H, -1, -1, -1) and native.resect_triple(n, max_hyp, H) == (H, -1, -1, -1)
    return H


@pytest.mark.parametrize("max_hyp", [1, 128, 65536])
def test_the_triple_of_every_hypothesis(sfm, max_hyp):
    native = sfm.native
    for n in (3, 4, 9, 10, 11, 64, 363, 1 << 20):
        H = rf.hypothesis_count(n, max_hyp)
        assert _check_numbering(native, n, max_hyp, range(H)) == min(rf.triple_count(n), max_hyp)
    assert [rf.triple_count(n) for n in (9, 10, 11)] == [84, 120, 165]
    assert native.resect_triple(10, 0, 119) == native.resect_triple(10, 128, 119) == (120, 7, 8, 9)      # 0 means 128


def test_the_reference_numbering_is_lexicographic():
    for n in (3, 4, 7, 12):
        got = list(zip(*[a.tolist() for a in rf.triples_of(n, range(rf.triple_count(n)))]))
        assert got == list(itertools.combinations(range(n), 3)), n
    # the last triples of the largest camera, in Python integers
    n = 1 << 20
    T = rf.triple_count(n)
    i, j, l = rf.triples_of(n, [T - 1, T - 2, T - 4, 0, n - 3])
    assert list(zip(i.tolist(), j.tolist(), l.tolist())) == [(n - 3, n - 2, n - 1), (n - 4, n - 2, n - 1), (n - 4, n - 3, n - 2),
                                                             (0, 1, 2), (0, 1, n - 1)]


def test_out_of_range_arguments(sfm):
    native = sfm.native
    for n, max_hyp in ((2, 128), (0, 128), (-1, 128), ((1 << 20) + 1, 128), (10, -1), (10, 65537)):
        assert native.resect_triple(n, max_hyp, 0) == (0, -1, -1, -1), (n, max_hyp)
    for kw in (dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(max_hyp=-1), dict(max_hyp=65537), dict(max_hyp=1.5),
               dict(iters=-1), dict(lam=-0.5), dict(lam=float("nan")), dict(mask=[1, 0]), dict(cam_scale=[1.0, float("inf"), 1.0])):
        args = dict(max_err2=16.0)
        args.update(kw)
        with pytest.raises(ValueError):
            native.check_resect(3, **args)
    assert native.check_resect(3, 16, 0, 1, 2, [1, 0, 1])[0:4] == (16.0, 0, 1.0, 2)
    uv, X = np.zeros((2, 5)), np.zeros((3, 5))
    for ptr in ([1, 5], [0, 3, 2, 5], [0, 4], []):
        with pytest.raises(ValueError, match="view_ptr"):
            native.check_resect_views(ptr, uv, X)
    with pytest.raises(ValueError, match="uv"):
        native.check_resect_views([0, 5], uv, np.zeros((3, 4)))
    assert native.RESECT_SUMMARY[0] == "cams_solved" and native.RESECT_HELD == rf.HELD == 16
    assert (native.RESECT_TOO_FEW, native.RESECT_NO_MODEL, native.RESECT_KEPT_HYPOTHESIS, native.RESECT_SAMPLED) == \
        (rf.TOO_FEW, rf.NO_MODEL, rf.KEPT_HYPOTHESIS, rf.SAMPLED)


@pytest.mark.parametrize("name", ["proto0", "proto1", "proto2"])
def test_the_reference_flags_exactly_the_displaced_observations(name):
    sc, cm, ref = rf.scene_and_reference(name)
    assert np.all(ref.best_hyp >= 0) and ref.summary[0] == sc.n_views
    assert np.array_equal(ref.inlier == 0, sc.displaced[cm.order])


@pytest.mark.parametrize("name,max_hyp", rf.CASES)
def test_every_camera_of_every_scene_is_settled(name, max_hyp, capsys):
    sc, cm, ref = rf.scene_and_reference(name, max_hyp)
    with capsys.disabled():
        print("\n%s, max_hyp %d: %d cameras, %d unsettled, worst d_c %.3e, summary %s"
              % (name, max_hyp, sc.n_views, int((~ref.settled).sum()), ref.d_c.max(), ref.summary.tolist()))
    assert ref.settled.all()
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.n_views and ref.summary[4] == ref.inlier.sum()


def test_the_special_scene_is_what_it_says():
    sc, cm, ref = rf.scene_and_reference("special")
    assert cm.counts[1] == 8 and cm.counts[2] == 12
    assert ref.status[1] & rf.NO_MODEL and ref.status[2] & rf.NO_MODEL and ref.best_hyp[0] >= 0 and ref.best_hyp[3] >= 0
    # the collinear camera: no triple of it has a frame
    lo, hi = cm.view_ptr[2], cm.view_ptr[3]
    X = cm.X[:, lo:hi].T
    i, j, l = rf.hypothesis_triples(12, 128)
    assert not np.cross(X[j] - X[i], X[l] - X[i]).any()


def test_the_paths_scene_has_every_count():
    sc, cm = rf.scene("paths")
    assert sorted(cm.counts.tolist()) == sorted(rf.PATHS_COUNTS)
    ref = rf.scene_and_reference("paths", 128)[2]
    assert np.array_equal((ref.status & rf.TOO_FEW) != 0, cm.counts < 4)
    assert np.array_equal((ref.status & rf.SAMPLED) != 0, np.array([rf.triple_count(n) > 128 and n >= 4 for n in cm.counts]))
