"""Host-side checks of the robust similarity (no GPU): the stratified sampler against the NumPy sampler and Python integers,
every argument the library and ``check_similarity`` refuse (before a device is looked for, outputs untouched), the NumPy
reference of tests/_similarity_reference.py on the scenes the GPU tests use -- EVERY set of every case of
tests/test_gpu_similarity.py and tests/test_gpu_ba_align.py is settled, so the GPU tests compare decisions exactly and leave
nothing out -- its tolerance of wrong correspondences, and ``geometry.apply_similarity`` against the formula."""
import ctypes

import numpy as np
import pytest

import _similarity_reference as sr


def test_the_sample_of_every_hypothesis(sfm):
    native = sfm.native
    for n in list(range(4, 71)) + [1025]:
        for max_hyp in (1, 128):
            want = sr.sample_indices(n, max_hyp)
            lo, hi = np.arange(3) * n // 3, np.arange(1, 4) * n // 3
            assert np.all(want >= lo) and np.all(want < hi) and np.all(np.diff(want, axis=1) > 0)       # one per third, ascending
            for h in range(max_hyp):
                H, idx = native.similarity_sample(n, max_hyp, h)
                assert H == max_hyp and idx == tuple(want[h].tolist()), (n, max_hyp, h)
            assert native.similarity_sample(n, max_hyp, -1) == (max_hyp, (-1,) * 3) == native.similarity_sample(n, max_hyp, max_hyp)
    assert native.similarity_sample(100, 0, 127) == native.similarity_sample(100, 128, 127)
    assert native.similarity_sample(1025, 65536, 65535)[1] == tuple(sr.sample_indices(1025, 65536)[65535].tolist())
    for n, max_hyp in ((3, 128), (0, 128), (-1, 128), (100, -1), (100, 65537)):
        assert native.similarity_sample(n, max_hyp, 0) == (0, (-1,) * 3), (n, max_hyp)
        assert sr.hypothesis_count(n, max_hyp) == 0


def test_the_numpy_sampler_is_the_rule_in_python_integers():
    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return z ^ (z >> 31)
    assert mix(0) == 0xE220A8397B1DCDAF                       # splitmix64's first output from state 0
    for n, h in ((4, 0), (17, 5), (363, 127), (5000, 999), (1 << 20, 65535)):
        want = [k * n // 3 + mix(3 * h + k) % ((k + 1) * n // 3 - k * n // 3) for k in range(3)]
        assert sr.sample_indices(n, h + 1)[h].tolist() == want


def _library_call(native, n_sets, set_ptr, M, src, dst, max_err2, max_hyp, iters, flags, sim):
    """sfm_similarity_ransac with every optional output present and filled with a mark: (status, the outputs)."""
    outs = dict(inlier=np.full(max(M, 1), 7, dtype=np.uint8), n_inliers=np.full(max(n_sets, 1), -7, dtype=np.int32),
                best_hyp=np.full(max(n_sets, 1), -7, dtype=np.int32), status=np.full(max(n_sets, 1), -7, dtype=np.int32),
                summary=np.full(6, -7, dtype=np.int64))
    ptr = None if set_ptr is None else native.iptr(np.asarray(set_ptr, dtype=np.int32))
    st = native.load().sfm_similarity_ransac(n_sets, ptr, M, None if src is None else native.dptr(src), None if dst is None else native.dptr(dst),
                                             max_err2, max_hyp, iters, flags, None if sim is None else native.dptr(sim),
                                             outs["inlier"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), native.iptr(outs["n_inliers"]),
                                             native.iptr(outs["best_hyp"]), native.iptr(outs["status"]),
                                             outs["summary"].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return st, outs


def test_every_bad_argument_is_refused_before_a_device_is_looked_for(sfm):
    native = sfm.native
    a = np.arange(15, dtype=np.float64).reshape(3, 5)
    good = dict(n_sets=1, set_ptr=[0, 5], M=5, src=a, dst=a, max_err2=1.0, max_hyp=128, iters=2, flags=0)
    bad = [dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(max_hyp=-1), dict(max_hyp=65537), dict(iters=-1), dict(flags=2),
           dict(flags=-1), dict(n_sets=-1), dict(M=-1), dict(set_ptr=None), dict(set_ptr=[1, 5]), dict(set_ptr=[0, 4]),
           dict(n_sets=3, set_ptr=[0, 3, 2, 5]), dict(src=None), dict(dst=None), dict(sim=None)]
    for kw in bad:
        args = dict(good)
        sim = np.full(13, -7.25)
        args["sim"] = sim
        args.update(kw)
        st, outs = _library_call(native, **args)
        assert st == native.E_SHAPE and native.last_error(), kw
        assert np.all(sim == -7.25) and all(np.all(o == (7 if o.dtype == np.uint8 else -7)) for o in outs.values()), kw
        st = native.load().sfm_similarity_ransac_dev(args["n_sets"], None if args["set_ptr"] is None else native.iptr(np.asarray(args["set_ptr"], dtype=np.int32)),
                                                     args["M"], None if args["src"] is None else 8, None if args["dst"] is None else 8,
                                                     args["max_err2"], args["max_hyp"], args["iters"], args["flags"],
                                                     None if args["sim"] is None else 8, None, None, None, None, None, None)
        assert st == native.E_SHAPE, kw
    # ... and by the Python checks, without the library
    for kw in (dict(max_err2=float("nan")), dict(max_err2=-1.0), dict(max_hyp=-1), dict(max_hyp=65537), dict(max_hyp=1.5), dict(iters=-1),
               dict(iters=0.5)):
        args = dict(max_err2=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            native.check_similarity(**args)
        with pytest.raises(ValueError):
            native.similarity_ransac([0, 5], a, a, **args)
        with pytest.raises(ValueError):
            native.similarity_ransac_dev([0, 5], 5, 0, 0, **args)
    assert native.check_similarity(1, 0, 2, True) == (1.0, 0, 2, native.SIMILARITY_RIGID)
    assert native.check_similarity(0.25) == (0.25, 0, 2, 0)
    for ptr in ([1, 5], [0, 3, 2, 5], [0, 4], []):
        with pytest.raises(ValueError, match="set_ptr"):
            native.similarity_ransac(ptr, a, a, 1.0)
    with pytest.raises(ValueError, match="src"):
        native.similarity_ransac([0, 5], a, np.zeros((3, 4)), 1.0)
    with pytest.raises(ValueError, match="src"):
        native.similarity_ransac([0, 5], np.zeros((2, 5)), np.zeros((2, 5)), 1.0)
    with pytest.raises(ValueError, match="outputs"):
        native.similarity_ransac([0, 5], a, a, 1.0, outputs=("mask",))
    assert (native.SIMILARITY_TOO_FEW, native.SIMILARITY_NO_MODEL, native.SIMILARITY_KEPT_HYPOTHESIS) == (sr.TOO_FEW, sr.NO_MODEL, sr.KEPT_HYPOTHESIS)
    assert (native.SIMILARITY_MAX_HYP, native.SIMILARITY_DEFAULT_HYP, native.SIMILARITY_MIN_SET) == (sr.HYP_MAX, sr.HYP_DEFAULT, sr.MIN_SET)
    assert len(native.SIMILARITY_SUMMARY) == 6 and native.SIMILARITY_OUTPUTS == ("inlier", "n_inliers", "best_hyp", "status", "summary")
    for name in ("sfm_similarity_ransac", "sfm_similarity_ransac_dev", "sfm_similarity_sample", "sfm_ba_transform", "sfm_ba_align"):
        assert name in native.EXPORTS


def test_the_version(sfm):
    assert sfm.native.load().sfm_version() >= 106


@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_every_set_of_every_case_is_settled(case, capsys):
    sc, ref = sr.case_reference(case)
    with capsys.disabled():
        print("\n%s: %d sets, %d unsettled, worst d_S %.3e, summary %s"
              % (sr.case_id(case), sc.counts.size, int((~ref.settled).sum()), ref.d_S.max(initial=0.0), ref.summary.tolist()))
    assert ref.settled.all(), np.flatnonzero(~ref.settled)
    assert np.all(ref.d_S < 1e-9)
    assert ref.summary[0] + ref.summary[1] + ref.summary[2] == sc.counts.size and ref.summary[4] == ref.inlier.sum()
    assert np.all(ref.status[sc.counts < sr.MIN_SET] == sr.TOO_FEW) and np.all((ref.status[sc.counts >= sr.MIN_SET] & sr.TOO_FEW) == 0)


def test_the_alignment_case_is_settled(sfm):
    sc, idx, targets, bad = sr.align_case(sfm.scenes)
    assert (sc.n_cams, sc.n_pts) == (6, 120) and bad.sum() == 20
    ref = sr.reference([0, idx.size], np.ascontiguousarray(sc.pts_init[:, idx]), targets, sr.MAX_ERR2, 128, 2)
    assert ref.settled.all() and ref.status[0] == 0 and np.array_equal(ref.inlier.astype(bool), ~bad)
    assert sr.sim_difference(ref.sim[0], sr.align_sim(), ref.ext[0]) < 1e-2
    rigid = sr.reference([0, idx.size], np.ascontiguousarray(sc.pts_init[:, idx]), targets, sr.MAX_ERR2, 128, 2, True)
    assert rigid.settled.all()


def test_the_scenes_reach_what_they_are_there_for():
    sc, ref = sr.scene_and_reference("degenerate")
    assert ref.status.tolist() == [sr.NO_MODEL, sr.NO_MODEL, 0] and not ref.sim[0].any() and not ref.sim[1].any()
    lo = int(sc.set_ptr[2])
    assert ref.inlier[lo + 17] == 0 and ref.n_inliers[2] == 59                       # the NaN row is never an inlier
    sc, ref = sr.scene_and_reference("ties", 1000, sr.ITERS, sr.EVERYONE)
    for k in range(2):                                                               # every valid hypothesis counts the whole set
        a, b = sr.set_of(sc, k)
        hyp = sr._hypotheses(a, b, 1000, 0, False)
        counts = sr._counts(hyp, sr.err2(hyp[1], hyp[2], hyp[3], a, b), sr.EVERYONE)
        assert (counts == a.shape[1]).sum() > 1 and ref.best_hyp[k] == int(np.flatnonzero(counts == a.shape[1])[0])
    sc, ref = sr.scene_and_reference("ties", 1000, sr.ITERS, sr.MAX_ERR2)
    for k in range(2):
        a, b = sr.set_of(sc, k)
        hyp = sr._hypotheses(a, b, 1000, 0, False)
        counts = sr._counts(hyp, sr.err2(hyp[1], hyp[2], hyp[3], a, b), sr.MAX_ERR2)
        assert (counts == counts.max()).sum() > 1 and ref.best_hyp[k] == int(np.argmax(counts))
    sc, ref = sr.scene_and_reference("rigid", 128, sr.ITERS, sr.MAX_ERR2, True)
    assert np.all(ref.sim[:, 0] == 1.0)
    sc, ref = sr.scene_and_reference("offset")
    assert np.all(np.abs(ref.sim[:, 10:13]) > 0.9e6)
    sc, ref = sr.scene_and_reference("kept", 128, sr.ITERS, sr.KEPT_ERR2)
    assert ref.status.tolist() == [sr.KEPT_HYPOTHESIS] * 2 and np.all(ref.stood == 0) and ref.summary[3] == 2
    sc, ref = sr.scene_and_reference("many_sets")
    assert sc.counts.size == 259 and sc.counts[0] == 0 and sc.counts[-1] == 4
    sc, ref = sr.scene_and_reference("paths", 128, 0)
    assert np.all(ref.status[ref.best_hyp >= 0] == 0) and np.all(ref.stood == 0)     # iters = 0: no round, no KEPT bit
    assert sorted(sc.counts.tolist()) == sorted(sr.PATHS_COUNTS)


def test_the_reference_tolerates_half_the_correspondences_being_wrong():
    sc, ref = sr.scene_and_reference("proto")
    a, b = sr.set_of(sc, 2)
    lo, hi = int(sc.set_ptr[2]), int(sc.set_ptr[3])
    bad = sc.bad[lo:hi]
    assert bad.sum() == 1000
    kept = ref.inlier[lo:hi].astype(bool)
    assert (kept & ~bad).sum() >= 0.95 * (~bad).sum() and not (kept & bad).any()
    plain = sr.plain_umeyama(a, b)
    within = ((sr.apply_sim(plain, a) - b) ** 2).sum(axis=0) <= sr.MAX_ERR2
    assert within[~bad].sum() < 0.5 * (~bad).sum()
    assert sr.sim_difference(ref.sim[2], sc.truth[2], ref.ext[2]) < 1e-2


def test_apply_similarity_against_the_formula(sfm):
    g = sfm.geometry
    rng = np.random.default_rng(3)
    A = sr.random_rotation(rng)
    s, t = 1.75, np.array([0.5, -2.0, 3.0])
    rots = np.stack([sr.random_rotation(rng) for _ in range(5)])
    locs = rng.standard_normal((5, 3))
    cams = g.pack_cameras(rots, locs)
    pts = rng.standard_normal((3, 11))
    new_cams, new_pts = g.apply_similarity((s, A, t), cams, pts)
    assert np.allclose(new_pts, s * A @ pts + t[:, None], rtol=0, atol=1e-14)
    assert np.allclose(new_cams[:, 0:3], (s * A @ locs.T + t[:, None]).T, rtol=0, atol=1e-14) and np.all(new_cams[:, 3] >= 0)
    for c in range(5):
        assert np.allclose(g.quaternion_to_rotation(new_cams[c, 3:7]), A @ rots[c], rtol=0, atol=1e-12)
    # the residual is invariant up to the factor s: R'^T (X' - C') = s R^T (X - C)
    X, Xn = pts[:, 4], new_pts[:, 4]
    assert np.allclose((A @ rots[2]).T @ (Xn - new_cams[2, 0:3]), s * rots[2].T @ (X - locs[2]), rtol=0, atol=1e-13)
    flat = np.concatenate(([s], A.ravel(), t))
    again = g.apply_similarity(flat, cams, pts)
    assert np.array_equal(again[0], new_cams) and np.array_equal(again[1], new_pts)
    assert g.apply_similarity(flat, None, pts)[0] is None and g.apply_similarity(flat, cams, None)[1] is None
    # a camera taken to a half turn has no canonical quaternion
    half = np.diag([1.0, -1.0, -1.0]) @ rots[1].T
    with pytest.raises(ValueError):
        g.apply_similarity((1.0, half, np.zeros(3)), cams, None)
