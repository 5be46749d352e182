"""What the GPU tests of the robust two-view geometry share: the call, the comparison with the reference of
tests/_twoview_ransac_reference.py (decisions exactly, the matrix per set in the G measure at max(1e-9, 100 d_G), d_G being the
reference's own spread) and the bit-for-bit comparison of a set across calls."""
import numpy as np

import _twoview_ransac_reference as tv


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(hip, sc, max_hyp=128, iters=tv.ITERS, max_err2=tv.MAX_ERR2):
    return hip.twoview_ransac(sc.set_ptr, sc.left, sc.right, max_err2, max_hyp, iters)


def check_against(ref, F, inlier, n_in, best, status, summary, where="", worst=None):
    """Exact decisions, matrices at the per-set bound, sets without a model as nine zeros.  worst: a dict whose "d_G" and
    "device" are raised to the largest reference spread and device difference seen."""
    assert ref.settled.all()
    assert np.array_equal(status, ref.status), where
    assert np.array_equal(best, ref.best_hyp), where
    assert np.array_equal(n_in, ref.n_inliers), where
    assert np.array_equal(inlier, ref.inlier), where
    assert np.array_equal(summary, ref.summary), where
    solved = ref.best_hyp >= 0
    for s in np.flatnonzero(solved):
        diff = tv.g_difference(F[s], ref.F[s], ref.c[s])
        if worst is not None and ref.d_G[s] < 1e-3:             # (the noise-free plane: any [e]x H is a solution)
            worst["d_G"] = max(worst["d_G"], ref.d_G[s]); worst["device"] = max(worst["device"], diff)
        print(where, "set", s, "d_G %.3e device %.3e" % (ref.d_G[s], diff))
        assert diff <= max(1e-9, 100.0 * ref.d_G[s]), (where, s, diff, ref.d_G[s])
        assert abs(np.linalg.norm(F[s]) - 1.0) < 1e-14 and F[s].flat[np.argmax(np.abs(F[s]))] > 0
    assert not F[~solved].any() and same_bits(F[~solved], np.zeros_like(F[~solved])), where


def subset(sc, sets):
    """The sets `sets` of the scene, in that order, as a call of their own."""
    parts = [tv.set_of(sc, s) for s in sets]
    counts = [p[0].shape[1] for p in parts]
    return tv.SimpleNamespace(set_ptr=np.concatenate(([0], np.cumsum(counts))).astype(np.int32),
                              left=np.ascontiguousarray(np.hstack([p[0] for p in parts])),
                              right=np.ascontiguousarray(np.hstack([p[1] for p in parts])))


def same_sets(hip, sc, whole, sets, max_hyp, what, iters=tv.ITERS, max_err2=tv.MAX_ERR2):
    """The sets `sets` of the scene in a call of their own give the bits they have in `whole`, the result of the whole scene."""
    sub = subset(sc, sets)
    F, inlier, n_in, best, status, _summary = run(hip, sub, max_hyp, iters, max_err2)
    for k, s in enumerate(sets):
        assert same_bits(F[k], whole[0][s]), (what, s)
        assert same_bits(inlier[sub.set_ptr[k]:sub.set_ptr[k + 1]], whole[1][sc.set_ptr[s]:sc.set_ptr[s + 1]]), (what, s)
        assert (n_in[k], best[k], status[k]) == (whole[2][s], whole[3][s], whole[4][s]), (what, s)
