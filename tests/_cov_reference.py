"""NumPy references of the resident scene's covariance blocks (sfm_ba_covariance), by two independent routes.

Route A, the Schur route: ``oracle.ba_reduced_system`` (through ``_robust_reference.reduced_system`` for the weighted
blocks), ``np.linalg.inv`` of the free cameras' principal submatrix S_ff, and per point D^-1 + Y^T Sigma Y over its track.
Route B, the full route: the dense Jacobian restricted to the free cameras and all observed points, ``inv(J^T J + lambda I)``,
optionally with one Newton step X <- X + X (I - H X) carried out in ``longdouble``.

Both return ``(cam_cov (V, 7, 7), pt_cov (N, 6) packed xx xy xz yy yz zz, sigma0_sq)``; a held camera's block and an
unobserved point's block are zero.  ``block_rel`` is the norm every comparison uses: per block, the largest absolute
difference over the largest absolute entry of the reference block."""
import numpy as np

import _robust_reference as rr

PACK = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])


def free_mask(n_cams, held):
    m = np.ones(n_cams, dtype=np.uint8)
    m[list(held)] = 0
    return m


def sigma0_sq(cost, n_obs, n_free, n_observed):
    dof = 2 * n_obs - 7 * n_free - 3 * n_observed
    return cost / dof if dof > 0 else 0.0


def block_rel(got, want):
    """max over blocks of max|got - want| / max|want| (blocks along axis 0; an all-zero reference block must be matched
    exactly)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.shape[0] == 0:
        return 0.0
    g, w = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(w))
    err, scale = np.max(np.abs(g - w), axis=1), np.max(np.abs(w), axis=1)
    zero = scale == 0
    assert not np.any(err[zero]), "a block that is zero in the reference is not zero"
    return float(np.max(err[~zero] / scale[~zero])) if (~zero).any() else 0.0


def route_a(cams, pts, cam_idx, pt_idx, uv, lam, mask, kind=rr.LOSS_NONE, delta=1.0, quirks=None, want_parts=False):
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    nv, npt, m = cams.shape[0], pts.shape[1], cam_idx.shape[0]
    t = rr.reduced_system(cams, pts, cam_idx, pt_idx, uv, lam, kind, delta, quirks)
    mask = np.ones(nv, dtype=np.uint8) if mask is None else np.asarray(mask)
    free = np.flatnonzero(mask != 0)
    rows = (7 * free[:, None] + np.arange(7)[None, :]).ravel()
    sigma = np.zeros((7 * nv, 7 * nv))
    if rows.size:
        sigma[np.ix_(rows, rows)] = np.linalg.inv(t["S"][np.ix_(rows, rows)])
    cam_cov = np.stack([sigma[7 * c:7 * c + 7, 7 * c:7 * c + 7] for c in range(nv)])
    pt_full = np.zeros((npt, 3, 3))
    order = np.argsort(pt_idx, kind="stable")
    bounds = np.searchsorted(pt_idx[order], np.arange(npt + 1))
    for p in range(npt):
        obs = order[bounds[p]:bounds[p + 1]]
        if obs.size == 0:
            continue
        r = (7 * cam_idx[obs][:, None] + np.arange(7)[None, :]).ravel()
        ys = t["Y"][obs].reshape(-1, 3)                                   # (7 deg, 3)
        pt_full[p] = t["D_inv"][p] + ys.T @ sigma[np.ix_(r, r)] @ ys
    n_observed = int(np.count_nonzero(np.bincount(pt_idx, minlength=npt)))
    out = (cam_cov, pt_full[:, PACK[0], PACK[1]], sigma0_sq(t["cost"], m, free.size, n_observed))
    return out + (t, sigma) if want_parts else out


def route_b(cams, pts, cam_idx, pt_idx, uv, lam, mask, kind=rr.LOSS_NONE, delta=1.0, quirks=None, newton=True):
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
    nv, npt, m = cams.shape[0], pts.shape[1], cam_idx.shape[0]
    t = rr.reduced_system(cams, pts, cam_idx, pt_idx, uv, lam, kind, delta, quirks)      # (for its Jp, Jx and cost only)
    mask = np.ones(nv, dtype=np.uint8) if mask is None else np.asarray(mask)
    free = np.flatnonzero(mask != 0)
    col_of_cam = -np.ones(nv, dtype=np.int64)
    col_of_cam[free] = 7 * np.arange(free.size)
    seen = np.flatnonzero(np.bincount(pt_idx, minlength=npt))
    col_of_pt = -np.ones(npt, dtype=np.int64)
    col_of_pt[seen] = 7 * free.size + 3 * np.arange(seen.size)
    n = 7 * free.size + 3 * seen.size
    jac = np.zeros((2 * m, n))
    for o in range(m):
        c, p = cam_idx[o], pt_idx[o]
        if col_of_cam[c] >= 0:
            jac[2 * o:2 * o + 2, col_of_cam[c]:col_of_cam[c] + 7] = t["Jp"][o]
        jac[2 * o:2 * o + 2, col_of_pt[p]:col_of_pt[p] + 3] = t["Jx"][o]
    h = jac.T @ jac + lam * np.eye(n)
    x = np.linalg.inv(h)
    if newton:
        hl, xl = h.astype(np.longdouble), x.astype(np.longdouble)
        x = (xl + xl @ (np.eye(n, dtype=np.longdouble) - hl @ xl)).astype(np.float64)
    x = 0.5 * (x + x.T)
    cam_cov = np.zeros((nv, 7, 7))
    for c in free:
        k = col_of_cam[c]
        cam_cov[c] = x[k:k + 7, k:k + 7]
    pt_full = np.zeros((npt, 3, 3))
    for p in seen:
        k = col_of_pt[p]
        pt_full[p] = x[k:k + 3, k:k + 3]
    return cam_cov, pt_full[:, PACK[0], PACK[1]], sigma0_sq(t["cost"], m, free.size, seen.size)


_STATE = {}


def adjusted_state(oracle, key, sc, uvn, lam=1e-3, iters=5):
    """The scene's state after ``iters`` oracle iterations, computed once per ``key`` and left unchanged."""
    if key not in _STATE:
        cams, pts = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, lam, iters)
        cams.setflags(write=False)
        pts.setflags(write=False)
        _STATE[key] = (cams, pts)
    return _STATE[key]


_AB = {}


def ab_disagreement(key, *args, **kwargs):
    """Route A against route B (plain float64, no Newton step) on one scene and setting, once per ``key``:
    (camera blocks, point blocks, |sigma0^2 difference| relative) and route A's result."""
    if key not in _AB:
        a = route_a(*args, **kwargs)
        b = route_b(*args, newton=False, **kwargs)
        for arr in a[0:2]:
            arr.setflags(write=False)
        s = abs(a[2] - b[2]) / abs(b[2]) if b[2] else abs(a[2])
        _AB[key] = ((block_rel(a[0], b[0]), block_rel(a[1], b[1]), s), a)
    return _AB[key]


# ---- the scenes and settings both test files run -------------------------------------------------------------------
# The two scenes the parity is specified on, and small instances of the four track-structured kinds of
# test_gpu_visibility_structure.py (an empty camera, a hub, two clusters, single observations).
SCENES = ("6x300", "12x200_tracks", "empty", "hub", "clusters2", "single")
_SCENES = {}


def scene(sfm, oracle, name):
    """(scene, normalised keys, cams, pts after 5 oracle iterations at lambda = 0.1, focal scale), once per name."""
    if name not in _SCENES:
        st = sfm.scenes.Structure
        if name == "6x300":
            sc = sfm.scenes.make_scene(6, 300, 0.7, seed=21)
        elif name == "12x200_tracks":
            sc = sfm.scenes.make_scene(12, 200, seed=3, structure=st(mean_track=4.0, heavy=0.1))
        elif name == "empty":
            sc = sfm.scenes.make_scene(8, 200, seed=1, structure=st(mean_track=3.0, empty=(4,)))
        elif name == "hub":
            sc = sfm.scenes.make_scene(12, 300, seed=9, structure=st(mean_track=2.0, hub=(0,)))
        elif name == "clusters2":
            sc = sfm.scenes.make_scene(10, 240, seed=10, structure=st(mean_track=3.0, clusters=2))
        else:
            sc = sfm.scenes.make_scene(8, 240, seed=11, structure=st(mean_track=3.0, single=0.15))
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        uvn.setflags(write=False)
        cams, pts = adjusted_state(oracle, name, sc, uvn, lam=0.1, iters=5)
        _SCENES[name] = (sc, uvn, cams, pts, float(np.sqrt(abs(sc.intrinsic[0, 0] * sc.intrinsic[1, 1]))))
    return _SCENES[name]


def settings(name):
    """(lambda, held cameras) a scene is run with: lambda in {0, 1e-6, 1e-3} with cameras {0, 1} held, and {0} held with
    lambda > 0 only.  Left out, because the system is singular by construction and NumPy has no inverse to compare with
    (the status paths have tests of their own): lambda = 0 on the two clusters (the second cluster's gauge is free whatever
    is held in the first) and on the scene with an empty camera (its block of S is lambda I).  lambda = 0 on the scene with
    single observations is run against ``without_single_points`` (``single_undamped``): D_p of such a point has rank 2 and
    NumPy cannot invert it, but the limit lambda -> 0 exists."""
    out = [(lam, (0, 1)) for lam in (0.0, 1e-6, 1e-3)] + [(lam, (0,)) for lam in (1e-6, 1e-3)]
    if name in ("clusters2", "single", "empty"):
        out = [s for s in out if s[0] > 0]
    return out


def tolerance(ab):
    """What the device may differ from route A by, given the A-against-B disagreement of the same scene and setting:
    100 x covers a different elimination order at that conditioning; never below the 1e-9 of the other parity tests."""
    return max(1e-9, 100.0 * ab)


def without_single_points(pt_ptr, cam_idx, pt_idx, uv, pts):
    """The scene without the points that have exactly one observation, and without that observation: the limit
    lambda -> 0 of the full scene, since Jx (Jx^T Jx + lambda I)^-1 Jx^T -> I_2 for a 2x3 Jx of rank 2 and the observation's
    share of S, Jp^T (I - ...) Jp, vanishes.  Returns (cam_idx, pt_idx, uv, pts, kept): ``kept`` the old indices of the
    points that stay (renumbered 0 ..)."""
    deg = np.diff(pt_ptr)
    kept = np.flatnonzero(deg != 1)
    new_of = -np.ones(deg.shape[0], dtype=np.int64)
    new_of[kept] = np.arange(kept.size)
    sel = deg[pt_idx] != 1
    return cam_idx[sel], new_of[pt_idx[sel]].astype(np.int32), np.ascontiguousarray(uv[:, sel]), np.ascontiguousarray(pts[:, kept]), kept


def single_undamped(sfm, oracle, quirks, kind, delta, held):
    """The scene with single observations at lambda = 0: ((A-B of camera blocks, of point blocks), cam_cov (V, 7, 7),
    pt_cov (N, 6) with zeros for the single points, sigma0^2 by the formula on the FULL scene's cost and counts, single
    mask (N,)), once per setting."""
    key = ("single0", quirks, kind, held)
    if key not in _AB:
        sc, uvn, cams, pts, _scale = scene(sfm, oracle, "single")
        cam_idx, pt_idx, uv, pts_kept, kept = without_single_points(sc.pt_ptr, sc.cam_idx, sc.pt_idx, uvn, pts)
        mask = free_mask(sc.n_cams, held)
        (cam_ab, pt_ab, _s), a = ab_disagreement(key + ("reduced",), cams, pts_kept, cam_idx, pt_idx, uv, 0.0, mask, kind, delta, quirks)
        pt_cov = np.zeros((sc.n_pts, 6))
        pt_cov[kept] = a[1]
        single = np.ones(sc.n_pts, dtype=bool)
        single[kept] = False
        n_observed = int(np.count_nonzero(np.diff(sc.pt_ptr)))
        s0 = sigma0_sq(rr.state_cost(cams, pts, sc.cam_idx, sc.pt_idx, uvn, kind, delta), sc.n_obs, int(mask.sum()), n_observed)
        _AB[key] = ((cam_ab, pt_ab), a[0], pt_cov, s0, single)
    return _AB[key]
