"""NumPy reference of the matrix-free bundle adjustment (sfm_ba_iterate_pcg), by two routes from the oracle's reduced system.

Both start from ``oracle.ba_reduced_system`` (through ``_robust_reference.reduced_system`` for the loss) and hold the cameras
with a zero mask entry by deleting their rows and columns of S:

``step_direct``   dp_f = solve(S_ff, rhs_f), then the camera update and the back substitution of ``oracle.ba_sparse``.
``step_pcg``      the algorithm the device runs, on the dense S: conjugate gradients from x = 0, preconditioned with the
                  7x7 diagonal blocks of S_ff, stopped when r.z <= tol^2 r0.z0 or after ``max_iters``; returns the count
                  and the r.z history.

``rel`` is the norm every comparison uses: the largest absolute difference over the largest absolute entry of the reference.
The scenes and settings are defined here once, for the host test (which measures what the reference's own PCG achieves on
them) and the device test (which holds the device to 1e-9 against ``step_direct``)."""
import numpy as np

import _robust_reference as rr

PCG_CONVERGED, PCG_MAX_ITERS, PCG_BREAKDOWN = 0, 1, 2

SCENES = ("6x300", "12x200_tracks", "hub", "empty", "clusters2", "single", "tracks40", "260", "hub70")
LAMBDAS = (5.0, 0.5)
LOSSES = ("none", "huber", "cauchy")
MASKS = ("none", "held01", "last3", "all_held")
EMPTY_CAMERA = 3
TRACK_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 70)
PER_LENGTH = 5


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def free_mask(n_cams, which):
    """uint8 (V,), 1 = free, or None for 'none'."""
    if which == "none":
        return None
    m = np.ones(n_cams, dtype=np.uint8)
    if which == "held01":
        m[[0, 1]] = 0
    elif which == "last3":
        m[:-3] = 0
    elif which == "all_held":
        m[:] = 0
    else:
        raise ValueError(which)
    return m


def _hub70():
    """The scene of test_gpu_covariance.py's track-length test: a hub of 70 cameras near the origin looking down +z at a
    cloud at depth 4 .. 8, PER_LENGTH points of every length in TRACK_LENGTHS, a point of length L seen by cameras
    0 .. L-1; the start cameras are a perturbation of those the keys were projected with."""
    deg = np.repeat(sorted(TRACK_LENGTHS, reverse=True), PER_LENGTH)
    seen = deg[:, None] > np.arange(max(TRACK_LENGTHS))[None, :]
    rng = np.random.default_rng(300)
    n, v = seen.shape
    pts = np.vstack((rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(4, 8, n)))
    pt_idx, cam_idx = (a.astype(np.int32) for a in np.nonzero(seen))
    pt_ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(seen.sum(axis=1), out=pt_ptr[1:])
    true = np.hstack((rng.uniform(-0.5, 0.5, (v, 3)), np.ones((v, 1)), rng.uniform(-0.05, 0.05, (v, 3))))
    true[:, 3:7] /= np.linalg.norm(true[:, 3:7], axis=1)[:, None]
    cams = true + np.hstack((rng.uniform(-0.02, 0.02, (v, 3)), np.zeros((v, 1)), rng.uniform(-0.005, 0.005, (v, 3))))
    cams[:, 3:7] /= np.linalg.norm(cams[:, 3:7], axis=1)[:, None]
    r = rr._oracle().obs_terms_vec(true, pts, cam_idx, pt_idx, np.zeros((2, cam_idx.shape[0])))[0]
    uv = np.ascontiguousarray(-r.T + rng.normal(0, 1e-3, (2, cam_idx.shape[0])))
    pts0 = pts + rng.normal(0, 0.01, pts.shape)
    return pt_ptr, cam_idx, pt_idx, uv, cams, pts0


class Case:
    """A scene as the tests use it: structure, normalised keys, start state, loss scale."""

    def __init__(self, name, n_cams, pt_ptr, cam_idx, pt_idx, uv, cams, pts, delta):
        self.name, self.n_cams, self.n_pts = name, int(n_cams), int(pt_ptr.shape[0] - 1)
        self.pt_ptr, self.cam_idx, self.pt_idx = pt_ptr, cam_idx, pt_idx
        self.uv, self.cams, self.pts, self.delta = uv, cams, pts, float(delta)
        for a in (self.pt_ptr, self.cam_idx, self.pt_idx, self.uv, self.cams, self.pts):
            a.setflags(write=False)


_CASES = {}


def case(sfm, name):
    if name in _CASES:
        return _CASES[name]
    st, mk = sfm.scenes.Structure, sfm.scenes.make_scene
    if name == "hub70":
        pt_ptr, cam_idx, pt_idx, uv, cams, pts = _hub70()
        c = Case(name, cams.shape[0], pt_ptr, cam_idx, pt_idx, uv, cams, pts, 5e-3)
    else:
        if name == "6x300":
            sc = mk(6, 300, 0.7, seed=21)
        elif name == "12x200_tracks":
            sc = mk(12, 200, seed=3, structure=st(mean_track=4, heavy=0.1))
        elif name == "hub":
            sc = mk(12, 300, seed=9, structure=st(mean_track=2.0, hub=(0,)))
        elif name == "empty":
            sc = mk(8, 200, seed=1, structure=st(mean_track=3.0, empty=(EMPTY_CAMERA,)))
        elif name == "clusters2":
            sc = mk(10, 240, seed=10, structure=st(mean_track=3.0, clusters=2))
        elif name == "single":
            sc = mk(8, 240, seed=11, structure=st(mean_track=3.0, single=0.15))
        elif name == "tracks40":
            sc = mk(40, 400, seed=40, structure=st(mean_track=5, heavy=0.05))
        elif name == "260":
            sc = mk(260, 40, 0.5, seed=260)
        else:
            raise ValueError(name)
        uvn = np.ascontiguousarray(sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic))
        scale = float(np.sqrt(abs(sc.intrinsic[0, 0] * sc.intrinsic[1, 1])))
        c = Case(name, sc.n_cams, sc.pt_ptr.copy(), sc.cam_idx.copy(), sc.pt_idx.copy(), uvn, sc.cams_init.copy(), sc.pts_init.copy(),
                 5.0 / scale)
    _CASES[name] = c
    return c


def loss_kind(loss):
    return {"none": rr.LOSS_NONE, "huber": rr.LOSS_HUBER, "cauchy": rr.LOSS_CAUCHY}[loss]


_SYSTEMS = {}


def system(c, cams, pts, lam, quirks, loss="none", key=None):
    """The reduced system of case ``c`` at (cams, pts); cached under ``key`` when one is given."""
    full = None if key is None else (c.name, lam, quirks, loss, key)
    if full is not None and full in _SYSTEMS:
        return _SYSTEMS[full]
    t = rr.reduced_system(np.asarray(cams).reshape(-1, 7), np.asarray(pts), c.cam_idx, c.pt_idx, c.uv, lam, loss_kind(loss), c.delta, quirks)
    if full is not None:
        _SYSTEMS[full] = t
    return t


def _free_rows(n_cams, mask):
    free = np.arange(n_cams) if mask is None else np.flatnonzero(np.asarray(mask) != 0)
    return free, (7 * free[:, None] + np.arange(7)[None, :]).ravel()


def apply_step(t, cams, pts, cam_idx, pt_idx, dp, mask):
    """cams += dp, q /= |q| on the free cameras (a held camera keeps its bits), pts += D^-1 (ex - sum W^T dp)."""
    cams = np.array(cams, dtype=np.float64, copy=True).reshape(-1, 7)
    free, _rows = _free_rows(cams.shape[0], mask)
    dp = dp.reshape(-1, 7)
    cams[free] = cams[free] + dp[free]
    cams[free, 3:7] /= np.sqrt(np.sum(np.square(cams[free, 3:7]), axis=1))[:, None]
    btd = np.zeros_like(t["ex"])
    np.add.at(btd, pt_idx, np.einsum('mij,mi->mj', t["W"], dp[cam_idx]))
    return cams, np.asarray(pts) + np.einsum('pij,pj->pi', t["D_inv"], t["ex"] - btd).T


def solve_direct(t, n_cams, mask):
    _free, rows = _free_rows(n_cams, mask)
    dp = np.zeros(7 * n_cams)
    if rows.size:
        dp[rows] = np.linalg.solve(t["S"][np.ix_(rows, rows)], t["rhs"][rows])
    return dp


def solve_pcg(t, n_cams, mask, tol, max_iters=None):
    """(dp (7V,), iterations, status, r.z history [rz0, rz1, ...])."""
    free, rows = _free_rows(n_cams, mask)
    dp = np.zeros(7 * n_cams)
    if max_iters is None or max_iters == 0:
        max_iters = min(7 * free.size, 1000)
    if rows.size == 0:
        return dp, 0, PCG_CONVERGED, [0.0]
    s, b = t["S"][np.ix_(rows, rows)], t["rhs"][rows]
    minv = np.zeros_like(s)
    for k in range(free.size):
        sl = slice(7 * k, 7 * k + 7)
        minv[sl, sl] = np.linalg.inv(s[sl, sl])
    x = np.zeros_like(b)
    r = b.copy()
    z = minv @ r
    p = z.copy()
    rz = rz0 = float(r @ z)
    hist = [rz0]
    if rz0 == 0.0:
        return dp, 0, PCG_CONVERGED, hist
    count, status = 0, PCG_MAX_ITERS
    while count < max_iters:
        q = s @ p
        pq = float(p @ q)
        if not (pq > 0.0 and np.isfinite(pq)):
            return np.zeros(7 * n_cams), count, PCG_BREAKDOWN, hist
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        z = minv @ r
        rz_new = float(r @ z)
        hist.append(rz_new)
        count += 1
        if rz_new <= tol * tol * rz0:
            status = PCG_CONVERGED
            break
        p = z + (rz_new / rz) * p
        rz = rz_new
    dp[rows] = x
    return dp, count, status, hist


def step_direct(c, cams, pts, lam, quirks, loss="none", mask=None, key=None):
    t = system(c, cams, pts, lam, quirks, loss, key)
    return apply_step(t, cams, pts, c.cam_idx, c.pt_idx, solve_direct(t, c.n_cams, mask), mask) + (t["cost"],)


def step_pcg(c, cams, pts, lam, quirks, loss="none", mask=None, tol=1e-13, max_iters=None, key=None):
    """(cams, pts, cost, iterations, status, r.z history)."""
    t = system(c, cams, pts, lam, quirks, loss, key)
    dp, count, status, hist = solve_pcg(t, c.n_cams, mask, tol, max_iters)
    return apply_step(t, cams, pts, c.cam_idx, c.pt_idx, dp, mask) + (t["cost"], count, status, hist)


def diagonal_block_pivots(c, lam, quirks):
    """Per camera, the smallest Cholesky pivot of its diagonal block S_cc at the case's start state, relative to the
    block's diagonal entry of the same row (the quantity the device's 1e-9 rule looks at); 0 for a block that does not
    factor.  A point of fewer than two observations is held (D_p^-1 = 0), as the device holds it at lambda = 0."""
    _r, jp, jx = rr._oracle().obs_terms_vec(np.array(c.cams), np.array(c.pts), c.cam_idx, c.pt_idx, c.uv, quirks)
    d = np.zeros((c.n_pts, 3, 3))
    np.add.at(d, c.pt_idx, np.einsum('mki,mkj->mij', jx, jx))
    d += lam * np.eye(3)
    deg = np.diff(c.pt_ptr)
    dinv = np.zeros_like(d)
    ok = (deg >= 2) | ((lam > 0) & (deg >= 1))
    dinv[ok] = np.linalg.inv(d[ok])
    w = np.einsum('mki,mkj->mij', jp, jx)
    blocks = np.zeros((c.n_cams, 7, 7)) + lam * np.eye(7)
    np.add.at(blocks, c.cam_idx, np.einsum('mki,mkj->mij', jp, jp) - np.einsum('mij,mjk,mlk->mil', w, dinv[c.pt_idx], w))
    out = np.zeros(c.n_cams)
    for cam in range(c.n_cams):
        a, worst = blocks[cam].copy(), np.inf
        for j in range(7):
            piv = a[j, j] - a[j, :j] @ a[j, :j]
            if not piv > 0:
                worst = 0.0
                break
            worst = min(worst, piv / blocks[cam, j, j])
            a[j, j] = np.sqrt(piv)
            for i in range(j + 1, 7):
                a[i, j] = (a[i, j] - a[i, :j] @ a[j, :j]) / a[j, j]
        out[cam] = worst
    return out


_PAIRS = {}


def both_routes(c, lam, quirks, loss, which, tol=1e-13):
    """Both routes from the case's start state, once per setting and left unchanged:
    dict(direct=(cams, pts), pcg=(cams, pts), count, status, worst_ratio, margin, disagreement, cost)."""
    k = (c.name, lam, quirks, loss, which, tol)
    if k not in _PAIRS:
        mask = free_mask(c.n_cams, which)
        dc, dpts, cost = step_direct(c, c.cams, c.pts, lam, quirks, loss, mask, key="start")
        pc, ppts, _cost, count, status, hist = step_pcg(c, c.cams, c.pts, lam, quirks, loss, mask, tol, key="start")
        ratios = [hist[i + 1] / hist[i] for i in range(len(hist) - 1) if hist[i] > 0]
        # how far the stopping rule's crossing is from the threshold, on either side (a factor >= 1)
        thr = tol * tol * hist[0]
        margin = float("inf")
        if count > 0 and thr > 0:
            margin = min(hist[count - 1] / thr, thr / hist[count] if hist[count] > 0 else float("inf"))
        for a in (dc, dpts, pc, ppts):
            a.setflags(write=False)
        _PAIRS[k] = dict(direct=(dc, dpts), pcg=(pc, ppts), count=count, status=status, cost=cost,
                         worst_ratio=max(ratios) if ratios else 0.0, margin=margin, disagreement=max(rel(pc, dc), rel(ppts, dpts)))
    return _PAIRS[k]


def tolerance(disagreement):
    """What the device may differ from ``step_direct`` by at low damping, given the disagreement of the two NumPy routes on
    the same setting: 100 x covers another summation order at that conditioning; never below the 1e-9 of the parity tests
    (the rule of tests/_cov_reference.py)."""
    return max(1e-9, 100.0 * disagreement)
