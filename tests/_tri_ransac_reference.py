"""NumPy float64 reference of the robust triangulation of ragged tracks (include/sfm_hip.h, block "robust triangulation"):
the rule literally -- pair numbering, inhomogeneous pair solve, angle gate, pair gate, lexicographic score, refit over the
winner's inliers, acceptance -- plus a SETTLED flag per point and the scenes the tests share.

A point is settled when the winner and the final mask are the same at max_err2 (1 - 1e-6), max_err2 and
max_err2 (1 + 1e-6), and the winner's cosine is more than 1e-9 below that of the best equal-count rival: its decisions
then do not hang on the last bits of a residual, so another correct implementation has to reproduce them exactly.
"""
from types import SimpleNamespace

import numpy as np

TOO_FEW, NO_MODEL, KEPT_HYPOTHESIS, SAMPLED = 1, 2, 4, 8
DEFAULT_HYP, MAX_HYP = 128, 65536
GROUPS = (0, 1, 4, 8, 16, 32, 64)
SETTLE_REL, SETTLE_COS = 1e-6, 1e-9

# the generator's constants (the issue's prototype): arc radius, cube edge, focal length, noise, displaced share and range
RADIUS, CUBE, FOCAL, NOISE_PX, BAD_SHARE, BAD_PX = 6.0, 3.0, 800.0, 0.5, 0.10, (30.0, 120.0)
# the thresholds every test uses
MAX_PX, MIN_ANGLE_DEG = 4.0, 1.5
MAX_ERR2 = MAX_PX ** 2
COS_MIN = float(np.cos(np.radians(MIN_ANGLE_DEG)))
# seeds of the three prototype scenes (n_views, n_pts, visibility) and of the GPU test's scene of track lengths
PROTOTYPE_SCENES = ((6, 300, 0.7, 101), (10, 300, 0.5, 102), (24, 200, 0.8, 103))
PATHS_SEED = 104
PATHS_LENGTHS = (0, 1, 2, 3, 7, 16, 17, 24, 25, 48, 49, 96, 97, 192, 193, 384, 385, 700)


# ---- the numbering of the hypotheses -----------------------------------------------------------------------------------
def hypothesis_count(n, max_hyp=DEFAULT_HYP):
    max_hyp = max_hyp or DEFAULT_HYP
    return 0 if n < 2 else min(n * (n - 1) // 2, max_hyp)


def pair_numbers(n, max_hyp=DEFAULT_HYP):
    """Pair number k of every hypothesis h of a track of n observations (Python integers: no overflow)."""
    max_hyp = max_hyp or DEFAULT_HYP
    n = int(n)
    total = n * (n - 1) // 2
    if total <= max_hyp:
        return list(range(total))
    return [h * total // max_hyp for h in range(max_hyp)]


def pairs_of(n, ks):
    """(i, j), i < j, of the pairs numbered ks in lexicographic order: r (2 n - r - 1) / 2 pairs precede row r."""
    n = int(n)
    rows = np.arange(n - 1, dtype=np.int64)
    offsets = rows * (2 * n - rows - 1) // 2
    ks = np.asarray(ks, dtype=np.int64)
    i = np.searchsorted(offsets, ks, side="right") - 1
    j = i + 1 + (ks - offsets[i])
    return i, j


def hypothesis_pairs(n, max_hyp=DEFAULT_HYP):
    return pairs_of(n, pair_numbers(n, max_hyp))


# ---- the arithmetic ----------------------------------------------------------------------------------------------------
def _solve3(N, g):
    """X = N^-1 g by the adjugate, batched over the leading axis; ok = finite, non-zero determinant and finite X."""
    a00, a10, a11, a20, a21, a22 = N[:, 0, 0], N[:, 1, 0], N[:, 1, 1], N[:, 2, 0], N[:, 2, 1], N[:, 2, 2]
    c00 = a11 * a22 - a21 * a21
    c10 = a20 * a21 - a10 * a22
    c20 = a10 * a21 - a20 * a11
    c11 = a00 * a22 - a20 * a20
    c21 = a10 * a20 - a00 * a21
    c22 = a00 * a11 - a10 * a10
    det = a00 * c00 + a10 * c10 + a20 * c20
    with np.errstate(all="ignore"):
        x = np.stack((c00 * g[:, 0] + c10 * g[:, 1] + c20 * g[:, 2],
                      c10 * g[:, 0] + c11 * g[:, 1] + c21 * g[:, 2],
                      c20 * g[:, 0] + c21 * g[:, 1] + c22 * g[:, 2]), axis=1) / det[:, None]
    ok = np.isfinite(det) & (det != 0.0) & np.all(np.isfinite(x), axis=1)
    return x, ok


def _rows(P, u, v):
    """The rows a = u p3 - p1, a = v p3 - p2 of every observation: (n, 2, 4)."""
    return np.stack((u[:, None] * P[:, 2, :] - P[:, 0, :], v[:, None] * P[:, 2, :] - P[:, 1, :]), axis=1)


def _err2(P, u, v, scale, X):
    """err2 (H, n) and s2 (H, n) of the points X (H, 3) in the observations of the track."""
    s = np.einsum("nrc,hc->hnr", P[:, :, 0:3], X) + P[None, :, :, 3]
    with np.errstate(all="ignore"):
        e = (scale ** 2)[None, :] * ((s[:, :, 0] / s[:, :, 2] - u[None, :]) ** 2 + (s[:, :, 1] / s[:, :, 2] - v[None, :]) ** 2)
    return e, s[:, :, 2]


def _inliers(e, s2, max_err2):
    with np.errstate(all="ignore"):
        return (s2 > 0.0) & np.isfinite(e) & (e <= max_err2)


def _refit(P, u, v, A, mask, lam, iters):
    """Step 6: the inhomogeneous solve over the masked observations, then `iters` damped Gauss-Newton steps."""
    a = A[mask].reshape(-1, 4)
    N = np.einsum("ri,rj->ij", a[:, 0:3], a[:, 0:3])[None]
    g = -np.einsum("r,ri->i", a[:, 3], a[:, 0:3])[None]
    x, ok = _solve3(N, g)
    if not ok[0]:
        return None
    x = x[0]
    Pm, um, vm = P[mask], u[mask], v[mask]
    for _ in range(iters):
        s = Pm[:, :, 0:3] @ x + Pm[:, :, 3]
        with np.errstate(all="ignore"):
            iz2 = 1.0 / (s[:, 2] * s[:, 2])
            ju = (s[:, 2, None] * Pm[:, 0, 0:3] - s[:, 0, None] * Pm[:, 2, 0:3]) * iz2[:, None]
            jv = (s[:, 2, None] * Pm[:, 1, 0:3] - s[:, 1, None] * Pm[:, 2, 0:3]) * iz2[:, None]
            eu, ev = s[:, 0] / s[:, 2] - um, s[:, 1] / s[:, 2] - vm
        N = (ju.T @ ju + jv.T @ jv + lam * np.eye(3))[None]
        b = (ju.T @ eu + jv.T @ ev)[None]
        d, ok = _solve3(N, b)
        if not ok[0]:
            return None
        x = x - d[0]
    return x if np.all(np.isfinite(x)) else None


def _decide(P, u, v, scale, A, X, base_valid, cs, i, j, e, s2, max_err2, cos_min, lam, iters, cache):
    """Steps 3 to 6 at one threshold: (best_hyp, x (3,), mask (n,), kept, margin of the winner's cosine)."""
    inl = _inliers(e, s2, max_err2)
    h_idx = np.arange(X.shape[0])
    valid = base_valid & np.isfinite(cs)
    if cos_min < 1.0:
        with np.errstate(all="ignore"):
            valid &= ~(cs > cos_min)
    valid &= inl[h_idx, i] & inl[h_idx, j]
    if not valid.any():
        return -1, None, None, False, np.inf
    count = np.where(valid, inl.sum(axis=1), -1)
    top = np.flatnonzero(count == count.max())
    order = top[np.lexsort((top, cs[top]))]           # the smaller cosine, then the lower h
    best = int(order[0])
    margin = float(cs[order[1]] - cs[best]) if order.size > 1 else np.inf
    mask = inl[best]
    key = mask.tobytes()
    if key not in cache:
        cache[key] = _refit(P, u, v, A, mask, lam, iters)
    x = cache[key]
    if x is not None:
        e1, s1 = _err2(P, u, v, scale, x[None])
        m1 = _inliers(e1, s1, max_err2)[0]
        if m1.sum() >= mask.sum():
            return best, x, m1, False, margin
    return best, X[best].copy(), mask.copy(), True, margin


def solve_track(P, u, v, scale, C, max_err2=MAX_ERR2, cos_min=COS_MIN, max_hyp=DEFAULT_HYP, lam=0.5, iters=3):
    """One track: P (n, 3, 4), u, v, scale (n,), C (n, 3) of its observations' cameras.  Returns a namespace with x (3,) or
    None (the point keeps its input), mask (n,) bool, n_inliers, best_hyp, status, settled."""
    max_hyp = max_hyp or DEFAULT_HYP
    n = u.shape[0]
    out = SimpleNamespace(x=None, mask=np.zeros(n, dtype=bool), n_inliers=0, best_hyp=-1, status=0, settled=True)
    if n < 2:
        out.status = TOO_FEW
        return out
    if n * (n - 1) // 2 > max_hyp:
        out.status |= SAMPLED
    i, j = hypothesis_pairs(n, max_hyp)
    A = _rows(P, u, v)
    a = np.concatenate((A[i], A[j]), axis=1)                                      # (H, 4, 4): u_i, v_i, u_j, v_j
    N = np.einsum("hri,hrj->hij", a[:, :, 0:3], a[:, :, 0:3])
    g = -np.einsum("hr,hri->hi", a[:, :, 3], a[:, :, 0:3])
    X, base_valid = _solve3(N, g)
    X = np.where(base_valid[:, None], X, 0.0)
    with np.errstate(all="ignore"):
        ri, rj = C[i] - X, C[j] - X
        cs = np.einsum("hc,hc->h", ri / np.linalg.norm(ri, axis=1)[:, None], rj / np.linalg.norm(rj, axis=1)[:, None])
    e, s2 = _err2(P, u, v, scale, X)
    cache = {}
    runs = [_decide(P, u, v, scale, A, X, base_valid, cs, i, j, e, s2, t, cos_min, lam, iters, cache)
            for t in (max_err2, max_err2 * (1.0 - SETTLE_REL), max_err2 * (1.0 + SETTLE_REL))]
    best, x, mask, kept, margin = runs[0]
    out.settled = all(r[0] == best and (best < 0 or (np.array_equal(r[2], mask) and r[3] == kept)) for r in runs[1:]) \
        and (best < 0 or margin > SETTLE_COS)
    if best < 0:
        out.status |= NO_MODEL
        return out
    out.x, out.mask, out.n_inliers, out.best_hyp = x, mask, int(mask.sum()), best
    if kept:
        out.status |= KEPT_HYPOTHESIS
    return out


def centres_of(projs):
    """C = -M^-1 p4 of projs (V, 3, 4) = [M | p4]."""
    return -np.linalg.solve(projs[:, :, 0:3], projs[:, :, 3:4])[:, :, 0]


def solve_tracks(pt_ptr, cam_idx, uv, projs, cam_scale=None, x_init=None, max_err2=MAX_ERR2, cos_min=COS_MIN, max_hyp=DEFAULT_HYP,
                 lam=0.5, iters=3, centres=None):
    """The whole call: X (4, n_pts), inlier (M,) uint8, n_inliers, best_hyp, status, summary (6,) int64, settled (n_pts,)."""
    pt_ptr = np.asarray(pt_ptr, dtype=np.int64)
    n_pts, m = pt_ptr.shape[0] - 1, cam_idx.shape[0]
    scale_all = np.ones(projs.shape[0]) if cam_scale is None else np.asarray(cam_scale, dtype=np.float64)
    centres = centres_of(projs) if centres is None else centres
    X = np.tile(np.array([[0.0], [0.0], [0.0], [1.0]]), (1, n_pts)) if x_init is None else np.array(x_init, dtype=np.float64)
    inlier = np.zeros(m, dtype=np.uint8)
    n_in = np.zeros(n_pts, dtype=np.int32); best = np.full(n_pts, -1, dtype=np.int32); status = np.zeros(n_pts, dtype=np.int32)
    settled = np.ones(n_pts, dtype=bool)
    summary = np.zeros(6, dtype=np.int64)
    for p in range(n_pts):
        lo, hi = pt_ptr[p], pt_ptr[p + 1]
        c = cam_idx[lo:hi]
        r = solve_track(projs[c], uv[0, lo:hi], uv[1, lo:hi], scale_all[c], centres[c], max_err2, cos_min, max_hyp, lam, iters)
        status[p], settled[p] = r.status, r.settled
        if r.x is None:
            summary[2 if r.status & TOO_FEW else 1] += 1
            continue
        X[0:3, p], X[3, p] = r.x, 1.0
        inlier[lo:hi] = r.mask
        n_in[p], best[p] = r.n_inliers, r.best_hyp
        summary[0] += 1
        summary[3] += bool(r.status & KEPT_HYPOTHESIS)
        summary[4] += r.n_inliers
        summary[5] += (hi - lo) - r.n_inliers
    return SimpleNamespace(X=X, inlier=inlier, n_inliers=n_in, best_hyp=best, status=status, summary=summary, settled=settled)


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _cameras(n_views, span_deg):
    """Cameras on an arc of radius RADIUS in the x-z plane, looking at the origin: rots (V, 3, 3) camera-to-world, centres."""
    ang = np.radians(np.linspace(-span_deg / 2.0, span_deg / 2.0, n_views))
    C = RADIUS * np.stack((np.sin(ang), np.zeros(n_views), -np.cos(ang)), axis=1)
    z = -C / np.linalg.norm(C, axis=1)[:, None]
    x = np.cross(np.array([0.0, 1.0, 0.0])[None, :], z)
    x /= np.linalg.norm(x, axis=1)[:, None]
    y = np.cross(z, x)
    return np.stack((x, y, z), axis=2), C


def _finish(rots, C, pts, pt_ptr, cam_idx, rng, displaced):
    """Observations of the given structure: normalised keys with NOISE_PX of noise, `displaced` ones moved by BAD_PX."""
    projs = np.concatenate((np.transpose(rots, (0, 2, 1)), -np.einsum("vji,vj->vi", rots, C)[:, :, None]), axis=2)
    pt_idx = np.repeat(np.arange(pts.shape[1]), np.diff(pt_ptr))
    s = np.einsum("mrc,mc->mr", projs[cam_idx][:, :, 0:3], pts[:, pt_idx].T) + projs[cam_idx][:, :, 3]
    pix = FOCAL * s[:, 0:2] / s[:, 2:3] + NOISE_PX * rng.standard_normal((cam_idx.shape[0], 2))
    shift = rng.uniform(BAD_PX[0], BAD_PX[1], cam_idx.shape[0])
    phi = rng.uniform(0.0, 2.0 * np.pi, cam_idx.shape[0])
    pix[displaced] += (shift[:, None] * np.stack((np.cos(phi), np.sin(phi)), axis=1))[displaced]
    return SimpleNamespace(n_views=rots.shape[0], n_pts=pts.shape[1], rots=rots, centres=C, projs=projs, pts_true=pts,
                           pt_ptr=pt_ptr.astype(np.int32), cam_idx=cam_idx.astype(np.int32), pt_idx=pt_idx,
                           uv=np.ascontiguousarray((pix / FOCAL).T), cam_scale=np.full(rots.shape[0], FOCAL),
                           displaced=displaced, lengths=np.diff(pt_ptr))


def make_scene(n_views, n_pts, visibility, seed, span_deg=120.0):
    """The issue's generator: Bernoulli visibility, BAD_SHARE of the observations displaced."""
    rng = np.random.default_rng(seed)
    rots, C = _cameras(n_views, span_deg)
    pts = rng.uniform(-CUBE / 2.0, CUBE / 2.0, (3, n_pts))
    seen = rng.random((n_pts, n_views)) < visibility
    pt_ptr = np.concatenate(([0], np.cumsum(seen.sum(axis=1))))
    cam_idx = np.nonzero(seen)[1]
    displaced = rng.random(cam_idx.shape[0]) < BAD_SHARE
    return _finish(rots, C, pts, pt_ptr, cam_idx, rng, displaced)


def make_paths_scene(seed=PATHS_SEED, n_views=700, extra=40):
    """Tracks of the lengths at which the kernels take another path (PATHS_LENGTHS), two of each where short, and `extra`
    tracks of 2 to 12 observations; views on a 330 degree arc.  The track of 3 has exactly one displaced observation."""
    rng = np.random.default_rng(seed)
    rots, C = _cameras(n_views, 330.0)
    lengths = [n for n in PATHS_LENGTHS for _ in range(2 if n < 100 else 1)] + list(rng.integers(2, 13, extra))
    lengths = np.array(lengths)[rng.permutation(len(lengths))]
    pts = rng.uniform(-CUBE / 2.0, CUBE / 2.0, (3, lengths.shape[0]))
    pt_ptr = np.concatenate(([0], np.cumsum(lengths)))
    cam_idx = np.concatenate([np.sort(rng.choice(n_views, n, replace=False)) for n in lengths] + [np.zeros(0, dtype=np.int64)])
    displaced = rng.random(cam_idx.shape[0]) < BAD_SHARE
    for p in np.flatnonzero(lengths == 3):
        displaced[pt_ptr[p]:pt_ptr[p + 1]] = [False, True, False]
    return _finish(rots, C, pts, pt_ptr, cam_idx.astype(np.int64), rng, displaced)


_CACHE = {}


def scene_and_reference(name):
    """A scene by name ("proto0" .. "proto2", "paths") and its reference at the tests' thresholds, computed once."""
    if name not in _CACHE:
        sc = make_paths_scene() if name == "paths" else make_scene(*PROTOTYPE_SCENES[int(name[-1])])
        _CACHE[name] = (sc, solve_tracks(sc.pt_ptr, sc.cam_idx, sc.uv, sc.projs, sc.cam_scale))
    return _CACHE[name]
