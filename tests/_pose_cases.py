"""Seeded cases and float64 references for the linear pose stage (test code only): the DLT triangulation
(tri_linear_kernel, tri_tracks_linear_kernel: csrc/sfm_dlt.h), the six-point PnP solve (pnp_six_point_kernel) and the
reprojection test of its RANSAC (pnp_is_inlier), all of csrc/sfm_core.hip.

Generators (every one takes a ``numpy.random.Generator``):

* ``dlt_scene``: k cameras and m points seen by all of them (one projection set, as one launch of the rectangular
  kernel takes); ``dlt_cases``: single tracks with their own projections (the ragged entry), k cycling over DLT_VIEWS.
  Kinds: ``scene`` (noise-free, normalised units, baseline 1, depth 4 .. 15), ``noisy``, ``narrow`` (baseline 10^-e,
  e in 0 .. 6), ``far`` (depth 10 .. 1e3 baselines), ``pixel`` (an intrinsic with f about 1e3 in the projections: row
  entries of about 1e3 cancel to O(1)), ``dupview`` (one view repeated exactly, k >= 3, so the rank stays 3) and
  ``scaled`` (the projections, and with them the whole design matrix, times 2^j);
* ``dlt_rank2``: planted degenerate tracks, see there;
* ``six_point_cases``: six 3-D points, their homogeneous pixel keys under a common intrinsic and a sample.  Kinds:
  ``scene``, ``noisy`` (0.1 .. 1 px, and every other one a sample with outliers: 1 .. 500 px), ``coplanar`` (points within 1e-6 .. 1e-1 of a plane), ``dup`` (one point within 1e-12 .. 1e-4
  of another), ``faraway`` (|C| up to 1e3, the points around the camera), ``homog`` (key third coordinate != 1: the
  solver does not re-normalise its keys) and ``repeat`` (a sample that repeats an index);
* ``pnp_scene``: n points, their keys under a pose, optional pixel noise and gross outliers.

The range of ``scaled``.  LAPACK scales internally; dlt_null_vector does not, and its rotation test forms
sqrt(al * be) from the squared column norms al, be <= 2k max|A|^2.  The product overflows once max|A| reaches
2^256 / sqrt(2k): with pixel rows of up to 2^14 and k <= 513 that is j = 256 - 14 - 5 = 237.  Downwards the product
only underflows to 0, which makes the test pass (a rotation that was due anyway); the squared norms themselves stay
normal while (2^j s3)^2 > 2^-1022, j > -511 + log2(1/s3), about -480 for the worst s3 generated here.  The kernel is
expected to serve j in SCALED_RANGE = -400 .. 200 and only that range is generated; |j| <= 200 keeps every
intermediate normal, so there a power of two commutes with every rounding and the result is bit-identical to j = 0.

References return the NumPy result exactly as the reference computes it, with the condition numbers that bound how far a
backward-stable float64 computation of the same thing can be from it (u = 2^-53 and C = 64 of _twoview_cases.py):

* DLT (np.linalg.svd of the 2k x 4 design matrix A, the last row of V^T, divided by its W).  Forming an entry
  u P[2][j] - P[r][j] rounds twice, an error of up to 2 u (|u P[2][j]| + |P[r][j]|); call mu the largest Euclidean
  norm of a row of those magnitudes.  The 2k rows give |dA|_F <= 2 u sqrt(2k) mu, the SVD adds a backward error of a
  modest multiple of u s0.  The null vector of A + dA is within |dA| / (s2 - s3) of that of A (Wedin), and x = v / v[3]
  moves by |dv| (1 + rho) / |v[3]| with rho = max|v| / |v[3]|, which is 4 rho |dv| relative to max|x| since
  max|v| >= 1/2.  So err <= C u sqrt(2k) max(s0, mu) / (s2 - s3) rho, the constants inside C;
* six point (np.linalg.svd of the 12 x 12 matrix W, v = last row, M = the 3 x 3 left block and m4 the last column of v
  reshaped (3, 4), R = (U_M V_M^T)^T, C = R (-m4) / s0(M), R negated when det R < 0 and C kept: the device's Q13
  convention, include/sfm_hip.h).  The keys inv(K) key round with a relative error mu u, mu = max |inv(K)| |key| /
  max|inv(K) key| (below 3 here: the principal point cancels), the products with X once more: a backward error of a few
  u |W|, so |dv| <= c u kW with kW = s0(W) / (s10(W) - s11(W)) and c a small constant.  The polar factor moves by
  2 |dM| / (s1(M) + s2(M)) (R.-C. Li), and dM is dv seen against |M| = s0(M): rotation err <= C u kW kP / s0(M), kP =
  1 + 2 s0(M) / (s1(M) + s2(M)).  C = R (-m4) / s0(M) has dC / |C| <= dR + |dv| / s0(M) + |dv| / |m4|; the first two are
  inside the rotation bound (kP / s0(M) >= 3 / s0(M)), so the centre is held to the rotation bound plus its own share
  C u kW / |m4|.  mu, c and the sqrt(3) between the 2-norm and the largest entry (together below 16) are inside C = 64;
  the float64 reference needs 0.2 of u (kW kP / s0(M) + kW / |m4|) against the exact answer.  det R changes sign only where s2(M) vanishes, so a case whose
  s2(M) / s0(M) is within its rotation bound is left out like one whose bound is vacuous (>= 0.5);
* reprojection value |key - P X / (P X)[2]| of pnp_is_inlier: see ``reprojection_values``.

err is max|got - want| / max|want| (``rel_err``).  tests/test_pose_oracle.py checks the float64 references against a
50-digit mpmath SVD under these bounds, so they are derived, not fitted to the kernels.
"""
import numpy as np

from _twoview_cases import C, U, random_intrinsic, random_rotation, rel_err  # noqa: F401  (re-exported)

DLT_KINDS = ("scene", "noisy", "narrow", "far", "pixel", "dupview", "scaled")
DLT_VIEWS = (2, 3, 4, 5, 9, 33)
SCALED_RANGE = (-400, 200)
SIX_KINDS = ("scene", "noisy", "coplanar", "dup", "faraway", "homog", "repeat")


def small_rotation(ang):
    a = np.linalg.norm(ang)
    k = np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]]) / max(a, 1e-300)
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * k @ k


# ------------------------------------------------------------------------------------------------ DLT
def dlt_scene(rng, k, kind, m, param=None):
    """dict(kind, k, projs (k, 3, 4), uv (k, 2, m), X (3, m), param).  ``param``: e of ``narrow``, j of ``scaled``
    (drawn when None)."""
    base, depth, noise, kmat = 1.0, rng.uniform(4.0, 15.0), 0.0, np.eye(3)
    if kind == "noisy":
        noise = 10.0 ** rng.uniform(-4.0, -2.5)
    elif kind == "narrow":
        param = rng.uniform(0.0, 6.0) if param is None else param
        base = 10.0 ** -param
    elif kind == "far":
        param = 10.0 ** rng.uniform(1.0, 3.0) if param is None else param
        depth = param
    elif kind == "pixel":
        kmat = random_intrinsic(rng)
        noise = rng.uniform(0.0, 0.5)
    elif kind == "scaled":
        param = int(rng.integers(SCALED_RANGE[0], SCALED_RANGE[1] + 1)) if param is None else int(param)
    elif kind not in ("scene", "dupview"):
        raise ValueError(kind)
    if kind == "dupview" and k < 3:
        raise ValueError("dupview needs k >= 3")
    t = np.linspace(-0.5, 0.5, k) + rng.uniform(-0.2, 0.2, k) / k
    projs = np.empty((k, 3, 4))
    for v in range(k):
        rot = small_rotation(rng.uniform(-0.1, 0.1, 3))
        loc = base * np.array([t[v], rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
        projs[v] = kmat @ np.hstack((rot.T, (rot.T @ -loc)[:, None]))
    pts = np.vstack((rng.uniform(-0.3, 0.3, m) * depth, rng.uniform(-0.3, 0.3, m) * depth, depth * rng.uniform(1.0, 1.5, m)))
    uv = np.empty((k, 2, m))
    for v in range(k):
        s = projs[v] @ np.vstack((pts, np.ones(m)))
        uv[v] = s[0:2] / s[2] + (noise * rng.normal(size=(2, m)) if noise else 0.0)
    if kind == "dupview":
        a, b = rng.choice(k, 2, replace=False)
        projs[b], uv[b] = projs[a], uv[a]
        param = (int(a), int(b))
    if kind == "scaled":
        projs = np.ldexp(projs, param)
    return dict(kind=kind, k=k, projs=projs, uv=uv, X=pts, param=param)


def dlt_cases(rng, count, views=DLT_VIEWS, kinds=DLT_KINDS):
    """``count`` single tracks (uv (k, 2, 1)) with their own projections, cycling over ``kinds`` and then ``views``."""
    out = []
    for c in range(count):
        kind = kinds[c % len(kinds)]
        k = views[(c // len(kinds)) % len(views)]
        out.append(dlt_scene(rng, max(k, 3) if kind == "dupview" else k, kind, 1))
    return out


def dlt_rank2(kind, m=4):
    """Planted degenerate tracks with shared projections: dict(projs, uv (k, 2, m), w_zero).
    ``twin``: two identical views only, so A has two distinct rows and a two-dimensional null space.
    ``parallel``: three cameras [I | -c_v] that all see the point at the key (0, 0): the rows are (-1, 0, 0, c_x) and
    (0, -1, 0, c_y), the third column of A is exactly zero, rank 3 with the null vector (0, 0, 1, 0): the point at
    infinity, W = 0 exactly (w_zero).  The zero column stays zero through the Givens QR and takes part in no rotation.
    ``twin_parallel``: the same with two identical views: rank 2 and the null space holds a W = 0 direction."""
    rng = np.random.default_rng(77)
    if kind == "twin":
        sc = dlt_scene(rng, 2, "scene", m)
        sc["projs"][1], sc["uv"][1] = sc["projs"][0], sc["uv"][0]
        return dict(projs=sc["projs"], uv=sc["uv"], w_zero=False)
    k = 3 if kind == "parallel" else 2
    projs = np.zeros((k, 3, 4))
    for v in range(k):
        projs[v, :, 0:3] = np.eye(3)
        projs[v, :, 3] = [0.25 * v - 0.5, 0.125 * v, 0.0] if kind == "parallel" else [0.5, 0.25, 0.0]
    return dict(projs=projs, uv=np.zeros((k, 2, m)), w_zero=True)


def dlt_design(projs, uv):
    """(A (m, 2k, 4), rows u P[2] - P[0] and v P[2] - P[1] per view, and the magnitudes |u| |P[2]| + |P[r]|)."""
    k, m = projs.shape[0], uv.shape[2]
    a, mag = np.empty((m, 2 * k, 4)), np.empty((m, 2 * k, 4))
    for v in range(k):
        for r in range(2):
            a[:, 2 * v + r] = uv[v, r][:, None] * projs[v, 2] - projs[v, r]
            mag[:, 2 * v + r] = np.abs(uv[v, r])[:, None] * np.abs(projs[v, 2]) + np.abs(projs[v, r])
    return a, mag


def dlt_ref(projs, uv):
    """(x (4, m) = last row of V^T over its W, dict(kappa, rho, bound (m,), s (m, 4), v (m, 4))): kappa =
    sqrt(2k) max(s0, mu) / (s2 - s3), rho = max|v| / |v[3]|, bound = C u kappa rho (inf where a division is by 0)."""
    a, mag = dlt_design(projs, uv)
    _, s, vh = np.linalg.svd(a, full_matrices=False)
    v = vh[:, -1, :]
    mu = np.max(np.linalg.norm(mag, axis=2), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (v / v[:, 3:4]).T
        kappa = np.sqrt(a.shape[1]) * np.maximum(s[:, 0], mu) / (s[:, 2] - s[:, 3])
        rho = np.max(np.abs(v), axis=1) / np.abs(v[:, 3])
        bound = C * U * kappa * rho
    bound = np.where(np.isfinite(bound), bound, np.inf)
    return x, dict(kappa=kappa, rho=rho, bound=bound, s=s, v=v)


def rel_err_cols(got, want):
    """rel_err per column of (4, m) arrays."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.max(np.abs(got - want), axis=0) / np.max(np.abs(want), axis=0)


# ------------------------------------------------------------------------------------------------ six point
def _look_at_pose(rng, centre_norm):
    """(R, C): a camera at distance ``centre_norm`` from the origin in a random direction with a random rotation."""
    d = rng.normal(size=3)
    return random_rotation(rng), centre_norm * d / np.linalg.norm(d)


def six_point_cases(rng, count, kmat, kinds=SIX_KINDS):
    """``count`` cases cycling over ``kinds``: dict(kind, X (4, 6) homogeneous with W = 1, key (3, 6) homogeneous
    pixels under ``kmat``, sample (6,) indices into the six columns, R, C, param).  Only ``repeat`` repeats an index."""
    out = []
    for c in range(count):
        kind = kinds[c % len(kinds)]
        rot, loc = _look_at_pose(rng, 10.0 ** rng.uniform(0, 3) if kind == "faraway" else rng.uniform(0.5, 5.0))
        param, sample = 0.0, np.arange(6)
        # points in the camera frame, in front of the camera, then to the world: X = R x_c + C
        xc = np.vstack((rng.uniform(-3, 3, 6), rng.uniform(-3, 3, 6), rng.uniform(4, 15, 6)))
        contaminated = kind == "noisy" and (c // len(kinds)) % 2 == 1
        if contaminated:
            # a sample with outliers, as the RANSAC draws them: keys off by 1 .. 500 px on a compact, well-scaled scene,
            # so that the two smallest singular values of W are both far from zero and near each other
            rot, loc = _look_at_pose(rng, rng.uniform(0.2, 1.0))
            xc = np.vstack((rng.uniform(-1, 1, 6), rng.uniform(-1, 1, 6), rng.uniform(1, 2, 6)))
            param = 10.0 ** rng.uniform(0.0, 2.7)
        if kind == "coplanar":
            param = 10.0 ** rng.uniform(-6, -1)
            a, b, d = rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(6, 10)
            xc[2] = a * xc[0] + b * xc[1] + d + param * rng.normal(size=6)
        elif kind == "dup":
            param = 10.0 ** rng.uniform(-12, -4)
            xc[:, 5] = xc[:, rng.integers(0, 5)] + param * rng.normal(size=3)
        elif kind == "repeat":
            i, j = sorted(rng.choice(6, 2, replace=False))
            sample[j] = sample[i]
            param = float(j)
        pts = rot @ xc + loc[:, None]
        key = kmat @ (rot.T @ (pts - loc[:, None]))
        key = key / key[2]
        if kind == "noisy":
            param = param if contaminated else rng.uniform(0.1, 1.0)
            key[0:2] += param * rng.normal(size=(2, 6))
        if kind == "homog":
            key = key * (rng.uniform(0.3, 3.0, 6) * rng.choice([-1.0, 1.0], 6))
        out.append(dict(kind=kind, X=np.vstack((pts, np.ones(6))), key=key, sample=sample, R=rot, C=loc, param=param))
    return out


def six_point_matrix(p2d, p3d):
    """The 12 x 12 system of the six-point solve: per point the rows (p2 X^T, 0, -p0 X^T) and (0, p2 X^T, -p1 X^T), X =
    (x, y, z, 1) (the point's own W is not read), p = the key in camera coordinates."""
    w = np.zeros((12, 12))
    for i in range(6):
        xh = np.array([p3d[0, i], p3d[1, i], p3d[2, i], 1.0])
        w[2 * i, 0:4] = p2d[2, i] * xh
        w[2 * i, 8:12] = -p2d[0, i] * xh
        w[2 * i + 1, 4:8] = p2d[2, i] * xh
        w[2 * i + 1, 8:12] = -p2d[1, i] * xh
    return w


def six_point_ref(key6, x6, kmat):
    """(R, C, dict(W, kW, kP, s0M, m4, mu, cond_r, cond_c, bound_r, bound_c, det_margin)) for six homogeneous pixel keys
    (3, 6) and points (4, 6); bound_* = C u cond_*."""
    kinv = np.linalg.inv(kmat)
    p = kinv @ key6
    w = six_point_matrix(p, x6)
    _, s, vh = np.linalg.svd(w)
    cam = vh[-1].reshape(3, 4)
    uu, ss, vvh = np.linalg.svd(cam[:, 0:3])
    rot = (uu @ vvh).T
    loc = (rot @ -cam[:, 3]) / ss[0]
    if np.linalg.det(rot) < 0:
        rot = -rot                      # the device's convention (Q13): C is invariant under the sign of v and stays
    mu = float(np.max((np.abs(kinv) @ np.abs(key6)) / np.max(np.abs(p), axis=0)))
    m4 = float(np.linalg.norm(cam[:, 3]))
    with np.errstate(divide="ignore", invalid="ignore"):
        k_w = s[0] / (s[10] - s[11]) if s[10] > s[11] else np.inf
        k_p = 1.0 + 2.0 * ss[0] / (ss[1] + ss[2]) if ss[1] + ss[2] > 0 else np.inf
        cond_r = k_w * k_p / ss[0]
        cond_c = cond_r + k_w / m4
    cond_r = cond_r if np.isfinite(cond_r) else np.inf
    cond_c = cond_c if np.isfinite(cond_c) else np.inf
    return rot, loc, dict(W=w, kW=k_w, kP=k_p, s0M=ss[0], m4=m4, mu=mu, cond_r=cond_r, cond_c=cond_c,
                          bound_r=C * U * cond_r, bound_c=C * U * cond_c, det_margin=ss[2] / ss[0])


def six_point_checkable(info):
    """Whether the first-order bounds say anything: both below 0.5 and det R safely away from a sign change."""
    return bool(info["bound_c"] < 0.5 and info["det_margin"] > info["bound_r"])


def six_point_launch(cases):
    """(uv_pix (3, 6 H), X (4, 6 H), samples (H, 6)) of one launch over all cases."""
    uv = np.hstack([c["key"] for c in cases])
    x = np.hstack([c["X"] for c in cases])
    samples = np.stack([c["sample"] + 6 * i for i, c in enumerate(cases)]).astype(np.int32)
    return uv, x, samples


# ------------------------------------------------------------------------------------------------ scoring
def pose_projection(kmat, rot, loc):
    """K [R^T | -R^T C] and the magnitudes |K| [|R^T| | |R^T| |C|] its entries are rounded against."""
    rt = np.hstack((rot.T, (rot.T @ -np.asarray(loc).reshape(3))[:, None]))
    rt_mag = np.hstack((np.abs(rot.T), (np.abs(rot.T) @ np.abs(np.asarray(loc).reshape(3)))[:, None]))
    return kmat @ rt, np.abs(kmat) @ rt_mag


def reprojection_values(proj, proj_mag, uv_pix, pts_h, dproj=None):
    """(val (n,), bound (n,)): val = |key - s / s[2]| with s = P X, as pnp_is_inlier forms it, and the bound on how far a
    float64 evaluation in any order (of P as well as of s) can be from it.  s[r] carries at most 8 u m[r], m = |P|mag |X|
    (three products summed for an entry of P, four for s, each a rounding of the running magnitude); a projection that is
    itself only known to within ``dproj`` ((3, 4), absolute, see ``pose_uncertainty``) adds dproj |X|.  The quotient q[r] = s[r] / s[2] moves by
    (ds[r] + |q[r]| ds[2]) / |s[2]| plus its own rounding u |q[r]|; the difference, the squares, their sum and the root
    add u (|key| + |q|) and 3 u val.  The sum over the rows bounds the Euclidean norm's change; C = 64 covers the
    constants named here (8 + the small ones), so the returned bound is C u (...) with unit constants inside."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = proj @ pts_h
        m = proj_mag @ np.abs(pts_h)
        q = s / s[2]
        val = np.sqrt(np.sum((uv_pix - q) ** 2, axis=0))
        ds = C * U * m + (0.0 if dproj is None else dproj @ np.abs(pts_h))
        bound = np.zeros(uv_pix.shape[1])
        for r in range(3):
            bound = bound + (ds[r] + np.abs(q[r]) * ds[2]) / np.abs(s[2]) + C * U * (np.abs(uv_pix[r]) + np.abs(q[r]))
        bound = bound + C * U * val
    return val, bound


def pose_uncertainty(kmat, loc, bound_r, bound_c):
    """How far K [R^T | -R^T C] can move, entry by entry, when R is known to bound_r max|R| <= bound_r and C to bound_c
    max|C|: |d(R^T C)| <= 3 bound_r max|C| + 3 bound_c max|C| per entry (three terms, |R| <= 1)."""
    cmax = float(np.max(np.abs(loc)))
    d = np.hstack((np.full((3, 3), bound_r), np.full((3, 1), 3.0 * (bound_r + bound_c) * cmax)))
    return np.abs(kmat) @ d


def pnp_scene(rng, n, kmat, noise=0.5, outlier_frac=0.0, pose=None):
    """dict(uv (3, n) homogeneous pixels, X (4, n), R, C, outliers): n points in front of a random camera (or of ``pose``
    = (R, C))."""
    rot, loc = _look_at_pose(rng, rng.uniform(0.5, 5.0)) if pose is None else pose
    xc = np.vstack((rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(4, 15, n)))
    pts = rot @ xc + loc[:, None]
    key = kmat @ xc
    key = key / key[2]
    key[0:2] += noise * rng.normal(size=(2, n))
    bad = rng.choice(n, int(round(outlier_frac * n)), replace=False) if outlier_frac else np.zeros(0, dtype=int)
    key[0:2, bad] += rng.uniform(30, 200, (2, bad.size)) * rng.choice([-1, 1], (2, bad.size))
    return dict(uv=key, X=np.vstack((pts, np.ones(n))), R=rot, C=loc, outliers=bad)


def gap_threshold(val, bound, target):
    """The threshold nearest ``target`` that sits in a gap of the finite values wider than twice the bounds on either side
    (|v - t| > 2 b for every value), or None."""
    ok = np.isfinite(val) & np.isfinite(bound)
    o = np.argsort(val[ok], kind="stable")
    v, b = val[ok][o], bound[ok][o]
    reach_up = np.maximum.accumulate(v + 2 * b)                      # the furthest reach of the values below a gap
    reach_down = np.minimum.accumulate((v - 2 * b)[::-1])[::-1]      # and of those above it
    best = None
    for i in range(len(v) - 1):
        lo, hi = reach_up[i], reach_down[i + 1]
        if hi > lo:
            t = min(max(target, lo + 0.25 * (hi - lo)), hi - 0.25 * (hi - lo))
            if best is None or abs(t - target) < abs(best - target):
                best = t
    return best


# ------------------------------------------------------------------------------------------------ one nonlinear step
def tri_step(projs, uv, x, lam, dtype=np.longdouble):
    """One damped Gauss-Newton step of the nonlinear triangulation in ``dtype`` arithmetic: projs (k, 3, 4), uv (k, 2, m),
    x (4, m) -> (x1 (4, m), delta (3, m), A (m, 3, 3) = J^T J + lam I, beta (m,)).  e = s / s[2] - key, J = d e / d (x, y, z),
    delta = inv(A) J^T e by the adjugate (the reference calls np.linalg.inv), x1 = x - delta, W as it came.  beta =
    | |s / s[2]| + |key| |_2 over the 2k residuals: the size of the terms the residuals are the differences of."""
    p, key, xx = projs.astype(dtype), uv.astype(dtype), x.astype(dtype)
    s = np.einsum("vrc,cm->vrm", p, xx)
    iz = 1 / s[:, 2]
    e = s[:, 0:2] * iz[:, None] - key
    jac = (s[:, 2][:, None, None] * p[:, 0:2, 0:3, None] - s[:, 0:2][:, :, None] * p[:, 2, 0:3][:, None, :, None]) * (iz * iz)[:, None, None]
    a = np.einsum("vrcm,vrdm->mcd", jac, jac) + dtype(lam) * np.eye(3, dtype=dtype)
    b = np.einsum("vrcm,vrm->mc", jac, e)
    c00 = a[:, 1, 1] * a[:, 2, 2] - a[:, 2, 1] * a[:, 2, 1]
    c10 = a[:, 2, 0] * a[:, 2, 1] - a[:, 1, 0] * a[:, 2, 2]
    c20 = a[:, 1, 0] * a[:, 2, 1] - a[:, 2, 0] * a[:, 1, 1]
    c11 = a[:, 0, 0] * a[:, 2, 2] - a[:, 2, 0] * a[:, 2, 0]
    c21 = a[:, 1, 0] * a[:, 2, 0] - a[:, 0, 0] * a[:, 2, 1]
    c22 = a[:, 0, 0] * a[:, 1, 1] - a[:, 1, 0] * a[:, 1, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        det = a[:, 0, 0] * c00 + a[:, 1, 0] * c10 + a[:, 2, 0] * c20
        delta = np.stack((c00 * b[:, 0] + c10 * b[:, 1] + c20 * b[:, 2],
                          c10 * b[:, 0] + c11 * b[:, 1] + c21 * b[:, 2],
                          c20 * b[:, 0] + c21 * b[:, 1] + c22 * b[:, 2])) / det
    x1 = xx.copy()
    x1[0:3] -= delta
    beta = np.sqrt(np.sum((np.abs(s[:, 0:2] * iz[:, None]) + np.abs(key)).astype(np.float64) ** 2, axis=(0, 1)))
    return x1, delta, a, beta


def tri_step_bound(x, delta, a, beta=None):
    """(bound (m,), kappa (m,)): |x1 - x1_ref|_2 <= C u (kappa(J^T J + lam I) |delta| + |x|), kappa the 2-norm condition number
    (inf for a singular matrix); C u kappa >= 0.5 makes the bound vacuous.  The form covers the solve (a relative error u kappa
    of delta) and the subtraction.  It leaves out that e = s / s[2] - key is itself rounded relative to |s / s[2]| + |key|, not
    to |e|: from a DLT result the residuals are small, e moves by u beta and delta by u beta |inv(A) J^T|.  With damping
    |inv(A) J^T| <= 1 / (2 sqrt(lam)) and the kappa |delta| of a start that has not converged yet covers it (the issue's form
    as it stands; a float64 evaluation reaches 0.4 of it); at lam = 0 it is 1 / smin(J) = 1 / sqrt(smin(A)), the largest term
    for far points, and a plain float64 NumPy evaluation of the step then misses the shorter form
    (tests/test_pose_oracle.py).  ``beta`` adds C u beta / sqrt(smin(A)): for the undamped step only."""
    a64 = np.asarray(a, dtype=np.float64)
    kappa = np.full(a64.shape[0], np.inf)
    ok = np.all(np.isfinite(a64), axis=(1, 2))
    sv = np.linalg.svd(a64[ok], compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa[ok] = np.where(sv[:, 2] > 0, sv[:, 0] / sv[:, 2], np.inf)
        bound = C * U * (kappa * np.linalg.norm(np.asarray(delta, dtype=np.float64), axis=0)
                         + np.linalg.norm(np.asarray(x, dtype=np.float64)[0:3], axis=0))
        if beta is not None:
            smin = np.full(a64.shape[0], 0.0)
            smin[ok] = sv[:, 2]
            bound = bound + C * U * beta / np.sqrt(smin)
    return np.where(np.isfinite(bound), bound, np.inf), kappa


def _solve(a, b):
    """Gaussian elimination with partial pivoting in the arrays' own dtype (np.linalg has no longdouble)."""
    a, b = a.copy(), b.copy()
    n = a.shape[0]
    for i in range(n):
        j = i + int(np.argmax(np.abs(a[i:, i])))
        a[[i, j]], b[[i, j]] = a[[j, i]], b[[j, i]]
        for r in range(i + 1, n):
            f = a[r, i] / a[i, i]
            a[r, i:] -= f * a[i, i:]
            b[r] -= f * b[i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - a[i, i + 1:] @ x[i + 1:]) / a[i, i]
    return x


def pnp_step(key, pts_h, kmat, rot0, loc0, lam, dtype=np.longdouble):
    """One damped Gauss-Newton step of the nonlinear PnP as the reference takes it (quirks Q1 and Q2 of include/sfm_hip.h:
    the effective rows are the u-row of every point and the v-row of the last one; the v-row of d/dC carries the
    reference's sign), in ``dtype`` arithmetic: (R (3, 3), C (3,), delta (7,), A (7, 7) = J^T J + lam I, x (7,) = (C0, q0)).
    The parameters are (C, q); q0 comes from R0 and is normalised, the step is added, q normalised again, R = R(q)."""
    one = dtype(1)
    r, c = np.asarray(rot0).astype(dtype), np.asarray(loc0).reshape(3).astype(dtype)
    qw = np.sqrt(one + r[0, 0] + r[1, 1] + r[2, 2]) / 2
    q = np.array([qw, (r[2, 1] - r[1, 2]) / (4 * qw), (r[0, 2] - r[2, 0]) / (4 * qw), (r[1, 0] - r[0, 1]) / (4 * qw)])
    x = np.concatenate((c, q / np.sqrt(np.sum(q * q))))
    w, xq, yq, zq = q                                           # the Jacobian is taken at the quaternion re-derived from R
    jq = 2 * np.array([[0, 0, -2 * yq, -2 * zq], [-zq, yq, xq, -w], [yq, zq, w, xq], [zq, yq, xq, w], [0, -2 * xq, 0, -2 * zq],
                       [-xq, -w, zq, yq], [-yq, zq, -w, xq], [xq, w, zq, yq], [0, -2 * xq, -2 * yq, 0]], dtype=dtype)
    pts = np.asarray(pts_h).astype(dtype)
    d = pts[0:3] - c[:, None]
    p = np.hstack((r.T, (r.T @ -c)[:, None])) @ pts
    n = pts.shape[1]
    jr = np.zeros((n, 2, 9), dtype=dtype)
    jc = np.zeros((n, 2, 3), dtype=dtype)
    for i in range(3):
        jr[:, 0, 3 * i], jr[:, 0, 3 * i + 2] = p[2] * d[i], -p[0] * d[i]
        jr[:, 1, 3 * i + 1], jr[:, 1, 3 * i + 2] = p[2] * d[i], -p[1] * d[i]
        jc[:, 0, i] = p[2] * -r[i, 0] - p[0] * -r[i, 2]
        jc[:, 1, i] = p[2] * -r[i, 1] - p[1] * r[i, 2]
    jac = np.concatenate((jc, jr @ jq), axis=2) / (p[2] * p[2])[:, None, None]
    mcam = np.linalg.inv(np.asarray(kmat, dtype=np.float64)).astype(dtype) @ np.asarray(key).astype(dtype)
    err = (mcam / mcam[2] - p / p[2])[0:2].T                   # (n, 2)
    rows = np.vstack((jac[:, 0], jac[-1:, 1]))
    rhs = np.concatenate((err[:, 0], err[-1:, 1]))
    a = rows.T @ rows + dtype(lam) * np.eye(7, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = _solve(a, rows.T @ rhs)
    x1 = x + delta
    qn = x1[3:7] / np.sqrt(np.sum(x1[3:7] * x1[3:7]))
    w, xq, yq, zq = qn
    rot = np.array([[1 - 2 * zq * zq - 2 * yq * yq, -2 * zq * w + 2 * yq * xq, 2 * yq * w + 2 * zq * xq],
                    [2 * xq * yq + 2 * w * zq, 1 - 2 * zq * zq - 2 * xq * xq, 2 * zq * yq - 2 * xq * w],
                    [2 * xq * zq - 2 * w * yq, 2 * yq * zq + 2 * w * xq, 1 - 2 * yq * yq - 2 * xq * xq]], dtype=dtype)
    return rot, x1[0:3], delta, a, x


PNP_STEP_SCENES = (("plain", 3.0, 300, None), ("faraway", 300.0, 300, None), ("coplanar", 3.0, 300, 1e-3),
                   ("two_per_thread", 3.0, 1100, None), ("split", 3.0, 3500, None))


def pnp_step_scenes(rng, kmat):
    """(name, uv (3, n), X (4, n), R0, C0) per entry of PNP_STEP_SCENES (name, |C|, n, distance from a plane): a noisy view
    (0.5 px) and the float64 six-point pose of its first six points, which is what the nonlinear kernel is started from.
    The point counts take the three size classes of pnp_nonlinear_kernel (up to 1 024, above, split from 3 000)."""
    for name, dist, n, planar in PNP_STEP_SCENES:
        d = rng.normal(size=3)
        sc = pnp_scene(rng, n, kmat, noise=0.5, pose=(small_rotation(rng.uniform(-0.5, 0.5, 3)), dist * d / np.linalg.norm(d)))
        if planar:
            xc = sc["R"].T @ (sc["X"][0:3] - sc["C"][:, None])
            xc[2] = 0.2 * xc[0] - 0.1 * xc[1] + 8.0 + planar * rng.normal(size=n)
            sc["X"][0:3] = sc["R"] @ xc + sc["C"][:, None]
            key = kmat @ xc
            sc["uv"] = key / key[2]
            sc["uv"][0:2] += 0.5 * rng.normal(size=(2, n))
        rot0, loc0, _ = six_point_ref(sc["uv"][:, 0:6], sc["X"][:, 0:6], kmat)
        yield name, sc["uv"], sc["X"], rot0, loc0


def pnp_step_bound(x, delta, a):
    """(bound, kappa): the parameter vector after the step is within C u (kappa(J^T J + lam I) |delta| + |x|) (2-norms, x the
    seven parameters).  The centre is three of them; the rotation is quadratic in the unit quaternion, |dR|max <= 4 |dq|."""
    a64 = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a64)) or not np.all(np.isfinite(np.asarray(delta, dtype=np.float64))):
        return np.inf, np.inf
    sv = np.linalg.svd(a64, compute_uv=False)
    kappa = sv[0] / sv[-1] if sv[-1] > 0 else np.inf
    return C * U * (kappa * float(np.linalg.norm(np.asarray(delta, dtype=np.float64))) + float(np.linalg.norm(np.asarray(x, dtype=np.float64)))), kappa


def six_point_null_residual(w, rot, loc):
    """For a pose (R, C) the solver returned from a W whose null space has more than one dimension: the polar factor
    dropped the symmetric factor H of M = R^T H, so the returned pose fixes the null vector only up to H (6 numbers) and the
    scale s of the last column -s R^T C.  Those p(H, s) form a 7-dimensional subspace of R^12 that a generic (wrong) pose's
    misses the null space of W with (7 + 2 < 12).  Returns (min |W p| / (|p| s0(W)) over the subspace, kP = 1 + 2 s0(H) /
    (s1(H) + s2(H)) of the minimiser's H)."""
    rt = np.asarray(rot).T
    cols = []
    for i in range(3):
        for j in range(i, 3):
            h = np.zeros((3, 3))
            h[i, j] = h[j, i] = 1.0
            cols.append(np.hstack((rt @ h, np.zeros((3, 1)))).ravel())
    cols.append(np.hstack((np.zeros((3, 3)), (-rt @ np.asarray(loc).reshape(3))[:, None])).ravel())
    q, r = np.linalg.qr(np.array(cols).T)
    _, sv, vh = np.linalg.svd(w @ q)
    coef = np.linalg.solve(r, vh[-1])
    h = np.array([[coef[0], coef[1], coef[2]], [coef[1], coef[3], coef[4]], [coef[2], coef[4], coef[5]]])
    sh = np.linalg.svd(h, compute_uv=False)
    k_p = 1.0 + 2.0 * sh[0] / (sh[1] + sh[2]) if sh[1] + sh[2] > 0 else np.inf
    return sv[-1] / np.linalg.svd(w, compute_uv=False)[0], k_p
