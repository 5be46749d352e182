"""Seeded cases and float64 references for the two-view initialisation (test code only).

Generators (every one takes a ``numpy.random.Generator``):

* ``two_view_scene``: a calibrated pair with different non-identity intrinsics left and right, points in front of
  both cameras, optional pixel noise, gross outliers and a (near-)planar structure;
* ``eight_point_cases``: 8-row samples of normalised pairs of the kinds ``scene`` (noise-free), ``noisy``,
  ``line`` (a planted F with a small F[2][2]), ``dup`` (one row a near-duplicate of another, offsets 1e-12 .. 1e-4),
  ``coplanar`` (points within 1e-6 .. 1e-2 of a plane) and ``repeat`` (a sample that repeats an index);
* ``essential_cases``: E = [t]x R from random (R, t), t also along each axis, some with a small E[2][2].

References return the oracle's result together with the condition numbers that bound how far a backward-stable
computation of the same thing can be from it (u = 2^-53, C = 64 for every test):

* eight point: err <= C u kW kP rho, kW = s0(W)/s7(W) of the 8x9 design matrix (null-vector angle), kP =
  1 + s0(f)/(s1(f) - s2(f)) (the rank-2 projection moves with the gap), rho = max|f2|/|f2[2][2]| (the division);
* essential: err <= C u mu kE rhoE, mu = max(|Kr|^T |F| |Kl|)/max|e| (cancellation in the product), kE as kP,
  rhoE = max|e|/|e[2][2]|;
* pose candidates: err <= C u mu kE.

err is max|got - want| / max|want|.  tests/test_twoview_oracle.py checks the float64 oracle itself against a
50-digit mpmath SVD under these bounds, so the bounds are derived, not fitted to the kernel.
"""
import numpy as np

import sfm_oracle as oracle

U = 2.0 ** -53
C = 64.0
KINDS = ("scene", "noisy", "line", "dup", "coplanar", "repeat")


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


def random_intrinsic(rng):
    f = rng.uniform(300.0, 1500.0)
    return np.array([[f, rng.uniform(-2.0, 2.0), rng.uniform(200.0, 900.0)],
                     [0.0, f * rng.uniform(0.8, 1.25), rng.uniform(150.0, 700.0)],
                     [0.0, 0.0, 1.0]])


def two_view_scene(rng, n, noise=0.0, outlier_frac=0.0, planar=None):
    """Left camera K_l [I | 0], right camera K_r [R | t].  Returns dict(left, right (3, n) homogeneous pixels,
    Kl, Kr, R, t, X (3, n), outliers (index array)).  ``planar``: points within that distance of a plane."""
    kl, kr = random_intrinsic(rng), random_intrinsic(rng)
    rot = _small_rotation(rng.uniform(-0.3, 0.3, 3))
    t = rng.normal(size=3)
    t *= rng.uniform(0.3, 2.0) / np.linalg.norm(t)
    pts = np.empty((3, 0))
    while pts.shape[1] < n:
        m = 2 * n + 16
        if planar is None:
            x = np.vstack((rng.uniform(-3, 3, m), rng.uniform(-3, 3, m), rng.uniform(4, 15, m)))
        else:
            a, b, d = rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(6, 10)
            xy = rng.uniform(-3, 3, (2, m))
            x = np.vstack((xy, a * xy[0] + b * xy[1] + d + planar * rng.normal(size=m)))
        z2 = (rot @ x + t[:, None])[2]
        pts = np.hstack((pts, x[:, z2 > 0.5]))
    pts = pts[:, :n]
    left = kl @ pts
    right = kr @ (rot @ pts + t[:, None])
    left, right = left / left[2], right / right[2]
    if noise:
        left[0:2] += rng.normal(0, noise, (2, n))
        right[0:2] += rng.normal(0, noise, (2, n))
    bad = rng.choice(n, int(round(outlier_frac * n)), replace=False) if outlier_frac else np.zeros(0, dtype=int)
    right[0:2, bad] += rng.uniform(30, 200, (2, bad.size)) * rng.choice([-1, 1], (2, bad.size))
    return dict(left=left, right=right, Kl=kl, Kr=kr, R=rot, t=t, X=pts, outliers=bad)


def _small_rotation(ang):
    a = np.linalg.norm(ang)
    k = np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]]) / max(a, 1e-300)
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * k @ k


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def _scene_pairs(rng, n, noise, planar=None):
    sc = two_view_scene(rng, n, noise=noise, planar=planar)
    pairs, _, _ = oracle.fund_normalize(sc["left"], sc["right"])
    return pairs


def _line_pairs(rng):
    """Eight normalised pairs on a planted rank-2 F0 with |F0[2][2]| = 10^-e max|F0| (e up to 5): x_r is a point
    of the epipolar line F0 x_l."""
    a = rng.normal(size=(3, 3))
    u, s, vh = np.linalg.svd(a)
    f0 = u @ np.diag([s[0], s[1], 0.0]) @ vh
    # set F0[2][2] small and re-project onto rank 2 (a few rounds settle both)
    for _ in range(4):
        f0[2, 2] = np.max(np.abs(f0)) * 10.0 ** -rng.uniform(0, 5) * rng.choice([-1, 1])
        u, s, vh = np.linalg.svd(f0)
        f0 = u @ np.diag([s[0], s[1], 0.0]) @ vh
    out = np.empty((8, 4))
    for i in range(8):
        xl = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), 1.0])
        line = f0 @ xl
        p0 = -line[2] * line[0:2] / (line[0:2] @ line[0:2])       # foot of the origin on the line
        d = np.array([-line[1], line[0]]) / np.linalg.norm(line[0:2])
        xr = p0 + d * rng.uniform(-1.5, 1.5)
        out[i] = [xl[0], xl[1], xr[0], xr[1]]
    return out


def eight_point_cases(rng, count, kinds=KINDS):
    """``count`` cases cycling over ``kinds``: dicts (kind, pairs (8, 4) normalised, sample (8,) indices into pairs,
    param).  Only ``repeat`` repeats an index."""
    out = []
    for c in range(count):
        kind = kinds[c % len(kinds)]
        sample = np.arange(8)
        param = 0.0
        if kind in ("scene", "noisy"):
            pairs = _scene_pairs(rng, 32, 0.0 if kind == "scene" else rng.uniform(0.1, 1.0))
            pairs = pairs[rng.choice(32, 8, replace=False)]
        elif kind == "line":
            pairs = _line_pairs(rng)
        elif kind == "dup":
            pairs = _scene_pairs(rng, 32, rng.uniform(0.0, 0.5))[rng.choice(32, 8, replace=False)]
            param = 10.0 ** rng.uniform(-12, -4)
            pairs[7] = pairs[rng.integers(0, 7)] + param * rng.normal(size=4)
        elif kind == "coplanar":
            param = 10.0 ** rng.uniform(-6, -2)
            pairs = _scene_pairs(rng, 32, 0.0, planar=param)[rng.choice(32, 8, replace=False)]
        elif kind == "repeat":
            pairs = _scene_pairs(rng, 32, rng.uniform(0.0, 0.5))[rng.choice(32, 8, replace=False)]
            i, j = sorted(rng.choice(8, 2, replace=False))
            sample[j] = sample[i]
            param = float(j)
        else:
            raise ValueError(kind)
        out.append(dict(kind=kind, pairs=pairs, sample=sample, param=param))
    return out


def design_matrix(p):
    """The 8x9 system of epipolar:150-160 for rows (x1, y1, x2, y2)."""
    x1, y1, x2, y2 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    return np.column_stack((x1 * x2, y1 * x2, x2, x1 * y2, y1 * y2, y2, x1, y1, np.ones(len(p))))


def eight_point_ref(pairs8):
    """(F = oracle.fund_eight_point, kW, kP, rho)."""
    f_or = oracle.fund_eight_point(pairs8)
    w = design_matrix(pairs8)
    s = np.linalg.svd(w, compute_uv=False)
    f = np.linalg.svd(w)[2][8].reshape(3, 3)
    u, sf, vh = np.linalg.svd(f)
    f2 = u @ np.diag([sf[0], sf[1], 0.0]) @ vh
    k_w = s[0] / s[7] if s[7] > 0 else np.inf
    k_p = 1.0 + sf[0] / (sf[1] - sf[2]) if sf[1] > sf[2] else np.inf
    rho = np.max(np.abs(f2)) / abs(f2[2, 2]) if f2[2, 2] != 0 else np.inf
    return f_or, k_w, k_p, rho


def eight_point_bound(k_w, k_p, rho):
    return C * U * k_w * k_p * rho


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def essential_cases(rng, count):
    """(E = [t]x R scaled by a random positive factor, R, t); t along x, y, z for the first three, and every fourth
    case has t moved so that |E[2][2]| is 1e-3 .. 1e-9 of max|E| but not 0."""
    out = []
    for c in range(count):
        rot = random_rotation(rng)
        if c < 3:
            t = np.eye(3)[c] * rng.uniform(0.5, 2.0)
        else:
            t = rng.normal(size=3)
        e = skew(t) @ rot
        if c % 4 == 3:
            # E[2][2] = (t x r_3)_2 with r_3 the third column of R: tilt t toward making it vanish, then leave a remainder
            # E[2][2] = t0 R[1][2] - t1 R[0][2] is linear in t: move t along its gradient to 10^-e max|E|
            g = np.array([rot[1, 2], -rot[0, 2], 0.0])
            t = t - (e[2, 2] / (g @ g)) * g
            t = t + 10.0 ** -rng.uniform(3, 9) * np.max(np.abs(skew(t) @ rot)) / (g @ g) * g
            e = skew(t) @ rot
        out.append((e * rng.uniform(0.2, 5.0), rot, t))
    return out


def fund_from_essential(e, kl, kr):
    """F with E = Kr^T F Kl (the relation essential_from_fundamental inverts)."""
    return np.linalg.inv(kr).T @ e @ np.linalg.inv(kl)


def essential_ref(fund, kl, kr):
    """(E = oracle.essential_from_fundamental, mu, kE, rhoE)."""
    e_or = oracle.essential_from_fundamental(fund, kl, kr)
    e = kr.T @ fund @ kl
    mu = np.max(np.abs(kr).T @ np.abs(fund) @ np.abs(kl)) / np.max(np.abs(e))
    s = np.linalg.svd(e, compute_uv=False)
    k_e = 1.0 + s[0] / (s[1] - s[2]) if s[1] > s[2] else np.inf
    rho = np.max(np.abs(e_or)) / 1.0          # e_or[2][2] == 1: max|e| / |e[2][2]| of the unit-diagonal form
    return e_or, mu, k_e, rho


def pose_ref(esse):
    """(candidate set [(R, c)] of oracle.pose_candidates, kE)."""
    r1, r2, c1, c2 = oracle.pose_candidates(esse)
    s = np.linalg.svd(esse, compute_uv=False)
    k_e = 1.0 + s[0] / (s[1] - s[2]) if s[1] > s[2] else np.inf
    return [r1, r2], c1.ravel(), k_e


def candidate_set_err(r_got, c_got, r_want, c_want):
    """Distance between {R1, R2} x {c, -c} sets: best pairing of the rotations, best sign of c (relative to max)."""
    d_r = min(max(rel_err(r_got[0], r_want[0]), rel_err(r_got[1], r_want[1])),
              max(rel_err(r_got[0], r_want[1]), rel_err(r_got[1], r_want[0])))
    d_c = min(rel_err(c_got, c_want), rel_err(c_got, -c_want))
    return max(d_r, d_c)


def epipolar_values(pairs, fs):
    """|x_r^T F_h x_l| for every hypothesis h (rows of fs (H, 3, 3)) and pair: (H, n), plus the matching
    sum_ij |x_r,i| |F_ij| |x_l,j| (the scale a rounding error in F or in the pairs is relative to)."""
    n = pairs.shape[0]
    xl = np.column_stack((pairs[:, 0:2], np.ones(n)))
    xr = np.column_stack((pairs[:, 2:4], np.ones(n)))
    val = np.abs(np.einsum("ni,hij,nj->hn", xr, fs, xl, optimize=True))
    mag = np.einsum("ni,hij,nj->hn", np.abs(xr), np.abs(fs), np.abs(xl), optimize=True)
    return val, mag
