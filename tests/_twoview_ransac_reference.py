"""The rule of the robust two-view geometry (include/sfm_hip.h, block "robust two-view geometry") in NumPy float64, with
a SETTLED flag per set, and the scenes the tests use.

Every null-vector problem is solved by two routes (``eigh`` of A^T A, and ``svd`` of the zero-padded design matrix) and every
decision is taken at ``max_err2 (1 -+ 1e-6)`` as well as at ``max_err2``: a set is settled iff all six runs agree on status,
winner, number of refit rounds that stood and final mask.  ``d_G`` is the largest difference between the six final matrices in
the G measure: ``G = S F S / |S F S|`` with ``S = diag(c, c, 1)``, ``c`` the RMS coordinate magnitude of the set's matches in
both images, the sign fixed as the rule fixes it.  (Entry-wise on F itself the quadratic-term entries, of order 1 / c^2,
would go unchecked.)

The scenes: ``CASES`` (the prototype scenes, every set size and max_hyp on one geometry, the degenerate sets) and, from
``two_views``, ``GEOMETRY_CASES`` (eight families of geometry at three thresholds and 0, 1, 2 and 5 refit rounds) and
``PATH_CASES`` (ties at the largest count, 259 sets in one call, non-finite coordinates)."""
import functools
from types import SimpleNamespace

import numpy as np

TOO_FEW, NO_MODEL, KEPT_HYPOTHESIS = 1, 2, 4
MIN_MATCHES, MIN_COUNT = 9, 9
HYP_DEFAULT, HYP_MAX = 128, 65536
MAX_ERR2, ITERS = 4.0, 2              # 2 px; what every test uses unless it says otherwise
EPS = 2.220446049250313e-16
_M64 = (1 << 64) - 1


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def mix(z):
    """The splitmix64 finaliser on Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _mix_array(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def hypothesis_count(n, max_hyp):
    if max_hyp == 0:
        max_hyp = HYP_DEFAULT
    return max_hyp if n >= MIN_MATCHES and 1 <= max_hyp <= HYP_MAX else 0


def sample_indices(n, H):
    """(H, 8) int64: the matches of hypotheses 0 .. H - 1 of a set of n >= 9 matches."""
    k = np.arange(8, dtype=np.int64)
    lo, hi = k * n // 8, (k + 1) * n // 8
    z = _mix_array((8 * np.arange(H, dtype=np.uint64)[:, None] + k.astype(np.uint64)[None, :]))
    return lo[None, :] + (z % (hi - lo).astype(np.uint64)[None, :]).astype(np.int64)


# ---- the pieces of the rule ------------------------------------------------------------------------------------------------
def hartley(p):
    """T = [s 0 -s mx; 0 s -s my; 0 0 1] of the points p (2, m): centroid, s = sqrt(2) / mean distance."""
    with np.errstate(all="ignore"):
        m = p.mean(axis=1)
        d = np.sqrt(((p - m[:, None]) ** 2).sum(axis=0)).mean()
        s = np.sqrt(2.0) / d
        return np.array([[s, 0, -m[0] * s], [0, s, -m[1] * s], [0, 0, 1.0]])


def _apply(T, p):
    return T[0, 0] * p + T[0:2, 2:3]


def design(ln, rn):
    """Design rows of normalised matches: ln, rn (..., 2, m) -> (..., m, 9)."""
    x1, y1, x2, y2 = ln[..., 0, :], ln[..., 1, :], rn[..., 0, :], rn[..., 1, :]
    return np.stack((x1 * x2, y1 * x2, x2, x1 * y2, y1 * y2, y2, x1, y1, np.ones_like(x1)), axis=-1)


def null_vectors(A, route):
    """(..., 9): the right singular vector of the smallest singular value of A (..., m, 9), by either route."""
    if route == 0:
        return np.linalg.eigh(np.swapaxes(A, -1, -2) @ A)[1][..., :, 0]
    if A.shape[-2] < 9:
        pad = np.zeros(A.shape[:-2] + (9 - A.shape[-2], 9))
        A = np.concatenate((A, pad), axis=-2)
    return np.linalg.svd(A)[2][..., -1, :]


def project(f):
    """Rank-2 projection of f (..., 3, 3) and its validity (matrix_rank's test on the two kept singular values)."""
    u, s, vt = np.linalg.svd(f)
    ok = np.isfinite(s).all(axis=-1) & (s[..., 1] > s[..., 0] * 3.0 * EPS)
    s = s.copy()
    s[..., 2] = 0.0
    return (u * s[..., None, :]) @ vt, ok


def canon(F):
    """F (..., 3, 3) at Frobenius norm 1, the entry of largest magnitude (the first of them) positive; and validity."""
    with np.errstate(all="ignore"):
        flat = F.reshape(F.shape[:-2] + (9,))
        nrm = np.sqrt((flat * flat).sum(axis=-1))
        ok = np.isfinite(nrm) & (nrm > 0)
        safe = np.where(ok[..., None], flat, 1.0)
        k = np.argmax(np.abs(safe), axis=-1)
        sign = np.where(np.take_along_axis(safe, k[..., None], axis=-1)[..., 0] < 0, -1.0, 1.0)
        out = flat / (sign * nrm)[..., None]
    return out.reshape(F.shape), ok


def sampson(F, l, r):
    """Squared Sampson distances of the matches l, r (2, n) against F (..., 3, 3): (..., n)."""
    with np.errstate(all="ignore"):
        one = np.ones((1, l.shape[1]))
        L, R = np.vstack((l, one)), np.vstack((r, one))
        a = F @ L
        b = np.swapaxes(F, -1, -2) @ R
        e = (R * a).sum(axis=-2)
        return e * e / (a[..., 0, :] ** 2 + a[..., 1, :] ** 2 + b[..., 0, :] ** 2 + b[..., 1, :] ** 2)


def inliers(d2, max_err2):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d2) & (d2 <= max_err2)


def fit(l, r, route):
    """The matrix of the matches l, r (2, m) in pixel coordinates (steps 3 and 5 over exactly these matches), and validity."""
    Tl, Tr = hartley(l), hartley(r)
    if not (np.isfinite(Tl).all() and np.isfinite(Tr).all()):
        return np.zeros((3, 3)), False
    f2, ok = project(null_vectors(design(_apply(Tl, l), _apply(Tr, r)), route).reshape(3, 3))
    F, ok2 = canon(Tr.T @ f2 @ Tl)
    return F, bool(ok and ok2)


def _hypotheses(l, r, H, route):
    """Steps 3 to 5 of one set: (idx (H, 8), F (H, 3, 3), valid (H,), d2 (H, n)); None without a finite normalisation."""
    n = l.shape[1]
    Tl, Tr = hartley(l), hartley(r)
    if not (np.isfinite(Tl).all() and np.isfinite(Tr).all()):
        return None
    ln, rn = _apply(Tl, l), _apply(Tr, r)
    idx = sample_indices(n, H)
    A = design(np.swapaxes(ln[:, idx], 0, 1), np.swapaxes(rn[:, idx], 0, 1))      # (H, 8, 9)
    f2, ok = project(null_vectors(A, route).reshape(H, 3, 3))
    F, ok2 = canon(Tr.T @ f2 @ Tl)
    F = np.where((ok & ok2)[:, None, None], F, 0.0)
    return idx, F, ok & ok2, sampson(F, l, r)


def _counts(hyp, max_err2):
    """Step 6: the inlier count of every hypothesis, -1 where it is not valid (its matrix, or the sample gate)."""
    idx, _Fh, valid, d2 = hyp
    ok = inliers(d2, max_err2)
    valid = valid & np.take_along_axis(ok, idx, axis=1).all(axis=1)               # the sample gate
    return np.where(valid, ok.sum(axis=1), -1)


def hypothesis_counts(l, r, max_err2, max_hyp, route=0):
    """What the pick sees of one set of n >= 9 matches: (H,) counts, -1 for a hypothesis that is not valid."""
    H = hypothesis_count(l.shape[1], max_hyp)
    hyp = _hypotheses(l, r, H, route)
    return np.full(H, -1) if hyp is None else _counts(hyp, max_err2)


def _run(l, r, hyp, max_err2, iters, route):
    """Steps 6 to 9 of one set at one threshold: (status, best_hyp, stood, mask, F)."""
    n = l.shape[1]
    none = (NO_MODEL, -1, 0, np.zeros(n, dtype=bool), np.zeros((3, 3)))
    if hyp is None:
        return none
    Fh = hyp[1]
    counts = _counts(hyp, max_err2)
    best = int(np.argmax(counts))                                                 # the first of the largest counts
    if counts[best] < MIN_COUNT:
        return none
    F, standing, stood = Fh[best], int(counts[best]), 0
    for _ in range(iters):
        m = inliers(sampson(F, l, r), max_err2)
        G, good = fit(l[:, m], r[:, m], route)
        c = int(inliers(sampson(G, l, r), max_err2).sum())
        if not (good and c >= standing):
            break
        F, standing, stood = G, c, stood + 1
    status = KEPT_HYPOTHESIS if iters > 0 and stood == 0 else 0
    return status, best, stood, inliers(sampson(F, l, r), max_err2), F


def rms_coordinate(l, r):
    with np.errstate(all="ignore"):
        c = float(np.sqrt(np.mean(np.concatenate((l.ravel(), r.ravel())) ** 2))) if l.size else 1.0
    return c if np.isfinite(c) and c > 0 else 1.0


def g_measure(F, c):
    """G = S F S / |S F S|, S = diag(c, c, 1), the sign as in step 5; zeros stay zeros."""
    S = np.diag([c, c, 1.0])
    G, ok = canon(S @ np.asarray(F, dtype=np.float64).reshape(3, 3) @ S)
    return G if ok else np.zeros((3, 3))


def g_difference(Fa, Fb, c):
    return float(np.max(np.abs(g_measure(Fa, c) - g_measure(Fb, c))))


def both_routes(l, r, max_hyp):
    """The hypotheses of one set of n >= 9 matches by both routes: they depend on neither max_err2 nor iters."""
    H = hypothesis_count(l.shape[1], max_hyp)
    return tuple(_hypotheses(l, r, H, route) for route in (0, 1))


def solve_set(l, r, max_err2, max_hyp, iters, hyps=None):
    """One set: the decisions of the run at (route 0, max_err2), the settled flag and d_G over the six runs.  hyps: what
    both_routes(l, r, max_hyp) returned, where a caller keeps it across thresholds and rounds."""
    n = l.shape[1]
    c = rms_coordinate(l, r)
    if n < MIN_MATCHES:
        return SimpleNamespace(status=TOO_FEW, best_hyp=-1, stood=0, mask=np.zeros(n, dtype=bool), F=np.zeros((3, 3)),
                               settled=True, d_G=0.0, c=c)
    if hyps is None:
        hyps = both_routes(l, r, max_hyp)
    runs = []
    for route in (0, 1):
        for f in (1.0, 1.0 - 1e-6, 1.0 + 1e-6):
            runs.append(_run(l, r, hyps[route], max_err2 * f, iters, route))
    first = runs[0]
    settled = all(o[0] == first[0] and o[1] == first[1] and o[2] == first[2] and np.array_equal(o[3], first[3]) for o in runs[1:])
    d_G = max(g_difference(first[4], o[4], c) for o in runs[1:])
    return SimpleNamespace(status=first[0], best_hyp=first[1], stood=first[2], mask=first[3], F=first[4], settled=settled,
                           d_G=d_G, c=c)


def reference(set_ptr, left, right, max_err2=MAX_ERR2, max_hyp=0, iters=ITERS, hyps=None):
    """The whole call: arrays as native.twoview_ransac returns them, plus settled (S,), d_G (S,), stood (S,), c (S,).
    hyps: per set what both_routes returned (None for a set below nine matches), or None to compute them here."""
    set_ptr = np.asarray(set_ptr, dtype=np.int64)
    S, M = set_ptr.shape[0] - 1, left.shape[1]
    out = SimpleNamespace(F=np.zeros((S, 3, 3)), inlier=np.zeros(M, dtype=np.uint8), n_inliers=np.zeros(S, dtype=np.int32),
                          best_hyp=np.zeros(S, dtype=np.int32), status=np.zeros(S, dtype=np.int32),
                          summary=np.zeros(6, dtype=np.int64), settled=np.zeros(S, dtype=bool), d_G=np.zeros(S),
                          stood=np.zeros(S, dtype=np.int32), c=np.zeros(S))
    for s in range(S):
        lo, hi = int(set_ptr[s]), int(set_ptr[s + 1])
        o = solve_set(left[:, lo:hi], right[:, lo:hi], max_err2, max_hyp, iters, None if hyps is None else hyps[s])
        out.F[s], out.inlier[lo:hi], out.n_inliers[s], out.best_hyp[s], out.status[s] = o.F, o.mask, o.mask.sum(), o.best_hyp, o.status
        out.settled[s], out.d_G[s], out.stood[s], out.c[s] = o.settled, o.d_G, o.stood, o.c
        if o.status & TOO_FEW:
            out.summary[2] += 1
        elif o.status & NO_MODEL:
            out.summary[1] += 1
        else:
            out.summary[0] += 1
            out.summary[3] += 1 if o.status & KEPT_HYPOTHESIS else 0
            out.summary[4] += int(o.mask.sum())
            out.summary[5] += int((~o.mask).sum())
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------
K = np.array([[800.0, 0, 320], [0, 800.0, 240], [0, 0, 1]])


def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def matches(n, frac, seed, noise=0.5):
    """n matches of two views (focal 800, points 4 - 9 units deep, `noise` px on both keys); a share `frac` of the right keys
    displaced by 30 - 120 px.  Returns left (2, n), right (2, n), displaced (n,) bool."""
    rng = np.random.default_rng(seed)
    X = np.vstack((rng.uniform(-2, 2, (2, n)), rng.uniform(4, 9, (1, n))))
    R, t = _rot_y(0.15), np.array([[-1.0], [0.1], [0.2]])
    l = K @ X
    l = l[:2] / l[2]
    r = K @ (R @ X + t)
    r = r[:2] / r[2]
    l = l + rng.normal(0, noise, l.shape)
    r = r + rng.normal(0, noise, r.shape)
    bad = rng.random(n) < frac
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(30, 120, n)
    r = r + bad * np.vstack((np.cos(ang), np.sin(ang))) * mag
    return l, r, bad


def _rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])


def two_views(n, seed, K=K, R=None, t=(-1.0, 0.1, 0.2), depth=(4.0, 9.0), noise=0.5, plane=0.0, second=None, second_share=0.0,
              offset=0.0, frac=0.0, displace=(30.0, 120.0)):
    """n matches of two views with intrinsics K under the motion x' = R x + t (R: rot_y(0.15) if None), the points
    `depth[0]` to `depth[1]` units deep and +-2 units wide, `noise` px on both keys.  A share `plane` of the points lies on
    the plane z = mid-depth + 0.1 x + 0.05 y; a share `second_share` of the matches follows the motion second = (R2, t2)
    instead; `offset` is added to every coordinate of both images; a share `frac` of the right keys is displaced by
    `displace[0]` to `displace[1]` px.  The shares are drawn per match, so every stratum of the sampler holds its part of
    each.  Returns left (2, n), right (2, n), displaced (n,) bool."""
    rng = np.random.default_rng(seed)
    R = _rot_y(0.15) if R is None else np.asarray(R, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64).reshape(3, 1)
    X = np.vstack((rng.uniform(-2, 2, (2, n)), rng.uniform(depth[0], depth[1], (1, n))))
    on_plane = rng.random(n) < plane
    X[2] = np.where(on_plane, 0.5 * (depth[0] + depth[1]) + 0.1 * X[0] + 0.05 * X[1], X[2])
    l = K @ X
    l = l[:2] / l[2]
    Y = R @ X + t
    moved = rng.random(n) < second_share
    if second is not None:
        Y = np.where(moved, np.asarray(second[0], dtype=np.float64) @ X + np.asarray(second[1], dtype=np.float64).reshape(3, 1), Y)
    r = K @ Y
    r = r[:2] / r[2]
    l = l + rng.normal(0, noise, l.shape)
    r = r + rng.normal(0, noise, r.shape)
    bad = rng.random(n) < frac
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(displace[0], displace[1], n)
    r = r + bad * np.vstack((np.cos(ang), np.sin(ang))) * mag
    return l + offset, r + offset, bad


def _batch(parts):
    counts = [p[0].shape[1] for p in parts]
    return SimpleNamespace(set_ptr=np.concatenate(([0], np.cumsum(counts))).astype(np.int32),
                           left=np.ascontiguousarray(np.hstack([p[0] for p in parts])),
                           right=np.ascontiguousarray(np.hstack([p[1] for p in parts])),
                           displaced=np.concatenate([p[2] for p in parts]), counts=np.array(counts))


PROTO = {"proto0": 0.0, "proto1": 0.1, "proto2": 0.3}
PROTO_COUNTS = (300, 2000)
PATHS_COUNTS = (0, 8, 9, 10, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000)
PATHS_HYP = (1, 63, 64, 65, 128, 1000)
LONG = 1000                           # batch independence: "the batch without the long sets" keeps the sets up to this size


def degenerate_parts():
    """A plane seen under a pure rotation (noise-free: every matrix [e]x H explains every match), 40 identical points, and
    a clean set of 60 matches with one NaN coordinate."""
    rng = np.random.default_rng(77)
    n = 120
    X = np.vstack((rng.uniform(-2, 2, (2, n)), np.full((1, n), 6.0)))
    l = K @ X
    l = l[:2] / l[2]
    r = K @ (_rot_y(0.1) @ X)
    r = r[:2] / r[2]
    same = (np.tile([[100.0], [50.0]], (1, 40)), np.tile([[120.0], [60.0]], (1, 40)), np.zeros(40, dtype=bool))
    ln, rn, bad = matches(60, 0.0, 78)
    rn = rn.copy()
    rn[1, 17] = np.nan
    return [(l, r, np.zeros(n, dtype=bool)), same, (ln, rn, bad)]


# ---- the geometry families: what two_views is given besides n and the seed; every one as sets of FAMILY_COUNTS matches -----
K_LARGE = np.array([[3200.0, 0, 2000], [0, 3200.0, 1500], [0, 0, 1]])
FAMILIES = {
    "half_displaced": dict(frac=0.5),
    "forward": dict(R=_rot_z(0.05), t=(0.03, -0.02, -1.0), frac=0.1),          # both epipoles inside the image
    "sideways": dict(R=np.eye(3), t=(-1.0, 0.0, 0.0), frac=0.1),               # both epipoles at infinity
    "large_image": dict(K=K_LARGE, noise=2.0, frac=0.1, displace=(120.0, 480.0)),
    "offset": dict(offset=1e4, frac=0.1),
    "plane_dominant": dict(plane=0.8, frac=0.1),
    "two_motions": dict(second=(_rot_y(-0.1) @ _rot_z(0.2), (0.6, -0.8, 0.3)), second_share=0.4, frac=0.05),
    "rolled": dict(R=_rot_z(0.6) @ _rot_y(0.15), frac=0.2),
}
FAMILY_COUNTS = (40, 130, 300)        # below and above one slice of 64, above one wave-row of 256
# One seed per count, chosen on the CPU so that the conditions of tests/test_twoview_ransac_host.py hold of the reference (every
# set settled at every setting, KEPT_HYPOTHESIS in every family, every number of standing rounds from 0 to 5).
FAMILY_SEEDS = {"half_displaced": (6, 2, 1), "forward": (1, 1, 6), "sideways": (5, 4, 7), "large_image": (7, 7, 5),
                "offset": (7, 8, 7), "plane_dominant": (4, 4, 7), "two_motions": (7, 5, 1), "rolled": (1, 5, 1)}
FAMILY_ERR2 = (1.0, 4.0, 16.0)        # times 16 for large_image: its pixels are a quarter the size
FAMILY_ITERS = (0, 1, 2, 5)
EVERYONE = 1e12                       # a threshold under which every finite match is every valid hypothesis' inlier
TIES_HYP = 1000
TIES_SEEDS = (3, 2)
MANY_SEED = 2
MANY_SIZES = (0, 8, 9, 12, 33, 70)
MANY_CYCLES = 43                      # 43 x 6 + 1 = 259 sets


def family_err2(name, max_err2):
    return 16.0 * max_err2 if name == "large_image" and max_err2 != EVERYONE else max_err2


def family_part(name, n, seed):
    return two_views(n, seed, **FAMILIES[name])


def ties_parts(seeds=(0, 0)):
    """Noise-free matches, 30 % displaced: every hypothesis whose eight matches are clean ties at the same count."""
    return [two_views(n, seed, noise=0.0, frac=0.3) for n, seed in zip((200, 203), seeds)]


def many_sets_parts(seed=0):
    """MANY_CYCLES rounds of sets of 0, 8, 9, 12, 33 and 70 matches and a last set of 8: the call begins and ends with a set
    below nine matches, and every round has two of them side by side."""
    sizes = MANY_SIZES * MANY_CYCLES + (8,)
    return [two_views(n, 100000 * seed + k, frac=0.1) for k, n in enumerate(sizes)]


def nonfinite_parts():
    """60 clean matches with one +inf coordinate, and 1 100 whose only NaN is match 1 050: in the second score block."""
    l0, r0, bad0 = two_views(60, 5)
    l0 = l0.copy()
    l0[0, 31] = np.inf
    l1, r1, bad1 = two_views(1100, 6)
    r1 = r1.copy()
    r1[0, 1050] = np.nan
    return [(l0, r0, bad0), (l1, r1, bad1)]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in FAMILIES:
        return _batch([family_part(name, n, seed) for n, seed in zip(FAMILY_COUNTS, FAMILY_SEEDS[name])])
    if name == "ties":
        return _batch(ties_parts(TIES_SEEDS))
    if name == "many_sets":
        return _batch(many_sets_parts(MANY_SEED))
    if name == "nonfinite":
        return _batch(nonfinite_parts())
    if name in PROTO:
        return _batch([matches(n, PROTO[name], 1000 + n + int(100 * PROTO[name])) for n in PROTO_COUNTS])
    if name == "paths":
        return _batch([matches(n, 0.1, n) for n in PATHS_COUNTS])
    if name == "degenerate":
        return _batch(degenerate_parts())
    raise KeyError(name)


def set_of(sc, s):
    lo, hi = int(sc.set_ptr[s]), int(sc.set_ptr[s + 1])
    return sc.left[:, lo:hi], sc.right[:, lo:hi]


@functools.lru_cache(maxsize=None)
def _scene_hypotheses(name, max_hyp):
    """Per set of the scene what both_routes returns: shared by every (max_err2, iters) the scene is referenced at."""
    sc = scene(name)
    return [both_routes(*set_of(sc, s), max_hyp) if sc.counts[s] >= MIN_MATCHES else None for s in range(sc.counts.size)]


@functools.lru_cache(maxsize=None)
def scene_and_reference(name, max_hyp=128, iters=ITERS, max_err2=MAX_ERR2):
    """The scene and its reference, computed once per (scene, max_hyp, iters, max_err2) and shared; treat both as read-only."""
    sc = scene(name)
    hyps = _scene_hypotheses(name, max_hyp) if name in FAMILIES else None     # the scenes referenced at many settings
    return sc, reference(sc.set_ptr, sc.left, sc.right, max_err2, max_hyp, iters, hyps)


CASES = [(name, 128) for name in PROTO] + [("paths", h) for h in PATHS_HYP] + [("degenerate", 128)]

# (scene, max_err2, max_hyp, iters): every family at every threshold and number of rounds, and once at EVERYONE
GEOMETRY_CASES = [(name, family_err2(name, e), 128, it) for name in FAMILIES for e in FAMILY_ERR2 for it in FAMILY_ITERS] + \
                 [(name, EVERYONE, 128, ITERS) for name in FAMILIES]
# the further scenes, in the same form
PATH_CASES = [("ties", MAX_ERR2, TIES_HYP, ITERS), ("many_sets", MAX_ERR2, 128, ITERS), ("nonfinite", MAX_ERR2, 128, ITERS)]


def case_reference(case):
    name, max_err2, max_hyp, iters = case
    return scene_and_reference(name, max_hyp, iters, max_err2)
