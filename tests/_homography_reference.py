"""The rule of the robust homography (include/sfm_hip.h, block "robust homography") in NumPy float64, with a SETTLED flag
per set, and the scenes the tests use.  Built like tests/_twoview_ransac_reference.py, whose sampler pieces, Hartley transform
and scene generator it imports.

Every null-vector problem is solved by two routes (``eigh`` of A^T A, and ``svd`` of the zero-padded design matrix; the second
route also takes the adjugate from the singular value decomposition where the first takes cofactors) and every decision is
taken at ``max_err2 (1 -+ 1e-6)`` as well as at ``max_err2``: a set is settled iff all six runs agree on status, winner,
number of refit rounds that stood and final mask.  ``d_H`` is the largest difference between the six final matrices in the
measure ``D^-1 H D / |D^-1 H D|`` with ``D = diag(c, c, 1)``, ``c`` the RMS coordinate magnitude of the set's matches in both
images, the sign fixed as the rule fixes it.  (Entry-wise on H itself the perspective row, of order 1 / c, would go
unchecked.)"""
import functools
from types import SimpleNamespace

import numpy as np

import _twoview_ransac_reference as tv
from _twoview_ransac_reference import EPS, K, K_LARGE, _batch, _mix_array, _rot_y, _rot_z, canon, mix, rms_coordinate, set_of, two_views

TOO_FEW, NO_MODEL, KEPT_HYPOTHESIS = 1, 2, 4
MIN_MATCHES, MIN_COUNT = 5, 5
HYP_DEFAULT, HYP_MAX = 128, 65536
MAX_ERR2, ITERS = 4.0, 2              # 2 px; what every test uses unless it says otherwise


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def hypothesis_count(n, max_hyp):
    if max_hyp == 0:
        max_hyp = HYP_DEFAULT
    return max_hyp if n >= MIN_MATCHES and 1 <= max_hyp <= HYP_MAX else 0


def sample_indices(n, H):
    """(H, 4) int64: the matches of hypotheses 0 .. H - 1 of a set of n >= 5 matches."""
    k = np.arange(4, dtype=np.int64)
    lo, hi = k * n // 4, (k + 1) * n // 4
    z = _mix_array((4 * np.arange(H, dtype=np.uint64)[:, None] + k.astype(np.uint64)[None, :]))
    return lo[None, :] + (z % (hi - lo).astype(np.uint64)[None, :]).astype(np.int64)


# ---- the pieces of the rule ------------------------------------------------------------------------------------------------
def hartley_pair(p):
    """(T, T^-1) of the points p (2, m): T = [s 0 -s mx; 0 s -s my; 0 0 1], centroid, s = sqrt(2) / mean distance."""
    with np.errstate(all="ignore"):
        m = p.mean(axis=1)
        d = np.sqrt(((p - m[:, None]) ** 2).sum(axis=0)).mean()
        s = np.sqrt(2.0) / d
        T = np.array([[s, 0, -m[0] * s], [0, s, -m[1] * s], [0, 0, 1.0]])
        Ti = np.array([[1.0 / s, 0, m[0]], [0, 1.0 / s, m[1]], [0, 0, 1.0]])
    return T, Ti


def _apply(T, p):
    return T[0, 0] * p + T[0:2, 2:3]


def design(ln, rn):
    """Design rows of normalised matches: ln, rn (..., 2, m) -> (..., 2 m, 9), the two rows of a match side by side."""
    x1, y1, x2, y2 = ln[..., 0, :], ln[..., 1, :], rn[..., 0, :], rn[..., 1, :]
    one, zero = np.ones_like(x1), np.zeros_like(x1)
    ra = np.stack((-x1, -y1, -one, zero, zero, zero, x2 * x1, x2 * y1, x2), axis=-1)
    rb = np.stack((zero, zero, zero, -x1, -y1, -one, y2 * x1, y2 * y1, y2), axis=-1)
    return np.stack((ra, rb), axis=-2).reshape(ra.shape[:-2] + (2 * ra.shape[-2], 9))


def null_vectors(A, route):
    """(..., 9): the right singular vector of the smallest singular value of A (..., m, 9), by either route."""
    if route == 0:
        return np.linalg.eigh(np.swapaxes(A, -1, -2) @ A)[1][..., :, 0]
    if A.shape[-2] < 9:
        A = np.concatenate((A, np.zeros(A.shape[:-2] + (9 - A.shape[-2], 9))), axis=-2)
    return np.linalg.svd(A, full_matrices=False)[2][..., -1, :]


def adjugate(h, route):
    """adj(h) of h (..., 3, 3): cofactors (route 0), or V diag(s1 s2, s0 s2, s0 s1) U^T det(U) det(V) (route 1)."""
    if route == 0:
        a, b, c, d, e, f, g, i, j = (h[..., r, k] for r in range(3) for k in range(3))
        return np.stack((e * j - f * i, c * i - b * j, b * f - c * e,
                         f * g - d * j, a * j - c * g, c * d - a * f,
                         d * i - e * g, b * g - a * i, a * e - b * d), axis=-1).reshape(h.shape)
    u, s, vt = np.linalg.svd(h)
    co = np.stack((s[..., 1] * s[..., 2], s[..., 0] * s[..., 2], s[..., 0] * s[..., 1]), axis=-1)
    sign = np.linalg.det(u) * np.linalg.det(vt)
    return sign[..., None, None] * (np.swapaxes(vt, -1, -2) * co[..., None, :]) @ np.swapaxes(u, -1, -2)


def models(h, Tl, Tli, Tr, Tri, route):
    """(H, G, valid) of the normalised matrices h (..., 3, 3): step 5 after the null vector."""
    with np.errstate(all="ignore"):
        s = np.linalg.svd(np.where(np.isfinite(h), h, 0.0), compute_uv=False)
        ok = np.isfinite(h).all(axis=(-1, -2)) & (s[..., 2] > s[..., 0] * 3.0 * EPS)
        H, ok1 = canon(Tri @ h @ Tl)
        G, ok2 = canon(Tli @ adjugate(h, route) @ Tr)
    return H, G, ok & ok1 & ok2


def half_terms(A, p, q):
    """(lhs, w^2) of half(A, p, q) of step 2 for the matrices A (..., 3, 3) and the points p, q (2, n): (..., n) each."""
    with np.errstate(all="ignore"):
        u = A[..., 0, 0, None] * p[0] + (A[..., 0, 1, None] * p[1] + A[..., 0, 2, None])
        v = A[..., 1, 0, None] * p[0] + (A[..., 1, 1, None] * p[1] + A[..., 1, 2, None])
        w = A[..., 2, 0, None] * p[0] + (A[..., 2, 1, None] * p[1] + A[..., 2, 2, None])
        eu, ev = u - q[0] * w, v - q[1] * w
        return eu * eu + ev * ev, w * w


def _within(terms, max_err2):
    with np.errstate(all="ignore"):
        lhs, ww = terms
        return np.isfinite(lhs) & (ww > 0) & (lhs <= max_err2 * ww)


def terms(H, G, l, r):
    """What the test of step 2 compares, for the models (H, G) (..., 3, 3) and the matches l, r (2, n): no threshold yet."""
    return half_terms(H, l, r), half_terms(G, r, l)


def inliers_of(tm, max_err2):
    return _within(tm[0], max_err2) & _within(tm[1], max_err2)


def inliers(H, G, l, r, max_err2):
    return inliers_of(terms(H, G, l, r), max_err2)


def transfer_error2(H, l, r):
    """Squared transfer error left to right of the matches l, r (2, n) under H (3, 3), in pixels squared (for the tests)."""
    with np.errstate(all="ignore"):
        p = H @ np.vstack((l, np.ones((1, l.shape[1]))))
        return ((p[:2] / p[2] - r) ** 2).sum(axis=0)


def fit(l, r, route):
    """The model of the matches l, r (2, m) in pixel coordinates (step 8 over exactly these matches): (H, G, valid)."""
    (Tl, Tli), (Tr, Tri) = hartley_pair(l), hartley_pair(r)
    if not all(np.isfinite(T).all() for T in (Tl, Tli, Tr, Tri)):
        return np.zeros((3, 3)), np.zeros((3, 3)), False
    h = null_vectors(design(_apply(Tl, l), _apply(Tr, r)), route).reshape(3, 3)
    H, G, ok = models(h, Tl, Tli, Tr, Tri, route)
    return H, G, bool(ok)


def _hypotheses(l, r, H, route):
    """Steps 3 to 5 of one set: (idx (H, 4), Hm (H, 3, 3), Gm (H, 3, 3), valid (H,)); None without a finite normalisation."""
    n = l.shape[1]
    (Tl, Tli), (Tr, Tri) = hartley_pair(l), hartley_pair(r)
    if not all(np.isfinite(T).all() for T in (Tl, Tli, Tr, Tri)):
        return None
    ln, rn = _apply(Tl, l), _apply(Tr, r)
    idx = sample_indices(n, H)
    A = design(np.swapaxes(ln[:, idx], 0, 1), np.swapaxes(rn[:, idx], 0, 1))      # (H, 8, 9)
    Hm, Gm, ok = models(null_vectors(A, route).reshape(H, 3, 3), Tl, Tli, Tr, Tri, route)
    Hm, Gm = np.where(ok[:, None, None], Hm, 0.0), np.where(ok[:, None, None], Gm, 0.0)
    return idx, Hm, Gm, ok


def _counts(hyp, l, r, max_err2, tm=None):
    """Steps 6 and 7: the inlier count of every hypothesis, -1 where it is not valid (its matrix, or the sample gate).
    tm: terms(Hm, Gm, l, r), where a caller keeps them across thresholds."""
    idx, Hm, Gm, valid = hyp
    ok = inliers_of(terms(Hm, Gm, l, r) if tm is None else tm, max_err2)
    valid = valid & np.take_along_axis(ok, idx, axis=1).all(axis=1)               # the sample gate
    return np.where(valid, ok.sum(axis=1), -1)


def hypothesis_counts(l, r, max_err2, max_hyp, route=0):
    """What the pick sees of one set of n >= 5 matches: (H,) counts, -1 for a hypothesis that is not valid."""
    H = hypothesis_count(l.shape[1], max_hyp)
    hyp = _hypotheses(l, r, H, route)
    return np.full(H, -1) if hyp is None else _counts(hyp, l, r, max_err2)


def _run(l, r, hyp, max_err2, iters, route, tm=None):
    """Steps 6 to 9 of one set at one threshold: (status, best_hyp, stood, mask, H)."""
    n = l.shape[1]
    none = (NO_MODEL, -1, 0, np.zeros(n, dtype=bool), np.zeros((3, 3)))
    if hyp is None:
        return none
    counts = _counts(hyp, l, r, max_err2, tm)
    best = int(np.argmax(counts))                                                 # the first of the largest counts
    if counts[best] < MIN_COUNT:
        return none
    Hs, Gs, standing, stood = hyp[1][best], hyp[2][best], int(counts[best]), 0
    for _ in range(iters):
        m = inliers(Hs, Gs, l, r, max_err2)
        Hn, Gn, good = fit(l[:, m], r[:, m], route)
        c = int(inliers(Hn, Gn, l, r, max_err2).sum())
        if not (good and c >= standing):
            break
        Hs, Gs, standing, stood = Hn, Gn, c, stood + 1
    status = KEPT_HYPOTHESIS if iters > 0 and stood == 0 else 0
    return status, best, stood, inliers(Hs, Gs, l, r, max_err2), Hs


def h_measure(H, c):
    """D^-1 H D / |D^-1 H D|, D = diag(c, c, 1), the sign as in step 5; zeros stay zeros."""
    M, ok = canon(np.diag([1.0 / c, 1.0 / c, 1.0]) @ np.asarray(H, dtype=np.float64).reshape(3, 3) @ np.diag([c, c, 1.0]))
    return M if ok else np.zeros((3, 3))


def h_difference(Ha, Hb, c):
    return float(np.max(np.abs(h_measure(Ha, c) - h_measure(Hb, c))))


def both_routes(l, r, max_hyp):
    """The hypotheses of one set of n >= 5 matches by both routes: they depend on neither max_err2 nor iters."""
    H = hypothesis_count(l.shape[1], max_hyp)
    return tuple(_hypotheses(l, r, H, route) for route in (0, 1))


def solve_set(l, r, max_err2, max_hyp, iters, hyps=None):
    """One set: the decisions of the run at (route 0, max_err2), the settled flag and d_H over the six runs."""
    n = l.shape[1]
    c = rms_coordinate(l, r)
    if n < MIN_MATCHES:
        return SimpleNamespace(status=TOO_FEW, best_hyp=-1, stood=0, mask=np.zeros(n, dtype=bool), H=np.zeros((3, 3)),
                               settled=True, d_H=0.0, c=c)
    if hyps is None:
        hyps = both_routes(l, r, max_hyp)
    runs = []
    for route in (0, 1):
        tm = None if hyps[route] is None else terms(hyps[route][1], hyps[route][2], l, r)
        for f in (1.0, 1.0 - 1e-6, 1.0 + 1e-6):
            runs.append(_run(l, r, hyps[route], max_err2 * f, iters, route, tm))
    first = runs[0]
    settled = all(o[0] == first[0] and o[1] == first[1] and o[2] == first[2] and np.array_equal(o[3], first[3]) for o in runs[1:])
    d_H = max(h_difference(first[4], o[4], c) for o in runs[1:])
    return SimpleNamespace(status=first[0], best_hyp=first[1], stood=first[2], mask=first[3], H=first[4], settled=settled,
                           d_H=d_H, c=c)


def reference(set_ptr, left, right, max_err2=MAX_ERR2, max_hyp=0, iters=ITERS, hyps=None):
    """The whole call: arrays as native.homography_ransac returns them, plus settled (S,), d_H (S,), stood (S,), c (S,)."""
    set_ptr = np.asarray(set_ptr, dtype=np.int64)
    S, M = set_ptr.shape[0] - 1, left.shape[1]
    out = SimpleNamespace(H=np.zeros((S, 3, 3)), inlier=np.zeros(M, dtype=np.uint8), n_inliers=np.zeros(S, dtype=np.int32),
                          best_hyp=np.zeros(S, dtype=np.int32), status=np.zeros(S, dtype=np.int32),
                          summary=np.zeros(6, dtype=np.int64), settled=np.zeros(S, dtype=bool), d_H=np.zeros(S),
                          stood=np.zeros(S, dtype=np.int32), c=np.zeros(S))
    for s in range(S):
        lo, hi = int(set_ptr[s]), int(set_ptr[s + 1])
        o = solve_set(left[:, lo:hi], right[:, lo:hi], max_err2, max_hyp, iters, None if hyps is None else hyps[s])
        out.H[s], out.inlier[lo:hi], out.n_inliers[s], out.best_hyp[s], out.status[s] = o.H, o.mask, o.mask.sum(), o.best_hyp, o.status
        out.settled[s], out.d_H[s], out.stood[s], out.c[s] = o.settled, o.d_H, o.stood, o.c
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
PROTO = {"proto0": 0.0, "proto1": 0.1, "proto2": 0.3}
PROTO_COUNTS = (300, 2000)
PATHS_COUNTS = (0, 4, 5, 6, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000)
PATHS_HYP = (1, 63, 64, 65, 128, 1000)
ALONE = (5, 63, 65, 257, 1025, 5000)  # batch independence: the sets run alone
LONG = 1000                           # ... and "the batch without the long sets" keeps the sets up to this size


def degenerate_parts():
    """All matches on one line (noise-free, exactly representable: every matrix of a four-dimensional family maps the line as
    the matches say), 40 identical points, and a clean set of 60 matches on the plane with one NaN coordinate."""
    x = 0.25 * np.arange(80, dtype=np.float64) * 7.0
    line = (np.vstack((x + 40.0, 0.5 * x + 10.0)), np.vstack((x + 70.0, 0.5 * x + 15.0)), np.zeros(80, dtype=bool))
    same = (np.tile([[100.0], [50.0]], (1, 40)), np.tile([[120.0], [60.0]], (1, 40)), np.zeros(40, dtype=bool))
    ln, rn, bad = two_views(60, 78, plane=1.0)
    rn = rn.copy()
    rn[1, 17] = np.nan
    return [line, same, (ln, rn, bad)]


# ---- the geometry families: what two_views is given besides n and the seed; every one as sets of FAMILY_COUNTS matches -----
FAMILIES = {
    "plane": dict(plane=1.0, frac=0.1),
    "rotation": dict(t=(0.0, 0.0, 0.0), frac=0.1),
    "rolled_plane": dict(R=_rot_z(0.6) @ _rot_y(0.15), plane=1.0, frac=0.2),
    "half_plane": dict(plane=0.5, frac=0.1),
    "general": dict(frac=0.1),
    "large_image": dict(K=K_LARGE, noise=2.0, plane=1.0, frac=0.1, displace=(120.0, 480.0)),
    "offset": dict(offset=1e4, plane=1.0, frac=0.1),
}
FAMILY_COUNTS = (40, 130, 300)        # below and above one slice of 64, above one wave-row of 256
# One seed per count, chosen on the CPU so that the conditions of tests/test_homography_host.py hold of the reference (every
# set settled at every setting, KEPT_HYPOTHESIS and every number of standing rounds from 0 to 5 occur, the verdicts of the
# plane, rotation and general families are what the families say).
FAMILY_SEEDS = {"plane": (1, 5, 2), "rotation": (3, 4, 6), "rolled_plane": (2, 1, 1), "half_plane": (1, 6, 5),
                "general": (6, 2, 8), "large_image": (1, 5, 2), "offset": (1, 6, 2)}
FAMILY_ERR2 = (1.0, 4.0, 16.0)        # times 16 for large_image: its pixels are a quarter the size
FAMILY_ITERS = (0, 1, 2, 5)
EVERYONE = 1e24                       # a threshold under which every finite match is every valid hypothesis' inlier
TIES_HYP = 1000
TIES_SEEDS = (2, 3)
MANY_SEED = 1
MANY_SIZES = (0, 4, 5, 12, 33, 70)
MANY_CYCLES = 43                      # 43 x 6 + 1 = 259 sets
PROTO_SEED, PATHS_SEED = 1000, 0


def family_err2(name, max_err2):
    return 16.0 * max_err2 if name == "large_image" and max_err2 != EVERYONE else max_err2


def family_part(name, n, seed):
    return two_views(n, seed, **FAMILIES[name])


def ties_parts(seeds=(0, 0)):
    """Noise-free matches on the plane, 30 % displaced.  Under EVERYONE every finite match is an inlier of every valid
    hypothesis; under MAX_ERR2 every hypothesis whose four matches are clean ties at the same count."""
    return [two_views(n, seed, noise=0.0, plane=1.0, frac=0.3) for n, seed in zip((200, 203), seeds)]


def many_sets_parts(seed=0):
    """MANY_CYCLES rounds of sets of 0, 4, 5, 12, 33 and 70 matches and a last set of 4: the call begins and ends with a set
    below five matches, and every round has two of them side by side."""
    sizes = MANY_SIZES * MANY_CYCLES + (4,)
    return [two_views(n, 100000 * seed + k, plane=1.0, frac=0.1) for k, n in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in FAMILIES:
        return _batch([family_part(name, n, seed) for n, seed in zip(FAMILY_COUNTS, FAMILY_SEEDS[name])])
    if name == "ties":
        return _batch(ties_parts(TIES_SEEDS))
    if name == "many_sets":
        return _batch(many_sets_parts(MANY_SEED))
    if name in PROTO:
        return _batch([two_views(n, PROTO_SEED + n + int(100 * PROTO[name]), plane=1.0, frac=PROTO[name]) for n in PROTO_COUNTS])
    if name == "paths":
        return _batch([two_views(n, PATHS_SEED + n, plane=1.0, frac=0.1) for n in PATHS_COUNTS])
    if name == "degenerate":
        return _batch(degenerate_parts())
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _scene_hypotheses(name, max_hyp):
    """Per set of the scene what both_routes returns: shared by every (max_err2, iters) the scene is referenced at."""
    sc = scene(name)
    return [both_routes(*set_of(sc, s), max_hyp) if sc.counts[s] >= MIN_MATCHES else None for s in range(sc.counts.size)]


@functools.lru_cache(maxsize=None)
def scene_and_reference(name, max_hyp=128, iters=ITERS, max_err2=MAX_ERR2):
    """The scene and its reference, computed once per (scene, max_hyp, iters, max_err2) and shared; treat both as read-only."""
    sc = scene(name)
    return sc, reference(sc.set_ptr, sc.left, sc.right, max_err2, max_hyp, iters, _scene_hypotheses(name, max_hyp))


# (scene, max_err2, max_hyp, iters)
CASES = [(name, MAX_ERR2, 128, ITERS) for name in PROTO] + [("paths", MAX_ERR2, h, ITERS) for h in PATHS_HYP] + \
        [("degenerate", MAX_ERR2, 128, ITERS)]
GEOMETRY_CASES = [(name, family_err2(name, e), 128, it) for name in FAMILIES for e in FAMILY_ERR2 for it in FAMILY_ITERS]
PATH_CASES = [("ties", EVERYONE, TIES_HYP, ITERS), ("ties", MAX_ERR2, TIES_HYP, ITERS), ("many_sets", MAX_ERR2, 128, ITERS)]
# what the further GPU tests run besides: no refit rounds
EXTRA_CASES = [("paths", MAX_ERR2, 128, 0)]
ALL_CASES = CASES + GEOMETRY_CASES + PATH_CASES + EXTRA_CASES


def case_reference(case):
    name, max_err2, max_hyp, iters = case
    return scene_and_reference(name, max_hyp, iters, max_err2)


def verdict(n_h, has_h, n_f, has_f, planar_ratio=0.8):
    """The verdict of processors.classify_matches from the two inlier counts."""
    if not (has_f or has_h):
        return "none"
    if has_h and (not has_f or n_h >= planar_ratio * n_f):
        return "degenerate"
    return "general"
