"""The rule of the robust similarity (include/sfm_hip.h, block "robust similarity") in NumPy float64, with a SETTLED flag per
set, and the scenes the tests use.

Every model is computed by two routes -- Umeyama's through ``np.linalg.svd`` of Sigma, and Horn's unit quaternion through
``eigh`` of the 4x4 matrix, with the scale as trace(A^T Sigma) / var_a -- and every decision is taken at ``max_err2 (1 -+ 1e-6)``
as well as at ``max_err2``: a set is settled iff all six runs agree on status, winner, the number of refit rounds that stood
(the kept-hypothesis bit with it) and the final mask.  ``d_S`` is the spread of the final model over those six runs in the
measure ``max(|ds| / s, max |dA|, |dt| / extent)``, ``extent`` the largest coordinate range of the set's finite ``dst``."""
import functools
from types import SimpleNamespace

import numpy as np

EPS = 2.220446049250313e-16
TOO_FEW, NO_MODEL, KEPT_HYPOTHESIS = 1, 2, 4
MIN_SET, MIN_COUNT = 4, 4
HYP_DEFAULT, HYP_MAX = 128, 65536
MAX_ERR2, ITERS = 0.05 ** 2, 3          # what every test uses unless it says otherwise
NOISE = 0.01
EVERYONE = 1e24                       # a threshold under which every finite correspondence is every valid hypothesis' inlier


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def _mix_array(z):
    z = z.astype(np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def hypothesis_count(n, max_hyp):
    if max_hyp == 0:
        max_hyp = HYP_DEFAULT
    return max_hyp if n >= MIN_SET and 1 <= max_hyp <= HYP_MAX else 0


def sample_indices(n, H):
    """(H, 3) int64: the correspondences of hypotheses 0 .. H - 1 of a set of n >= 4."""
    k = np.arange(3, dtype=np.int64)
    lo, hi = k * n // 3, (k + 1) * n // 3
    z = _mix_array(3 * np.arange(H, dtype=np.uint64)[:, None] + k.astype(np.uint64)[None, :])
    return lo[None, :] + (z % (hi - lo).astype(np.uint64)[None, :]).astype(np.int64)


# ---- the pieces of the rule ------------------------------------------------------------------------------------------------
def _quat_rot(q):
    w, x, y, z = (q[..., k] for k in range(4))
    return np.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), axis=-1).reshape(q.shape[:-1] + (3, 3))


def models(a, b, route, rigid=False):
    """Step 4 for the correspondences a, b (..., 3, m): (s (...,), A (..., 3, 3), t (..., 3), valid (...,))."""
    with np.errstate(all="ignore"):
        m = a.shape[-1]
        mu_a, mu_b = a.mean(axis=-1), b.mean(axis=-1)
        da, db = a - mu_a[..., None], b - mu_b[..., None]
        Sg = db @ np.swapaxes(da, -1, -2) / m
        var_a = (da * da).sum(axis=(-1, -2)) / m
        finite = np.isfinite(Sg).all(axis=(-1, -2)) & np.isfinite(var_a)
        Sg0 = np.where(finite[..., None, None], Sg, 0.0)
        U, D, Vt = np.linalg.svd(Sg0)
        if route == 0:
            d = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
            S = np.ones(D.shape)
            S[..., 2] = d
            A = (U * S[..., None, :]) @ Vt
            s = (D * S).sum(axis=-1) / var_a
        else:
            M = np.swapaxes(Sg0, -1, -2)                                   # M[i][j] = mean a'_i b'_j
            xx, xy, xz, yx, yy, yz, zx, zy, zz = (M[..., i, j] for i in range(3) for j in range(3))
            N = np.stack((xx + yy + zz, yz - zy, zx - xz, xy - yx,
                          yz - zy, xx - yy - zz, xy + yx, zx + xz,
                          zx - xz, xy + yx, -xx + yy - zz, yz + zy,
                          xy - yx, zx + xz, yz + zy, -xx - yy + zz), axis=-1).reshape(M.shape[:-2] + (4, 4))
            A = _quat_rot(np.linalg.eigh(N)[1][..., :, 3])
            s = (A * Sg0).sum(axis=(-1, -2)) / var_a
        if rigid:
            s = np.ones_like(s)
        t = mu_b - s[..., None] * (A @ mu_a[..., None])[..., 0]
        valid = finite & np.isfinite(s) & np.isfinite(t).all(axis=-1) & (var_a > 0) & (s > 0) & (D[..., 1] > 3.0 * EPS * D[..., 0])
    return s, A, t, valid


def err2(s, A, t, a, b):
    """What the test of step 2 compares: (..., n) for models (...,) and correspondences a, b (3, n)."""
    with np.errstate(all="ignore"):
        Mx = s[..., None, None] * A
        e = b - (Mx @ a + t[..., None])
        return (e * e).sum(axis=-2)


def inliers_of(e2, max_err2):
    with np.errstate(all="ignore"):
        return np.isfinite(e2) & (e2 <= max_err2)


def _hypotheses(a, b, H, route, rigid):
    idx = sample_indices(a.shape[1], H)
    s, A, t, ok = models(np.swapaxes(a[:, idx], 0, 1), np.swapaxes(b[:, idx], 0, 1), route, rigid)
    return idx, s, A, t, ok


def _counts(hyp, e2, max_err2):
    idx, _, _, _, valid = hyp
    ok = inliers_of(e2, max_err2)
    valid = valid & np.take_along_axis(ok, idx, axis=1).all(axis=1)               # the sample gate
    return np.where(valid, ok.sum(axis=1), -1)


def _one(s, A, t, a, b, max_err2):
    return inliers_of(err2(np.asarray(s), A, t, a, b), max_err2)


def _run(a, b, hyp, e2, max_err2, iters, route, rigid):
    """Steps 5 to 8 of one set at one threshold: (status, best_hyp, stood, mask, sim (13,))."""
    n = a.shape[1]
    counts = _counts(hyp, e2, max_err2)
    best = int(np.argmax(counts))                                                 # the first of the largest counts
    if counts[best] < MIN_COUNT:
        return NO_MODEL, -1, 0, np.zeros(n, dtype=bool), np.zeros(13)
    s, A, t, standing, stood = hyp[1][best], hyp[2][best], hyp[3][best], int(counts[best]), 0
    for _ in range(iters):
        m = _one(s, A, t, a, b, max_err2)
        sn, An, tn, good = models(a[:, m], b[:, m], route, rigid)
        c = int(_one(sn, An, tn, a, b, max_err2).sum()) if good else -1
        if not (good and c >= standing):
            break
        s, A, t, standing, stood = sn, An, tn, c, stood + 1
    status = KEPT_HYPOTHESIS if iters > 0 and stood == 0 else 0
    return status, best, stood, _one(s, A, t, a, b, max_err2), np.concatenate(([float(s)], np.asarray(A).ravel(), t))


def extent(b):
    fin = np.isfinite(b).all(axis=0)
    if not fin.any():
        return 1.0
    return max(float(np.max(b[:, fin].max(axis=1) - b[:, fin].min(axis=1))), 1e-300)


def sim_difference(p, q, ext):
    """The measure of d_S between two models of 13 doubles."""
    p, q = np.asarray(p, dtype=np.float64).ravel(), np.asarray(q, dtype=np.float64).ravel()
    if not (p[0] > 0 and q[0] > 0):
        return 0.0 if np.array_equal(p, q) else np.inf
    return max(abs(p[0] - q[0]) / q[0], float(np.max(np.abs(p[1:10] - q[1:10]))), float(np.linalg.norm(p[10:] - q[10:])) / ext)


def solve_set(a, b, max_err2, max_hyp, iters, rigid=False):
    """One set: the decisions of the run at (route 0, max_err2), the settled flag and d_S over the six runs."""
    n = a.shape[1]
    ext = extent(b)
    if n < MIN_SET:
        return SimpleNamespace(status=TOO_FEW, best_hyp=-1, stood=0, mask=np.zeros(n, dtype=bool), sim=np.zeros(13), settled=True,
                               d_S=0.0, ext=ext)
    H = hypothesis_count(n, max_hyp)
    runs = []
    for route in (0, 1):
        hyp = _hypotheses(a, b, H, route, rigid)
        e2 = err2(hyp[1], hyp[2], hyp[3], a, b)
        for f in (1.0, 1.0 - 1e-6, 1.0 + 1e-6):
            runs.append(_run(a, b, hyp, e2, max_err2 * f, iters, route, rigid))
    first = runs[0]
    settled = all(o[0] == first[0] and o[1] == first[1] and o[2] == first[2] and np.array_equal(o[3], first[3]) for o in runs[1:])
    d_S = max(sim_difference(o[4], first[4], ext) for o in runs[1:])
    return SimpleNamespace(status=first[0], best_hyp=first[1], stood=first[2], mask=first[3], sim=first[4], settled=settled,
                           d_S=d_S, ext=ext)


def reference(set_ptr, src, dst, max_err2=MAX_ERR2, max_hyp=0, iters=ITERS, rigid=False):
    """The whole call: arrays as native.similarity_ransac returns them, plus settled (S,), d_S (S,), stood (S,), ext (S,)."""
    set_ptr = np.asarray(set_ptr, dtype=np.int64)
    S, M = set_ptr.shape[0] - 1, src.shape[1]
    out = SimpleNamespace(sim=np.zeros((S, 13)), inlier=np.zeros(M, dtype=np.uint8), n_inliers=np.zeros(S, dtype=np.int32),
                          best_hyp=np.zeros(S, dtype=np.int32), status=np.zeros(S, dtype=np.int32),
                          summary=np.zeros(6, dtype=np.int64), settled=np.zeros(S, dtype=bool), d_S=np.zeros(S),
                          stood=np.zeros(S, dtype=np.int32), ext=np.zeros(S))
    for k in range(S):
        lo, hi = int(set_ptr[k]), int(set_ptr[k + 1])
        o = solve_set(src[:, lo:hi], dst[:, lo:hi], max_err2, max_hyp, iters, rigid)
        out.sim[k], out.inlier[lo:hi], out.n_inliers[k], out.best_hyp[k], out.status[k] = o.sim, o.mask, o.mask.sum(), o.best_hyp, o.status
        out.settled[k], out.d_S[k], out.stood[k], out.ext[k] = o.settled, o.d_S, o.stood, o.ext
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


def plain_umeyama(a, b):
    """The fit over all correspondences, no test: what a caller without the estimator would compute."""
    s, A, t, _ = models(a, b, 0)
    return np.concatenate(([float(s)], A.ravel(), t))


def apply_sim(sim, a):
    sim = np.asarray(sim, dtype=np.float64).ravel()
    return sim[0] * (sim[1:10].reshape(3, 3) @ a) + sim[10:, None]


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def random_rotation(rng):
    q = rng.standard_normal(4)
    return _quat_rot(q / np.linalg.norm(q))


def two_frames(n, seed, frac=0.1, noise=NOISE, scale=None, offset=0.0):
    """(src (3, n), dst (3, n), bad (n,) bool, sim (13,)): points in a 8 x 6 x 4 box, s in 0.3 .. 3, Gaussian noise on dst,
    a fraction `frac` of the correspondences displaced by 1 .. 4.5 units in a random direction; `offset` is added to every
    coordinate of dst."""
    rng = np.random.default_rng(7919 * seed + n)
    a = (rng.random((3, n)) - 0.5) * np.array([[8.0], [6.0], [4.0]])
    A = random_rotation(rng)
    s = float(rng.uniform(0.3, 3.0)) if scale is None else float(scale)
    t = rng.uniform(-5.0, 5.0, 3) + offset
    b = s * (A @ a) + t[:, None] + noise * rng.standard_normal((3, n))
    bad = np.zeros(n, dtype=bool)
    n_bad = int(frac * n)
    if n_bad:
        bad[rng.permutation(n)[:n_bad]] = True
        d = rng.standard_normal((3, n_bad))
        b[:, bad] += d / np.linalg.norm(d, axis=0) * rng.uniform(1.0, 4.5, n_bad)
    return a, b, bad, np.concatenate(([s], A.ravel(), t))


def _batch(parts):
    counts = np.array([p[0].shape[1] for p in parts], dtype=np.int64)
    set_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    src = np.ascontiguousarray(np.concatenate([p[0] for p in parts], axis=1)) if parts else np.zeros((3, 0))
    dst = np.ascontiguousarray(np.concatenate([p[1] for p in parts], axis=1)) if parts else np.zeros((3, 0))
    bad = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, dtype=bool)
    return SimpleNamespace(set_ptr=set_ptr, src=src, dst=dst, bad=bad, counts=counts, truth=[p[3] for p in parts])


def set_of(sc, k):
    lo, hi = int(sc.set_ptr[k]), int(sc.set_ptr[k + 1])
    return sc.src[:, lo:hi], sc.dst[:, lo:hi]


PROTO = ((300, 0.1), (300, 0.3), (2000, 0.5))
PATHS_COUNTS = (0, 4, 5, 3, 63, 64, 65, 2, 1023, 1024, 1025, 0, 2049, 1)      # empty sets and sets below 4 between others
PATHS_HYP = (1, 2, 64, 65, 128, 1000)
ALONE = (1, 4, 6, 10, 12)             # batch independence: these sets of `paths` in a call of their own
MANY_SIZES = (0, 3, 4, 12, 33, 70)
MANY_CYCLES = 43                      # 43 x 6 + 1 = 259 sets
# Seeds chosen on the CPU so that every set of every case below is settled, and so that the plain fit over the half-wrong
# prototype set is as poor as such a fit usually is (the displacements are zero-mean: over 1 000 of them the plain fit keeps
# between a tenth and two thirds of the clean correspondences, by the seed).  tests/test_similarity_host.py asserts both.
PROTO_SEED, PATHS_SEED, RIGID_SEED, MANY_SEED, OFFSET_SEED, TIES_SEED = 3, 1, 1, 1, 1, 1
OFFSET = 1e6
KEPT_SETS, KEPT_ERR2 = ((40, 22), (130, 14)), 0.02 ** 2      # a threshold near the noise: no refit round keeps the winner's count


def degenerate_parts():
    """All src on one line along the x axis (Sigma has exactly one non-zero column: no model), 40 identical src, and a clean
    set of 60 with one NaN row in dst."""
    x = 0.25 * np.arange(80, dtype=np.float64)
    line_a = np.vstack((x, np.zeros(80), np.zeros(80)))
    rng = np.random.default_rng(5)
    line = (line_a, 2.0 * line_a[[1, 0, 2]] + 0.001 * rng.standard_normal((3, 80)), np.zeros(80, dtype=bool), np.zeros(13))
    same = (np.tile([[1.0], [2.0], [3.0]], (1, 40)), np.tile([[4.0], [5.0], [6.0]], (1, 40)), np.zeros(40, dtype=bool), np.zeros(13))
    a, b, bad, sim = two_frames(60, 78, frac=0.0)
    b = b.copy()
    b[1, 17] = np.nan
    return [line, same, (a, b, bad, sim)]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "proto":
        return _batch([two_frames(n, PROTO_SEED + k, frac=f) for k, (n, f) in enumerate(PROTO)])
    if name == "paths":
        return _batch([two_frames(n, PATHS_SEED + n, frac=0.1) for n in PATHS_COUNTS])
    if name == "rigid":
        return _batch([two_frames(n, RIGID_SEED + n, frac=0.2, scale=1.0) for n in (40, 300)])
    if name == "many_sets":
        sizes = MANY_SIZES * MANY_CYCLES + (4,)
        return _batch([two_frames(n, 1000 * MANY_SEED + k, frac=0.1) for k, n in enumerate(sizes)])
    if name == "degenerate":
        return _batch(degenerate_parts())
    if name == "ties":
        return _batch([two_frames(n, TIES_SEED + n, frac=0.3, noise=0.0) for n in (200, 203)])
    if name == "kept":
        return _batch([two_frames(n, seed, frac=0.3) for n, seed in KEPT_SETS])
    if name == "offset":
        return _batch([two_frames(n, OFFSET_SEED + n, frac=0.2, offset=OFFSET) for n in (130, 1025)])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene_and_reference(name, max_hyp=128, iters=ITERS, max_err2=MAX_ERR2, rigid=False):
    """The scene and its reference, computed once per setting and shared; treat both as read-only."""
    sc = scene(name)
    return sc, reference(sc.set_ptr, sc.src, sc.dst, max_err2, max_hyp, iters, rigid)


# ---- the resident scene of tests/test_gpu_ba_align.py: 6 cameras x 120 points of scenes.make_scene -------------------------
ALIGN_SCENE = (6, 120, 0.8, 11)       # make_scene's n_cams, n_pts, visibility, seed
ALIGN_SIM = (1.6, (0.3, -0.2, 0.5), (2.0, -1.0, 4.0))      # s, the rotation vector of A, t
ALIGN_SEED, ALIGN_N, ALIGN_FRAC = 4, 100, 0.2


def _rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def align_sim():
    return np.concatenate(([ALIGN_SIM[0]], _rodrigues(ALIGN_SIM[1]).ravel(), ALIGN_SIM[2]))


def align_case(scenes):
    """(scene, point_idx (n,), targets (3, n), bad (n,)) of the alignment tests: targets are ALIGN_SIM of the scene's initial
    points with Gaussian noise, a fifth of them displaced by 1 .. 4.5 units.  `scenes` is the package's scenes module."""
    sc = scenes.make_scene(*ALIGN_SCENE[:3], seed=ALIGN_SCENE[3])
    rng = np.random.default_rng(ALIGN_SEED)
    idx = rng.permutation(sc.n_pts)[:ALIGN_N].astype(np.int32)
    targets = apply_sim(align_sim(), sc.pts_init[:, idx]) + NOISE * rng.standard_normal((3, ALIGN_N))
    bad = np.zeros(ALIGN_N, dtype=bool)
    bad[rng.permutation(ALIGN_N)[:int(ALIGN_FRAC * ALIGN_N)]] = True
    d = rng.standard_normal((3, int(bad.sum())))
    targets[:, bad] += d / np.linalg.norm(d, axis=0) * rng.uniform(1.0, 4.5, int(bad.sum()))
    return sc, idx, np.ascontiguousarray(targets), bad


# (scene, max_err2, max_hyp, iters, rigid)
CASES = [("proto", MAX_ERR2, 128, ITERS, False)] + [("paths", MAX_ERR2, h, ITERS, False) for h in PATHS_HYP] + \
        [("paths", MAX_ERR2, 128, 0, False), ("rigid", MAX_ERR2, 128, ITERS, True), ("many_sets", MAX_ERR2, 128, ITERS, False),
         ("degenerate", MAX_ERR2, 128, ITERS, False), ("ties", EVERYONE, 1000, ITERS, False), ("ties", MAX_ERR2, 1000, ITERS, False),
         ("offset", MAX_ERR2, 128, ITERS, False), ("kept", KEPT_ERR2, 128, ITERS, False)]


def case_reference(case):
    name, max_err2, max_hyp, iters, rigid = case
    return scene_and_reference(name, max_hyp, iters, max_err2, rigid)


def case_id(case):
    return "%s-e%g-h%d-i%d%s" % (case[0], case[1], case[2], case[3], "-rigid" if case[4] else "")
