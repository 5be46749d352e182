"""NumPy float64 reference of the robust resection of cameras (include/sfm_hip.h, block "robust resection"): the rule
literally -- triple numbering, Grunert's quartic (companion-matrix eigenvalues, the batched form of ``np.roots``, plus two
Newton steps), the two frames, triple gate, lexicographic score, refit over the winner's inliers with the oracle's
``obs_terms_vec``, acceptance, judgement at the prepared camera -- plus a SETTLED flag per camera and the scenes the tests share.

A camera is settled when winner, final mask and KEPT bit are the same at max_err2 (1 - 1e-6), max_err2 and
max_err2 (1 + 1e-6), the same again with the three points of every triple handed to the solver in the two rotated orders,
and the winner's count is strictly above every other root of its own triple: its decisions then do not hang on the last
bits of a residual or on how the quartic was solved, so another correct implementation has to reproduce them exactly.
``d_c`` is the largest difference of the final camera between the three orders: what the arithmetic of a hypothesis leaves
open, and the scale of the tests' bound on the cameras."""
from types import SimpleNamespace

import numpy as np

import _robust_reference as rob
import _tri_ransac_reference as rr

TOO_FEW, NO_MODEL, KEPT_HYPOTHESIS, SAMPLED, HELD = 1, 2, 4, 8, 16
DEFAULT_HYP, MAX_HYP, MAX_OBS, MIN_COUNT = 128, 65536, 1 << 20, 4
SETTLE_REL = 1e-6
ROOT_IMAG = 1e-7                   # an eigenvalue is a real root when |imag| <= ROOT_IMAG (1 + |real|)
MAX_PX = 4.0
MAX_ERR2 = MAX_PX ** 2
ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))
HYP_CHUNK = 64                     # hypotheses scored at a time (memory)

# observation counts of the "paths" scene: every boundary of the kernels (the 64-observation slice, the wave's 256, the
# workgroup's 1 024, several blocks) and the counts around T = 128
PATHS_COUNTS = (0, 1, 3, 4, 5, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000)
PATHS_SEED = 312
PATHS_HYPS = (1, 32, 128, 1000)


# ---- the numbering of the hypotheses -----------------------------------------------------------------------------------
def triple_count(n):
    n = int(n)
    return n * (n - 1) * (n - 2) // 6


def hypothesis_count(n, max_hyp=DEFAULT_HYP):
    max_hyp = max_hyp or DEFAULT_HYP
    return 0 if n < 3 else min(triple_count(n), max_hyp)


def triple_numbers(n, max_hyp=DEFAULT_HYP):
    """Triple number k of every hypothesis h of a camera of n observations (Python integers: no overflow)."""
    max_hyp = max_hyp or DEFAULT_HYP
    total = triple_count(n)
    if total <= max_hyp:
        return list(range(total))
    return [h * total // max_hyp for h in range(max_hyp)]


def triples_of(n, ks):
    """(i, j, l), i < j < l, of the triples numbered ks in lexicographic order: C(n, 3) - C(n - i, 3) triples precede first
    index i, and inside it the pairs (j, l) of the n - i - 1 later observations follow in rr.pairs_of's order."""
    n = int(n)
    ks = np.asarray(ks, dtype=np.int64)
    m = n - np.arange(n - 1, dtype=np.int64)                      # n - i for i = 0 .. n - 2   (all < 2^63: n <= 2^20)
    first = triple_count(n) - m * (m - 1) * (m - 2) // 6
    i = np.searchsorted(first, ks, side="right") - 1
    rest = ks - first[i]
    cnt = n - i - 1                                               # observations after i
    b = 2.0 * cnt - 1.0
    r = ((b - np.sqrt(np.maximum(b * b - 8.0 * rest, 0.0))) * 0.5).astype(np.int64)
    r = np.clip(r, 0, np.maximum(cnt - 2, 0))
    for _ in range(4):                                            # the square root is right to within a unit or two
        r = np.where((r > 0) & (r * (2 * cnt - r - 1) // 2 > rest), r - 1, r)
        r = np.where((r < cnt - 2) & ((r + 1) * (2 * cnt - r - 2) // 2 <= rest), r + 1, r)
    j = i + 1 + r
    l = j + 1 + (rest - r * (2 * cnt - r - 1) // 2)
    return i, j, l


def hypothesis_triples(n, max_hyp=DEFAULT_HYP):
    return triples_of(n, triple_numbers(n, max_hyp))


# ---- the poses of a triple ---------------------------------------------------------------------------------------------
def _frames(a, b, c):
    """Right-handed frames (H, 3, 3), columns e1, e2, e3, spanned by (b - a, (b - a) x (c - a)); ok = non-zero normal."""
    with np.errstate(all="ignore"):
        d1 = b - a
        nrm = np.cross(d1, c - a)
        n2 = np.einsum("...k,...k->...", nrm, nrm)
        e1 = d1 / np.linalg.norm(d1, axis=-1)[..., None]
        e3 = nrm / np.sqrt(n2)[..., None]
        e2 = np.cross(e3, e1)
    return np.stack((e1, e2, e3), axis=-1), n2 > 0.0


def p3p_poses(f, X):
    """Poses of H triples: f (H, 3, 3) unit bearings and X (H, 3, 3) world points, rows in the order handed to the solver.
    Returns M (H, 4, 3, 3) = R^T, t (H, 4, 3), s1 (H, 4) the depth of the first point, valid (H, 4); unsorted."""
    with np.errstate(all="ignore"):
        a2 = np.sum((X[:, 1] - X[:, 2]) ** 2, axis=1)
        b2 = np.sum((X[:, 0] - X[:, 2]) ** 2, axis=1)
        c2 = np.sum((X[:, 0] - X[:, 1]) ** 2, axis=1)
        ca = np.einsum("hk,hk->h", f[:, 1], f[:, 2])
        cb = np.einsum("hk,hk->h", f[:, 0], f[:, 2])
        cg = np.einsum("hk,hk->h", f[:, 0], f[:, 1])
        ok = np.isfinite(a2) & np.isfinite(b2) & np.isfinite(c2) & (a2 != 0) & (b2 != 0) & (c2 != 0)
        p, q = (a2 - c2) / b2, (a2 + c2) / b2
        A4 = (p - 1) ** 2 - 4 * (c2 / b2) * ca ** 2
        A3 = 4 * (p * (1 - p) * cb - (1 - q) * ca * cg + 2 * (c2 / b2) * ca ** 2 * cb)
        A2 = 2 * (p ** 2 - 1 + 2 * p ** 2 * cb ** 2 + 2 * ((b2 - c2) / b2) * ca ** 2 - 4 * q * ca * cb * cg + 2 * ((b2 - a2) / b2) * cg ** 2)
        A1 = 4 * (-p * (1 + p) * cb + 2 * (a2 / b2) * cg ** 2 * cb - (1 - q) * ca * cg)
        A0 = (1 + p) ** 2 - 4 * (a2 / b2) * cg ** 2
        coef = np.stack((A4, A3, A2, A1, A0), axis=1)
        ok &= np.all(np.isfinite(coef), axis=1) & (A4 != 0)
        H = f.shape[0]
        comp = np.zeros((H, 4, 4))
        comp[:, 1, 0] = comp[:, 2, 1] = comp[:, 3, 2] = 1.0
        mon = np.where(ok[:, None], coef[:, 1:] / np.where(ok, A4, 1.0)[:, None], 0.0)
        comp[:, 0, :] = -mon
        ev = np.linalg.eigvals(comp) if H else np.zeros((0, 4), dtype=complex)
        real = np.abs(ev.imag) <= ROOT_IMAG * (1.0 + np.abs(ev.real))
        y = ev.real.copy()
        for _ in range(2):                                                        # Newton polish on the quartic itself
            val = (((A4[:, None] * y + A3[:, None]) * y + A2[:, None]) * y + A1[:, None]) * y + A0[:, None]
            der = ((4 * A4[:, None] * y + 3 * A3[:, None]) * y + 2 * A2[:, None]) * y + A1[:, None]
            step = val / der
            y = np.where(np.isfinite(step), y - step, y)
        div = 2 * (cg[:, None] - y * ca[:, None])
        x = ((p[:, None] - 1) * y * y - 2 * p[:, None] * cb[:, None] * y + 1 + p[:, None]) / div
        den = 1 + y * y - 2 * y * cb[:, None]
        s1 = np.sqrt(b2[:, None] / den)
        valid = ok[:, None] & real & (div != 0) & np.isfinite(x) & np.isfinite(s1) & (x > 0) & (y > 0) & (s1 > 0)
        # the triangle in the camera frame and in the world
        Pc = np.stack((s1[:, :, None] * f[:, None, 0, :], (x * s1)[:, :, None] * f[:, None, 1, :],
                       (y * s1)[:, :, None] * f[:, None, 2, :]), axis=2)          # (H, 4, 3 points, 3)
        Fc, okc = _frames(Pc[:, :, 0], Pc[:, :, 1], Pc[:, :, 2])
        Fw, okw = _frames(X[:, 0], X[:, 1], X[:, 2])
        M = np.einsum("hrik,hjk->hrij", Fc, Fw)                                   # M Fw = Fc
        t = Pc[:, :, 0] - np.einsum("hrij,hj->hri", M, X[:, 0])
        valid &= okc & okw[:, None] & np.all(np.isfinite(M), axis=(2, 3)) & np.all(np.isfinite(t), axis=2)
        tr1 = 1.0 + M[:, :, 0, 0] + M[:, :, 1, 1] + M[:, :, 2, 2]                 # rot_to_quat's domain: qw = sqrt(tr1) / 2 >= 1e-6
        valid &= (tr1 >= 0) & (np.sqrt(np.maximum(tr1, 0.0)) / 2.0 >= 1e-6)
    return M, t, s1, valid


def _err2(M, t, u, v, scale, X):
    """err2 and s2, (..., n), of the poses M (..., 3, 3), t (..., 3) in the observations u, v, scale (n,), X (n, 3)."""
    with np.errstate(all="ignore"):
        s = M @ X.T + t[..., None]                                                # (..., 3, n)
        s0, s1, s2 = s[..., 0, :], s[..., 1, :], s[..., 2, :]
        e = (scale ** 2) * ((s0 / s2 - u) ** 2 + (s1 / s2 - v) ** 2)
    return e, s2


def _inliers(e, s2, max_err2):
    with np.errstate(all="ignore"):
        return (s2 > 0.0) & np.isfinite(e) & (e <= max_err2)


def _prepared(cam7):
    """M = R(q)^T and t = R(q)^T (-C) of a camera [C, q]: the screen's projection."""
    R = rob._oracle().quat_to_rot_unchecked(cam7[3:7])
    return R.T, R.T @ -cam7[0:3]


def _refit(cam7, u, v, X, mask, lam, iters, quirks):
    """`iters` steps of the motion-only update over the masked observations; None when a step fails."""
    oracle = rob._oracle()
    cam = cam7.copy()
    idx = np.flatnonzero(mask)
    zeros = np.zeros(idx.shape[0], dtype=np.int64)
    uv = np.stack((u[idx], v[idx]))
    pts = np.ascontiguousarray(X[idx].T)
    for _ in range(iters):
        try:
            with np.errstate(all="ignore"):
                r, jp, _jx = oracle.obs_terms_vec(cam[None, :], pts, zeros, np.arange(idx.shape[0]), uv, quirks)
                U = np.einsum("mki,mkj->ij", jp, jp)
                g = np.einsum("mki,mk->i", jp, r)
            if not (np.isfinite(U).all() and np.isfinite(g).all()):
                return None
            cam = cam + np.linalg.solve(U + lam * np.eye(7), g)
            cam[3:7] /= np.sqrt(np.sum(np.square(cam[3:7])))
            if not np.isfinite(cam).all():
                return None
            oracle.rot_to_quat(oracle.quat_to_rot(cam[3:7]))
        except (np.linalg.LinAlgError, ValueError):
            return None
    return cam


def _score(u, v, X, scale, tri, order, thresholds):
    """Poses of every hypothesis with its points in `order`, sorted by the depth of observation i, and per threshold their
    inlier counts (-1 where invalid or refused by the triple gate): M, t (H, 4, ...), counts (len(thresholds), H, 4)."""
    n = u.shape[0]
    f = np.stack((u, v, np.ones(n)), axis=1)
    f /= np.linalg.norm(f, axis=1)[:, None]
    idx = np.stack(tri, axis=1)[:, list(order)]                                  # (H, 3)
    M, t, _s1, valid = p3p_poses(f[idx], X[idx])
    H = idx.shape[0]
    with np.errstate(all="ignore"):
        key = np.linalg.norm(np.einsum("hrij,hj->hri", M, X[tri[0]]) + t, axis=2)      # depth of observation i
    key = np.where(valid, key, np.inf)
    srt = np.argsort(key, axis=1, kind="stable")
    hh = np.arange(H)[:, None]
    M, t, valid = M[hh, srt], t[hh, srt], valid[hh, srt]
    counts = np.full((len(thresholds), H, 4), -1, dtype=np.int64)
    hv, rv = np.nonzero(valid)                                                    # only the valid poses are scored
    for lo in range(0, hv.shape[0], 4 * HYP_CHUNK):
        hs, rs = hv[lo:lo + 4 * HYP_CHUNK], rv[lo:lo + 4 * HYP_CHUNK]
        e, s2 = _err2(M[hs, rs], t[hs, rs], u, v, scale, X)                       # (k, n)
        ks = np.arange(hs.shape[0])[:, None]
        for k, thr in enumerate(thresholds):
            inl = _inliers(e, s2, thr)
            gate = inl[ks, idx[hs]].all(axis=1)                                   # the three generating observations
            counts[k, hs, rs] = np.where(gate, inl.sum(axis=1), -1)
    return M, t, counts


def _finish(u, v, X, scale, M, t, counts, thr, lam, iters, quirks, cache):
    """Steps 5 and 6 at one threshold: (best_hyp, cam7, mask, kept, strict) or (-1, None, None, False, True)."""
    oracle = rob._oracle()
    if counts.size == 0 or counts.max() < MIN_COUNT:
        return -1, None, None, False, True
    h, r = np.unravel_index(int(np.argmax(counts)), counts.shape)                # the first of the largest: lower h, then lower r
    own = np.delete(counts[h], r)
    strict = bool(np.all(own < counts[h, r]))
    Mw, tw = M[h, r], t[h, r]
    cam_h = np.concatenate((-Mw.T @ tw, oracle.rot_to_quat(Mw.T)))
    e, s2 = _err2(Mw, tw, u, v, scale, X)
    mask = _inliers(e, s2, thr)
    key = (mask.tobytes(), cam_h.tobytes())
    if key not in cache:
        cache[key] = _refit(cam_h, u, v, X, mask, lam, iters, quirks)
    cam = cache[key]
    if cam is not None:
        m1 = _inliers(*_err2(*_prepared(cam), u, v, scale, X), thr)
        if m1.sum() >= counts[h, r]:
            return int(h), cam, m1, False, strict
    mh = _inliers(*_err2(*_prepared(cam_h), u, v, scale, X), thr)
    return int(h), cam_h, mh, True, strict


def solve_camera(u, v, X, scale, max_err2=MAX_ERR2, max_hyp=DEFAULT_HYP, lam=0.5, iters=3, quirks=None):
    """One camera: normalised keys u, v (n,), its points X (n, 3), its scale.  Returns a namespace with cam (7,) or None (the
    camera keeps its input), mask (n,) bool, n_inliers, best_hyp, status, settled, d_c."""
    quirks = rob._oracle().QUIRKS_REFERENCE if quirks is None else quirks
    max_hyp = max_hyp or DEFAULT_HYP
    n = u.shape[0]
    out = SimpleNamespace(cam=None, mask=np.zeros(n, dtype=bool), n_inliers=0, best_hyp=-1, status=0, settled=True, d_c=0.0)
    if n < 4:
        out.status = TOO_FEW
        return out
    if triple_count(n) > max_hyp:
        out.status |= SAMPLED
    tri = hypothesis_triples(n, max_hyp)
    sc = np.full(n, float(scale))
    thresholds = (max_err2, max_err2 * (1.0 - SETTLE_REL), max_err2 * (1.0 + SETTLE_REL))
    runs, cache = [], {}
    for order in ORDERS:
        M, t, counts = _score(u, v, X, sc, tri, order, thresholds)
        runs += [_finish(u, v, X, sc, M, t, counts[k], thr, lam, iters, quirks, cache) for k, thr in enumerate(thresholds)]
    best, cam, mask, kept, strict = runs[0]
    out.settled = strict and all(r[0] == best and (best < 0 or (np.array_equal(r[2], mask) and r[3] == kept)) for r in runs[1:])
    if best < 0:
        out.status |= NO_MODEL
        return out
    out.d_c = max([float(np.max(np.abs(r[1] - cam))) for r in (runs[3], runs[6]) if r[1] is not None] + [0.0])
    out.cam, out.mask, out.n_inliers, out.best_hyp = cam, mask, int(mask.sum()), best
    if kept:
        out.status |= KEPT_HYPOTHESIS
    return out


def judge_camera(cam7, u, v, X, scale, max_err2=MAX_ERR2):
    """The inlier mask of a camera [C, q] over its observations (a held camera is judged, nothing else)."""
    return _inliers(*_err2(*_prepared(np.asarray(cam7, dtype=np.float64)), u, v, np.full(u.shape[0], float(scale)), X), max_err2)


def solve_views(view_ptr, uv, X, cam_scale=None, cams_init=None, max_err2=MAX_ERR2, max_hyp=DEFAULT_HYP, lam=0.5, iters=3,
                quirks=None, held=None):
    """The whole call in the free form's layout: view_ptr (V + 1,), uv (2, M), X (3, M) camera-major.  Returns cams (V, 7),
    inlier (M,) uint8, n_inliers, best_hyp, status, summary (6,) int64, settled (V,), d_c (V,)."""
    view_ptr = np.asarray(view_ptr, dtype=np.int64)
    nv, m = view_ptr.shape[0] - 1, uv.shape[1]
    scale_all = np.ones(nv) if cam_scale is None else np.asarray(cam_scale, dtype=np.float64)
    cams = np.tile(np.array([0.0, 0, 0, 1, 0, 0, 0]), (nv, 1)) if cams_init is None else np.array(cams_init, dtype=np.float64).reshape(nv, 7)
    inlier = np.zeros(m, dtype=np.uint8)
    n_in = np.zeros(nv, dtype=np.int32); best = np.full(nv, -1, dtype=np.int32); status = np.zeros(nv, dtype=np.int32)
    settled = np.ones(nv, dtype=bool); d_c = np.zeros(nv)
    summary = np.zeros(6, dtype=np.int64)
    for c in range(nv):
        lo, hi = view_ptr[c], view_ptr[c + 1]
        u, v, Xc = uv[0, lo:hi], uv[1, lo:hi], np.ascontiguousarray(X[:, lo:hi].T)
        if held is not None and held[c]:
            mask = judge_camera(cams[c], u, v, Xc, scale_all[c], max_err2)
            inlier[lo:hi] = mask
            n_in[c], status[c] = int(mask.sum()), HELD
            summary[4] += n_in[c]
            continue
        r = solve_camera(u, v, Xc, scale_all[c], max_err2, max_hyp, lam, iters, quirks)
        status[c], settled[c], d_c[c] = r.status, r.settled, r.d_c
        if r.cam is None:
            summary[2 if r.status & TOO_FEW else 1] += 1
            continue
        cams[c] = r.cam
        inlier[lo:hi] = r.mask
        n_in[c], best[c] = r.n_inliers, r.best_hyp
        summary[0] += 1
        summary[3] += bool(r.status & KEPT_HYPOTHESIS)
        summary[4] += r.n_inliers
        summary[5] += (hi - lo) - r.n_inliers
    return SimpleNamespace(cams=cams, inlier=inlier, n_inliers=n_in, best_hyp=best, status=status, summary=summary,
                           settled=settled, d_c=d_c)


# ---- scenes ------------------------------------------------------------------------------------------------------------
def camera_major(sc, pts=None):
    """The scene `sc` of _tri_ransac_reference (observations sorted by point, then camera) in the free form's layout, with
    the points `pts` (3, N; default: the true ones): view_ptr, order (M,) scene index of every camera-major entry, uv, X."""
    pts = sc.pts_true if pts is None else pts
    order = np.argsort(sc.cam_idx, kind="stable")
    view_ptr = np.concatenate(([0], np.cumsum(np.bincount(sc.cam_idx, minlength=sc.n_views)))).astype(np.int32)
    return SimpleNamespace(view_ptr=view_ptr, order=order, uv=np.ascontiguousarray(sc.uv[:, order]),
                           X=np.ascontiguousarray(pts[:, sc.pt_idx[order]]), counts=np.diff(view_ptr))


def cams_of(sc):
    """The true cameras [C, q] of a scene, (V, 7)."""
    oracle = rob._oracle()
    return np.stack([np.concatenate((sc.centres[c], oracle.rot_to_quat(sc.rots[c]))) for c in range(sc.n_views)])


def make_scene(n_views, n_pts, visibility, seed, share=rr.BAD_SHARE):
    """rr.make_scene with the displaced share as a parameter (the same scene at the same share)."""
    rng = np.random.default_rng(seed)
    rots, C = rr._cameras(n_views, 120.0)
    pts = rng.uniform(-rr.CUBE / 2.0, rr.CUBE / 2.0, (3, n_pts))
    seen = rng.random((n_pts, n_views)) < visibility
    pt_ptr = np.concatenate(([0], np.cumsum(seen.sum(axis=1))))
    cam_idx = np.nonzero(seen)[1]
    displaced = rng.random(cam_idx.shape[0]) < share
    return rr._finish(rots, C, pts, pt_ptr, cam_idx, rng, displaced)


def make_paths_scene(seed=PATHS_SEED):
    """One camera per entry of PATHS_COUNTS, in a shuffled order, on a 330 degree arc; camera c sees a random subset of that
    many of the 5 000 points, 10 % of the observations displaced."""
    rng = np.random.default_rng(seed)
    counts = np.array(PATHS_COUNTS)[rng.permutation(len(PATHS_COUNTS))]
    nv, n_pts = counts.shape[0], int(max(PATHS_COUNTS))
    rots, C = rr._cameras(nv, 330.0)
    pts = rng.uniform(-rr.CUBE / 2.0, rr.CUBE / 2.0, (3, n_pts))
    seen = np.zeros((n_pts, nv), dtype=bool)
    for c, n in enumerate(counts):
        seen[rng.choice(n_pts, n, replace=False), c] = True
    pt_ptr = np.concatenate(([0], np.cumsum(seen.sum(axis=1))))
    cam_idx = np.nonzero(seen)[1]
    displaced = rng.random(cam_idx.shape[0]) < rr.BAD_SHARE
    return rr._finish(rots, C, pts, pt_ptr, cam_idx, rng, displaced)


def make_special_scene(seed=312):
    """Four cameras over 60 points: camera 0 and 3 ordinary (10 % displaced), camera 1 with eight observations whose keys are
    all replaced by random ones (no model), camera 2 seeing only the twelve points 0 .. 11, which lie on a line parallel
    to the x axis at dyadic coordinates -- every cross product of two of their differences is exactly zero."""
    rng = np.random.default_rng(seed)
    nv, n_pts = 4, 60
    rots, C = rr._cameras(nv, 120.0)
    pts = rng.uniform(-rr.CUBE / 2.0, rr.CUBE / 2.0, (3, n_pts))
    pts[:, 0:12] = np.stack((np.arange(12) / 8.0 - 0.75, np.full(12, 0.25), np.full(12, 0.5)))
    seen = rng.random((n_pts, nv)) < 0.8
    seen[:, 1] = False; seen[12:20, 1] = True
    seen[:, 2] = False; seen[0:12, 2] = True
    pt_ptr = np.concatenate(([0], np.cumsum(seen.sum(axis=1))))
    cam_idx = np.nonzero(seen)[1]
    displaced = (rng.random(cam_idx.shape[0]) < rr.BAD_SHARE) & (cam_idx != 2)
    sc = rr._finish(rots, C, pts, pt_ptr, cam_idx, rng, displaced)
    bad = cam_idx == 1
    sc.uv[:, bad] = rng.uniform(-0.25, 0.25, (2, int(bad.sum())))
    sc.displaced = displaced | bad
    return sc


SCENES = {
    "proto0": lambda: make_scene(*rr.PROTOTYPE_SCENES[0]),
    "proto1": lambda: make_scene(*rr.PROTOTYPE_SCENES[1]),
    "proto2": lambda: make_scene(*rr.PROTOTYPE_SCENES[2]),
    "proto0_30": lambda: make_scene(*rr.PROTOTYPE_SCENES[0], share=0.30),
    "paths": make_paths_scene,
    "special": make_special_scene,
}
# every (scene, max_hyp) a test uses: test_resect_host.py asserts that each camera of each is settled
CASES = [(name, 128) for name in ("proto0", "proto1", "proto2", "proto0_30", "special")] + [("paths", h) for h in PATHS_HYPS]

_CACHE = {}


def scene(name):
    """A scene by name with its camera-major form at the true points, built once."""
    if ("scene", name) not in _CACHE:
        sc = SCENES[name]()
        _CACHE[("scene", name)] = (sc, camera_major(sc))
    return _CACHE[("scene", name)]


def scene_and_reference(name, max_hyp=128):
    """(scene, camera-major form, reference at the tests' thresholds from the true points), computed once."""
    if (name, max_hyp) not in _CACHE:
        sc, cm = scene(name)
        _CACHE[(name, max_hyp)] = (sc, cm, solve_views(cm.view_ptr, cm.uv, cm.X, sc.cam_scale, None, MAX_ERR2, max_hyp))
    return _CACHE[(name, max_hyp)]
