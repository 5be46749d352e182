"""The rule of the robust essential matrix (include/sfm_hip.h, block "robust essential matrix") in NumPy float64, with a
SETTLED flag per set, and the scenes the tests use.

The minimal solver is written twice.  Route 0 takes the null space from the SVD of the 5x9 matrix, writes the ten cubics as
a cubic matrix polynomial in z over the ten monomials in (x, y) and reads the solutions off the eigenpairs of its 30x30
linearisation (no elimination, no scalar polynomial).  Route 1 takes the null space from ``eigh`` of A^T A (another basis), eliminates in the hidden-variable
order, forms the degree-10 polynomial in z as the determinant of a 3x3 polynomial matrix, takes ``np.roots`` of it (the
eigenvalues of its companion matrix) and substitutes back.  Both end with two Gauss-Newton steps on their own ten cubics.
Every decision is also taken at ``max_err2 (1 -+ 1e-6)``: a set is SETTLED iff all six runs agree on status, best_hyp,
best_root, n_valid and the mask, and the ordering keys (E[0] of the canonical solutions) of the winner's sample are at least
1e-6 apart by both routes.  ``d_E`` is the largest entry-wise difference between the routes' winning matrices, ``d_G`` that
of their pixel matrices in the G measure of tests/_twoview_ransac_reference.py.

The scenes come from ``two_views`` of that module; the seeds are chosen on the CPU so that every set of every parity case is
settled (tests/test_essential_host.py checks it)."""
import functools
from types import SimpleNamespace

import numpy as np

import _twoview_ransac_reference as tv

TOO_FEW, NO_MODEL = 1, 2
MIN_MATCHES, MIN_COUNT, MAX_SOL = 6, 6, 10
HYP_DEFAULT, HYP_MAX = 128, 65536
MAX_ERR2 = 4.0
KEY_GAP = 1e-6
REAL_TOL = 1e-9                       # a root counts as real iff |imag| <= REAL_TOL (1 + |root|)
K = tv.K


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def hypothesis_count(n, max_hyp):
    if max_hyp == 0:
        max_hyp = HYP_DEFAULT
    return max_hyp if n >= MIN_MATCHES and 1 <= max_hyp <= HYP_MAX else 0


def sample_indices(n, H):
    """(H, 5) int64: the matches of hypotheses 0 .. H - 1 of a set of n >= 6 matches."""
    k = np.arange(5, dtype=np.int64)
    lo, hi = k * n // 5, (k + 1) * n // 5
    z = tv._mix_array((5 * np.arange(H, dtype=np.uint64)[:, None] + k.astype(np.uint64)[None, :]))
    return lo[None, :] + (z % (hi - lo).astype(np.uint64)[None, :]).astype(np.int64)


# ---- rays and pixel matrices -----------------------------------------------------------------------------------------------
def rays(Km, p):
    """(2, n): the first two components of K^-1 (x, y, 1)^T by back substitution."""
    with np.errstate(all="ignore"):
        r1 = (p[1] - Km[1, 2]) / Km[1, 1]
        r0 = (p[0] - Km[0, 1] * r1 - Km[0, 2]) / Km[0, 0]
    return np.vstack((r0, r1))


def _inv_upper(Km):
    a, b, c, d, e = Km[0, 0], Km[0, 1], Km[0, 2], Km[1, 1], Km[1, 2]
    return np.array([[1 / a, -b / (a * d), (b * e - c * d) / (a * d)], [0, 1 / d, -e / d], [0, 0, 1.0]])


def to_pixels(E, Kl, Kr):
    """F = K_r^-T E K_l^-1 at Frobenius norm 1, the entry of largest magnitude positive; and validity."""
    with np.errstate(all="ignore"):
        return tv.canon(_inv_upper(Kr).T @ E @ _inv_upper(Kl))


# ---- polynomials in (x, y, z) on a dense exponent grid: P[..., i, j, k] multiplies x^i y^j z^k ---------------------------------
def _pmul_linear(P, L):
    """P (..., a, a, a) times the linear form L (..., 2, 2, 2): (..., a + 1, a + 1, a + 1)."""
    a = P.shape[-1]
    out = np.zeros(P.shape[:-3] + (a + 1,) * 3)
    for dx, dy, dz in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        out[..., dx:dx + a, dy:dy + a, dz:dz + a] += P * L[..., dx, dy, dz][..., None, None, None]
    return out


def _cubics(N):
    """The ten cubics of E = x N0 + y N1 + z N2 + N3, N (H, 4, 9): (H, 10, 4, 4, 4)."""
    H = N.shape[0]
    E = np.zeros((H, 3, 3, 2, 2, 2))
    E[..., 1, 0, 0], E[..., 0, 1, 0], E[..., 0, 0, 1], E[..., 0, 0, 0] = (N[:, v].reshape(H, 3, 3) for v in range(4))
    EEt = np.zeros((H, 3, 3, 3, 3, 3))
    for i in range(3):
        for k in range(3):
            for m in range(3):
                EEt[:, i, k] += _pmul_linear(E[:, i, m], E[:, k, m])
    tr = EEt[:, 0, 0] + EEt[:, 1, 1] + EEt[:, 2, 2]
    out = np.zeros((H, 10, 4, 4, 4))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                lam = 2.0 * EEt[:, i, k] - (tr if i == k else 0.0)
                out[:, 3 * i + j] += _pmul_linear(lam, E[:, k, j])
    for t in range(3):
        u, v = (t + 1) % 3, (t + 2) % 3
        minor = _pmul_linear(E[:, 1, u], E[:, 2, v]) - _pmul_linear(E[:, 1, v], E[:, 2, u])
        out[:, 9] += _pmul_linear(minor, E[:, 0, t])
    return out


# the monomial order of the elimination and of the polish, as exponent triples
_HIDDEN = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
           (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _matrix(C, order):
    M = np.stack([C[..., i, j, k] for i, j, k in order], axis=-1)
    with np.errstate(all="ignore"):
        return M / np.max(np.abs(M), axis=-1, keepdims=True)


def _monomials(p, order):
    """p (..., 3) -> (..., 20) values, and the three gradients."""
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        m = np.stack([x ** i * y ** j * z ** k for i, j, k in order], axis=-1)
        gx = np.stack([i * x ** max(i - 1, 0) * y ** j * z ** k for i, j, k in order], axis=-1)
        gy = np.stack([j * x ** i * y ** max(j - 1, 0) * z ** k for i, j, k in order], axis=-1)
        gz = np.stack([k * x ** i * y ** j * z ** max(k - 1, 0) for i, j, k in order], axis=-1)
    return m, gx, gy, gz


def _polish(M, order, p, steps=2):
    """Gauss-Newton steps of p (H, R, 3) on the cubics M (H, 10, 20); a step that is not finite is left out."""
    for _ in range(steps):
        m, gx, gy, gz = _monomials(p, order)
        with np.errstate(all="ignore"):
            f = np.einsum("hqc,hrc->hrq", M, m)
            J = np.stack([np.einsum("hqc,hrc->hrq", M, g) for g in (gx, gy, gz)], axis=-1)      # (H, R, 10, 3)
            S = np.einsum("hrqa,hrqb->hrab", J, J)
            rhs = np.einsum("hrqa,hrq->hra", J, f)
            c = np.stack([np.cross(S[..., 1], S[..., 2]), np.cross(S[..., 2], S[..., 0]), np.cross(S[..., 0], S[..., 1])], axis=-2)
            det = np.einsum("hra,hra->hr", S[..., 0], c[..., 0, :])
            d = np.einsum("hrab,hrb->hra", c, rhs) / det[..., None]
        ok = np.isfinite(d).all(axis=-1, keepdims=True)
        p = np.where(ok, p - np.where(ok, d, 0.0), p)
    return p


def _safe(A):
    """A with every non-finite matrix of the batch replaced by zeros, and which ones were finite."""
    ok = np.isfinite(A).all(axis=(-1, -2))
    return np.where(ok[..., None, None], A, 0.0), ok


def _solve_batch(A, B):
    """A^-1 B per matrix; NaN where A is singular or not finite."""
    A, ok = _safe(A)
    out = np.full(B.shape, np.nan)
    for h in range(A.shape[0]):
        if ok[h] and np.isfinite(B[h]).all():
            try:
                out[h] = np.linalg.solve(A[h], B[h])
            except np.linalg.LinAlgError:
                pass
    return out


_XY = [(3, 0), (2, 1), (1, 2), (0, 3), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]      # the monomials in (x, y) of route 0


def _points_route0(C):
    """(H, 10, 3) complex: the solutions of the cubics C (H, 10, 4, 4, 4) as a polynomial eigenproblem in z:
    (C0 + C1 z + C2 z^2 + C3 z^3) v = 0 with v the ten monomials in (x, y), linearised in w = 1 / z (C0 is regular where C3
    never is); the ten eigenvalues of largest magnitude are the finite z."""
    H = C.shape[0]
    Ck = [np.stack([C[:, :, i, j, k] for i, j in _XY], axis=-1) for k in range(4)]
    T = np.zeros((H, 30, 30))
    T[:, 0:10, 10:20] = np.eye(10)
    T[:, 10:20, 20:30] = np.eye(10)
    T[:, 20:30, :] = -_solve_batch(Ck[0], np.concatenate((Ck[3], Ck[2], Ck[1]), axis=-1))
    T, ok = _safe(T)
    w, vec = np.linalg.eig(T)
    srt = np.argsort(-np.abs(w), axis=1, kind="stable")[:, :10]
    w = np.take_along_axis(w, srt, axis=1)
    vec = np.take_along_axis(vec, srt[:, None, :], axis=2)
    with np.errstate(all="ignore"):
        p = np.stack((vec[:, 7, :] / vec[:, 9, :], vec[:, 8, :] / vec[:, 9, :], 1.0 / w), axis=-1)
    return np.where(ok[:, None, None], p, np.nan)


def _points_route1(M):
    """(H, 10, 3) complex: the solutions of the cubics M (H, 10, 20) in the _HIDDEN order, z hidden."""
    H = M.shape[0]
    R = _solve_batch(M[:, :, :10], M[:, :, 10:])
    B = np.zeros((H, 3, 3, 5))                                          # ascending powers of z
    for t in range(3):
        e, f = R[:, 4 + 2 * t], R[:, 5 + 2 * t]
        for v, (c0, ln) in enumerate(((0, 3), (3, 3), (6, 4))):
            for q in range(ln):
                pw = ln - 1 - q
                B[:, t, v, pw] += e[:, c0 + q]
                B[:, t, v, pw + 1] -= f[:, c0 + q]
    out = np.full((H, 10, 3), np.nan, dtype=complex)
    for h in range(H):
        if not np.isfinite(B[h]).all():
            continue
        P = np.polynomial.polynomial
        det = np.zeros(1)
        for r in range(3):
            u, v = (r + 1) % 3, (r + 2) % 3
            minor = P.polysub(P.polymul(B[h, u, 0], B[h, v, 1]), P.polymul(B[h, u, 1], B[h, v, 0]))
            det = P.polyadd(det, P.polymul(minor, B[h, r, 2]))
        det = np.concatenate((det, np.zeros(11)))[:11]
        if det[10] == 0 or not np.isfinite(det / det[10]).all():
            continue
        zs = np.roots(det[::-1])
        for k, z in enumerate(zs[:10]):
            Bz = np.array([[P.polyval(z, B[h, t, v]) for v in range(3)] for t in range(3)])
            nv = np.linalg.svd(Bz)[2][-1].conj()
            with np.errstate(all="ignore"):
                out[h, k] = (nv[0] / nv[2], nv[1] / nv[2], z)
    return out


def solve_samples(a, b, route):
    """The canonical solutions of H samples, a, b (H, 5, 2) rays: E (H, 10, 3, 3) by ascending E[0, 0] with NaN beyond the
    count, and count (H,)."""
    H = a.shape[0]
    one = np.ones((H, 5, 1))
    A = np.einsum("hki,hkj->hkij", np.concatenate((b, one), axis=2), np.concatenate((a, one), axis=2)).reshape(H, 5, 9)
    A, ok = _safe(A)
    if route == 0:
        N = np.linalg.svd(A)[2][:, 5:9, :]
        order, points = _HIDDEN, _points_route0
    else:
        N = np.swapaxes(np.linalg.eigh(np.swapaxes(A, 1, 2) @ A)[1][:, :, :4], 1, 2)[:, ::-1, :]
        order, points = _HIDDEN, _points_route1
    C = _cubics(N)
    M = _matrix(C, order)
    p = points(C if route == 0 else M)
    with np.errstate(all="ignore"):
        real = np.isfinite(p).all(axis=-1) & (np.abs(p.imag) <= REAL_TOL * (1.0 + np.abs(p))).all(axis=-1) & ok[:, None]
        p = _polish(np.where(np.isfinite(M).all(axis=(1, 2))[:, None, None], M, 0.0), order, np.where(real[..., None], p.real, 0.0))
        E = np.einsum("hra,hac->hrc", np.concatenate((p, np.ones(p.shape[:2] + (1,))), axis=-1), N).reshape(H, 10, 3, 3)
    E, good = tv.canon(E)
    good = good & real & np.isfinite(E).all(axis=(-1, -2))
    key = np.where(good, E[..., 0, 0], np.inf)
    srt = np.argsort(key, axis=1, kind="stable")
    E = np.take_along_axis(E, srt[:, :, None, None], axis=1)
    good = np.take_along_axis(good, srt, axis=1)
    return np.where(good[..., None, None], E, np.nan), good.sum(axis=1)


def solve_one(a, b, route=0):
    """(n, 3, 3): the solutions of one sample, as native.essential_solve returns them."""
    E, cnt = solve_samples(np.asarray(a, dtype=np.float64)[None], np.asarray(b, dtype=np.float64)[None], route)
    return E[0, :int(cnt[0])]


# ---- the rule ------------------------------------------------------------------------------------------------------------
def _hypotheses(l, r, Kl, Kr, H, route):
    """Steps 2 to 5 of one set: (idx (H, 5), E (H, 10, 3, 3), F, have (H, 10), d2 (H, 10, n), key gap (H,))."""
    idx = sample_indices(l.shape[1], H)
    a, b = rays(Kl, l), rays(Kr, r)
    E, cnt = solve_samples(np.swapaxes(a[:, idx], 0, 1).transpose(0, 2, 1), np.swapaxes(b[:, idx], 0, 1).transpose(0, 2, 1), route)
    have = np.arange(MAX_SOL)[None, :] < cnt[:, None]
    E0 = np.where(have[..., None, None], E, 0.0)
    F, okF = to_pixels(E0, Kl, Kr)
    have_F = have & okF
    F = np.where(have_F[..., None, None], F, 0.0)
    key = np.where(have, E0[..., 0, 0], np.inf)
    with np.errstate(all="ignore"):
        gap = np.where(cnt > 1, np.min(np.where(have[:, 1:], np.diff(key, axis=1), np.inf), axis=1), np.inf)
    return idx, E0, F, have_F, tv.sampson(F, l, r), gap


def _run(l, hyp, max_err2):
    """Steps 6 to 8 of one set at one threshold: (status, best_hyp, best_root, n_valid, mask, E, F, key gap of the winner)."""
    n = l.shape[1]
    idx, E, F, have, d2, gap = hyp
    ok = tv.inliers(d2, max_err2)                                                        # (H, 10, n)
    gate = np.take_along_axis(ok, np.broadcast_to(idx[:, None, :], ok.shape[:2] + (5,)), axis=2).all(axis=2)
    valid = have & gate
    counts = np.where(valid, ok.sum(axis=2), -1).reshape(-1)
    best = int(np.argmax(counts))                                                        # the first of the largest counts
    n_valid = int(valid.sum())
    if counts[best] < MIN_COUNT:
        return NO_MODEL, -1, -1, n_valid, np.zeros(n, dtype=bool), np.zeros((3, 3)), np.zeros((3, 3)), np.inf
    h, r = divmod(best, MAX_SOL)
    return 0, h, r, n_valid, ok[h, r], E[h, r], F[h, r], float(gap[h])


def both_routes(l, r, Kl, Kr, max_hyp):
    H = hypothesis_count(l.shape[1], max_hyp)
    return tuple(_hypotheses(l, r, Kl, Kr, H, route) for route in (0, 1))


def solve_set(l, r, Kl=K, Kr=K, max_err2=MAX_ERR2, max_hyp=0, hyps=None):
    """One set: the decisions of the run at (route 0, max_err2), the settled flag, d_E and d_G over the six runs."""
    n = l.shape[1]
    c = tv.rms_coordinate(l, r)
    if n < MIN_MATCHES:
        return SimpleNamespace(status=TOO_FEW, best_hyp=-1, best_root=-1, n_valid=0, mask=np.zeros(n, dtype=bool), E=np.zeros((3, 3)),
                               F=np.zeros((3, 3)), settled=True, d_E=0.0, d_G=0.0, c=c)
    if hyps is None:
        hyps = both_routes(l, r, Kl, Kr, max_hyp)
    runs = [_run(l, hyps[route], max_err2 * f) for route in (0, 1) for f in (1.0, 1.0 - 1e-6, 1.0 + 1e-6)]
    first = runs[0]
    settled = all(o[:4] == first[:4] and np.array_equal(o[4], first[4]) for o in runs[1:]) and all(o[7] >= KEY_GAP for o in runs)
    d_E = max(float(np.max(np.abs(first[5] - o[5]))) for o in runs[1:])
    d_G = max(tv.g_difference(first[6], o[6], c) for o in runs[1:])
    return SimpleNamespace(status=first[0], best_hyp=first[1], best_root=first[2], n_valid=first[3], mask=first[4], E=first[5],
                           F=first[6], settled=bool(settled), d_E=d_E, d_G=d_G, c=c)


def reference(set_ptr, left, right, Kl=K, Kr=K, max_err2=MAX_ERR2, max_hyp=0):
    """The whole call: arrays as native.essential_ransac returns them, plus settled (S,), d_E (S,), d_G (S,), c (S,)."""
    set_ptr = np.asarray(set_ptr, dtype=np.int64)
    S, M = set_ptr.shape[0] - 1, left.shape[1]
    out = SimpleNamespace(E=np.zeros((S, 3, 3)), F=np.zeros((S, 3, 3)), inlier=np.zeros(M, dtype=np.uint8),
                          n_inliers=np.zeros(S, dtype=np.int32), best_hyp=np.zeros(S, dtype=np.int32),
                          best_root=np.zeros(S, dtype=np.int32), n_valid=np.zeros(S, dtype=np.int32), status=np.zeros(S, dtype=np.int32),
                          summary=np.zeros(6, dtype=np.int64), settled=np.zeros(S, dtype=bool), d_E=np.zeros(S), d_G=np.zeros(S),
                          c=np.zeros(S))
    for s in range(S):
        lo, hi = int(set_ptr[s]), int(set_ptr[s + 1])
        o = solve_set(left[:, lo:hi], right[:, lo:hi], Kl, Kr, max_err2, max_hyp)
        out.E[s], out.F[s], out.inlier[lo:hi], out.n_inliers[s] = o.E, o.F, o.mask, o.mask.sum()
        out.best_hyp[s], out.best_root[s], out.n_valid[s], out.status[s] = o.best_hyp, o.best_root, o.n_valid, o.status
        out.settled[s], out.d_E[s], out.d_G[s], out.c[s] = o.settled, o.d_E, o.d_G, o.c
        if o.status & TOO_FEW:
            out.summary[2] += 1
        elif o.status & NO_MODEL:
            out.summary[1] += 1
        else:
            out.summary[0] += 1
            out.summary[4] += int(o.mask.sum())
            out.summary[5] += int((~o.mask).sum())
    return out


# ---- scenes ----------------------------------------------------------------------------------------------------------------
FAMILIES = ("half_displaced", "forward", "sideways", "large_image", "offset", "rolled", "two_motions")     # the general ones
FAMILY_COUNTS = tv.FAMILY_COUNTS
PATHS_COUNTS = (0, 5, 6, 7, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
PATHS_HYP = (1, 3, 4, 5, 63, 64, 65, 128, 1000)      # on the sets of HYPS_COUNTS: the lane-group, wave and batch edges
HYPS_COUNTS = (7, 65, 300)
LONG = 1000
EVERYONE = tv.EVERYONE
TIES_HYP = 64
MANY_SIZES = (0, 5, 6, 9, 33, 70)
MANY_CYCLES = 43                      # 43 x 6 + 1 = 259 sets
# Seeds chosen on the CPU so that every set is settled (test_essential_host.py::test_every_parity_set_is_settled).
FAMILY_SEEDS = {name: (1, 1, 1) for name in FAMILIES}
PATHS_SEED = 0
TIES_SEEDS = (1, 2)
MANY_SEED = 0


def family_intrinsics(name):
    """The intrinsics of a family's images: `offset` moves every pixel, and so the principal point."""
    Km = np.array(tv.FAMILIES[name].get("K", K), dtype=np.float64)
    Km[0:2, 2] += tv.FAMILIES[name].get("offset", 0.0)
    return Km


def family_err2(name, max_err2=MAX_ERR2):
    return 16.0 * max_err2 if name == "large_image" and max_err2 != EVERYONE else max_err2


def degenerate_parts():
    """40 identical points, a noise-free pure rotation, and 60 clean matches with one NaN and one inf coordinate."""
    rng = np.random.default_rng(77)
    n = 120
    X = np.vstack((rng.uniform(-2, 2, (2, n)), rng.uniform(4, 9, (1, n))))
    l = K @ X
    l = l[:2] / l[2]
    r = K @ (tv._rot_y(0.1) @ X)
    r = r[:2] / r[2]
    same = (np.tile([[100.0], [50.0]], (1, 40)), np.tile([[120.0], [60.0]], (1, 40)), np.zeros(40, dtype=bool))
    ln, rn, bad = tv.two_views(60, 78)
    ln, rn = ln.copy(), rn.copy()
    rn[1, 17] = np.nan
    ln[0, 40] = np.inf
    return [same, (l, r, np.zeros(n, dtype=bool)), (ln, rn, bad)]


@functools.lru_cache(maxsize=None)
def scene(name):
    if name in FAMILIES:
        return tv._batch([tv.family_part(name, n, seed) for n, seed in zip(FAMILY_COUNTS, FAMILY_SEEDS[name])])
    if name == "paths":
        return tv._batch([tv.two_views(n, 1000 * PATHS_SEED + n, frac=0.1) for n in PATHS_COUNTS])
    if name == "hyps":
        return tv._batch([tv.two_views(n, 1000 * PATHS_SEED + n, frac=0.1) for n in HYPS_COUNTS])
    if name == "ties":
        return tv._batch([tv.two_views(n, seed, noise=0.0, frac=0.3) for n, seed in zip((60, 67), TIES_SEEDS)])
    if name == "many_sets":
        sizes = MANY_SIZES * MANY_CYCLES + (5,)
        return tv._batch([tv.two_views(n, 100000 * MANY_SEED + k, frac=0.1) for k, n in enumerate(sizes)])
    if name == "degenerate":
        return tv._batch(degenerate_parts())
    raise KeyError(name)


# (scene, max_err2, max_hyp)
CASES = [("paths", MAX_ERR2, 128)] + [("hyps", MAX_ERR2, h) for h in PATHS_HYP] + [(name, family_err2(name), 128) for name in FAMILIES] + \
        [("ties", EVERYONE, TIES_HYP), ("many_sets", MAX_ERR2, 16)]
UNSETTLED_CASES = [("degenerate", MAX_ERR2, 128)]      # no parity asserted: the invariants of the outputs only


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """The scene, its intrinsics and its reference, computed once per case and shared; treat all as read-only."""
    name, max_err2, max_hyp = case
    sc = scene(name)
    Km = family_intrinsics(name) if name in FAMILIES else K
    return sc, Km, reference(sc.set_ptr, sc.left, sc.right, Km, Km, max_err2, max_hyp)


def sample_of(name, n, seed, h=0):
    """The rays (5, 2), (5, 2) of hypothesis h of a noise-free general set, and its true essential matrix (canonical)."""
    kw = dict(tv.FAMILIES[name])
    kw.update(noise=0.0, frac=0.0, second_share=0.0)
    l, r, _ = tv.two_views(n, seed, **kw)
    Km = family_intrinsics(name)
    idx = sample_indices(n, h + 1)[h]
    a, b = rays(Km, l)[:, idx].T, rays(Km, r)[:, idx].T
    R = tv._rot_y(0.15) if kw.get("R") is None else np.asarray(kw["R"], dtype=np.float64)
    t = np.asarray(kw.get("t", (-1.0, 0.1, 0.2)), dtype=np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return np.ascontiguousarray(a), np.ascontiguousarray(b), tv.canon(tx @ R)[0]
