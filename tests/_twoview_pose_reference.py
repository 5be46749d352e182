"""The rule of the relative pose of a verified pair (include/sfm_hip.h, block "relative pose of a verified pair") in NumPy
float64, with a SETTLED flag per set, and the scenes the tests use.  Built like tests/_homography_reference.py.

The small algebra is done by two routes (``numpy.linalg.svd``, and ``eigh`` of E0 E0^T / Hn^T Hn with the other side's
vectors derived from the matrix), every decision about parallax is taken at ``cos2_min (1 -+ 1e-6)`` as well as at
``cos2_min``, and the in-front test is taken with d, m1, m2 compared against ``-+1e-12`` of their scale as well as against
0: 18 runs.  A set is settled iff all runs agree in candidate order, validity, every mask byte, every count, winner and
status, and the choices inside the algebra (the rank tests, the order of the two traces, the entry that fixes the sign of t,
the sign vote, l0 - l2 > 0) have a margin.  ``d_P`` is the spread of the winning (R, t, n) over the runs.

The rank tests take the singular values of ``numpy.linalg.svd`` in both routes (the square root of an eigenvalue of the
Gram matrix cannot resolve a ratio of 3 eps) and are settled iff the ratio is a factor 4 away from the bound."""
import functools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

FROM_F, FROM_H = 0, 1
EMPTY, NO_MODEL, NO_POSE, TIED, NO_PARALLAX = 1, 2, 4, 8, 16
EPS = float(np.finfo(np.float64).eps)
MIN_ANGLE_DEG = 2.0
COS2_MIN = math.cos(math.radians(MIN_ANGLE_DEG)) ** 2
MIN_PARALLAX = 8
REL = 1e-6                            # the decisions about parallax are also taken at cos2_min (1 -+ REL)
TOL = 1e-12                           # ... and the in-front test at -+TOL of the scale of d, m1, m2
GAP = 1e-9                            # the margin of the choices inside the algebra

K_LEFT = np.array([[800.0, 0.5, 320.0], [0.0, 780.0, 240.0], [0.0, 0.0, 1.0]])
K_RIGHT = np.array([[790.0, -0.25, 330.0], [0.0, 805.0, 236.0], [0.0, 0.0, 1.0]])


# ---- the test of step 4 with exact fused multiply-adds (scalar; for the host hook) -----------------------------------------
def fma(a, b, c):
    """round(a b + c) with one rounding, as __builtin_fma gives it."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        return a * b + c              # the sign of a zero sum follows the operands: the plain expression has it
    try:
        return float(exact)
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def pose_test_exact(R, t, a, b, cos2_min):
    """(front, parallax) of one match in the operation order the header states."""
    R = [float(v) for v in np.asarray(R).reshape(9)]
    t = [float(v) for v in t]
    a0, a1, b0, b1 = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    with np.errstate(all="ignore"):
        ap = [fma(R[3 * i], a0, fma(R[3 * i + 1], a1, R[3 * i + 2])) for i in range(3)]
        p = fma(ap[0], ap[0], fma(ap[1], ap[1], _mul(ap[2], ap[2])))
        q = fma(b0, b0, fma(b1, b1, 1.0))
        r = fma(ap[0], b0, fma(ap[1], b1, ap[2]))
        d = fma(p, q, -_mul(r, r))
        bt = fma(b0, t[0], fma(b1, t[1], t[2]))
        at = fma(ap[0], t[0], fma(ap[1], t[1], _mul(ap[2], t[2])))
        m1 = fma(r, bt, -_mul(q, at))
        m2 = fma(p, bt, -_mul(r, at))
        front = all(math.isfinite(v) for v in (d, m1, m2)) and d > 0.0 and m1 > 0.0 and m2 > 0.0
        narrow = r > 0.0 and _mul(r, r) > _mul(cos2_min, _mul(p, q))
    return int(front), int(front and not narrow)


def _mul(a, b):
    return float(np.float64(a) * np.float64(b))


# ---- the pieces of the rule ------------------------------------------------------------------------------------------------
def rays(K, p):
    """(2, n): the first two components of K^-1 (x, y, 1) by back substitution."""
    with np.errstate(all="ignore"):
        r1 = (p[1] - K[1, 2]) / K[1, 1]
        r0 = (p[0] - K[0, 1] * r1 - K[0, 2]) / K[0, 0]
    return np.vstack((r0, r1))


def canon3(t):
    """(t / |t| with the entry of largest magnitude positive, the sign applied, valid, settled)."""
    with np.errstate(all="ignore"):
        mag = np.abs(t)
        k = int(np.argmax(mag)) if np.all(np.isfinite(t)) else 0
        sign = -1.0 if t[k] < 0 else 1.0
        ss = float(t @ t)
        valid = bool(np.isfinite(ss) and ss > 0.0)
        out = t / (sign * np.sqrt(ss))
        rest = np.delete(mag, k)
        settled = (not valid) or bool(np.all(mag[k] - rest > GAP * np.sqrt(ss)))
    return out, sign, valid, settled


def _rank_test(M, index):
    """(valid, settled) of s[index] > 3 eps s[0] with the singular values of M."""
    if not np.all(np.isfinite(M)):
        return False, True
    s = np.linalg.svd(M, compute_uv=False)
    bound = 3.0 * EPS * s[0]
    valid = bool(s[index] > bound)
    settled = bool(s[index] > 4.0 * bound or s[index] < 0.25 * bound or s[0] == 0.0)
    return valid, settled


def _emit(R, t, nrm, ok):
    """The four candidates of two rotations: the larger trace first.  Returns (R (4, 3, 3), t (4, 3), n (4, 3), ok (4,), settled)."""
    with np.errstate(all="ignore"):
        tr = [float(np.trace(R[0])), float(np.trace(R[1]))]
        first = 1 if tr[1] > tr[0] else 0
        settled = bool(abs(tr[1] - tr[0]) > GAP) or not (ok[0] or ok[1])
    Rs, ts, ns, oks = np.zeros((4, 3, 3)), np.zeros((4, 3)), np.zeros((4, 3)), np.zeros(4, dtype=bool)
    for i in range(2):
        src = first if i == 0 else 1 - first
        for j in range(2):
            if ok[src]:
                sg = -1.0 if j else 1.0
                Rs[2 * i + j], ts[2 * i + j], ns[2 * i + j], oks[2 * i + j] = R[src], sg * t[src], sg * nrm[src], True
    return Rs, ts, ns, oks, settled


def _none():
    return SimpleNamespace(R=np.zeros((4, 3, 3)), t=np.zeros((4, 3)), n=np.zeros((4, 3)), ok=np.zeros(4, dtype=bool), model_ok=False,
                           settled=True)


def candidates_f(F, Kl, Kr, route):
    with np.errstate(all="ignore"):
        E = Kr.T @ F @ Kl
        valid, settled = _rank_test(E, 1)
        if not valid:
            c = _none()
            c.settled = settled
            return c
        if route == 0:
            U, _s, Vt = np.linalg.svd(E)
            u0, u1, v0, v1 = U[:, 0], U[:, 1], Vt[0], Vt[1]
        else:
            _w, U = np.linalg.eigh(E @ E.T)
            u0, u1 = U[:, 2], U[:, 1]
            v0, v1 = E.T @ u0, E.T @ u1
            v0, v1 = v0 / np.linalg.norm(v0), v1 / np.linalg.norm(v1)
        u2, v2 = np.cross(u0, u1), np.cross(v0, v1)
        skew = np.outer(u1, v0) - np.outer(u0, v1)
        axis = np.outer(u2, v2)
        R = [axis + skew, axis - skew]
        t0, _sign, tok, tset = canon3(u2)
        ok = bool(valid and tok and np.all(np.isfinite(R[0])) and np.all(np.isfinite(R[1])))
        Rs, ts, ns, oks, oset = _emit(R, [t0, t0], [np.zeros(3), np.zeros(3)], [ok, ok])
    return SimpleNamespace(R=Rs, t=ts, n=ns, ok=oks, model_ok=ok, settled=settled and tset and oset)


def candidates_h(H, Kl, Kr, a, b, route):
    """a, b (2, m): the rays of the selected matches (the sign vote)."""
    with np.errstate(all="ignore"):
        P = H @ Kl
        Hn = np.zeros((3, 3))
        Hn[2] = P[2]
        Hn[1] = (P[1] - Kr[1, 2] * Hn[2]) / Kr[1, 1]
        Hn[0] = (P[0] - Kr[0, 1] * Hn[1] - Kr[0, 2] * Hn[2]) / Kr[0, 0]
        valid, settled = _rank_test(Hn, 2)
        if not valid:
            c = _none()
            c.settled = settled
            return c
        if route == 0:
            _U, s, Vt = np.linalg.svd(Hn)
            v0, v1, s1 = Vt[0], Vt[1], s[1]
            l0, l2 = (s[0] / s1) ** 2, (s[2] / s1) ** 2
        else:
            w, V = np.linalg.eigh(Hn.T @ Hn)
            v0, v1, s1 = V[:, 2], V[:, 1], np.sqrt(w[1])
            l0, l2 = w[2] / w[1], w[0] / w[1]
        Hs = Hn / s1
        ah = np.vstack((a, np.ones((1, a.shape[1]))))
        bh = np.vstack((b, np.ones((1, b.shape[1]))))
        Ha = Hs @ ah
        vote = (bh * Ha).sum(axis=0)
        scale = (np.abs(bh) * np.abs(Ha)).sum(axis=0) * TOL
        pos, neg = int((vote > 0).sum()), int((vote < 0).sum())
        unsure = int((np.abs(vote) <= scale).sum())
        settled = settled and (abs(pos - neg) > unsure or unsure == 0)
        if neg > pos:
            Hs = -Hs
        v2 = np.cross(v0, v1)
        valid = bool(l0 - l2 > 0.0)
        settled = settled and bool(l0 - l2 > GAP)
        if not valid:
            c = _none()
            c.settled = settled
            return c
        al, be, den = np.sqrt(max(1.0 - l2, 0.0)), np.sqrt(max(l0 - 1.0, 0.0)), np.sqrt(l0 - l2)
        R, t, nrm, ok = [], [], [], []
        for sb in (be, -be):
            u = (al * v0 + sb * v2) / den
            n = np.cross(v1, u)
            w1, hu = Hs @ v1, Hs @ u
            Ri = np.outer(w1, v1) + np.outer(hu, u) + np.outer(np.cross(w1, hu), n)
            T = (Hs - Ri) @ n
            t0, sign, tok, tset = canon3(T)
            good = bool(tok and np.all(np.isfinite(Ri)))
            settled = settled and (tset or not good) and bool(np.linalg.norm(T) > GAP or not good)
            R.append(Ri); t.append(t0); nrm.append(sign * n); ok.append(good)
        Rs, ts, ns, oks, oset = _emit(R, t, nrm, ok)
    return SimpleNamespace(R=Rs, t=ts, n=ns, ok=oks, model_ok=True, settled=settled and oset)


def front_terms(R, t, a, b):
    """p, q, r, d, m1, m2, a' of the matches a, b (2, n) against (R, t), each (n,) (a' (3, n)), and the scales of d, m1, m2."""
    with np.errstate(all="ignore"):
        ap = R[:, 0:1] * a[0] + R[:, 1:2] * a[1] + R[:, 2:3]
        p = (ap * ap).sum(axis=0)
        q = b[0] * b[0] + b[1] * b[1] + 1.0
        r = ap[0] * b[0] + ap[1] * b[1] + ap[2]
        d = p * q - r * r
        bt = b[0] * t[0] + b[1] * t[1] + t[2]
        at = ap[0] * t[0] + ap[1] * t[1] + ap[2] * t[2]
        m1, m2 = r * bt - q * at, p * bt - r * at
        sd = p * q + r * r
        s1 = np.abs(r * bt) + np.abs(q * at)
        s2 = np.abs(p * bt) + np.abs(r * at)
    return SimpleNamespace(ap=ap, p=p, q=q, r=r, d=d, m1=m1, m2=m2, sd=sd, s1=s1, s2=s2)


def front_of(w, sel, cos2, tol):
    """(front, parallax) boolean (n,) of the terms w over the selected matches."""
    with np.errstate(all="ignore"):
        finite = np.isfinite(w.d) & np.isfinite(w.m1) & np.isfinite(w.m2)
        front = sel & finite & (w.d > tol * w.sd) & (w.m1 > tol * w.s1) & (w.m2 > tol * w.s2)
        narrow = (w.r > 0.0) & (w.r * w.r > cos2 * (w.p * w.q))
    return front, front & ~narrow


def midpoints(R, t, a, b):
    """(3, n): the midpoint (lambda1 a' + t + lambda2 b) / 2 of every match, taken back to the left frame."""
    w = front_terms(R, t, a, b)
    with np.errstate(all="ignore"):
        l1, l2 = w.m1 / w.d, w.m2 / w.d
        bh = np.vstack((b, np.ones((1, a.shape[1]))))
        mid = 0.5 * (l1 * w.ap + t[:, None] + l2 * bh)
        return R.T @ (mid - t[:, None])


def _decide(c, a, b, sel, terms, cos2, tol, min_parallax):
    n = a.shape[1]
    counts = np.full(4, -1, dtype=np.int64)
    fronts = [None] * 4
    for k in range(4):
        if c.ok[k]:
            fronts[k] = front_of(terms[k], sel, cos2, tol)
            counts[k] = int(fronts[k][0].sum())
    best, best_cnt = -1, 0
    for k in range(4):
        if c.ok[k] and counts[k] > best_cnt:
            best, best_cnt = k, int(counts[k])
    status = 0
    if not sel.any():
        status |= EMPTY
    if not c.model_ok:
        status |= NO_MODEL
    obs = np.zeros(n, dtype=np.uint8)
    n_front = n_par = 0
    if best < 0:
        status |= NO_POSE
    else:
        if any(c.ok[k] and k != best and counts[k] == best_cnt for k in range(4)):
            status |= TIED
        front, par = fronts[best]
        obs = front.astype(np.uint8) + par.astype(np.uint8)
        n_front, n_par = int(front.sum()), int(par.sum())
        if n_par < min_parallax:
            status |= NO_PARALLAX
    return SimpleNamespace(counts=counts, best=best, status=status, obs=obs, n_front=n_front, n_par=n_par)


def solve_set(l, r, mask, model, kind, Kl=K_LEFT, Kr=K_RIGHT, cos2_min=COS2_MIN, min_parallax=MIN_PARALLAX):
    """One set: l, r (2, n) pixel coordinates, mask (n,) bool.  Returns the outputs of the set, `settled` and `d_P`."""
    n = l.shape[1]
    a, b = rays(Kl, l), rays(Kr, r)
    with np.errstate(all="ignore"):
        sel = np.asarray(mask, dtype=bool) & np.isfinite(a).all(axis=0) & np.isfinite(b).all(axis=0)
    model = np.asarray(model, dtype=np.float64).reshape(3, 3)
    runs, settled, cands = [], True, []
    for route in (0, 1):
        c = candidates_f(model, Kl, Kr, route) if kind == FROM_F else candidates_h(model, Kl, Kr, a[:, sel], b[:, sel], route)
        settled = settled and c.settled
        cands.append(c)
        terms = [front_terms(c.R[k], c.t[k], a, b) if c.ok[k] else None for k in range(4)]
        for cos2 in (cos2_min, cos2_min * (1.0 - REL), min(cos2_min * (1.0 + REL), 1.0)):
            for tol in (0.0, -TOL, TOL):
                runs.append((route, _decide(c, a, b, sel, terms, cos2, tol, min_parallax)))
    first = runs[0][1]
    c0 = cands[0]
    settled = settled and np.array_equal(cands[0].ok, cands[1].ok) and cands[0].model_ok == cands[1].model_ok
    d_P = 0.0
    for route, run in runs:
        settled = settled and (np.array_equal(run.counts, first.counts) and run.best == first.best and run.status == first.status
                               and np.array_equal(run.obs, first.obs) and run.n_par == first.n_par)
    if first.best >= 0 and cands[1].ok[first.best]:
        k = first.best
        d_P = max(float(np.abs(cands[1].R[k] - c0.R[k]).max()), float(np.abs(cands[1].t[k] - c0.t[k]).max()),
                  float(np.abs(cands[1].n[k] - c0.n[k]).max()))
    # the candidate order: the same rotations and translations at the same numbers in both routes
    with np.errstate(all="ignore"):
        for k in range(4):
            if cands[0].ok[k] and cands[1].ok[k]:
                settled = settled and bool(np.abs(cands[1].R[k] - c0.R[k]).max() < 1e-6 and np.abs(cands[1].t[k] - c0.t[k]).max() < 1e-6)
    won = first.best >= 0
    R = c0.R[first.best] if won else np.zeros((3, 3))
    t = c0.t[first.best] if won else np.zeros(3)
    nrm = c0.n[first.best] if won else np.zeros(3)
    X = np.full((3, n), np.nan)
    d_X = 0.0
    if won:
        in_front = first.obs > 0
        X[:, in_front] = midpoints(R, t, a, b)[:, in_front]
        if cands[1].ok[first.best] and in_front.any():      # the spread of the points themselves over the two routes, relative
            other = midpoints(cands[1].R[first.best], cands[1].t[first.best], a, b)[:, in_front]
            with np.errstate(all="ignore"):
                d_X = float((np.abs(other - X[:, in_front]).max(axis=0) / np.linalg.norm(X[:, in_front], axis=0)).max())
    return SimpleNamespace(R=R, t=t, n=nrm, cand_front=first.counts.astype(np.int32), n_front=first.n_front, n_parallax=first.n_par,
                           best=first.best, status=first.status, obs=first.obs, X=X, settled=bool(settled), d_P=d_P, d_X=d_X, n_sel=int(sel.sum()),
                           cands=c0)


def reference(set_ptr, left, right, mask, models, kinds, Kl=K_LEFT, Kr=K_RIGHT, cos2_min=COS2_MIN, min_parallax=MIN_PARALLAX):
    set_ptr = np.asarray(set_ptr)
    S, M = set_ptr.shape[0] - 1, left.shape[1]
    mask = np.ones(M, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    out = SimpleNamespace(R=np.zeros((S, 3, 3)), t=np.zeros((S, 3)), n=np.zeros((S, 3)), cand_front=np.zeros((S, 4), dtype=np.int32),
                          n_front=np.zeros(S, dtype=np.int32), n_parallax=np.zeros(S, dtype=np.int32), best=np.zeros(S, dtype=np.int32),
                          status=np.zeros(S, dtype=np.int32), obs=np.zeros(M, dtype=np.uint8), X=np.full((3, M), np.nan),
                          settled=np.zeros(S, dtype=bool), d_P=np.zeros(S), d_X=np.zeros(S), summary=np.zeros(6, dtype=np.int64), sets=[])
    for s in range(S):
        lo, hi = int(set_ptr[s]), int(set_ptr[s + 1])
        q = solve_set(left[:, lo:hi], right[:, lo:hi], mask[lo:hi], models[s], int(kinds[s]), Kl, Kr, cos2_min, min_parallax)
        out.R[s], out.t[s], out.n[s], out.cand_front[s] = q.R, q.t, q.n, q.cand_front
        out.n_front[s], out.n_parallax[s], out.best[s], out.status[s] = q.n_front, q.n_parallax, q.best, q.status
        out.obs[lo:hi], out.X[:, lo:hi], out.settled[s], out.d_P[s] = q.obs, q.X, q.settled, q.d_P
        out.d_X[s] = q.d_X
        out.sets.append(q)
        if q.best >= 0:
            out.summary[0] += 1
            out.summary[3] += bool(q.status & TIED)
            out.summary[4] += q.n_front
            out.summary[5] += q.n_sel - q.n_front
        else:
            out.summary[2 if q.status & EMPTY else 1] += 1
    return out


# ---- scenes --------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.identity(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.identity(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


PLANE_N, PLANE_D = _unit([0.3, -0.2, 1.0]), 6.0
# family: (rotation vector, translation (unit, or None: the camera only rotates), depth range, on the plane, kind)
FAMILIES = {
    "general": ((0.05, -0.10, 0.03), _unit([1.0, 0.12, 0.05]), (4.0, 8.0), False, FROM_F),
    "forward": ((0.02, 0.03, -0.04), _unit([0.03, -0.05, 1.0]), (4.0, 8.0), False, FROM_F),
    "plane": ((0.04, -0.12, 0.02), _unit([1.0, -0.2, 0.1]), None, True, FROM_H),
    "rotation": ((0.03, -0.15, 0.05), None, (4.0, 8.0), False, FROM_H),
    "behind": ((0.05, -0.10, 0.03), _unit([1.0, 0.12, 0.05]), (-8.0, -4.0), False, FROM_F),
}
NOISE_PX = 0.3
# For a camera that only rotated the two rays of a match are parallel but for the noise of the keys, and the midpoint
# divides by d = p q - r r, of the order of (noise / focal length)^2: at 0.3 px the reference's OWN two routes differ by
# 4e-8 in X (d_X), forty times the bound max(1e-9, 100 d_P) the GPU tests apply to X -- no computation of the rule can be
# held to that bound there.  The keys of this family carry 2 px, at which the reference meets the bound itself (every set
# of every scene has to: tests/test_twoview_pose_host.py) and no match reaches two degrees of parallax.
FAMILY_NOISE = {"rotation": 2.0}
FAMILY_COUNTS = (40, 130, 300)
SIZES = (0, 1, 4, 63, 64, 65, 1023, 1024, 1025, 2049)
MANY_SIZES = (0, 4, 5, 12, 33, 70)
MANY_CYCLES = 43                      # 43 x 6 + 1 = 259 sets


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def planted(name):
    rv, t, _depth, _plane, _kind = FAMILIES[name]
    return rodrigues(rv), (np.zeros(3) if t is None else t)


def fit_homography(l, r):
    """The least-squares homography of the matches (Hartley-normalised DLT), Frobenius norm 1."""
    def norm(p):
        m = p.mean(axis=1)
        s = math.sqrt(2.0) / np.sqrt(((p - m[:, None]) ** 2).sum(axis=0)).mean()
        return np.array([[s, 0, -s * m[0]], [0, s, -s * m[1]], [0, 0, 1.0]])
    Tl, Tr = norm(l), norm(r)
    p, q = Tl[0, 0] * l + Tl[0:2, 2:3], Tr[0, 0] * r + Tr[0:2, 2:3]
    n = l.shape[1]
    A = np.zeros((2 * n, 9))
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = -p[0], -p[1], -1.0
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = q[0] * p[0], q[0] * p[1], q[0]
    A[1::2, 3], A[1::2, 4], A[1::2, 5] = -p[0], -p[1], -1.0
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = q[1] * p[0], q[1] * p[1], q[1]
    h = np.linalg.svd(A)[2][-1].reshape(3, 3)
    H = np.linalg.inv(Tr) @ h @ Tl
    return H / np.linalg.norm(H)


def family_part(name, n, seed, displaced_share=0.0, noise=None, Kl=K_LEFT, Kr=K_RIGHT):
    """(left (2, n), right (2, n), displaced (n,) bool, model (3, 3), kind) of one set of the family."""
    rv, t, depth, on_plane, kind = FAMILIES[name]
    noise = FAMILY_NOISE.get(name, NOISE_PX) if noise is None else noise
    rng = np.random.default_rng([seed, n, sorted(FAMILIES).index(name)])
    R, tt = planted(name)
    xy = rng.uniform(-2.0, 2.0, size=(2, n))
    if on_plane:
        z = (PLANE_D - PLANE_N[0] * xy[0] - PLANE_N[1] * xy[1]) / PLANE_N[2]
    else:
        z = rng.uniform(depth[0], depth[1], size=n)
    X = np.vstack((xy * (np.abs(z) / 6.0), z))
    if on_plane:
        X = np.vstack((xy, z))
    Y = R @ X + tt[:, None]
    l = (Kl @ (X / X[2]))[:2] + noise * rng.standard_normal((2, n))
    r = (Kr @ (Y / Y[2]))[:2] + noise * rng.standard_normal((2, n))
    displaced = np.zeros(n, dtype=bool)
    if displaced_share > 0 and n > 0:
        displaced[rng.permutation(n)[: int(round(displaced_share * n))]] = True
        r[:, displaced] += rng.uniform(30.0, 120.0, size=(2, int(displaced.sum()))) * rng.choice([-1.0, 1.0], size=(2, int(displaced.sum())))
    if kind == FROM_F:
        model = np.linalg.inv(Kr).T @ (skew(tt) @ R) @ np.linalg.inv(Kl)
    elif on_plane:
        model = Kr @ (R + np.outer(tt, PLANE_N) / PLANE_D) @ np.linalg.inv(Kl)
    elif noise > 0:                   # the camera only rotated: the homography fitted to 60 noisy matches of the same motion
        fit_rng = np.random.default_rng([seed, n, 1000])
        Xf = np.vstack((fit_rng.uniform(-2.0, 2.0, size=(2, 60)), fit_rng.uniform(depth[0], depth[1], size=(1, 60))))
        Yf = R @ Xf
        model = fit_homography((Kl @ (Xf / Xf[2]))[:2] + noise * fit_rng.standard_normal((2, 60)),
                               (Kr @ (Yf / Yf[2]))[:2] + noise * fit_rng.standard_normal((2, 60)))
    else:                             # ... or K R K^-1 itself
        model = Kr @ R @ np.linalg.inv(Kl)
    return l, r, displaced, model / np.linalg.norm(model), kind


def _assemble(parts):
    counts = np.array([p[0].shape[1] for p in parts], dtype=np.int64)
    set_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    left = np.ascontiguousarray(np.hstack([p[0] for p in parts])) if parts else np.zeros((2, 0))
    right = np.ascontiguousarray(np.hstack([p[1] for p in parts])) if parts else np.zeros((2, 0))
    displaced = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, dtype=bool)
    models = np.stack([p[3] for p in parts]) if parts else np.zeros((0, 3, 3))
    kinds = np.array([p[4] for p in parts], dtype=np.int32)
    return SimpleNamespace(set_ptr=set_ptr, left=left, right=right, displaced=displaced, mask=~displaced, models=models, kinds=kinds,
                           counts=counts, names=[p[5] if len(p) > 5 else "" for p in parts])


FAMILY_SEEDS = {name: (2, 4, 6) if name == "forward" else (1, 2, 3) for name in FAMILIES}    # seeds at which every set is settled
SIZES_SEED, MANY_SEED, SPECIAL_SEED = 4, 5, 6


@functools.lru_cache(maxsize=None)
def scene(name):
    """Scenes: "<family>" / "<family>_displaced" (three sets), "sizes" (every set size, general F and plane H alternating),
    "many" (259 small sets of every family, clean and displaced), "special" (the degenerate inputs)."""
    if name.split("_")[0] in FAMILIES:
        fam = name.split("_")[0]
        share = 0.1 if name.endswith("_displaced") else 0.0
        return _assemble([family_part(fam, n, seed, share) + (fam,) for n, seed in zip(FAMILY_COUNTS, FAMILY_SEEDS[fam])])
    if name == "sizes":
        return _assemble([family_part(("general", "plane")[i % 2], n, SIZES_SEED + i, 0.1 if i % 3 == 0 else 0.0) + (("general", "plane")[i % 2],)
                          for i, n in enumerate(SIZES)])
    if name == "many":
        fams = sorted(FAMILIES)
        sizes = list(MANY_SIZES) * MANY_CYCLES + [MANY_SIZES[0]]
        return _assemble([family_part(fams[i % 5], n, MANY_SEED + i, 0.1 if (i // 5) % 2 else 0.0) + (fams[i % 5],)
                          for i, n in enumerate(sizes)])
    if name == "special":
        parts = []
        g = family_part("general", 70, SPECIAL_SEED)
        p = family_part("plane", 70, SPECIAL_SEED)
        parts.append(g + ("masked_out",))                                       # 0: a mask of zeros (set below)
        l, r = g[0].copy(), g[1].copy()
        r[1, 17] = np.nan
        l[0, 40] = np.nan
        parts.append((l, r) + g[2:] + ("nan_coordinate",))                      # 1: two matches with a NaN coordinate
        parts.append(g + ("clean_general",))                                    # 2: the same set without them
        rank1 = np.zeros((3, 3)); rank1[2, 2] = 1.0
        parts.append(g[:3] + (rank1, FROM_F, "rank1_F"))                        # 3: E0 = e2 e2^T exactly
        sing = p[3].copy(); sing[:, 0] = 0.0
        parts.append(p[:3] + (sing, FROM_H, "singular_H"))                      # 4: a zero column
        parts.append(g[:3] + (np.full((3, 3), np.nan), FROM_F, "nan_F"))        # 5
        nanh = p[3].copy(); nanh[1, 1] = np.nan
        parts.append(p[:3] + (nanh, FROM_H, "nan_H"))                           # 6
        parts.append(p + ("clean_plane",))                                      # 7
        parts.append(g[:3] + (np.zeros((3, 3)), FROM_H, "zero_H"))              # 8
        sc = _assemble(parts)
        sc.mask = sc.mask.copy()
        sc.mask[sc.set_ptr[0]:sc.set_ptr[1]] = False
        return sc
    raise KeyError(name)


NO_MASK_CASE = "general_displaced"     # ... run once more with every match voting
OPTION_SCENE = "forward"              # ... and this one at other options: (cos2_min, min_parallax)
OPTION_CASES = ((0.0, 0), (1.0, 1), (COS2_MIN, 0), (0.9999, 1000))
FAMILY_CASES = [f + suffix for f in FAMILIES for suffix in ("", "_displaced")]
CASES = FAMILY_CASES + ["sizes", "many", "special"]


@functools.lru_cache(maxsize=None)
def scene_and_reference(name):
    sc = scene(name)
    return sc, reference(sc.set_ptr, sc.left, sc.right, sc.mask, sc.models, sc.kinds)


def subset(sc, sets):
    """The scene of the sets `sets` of sc alone."""
    sets = list(sets)
    cols = np.concatenate([np.arange(sc.set_ptr[s], sc.set_ptr[s + 1]) for s in sets]) if sets else np.zeros(0, dtype=int)
    counts = sc.counts[sets]
    return SimpleNamespace(set_ptr=np.concatenate(([0], np.cumsum(counts))).astype(np.int32), left=np.ascontiguousarray(sc.left[:, cols]),
                           right=np.ascontiguousarray(sc.right[:, cols]), mask=sc.mask[cols], models=sc.models[sets], kinds=sc.kinds[sets],
                           counts=counts, cols=cols)


def pose_distance(R, t, R0, t0):
    return max(float(np.abs(R - R0).max()), float(np.abs(t - t0).max()))


def to_reference_convention(R, t):
    """(rot, centre) as extract_cam_pose_from_essential_mat returns them: rot = R^T, centre = -R^T t (3, 1)."""
    return R.T.copy(), (-R.T @ t).reshape(3, 1)
