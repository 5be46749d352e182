"""The rule of the refinement of a relative pose (include/sfm_hip.h, block "refinement of a relative pose") in NumPy float64,
with a SETTLED flag per set, and the scenes the tests use.  Built like tests/_twoview_pose_reference.py, whose families,
intrinsics and helpers it takes.

The iteration is done by two routes: the 21 sums per slice of 64 consecutive matches added in slice order and a 5x5 Cholesky
factorisation written out here, and plain ``J @ J.T`` with ``numpy.linalg.lstsq`` on the damped system.  The judge's decisions
are also taken at ``max_err2 (1 -+ 1e-6)``, and the in-front test with ``cos2_min`` and its tolerance varied as
``_twoview_pose_reference`` varies them.  A set is settled iff all runs agree in status, n_used, every mask byte, every count
and the guard's decision, and the guard's ratio c_out / c_in is 1e-6 away from ``1 + 2^-30``.  ``d_P`` is the spread of the
two routes' (R_out, t_out)."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import _twoview_pose_reference as tp

EMPTY, TOO_FEW, BAD_POSE, SINGULAR, NONFINITE, KEPT_INPUT = 1, 2, 4, 8, 16, 32
MIN_USED = 8
GUARD = 1.0 + 2.0 ** -30
GUARD_MARGIN = 1e-6
REL = 1e-6                            # the inlier decisions are also taken at max_err2 (1 -+ REL)
ITERS, LAMBDA = 6, 0.0
MAX_ERR2 = 4.0                        # two pixels
K_LEFT, K_RIGHT, COS2_MIN = tp.K_LEFT, tp.K_RIGHT, tp.COS2_MIN
TRIU = np.triu_indices(5)


# ---- the pieces of the rule ------------------------------------------------------------------------------------------------
def basis(t):
    """(b1, b2) of the chart of t: k the index of the smallest |t_k|, the lowest on a tie."""
    k = int(np.argmin(np.abs(t)))
    e = np.zeros(3)
    e[k] = 1.0
    c = np.cross(t, e)
    b1 = c / np.linalg.norm(c)
    return b1, np.cross(t, b1)


def model(R, t, Kl=K_LEFT, Kr=K_RIGHT):
    """(F (3, 3), dF (5, 3, 3), b1, b2) of the pose (R, t) as given."""
    with np.errstate(all="ignore"):
        il, irt = np.linalg.inv(Kl), np.linalg.inv(Kr).T
        b1, b2 = basis(t)
        dE = [tp.skew(t) @ tp.skew(e) @ R for e in np.identity(3)] + [tp.skew(b1) @ R, tp.skew(b2) @ R]
        return irt @ (tp.skew(t) @ R) @ il, np.stack([irt @ d @ il for d in dE]), b1, b2


def residuals(F, dF, l, r):
    """(r (n,), J (5, n)) of the matches l, r (2, n) against F and its derivatives."""
    n = l.shape[1]
    with np.errstate(all="ignore"):
        x, y = np.vstack((l, np.ones((1, n)))), np.vstack((r, np.ones((1, n))))
        a, b = F @ x, F.T @ y
        e = (y * a).sum(axis=0)
        s = a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2
        res = e / np.sqrt(s)
        J = np.zeros((5, n))
        for j in range(5):
            da, db = dF[j] @ x, dF[j].T @ y
            J[j] = (y * da).sum(axis=0) / np.sqrt(s) - e * (a[0] * da[0] + a[1] * da[1] + b[0] * db[0] + b[1] * db[1]) / s ** 1.5
    return res, J


def move(R, t, b1, b2, d):
    with np.errstate(all="ignore"):
        u = t + d[3] * b1 + d[4] * b2
        return tp.rodrigues(d[:3]) @ R, u / np.linalg.norm(u)


def _sums(route, res, J):
    """(c, U (5, 5), g (5,)) of the residuals and Jacobian rows, the unselected ones already zero."""
    with np.errstate(all="ignore"):
        if route == 1:
            return float(res @ res), J @ J.T, J @ res
        c, U, g = 0.0, np.zeros((5, 5)), np.zeros(5)
        for lo in range(0, res.shape[0], 64):         # slices of 64 consecutive matches, added in slice order
            rs, Js = res[lo:lo + 64], J[:, lo:lo + 64]
            c = c + float((rs * rs).sum())
            U = U + (Js[:, None, :] * Js[None, :, :]).sum(axis=2)
            g = g + (Js * rs).sum(axis=1)
        return c, U, g


def cholesky_solve(A, rhs):
    """(x, ok): A x = rhs by the Cholesky factorisation of the rule; not ok if a pivot is not finite or not > 0."""
    L = np.zeros((5, 5))
    with np.errstate(all="ignore"):
        for j in range(5):
            p = A[j, j] - float(L[j, :j] @ L[j, :j])
            if not (math.isfinite(p) and p > 0.0):
                return np.zeros(5), False
            L[j, j] = math.sqrt(p)
            for i in range(j + 1, 5):
                L[i, j] = (A[j, i] - float(L[i, :j] @ L[j, :j])) / L[j, j]
        y = np.zeros(5)
        for i in range(5):
            y[i] = (rhs[i] - float(L[i, :i] @ y[:i])) / L[i, i]
        x = np.zeros(5)
        for i in range(4, -1, -1):
            x[i] = (y[i] - float(L[i + 1:, i] @ x[i + 1:])) / L[i, i]
    return x, True


def _step(route, U, g, lam):
    A = U + lam * np.diag(np.diag(U))
    if route == 0:
        return cholesky_solve(A, -g)
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(g))):
        return np.zeros(5), False
    d, _res, rank, sv = np.linalg.lstsq(A, -g, rcond=None)
    return d, bool(rank == 5 and np.all(np.diag(A) > 0.0))


def canon9(F):
    """F scaled to Frobenius norm 1 with its entry of largest magnitude (the first of them) positive, or zeros."""
    with np.errstate(all="ignore"):
        f = F.reshape(9)
        ss = float(f @ f)
        if not (math.isfinite(ss) and ss > 0.0):
            return np.zeros((3, 3)), False
        k = int(np.argmax(np.abs(f)))
        return F / ((-1.0 if f[k] < 0 else 1.0) * math.sqrt(ss)), True


def iterate(route, l, r, sel, R_in, t_in, Kl, Kr, lam, iters):
    """Steps 2, 5 to 8 of the rule for one set by one route."""
    n_used = int(sel.sum())
    with np.errstate(all="ignore"):
        ss = float(t_in @ t_in)
        good = bool(np.all(np.isfinite(R_in)) and np.all(np.isfinite(t_in)) and math.isfinite(ss) and ss > 0.0)
    status = 0 if good else BAD_POSE
    if n_used == 0:
        status |= EMPTY
    if n_used < MIN_USED:
        status |= TOO_FEW
    out = SimpleNamespace(R=R_in.copy(), t=t_in.copy(), cost=np.zeros(2), info=np.zeros((5, 5)), status=status | KEPT_INPUT, n_used=n_used,
                          ratio=None, moved=False, grad=np.zeros(2))
    if status:
        return out
    R, t = R_in.copy(), t_in / math.sqrt(ss)
    steps, c_in, U_in, grad = 0, 0.0, None, [0.0, 0.0]
    for p in range(iters + 1):
        F, dF, b1, b2 = model(R, t, Kl, Kr)
        res, J = residuals(F, dF, l, r)
        res, J = np.where(sel, res, 0.0), np.where(sel[None, :], J, 0.0)
        c, U, g = _sums(route, res, J)
        if p == 0:
            c_in, U_in, grad[0] = c, U, float(np.abs(g).max())
        stop = p == iters
        if not stop:
            d, ok = _step(route, U, g, lam)
            if ok:
                R, t = move(R, t, b1, b2, d)
                steps += 1
            else:
                status |= SINGULAR
                stop = True
        c_out, U_out, grad[1] = c, U, float(np.abs(g).max())
        if stop:
            break
    moved = steps > 0
    if moved:
        finite = bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and math.isfinite(c_in) and math.isfinite(c_out))
        if not finite:
            status |= NONFINITE
        moved = finite and c_out <= c_in * GUARD
        out.ratio = c_out / c_in if finite and c_in > 0 else None
    elif not math.isfinite(c_in):
        status |= NONFINITE
    if moved:
        out.R, out.t, out.cost, out.info = R, t, np.array([c_in, c_out]), U_out
    else:
        status |= KEPT_INPUT
        out.cost, out.info = np.array([c_in, c_in]), U_in
    out.status, out.moved, out.grad = status, moved, np.array(grad)
    return out


def judge(R, t, status, l, r, sel, Kl, Kr, max_err2, cos2, tol):
    """Step 9 at (R, t): obs_res, obs_inlier, obs_front, F_out, the counts over the selected matches."""
    n = l.shape[1]
    good = not status & BAD_POSE
    with np.errstate(all="ignore"):
        finite = np.isfinite(l).all(axis=0) & np.isfinite(r).all(axis=0)
        res, inl, front = np.full(n, np.nan), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.uint8)
        Fn = np.zeros((3, 3))
        if good:
            F = model(R, t, Kl, Kr)[0]
            res = np.where(finite, residuals(F, np.zeros((5, 3, 3)), l, r)[0], np.nan)
            Fn, ok = canon9(F)
            if ok:
                rn = residuals(Fn, np.zeros((5, 3, 3)), l, r)[0]
                d2 = rn * rn
                inl = finite & np.isfinite(d2) & (d2 <= max_err2)
            a, b = tp.rays(Kl, l), tp.rays(Kr, r)
            rays_ok = np.isfinite(a).all(axis=0) & np.isfinite(b).all(axis=0)
            fr, par = tp.front_of(tp.front_terms(R, t, a, b), rays_ok, cos2, tol)
            front = fr.astype(np.uint8) + par.astype(np.uint8)
    return SimpleNamespace(res=res, inlier=inl.astype(np.uint8), front=front, F=Fn, n_inliers=int((inl & sel).sum()),
                           n_front=int(((front > 0) & sel).sum()), n_parallax=int(((front > 1) & sel).sum()))


def solve_set(l, r, mask, R_in, t_in, Kl=K_LEFT, Kr=K_RIGHT, lam=LAMBDA, iters=ITERS, max_err2=MAX_ERR2, cos2_min=COS2_MIN):
    """One set: l, r (2, n) pixel coordinates, mask (n,) bool.  Returns the outputs of the set, `settled` and `d_P`."""
    n = l.shape[1]
    R_in, t_in = np.asarray(R_in, dtype=np.float64).reshape(3, 3), np.asarray(t_in, dtype=np.float64).reshape(3)
    with np.errstate(all="ignore"):
        sel = np.asarray(mask, dtype=bool) & np.isfinite(l).all(axis=0) & np.isfinite(r).all(axis=0)
    routes = [iterate(route, l, r, sel, R_in, t_in, Kl, Kr, lam, iters) for route in (0, 1)]
    first = routes[0]
    settled = routes[1].status == first.status and routes[1].n_used == first.n_used and routes[1].moved == first.moved
    for q in routes:
        if q.ratio is not None:
            settled = settled and abs(q.ratio - GUARD) > GUARD_MARGIN
    with np.errstate(all="ignore"):
        d_P = max(float(np.abs(routes[1].R - first.R).max()), float(np.abs(routes[1].t - first.t).max())) if not first.status & BAD_POSE else 0.0
    base = judge(first.R, first.t, first.status, l, r, sel, Kl, Kr, max_err2, cos2_min, 0.0)
    for q in routes:
        for err2 in (max_err2, max_err2 * (1.0 - REL), max_err2 * (1.0 + REL)):
            for cos2 in (cos2_min, cos2_min * (1.0 - tp.REL), min(cos2_min * (1.0 + tp.REL), 1.0)):
                for tol in (0.0, -tp.TOL, tp.TOL):
                    if err2 != max_err2 and (cos2 != cos2_min or tol != 0.0):
                        continue
                    j = judge(q.R, q.t, q.status, l, r, sel, Kl, Kr, err2, cos2, tol)
                    settled = settled and (np.array_equal(j.inlier, base.inlier) and np.array_equal(j.front, base.front)
                                           and (j.n_inliers, j.n_front, j.n_parallax) == (base.n_inliers, base.n_front, base.n_parallax))
    X = np.full((3, n), np.nan)
    d_X = 0.0
    in_front = base.front > 0
    if in_front.any():
        a, b = tp.rays(Kl, l), tp.rays(Kr, r)
        X[:, in_front] = tp.midpoints(first.R, first.t, a, b)[:, in_front]
        other = tp.midpoints(routes[1].R, routes[1].t, a, b)[:, in_front]
        with np.errstate(all="ignore"):
            d_X = float((np.abs(other - X[:, in_front]).max(axis=0) / np.linalg.norm(X[:, in_front], axis=0)).max())
    with np.errstate(all="ignore"):
        d_cost = float(np.abs(routes[1].cost - first.cost).max() / max(float(np.abs(first.cost).max()), 1e-300))
    return SimpleNamespace(R=first.R, t=first.t, cost=first.cost, info=first.info, status=first.status, n_used=first.n_used, F=base.F,
                           res=base.res, inlier=base.inlier, front=base.front, X=X, n_inliers=base.n_inliers, n_front=base.n_front,
                           n_parallax=base.n_parallax, settled=bool(settled), d_P=d_P, d_X=d_X, d_cost=d_cost, grad=first.grad,
                           ratio=first.ratio, other=routes[1])


def reference(set_ptr, left, right, mask, R_in, t_in, Kl=K_LEFT, Kr=K_RIGHT, lam=LAMBDA, iters=ITERS, max_err2=MAX_ERR2, cos2_min=COS2_MIN):
    set_ptr = np.asarray(set_ptr)
    S, M = set_ptr.shape[0] - 1, left.shape[1]
    mask = np.ones(M, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    out = SimpleNamespace(R=np.zeros((S, 3, 3)), t=np.zeros((S, 3)), F=np.zeros((S, 3, 3)), cost=np.zeros((2, S)), info=np.zeros((S, 15)),
                          n_used=np.zeros(S, dtype=np.int32), status=np.zeros(S, dtype=np.int32), res=np.full(M, np.nan),
                          inlier=np.zeros(M, dtype=np.uint8), front=np.zeros(M, dtype=np.uint8), X=np.full((3, M), np.nan),
                          n_inliers=np.zeros(S, dtype=np.int32), n_front=np.zeros(S, dtype=np.int32), n_parallax=np.zeros(S, dtype=np.int32),
                          settled=np.zeros(S, dtype=bool), d_P=np.zeros(S), d_X=np.zeros(S), d_cost=np.zeros(S),
                          summary=np.zeros(6, dtype=np.int64), sets=[])
    for s in range(S):
        lo, hi = int(set_ptr[s]), int(set_ptr[s + 1])
        q = solve_set(left[:, lo:hi], right[:, lo:hi], mask[lo:hi], R_in[s], t_in[s], Kl, Kr, lam, iters, max_err2, cos2_min)
        out.R[s], out.t[s], out.F[s], out.cost[:, s], out.info[s] = q.R, q.t, q.F, q.cost, q.info[TRIU]
        out.n_used[s], out.status[s], out.n_inliers[s], out.n_front[s], out.n_parallax[s] = q.n_used, q.status, q.n_inliers, q.n_front, q.n_parallax
        out.res[lo:hi], out.inlier[lo:hi], out.front[lo:hi], out.X[:, lo:hi] = q.res, q.inlier, q.front, q.X
        out.settled[s], out.d_P[s], out.d_X[s], out.d_cost[s] = q.settled, q.d_P, q.d_X, q.d_cost
        out.sets.append(q)
        if q.status & BAD_POSE:
            out.summary[1] += 1
        elif q.status & (EMPTY | TOO_FEW):
            out.summary[2] += 1
        else:
            out.summary[0] += 1
            out.summary[3] += bool(q.status & KEPT_INPUT)
            out.summary[4] += q.n_inliers
            out.summary[5] += q.n_used - q.n_inliers
    return out


# ---- scenes --------------------------------------------------------------------------------------------------------------
TURN = tp.rodrigues((0.01, -0.02, 0.015))
ROTATION_T = tp._unit([1.0, 0.2, -0.1])     # a camera that only rotated has no baseline: the start takes this direction
SIZES = (0, 1, 4, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2049)
FAMILY_SEEDS = {name: (1, 2, 3) for name in tp.FAMILIES}
SIZES_SEED, MANY_SEED, SPECIAL_SEED = 4, 7, 6       # seeds at which every set is settled


def planted(name):
    R, t = tp.planted(name)
    return R, (ROTATION_T if name == "rotation" else t)


def start_pose(name):
    """The planted pose turned by TURN, the translation turned the other way."""
    R, t = planted(name)
    return TURN @ R, TURN.T @ t


def _assemble(parts):
    sc = tp._assemble(parts)
    poses = [start_pose(name) for name in sc.names]
    sc.R_in = np.stack([p[0] for p in poses]) if poses else np.zeros((0, 3, 3))
    sc.t_in = np.stack([p[1] for p in poses]) if poses else np.zeros((0, 3))
    return sc


@functools.lru_cache(maxsize=None)
def scene(name):
    """Scenes: "<family>" / "<family>_displaced" (three sets of 40, 130 and 300 matches), "sizes" (every set size, general and
    plane alternating), "many" (259 small sets of every family, clean and displaced), "special" (the degenerate inputs)."""
    if name.split("_")[0] in tp.FAMILIES:
        fam = name.split("_")[0]
        share = 0.1 if name.endswith("_displaced") else 0.0
        return _assemble([tp.family_part(fam, n, seed, share) + (fam,) for n, seed in zip(tp.FAMILY_COUNTS, FAMILY_SEEDS[fam])])
    if name == "sizes":
        return _assemble([tp.family_part(("general", "plane")[i % 2], n, SIZES_SEED + i, 0.1 if i % 3 == 0 else 0.0) + (("general", "plane")[i % 2],)
                          for i, n in enumerate(SIZES)])
    if name == "many":
        fams = sorted(tp.FAMILIES)
        sizes = list(tp.MANY_SIZES) * tp.MANY_CYCLES + [tp.MANY_SIZES[0]]
        return _assemble([tp.family_part(fams[i % 5], n, MANY_SEED + i, 0.1 if (i // 5) % 2 else 0.0) + (fams[i % 5],)
                          for i, n in enumerate(sizes)])
    if name == "special":
        g = tp.family_part("general", 70, SPECIAL_SEED)
        l, r = g[0].copy(), g[1].copy()
        r[1, 17] = np.nan
        l[0, 40] = np.nan
        sc = _assemble([g + ("general",), (l, r) + g[2:] + ("general",), g + ("general",), g + ("general",), g + ("general",),
                        g + ("general",)])
        sc.names = ["masked_out", "nan_coordinate", "clean_general", "zero_pose", "nan_pose", "no_winner"]
        sc.mask = sc.mask.copy()
        sc.mask[sc.set_ptr[0]:sc.set_ptr[1]] = False
        sc.t_in[3] = 0.0                                    # 3: a zero translation
        sc.R_in[4, 1, 1] = np.nan                           # 4: a NaN in the rotation
        sc.R_in[5], sc.t_in[5] = 0.0, 0.0                   # 5: what sfm_twoview_pose returns for a set without a winner
        return sc
    raise KeyError(name)


FAMILY_CASES = [f + suffix for f in tp.FAMILIES for suffix in ("", "_displaced")]
CASES = FAMILY_CASES + ["sizes", "many", "special"]
# (scene, iters, lambda): the options besides the defaults
OPTION_CASES = [("general_displaced", 0, 0.0), ("general_displaced", 1, 0.0), ("general_displaced", 2, 0.0), ("sizes", 2, 1e-3),
                ("general_displaced", 6, 1e-3), ("plane", 1, 1e-3), ("sizes", 0, 0.0)]
PARITY_CASES = [(name, ITERS, LAMBDA) for name in CASES] + OPTION_CASES


@functools.lru_cache(maxsize=None)
def scene_and_reference(name, iters=ITERS, lam=LAMBDA):
    sc = scene(name)
    return sc, reference(sc.set_ptr, sc.left, sc.right, sc.mask, sc.R_in, sc.t_in, lam=lam, iters=iters)


def subset(sc, sets):
    """The scene of the sets `sets` of sc alone."""
    sets = list(sets)
    sub = tp.subset(sc, sets)
    sub.R_in, sub.t_in = sc.R_in[sets], sc.t_in[sets]
    return sub


def baseline_angle_deg(t, t0):
    """The angle between the baseline directions t and t0 (a baseline has no sign here)."""
    c = abs(float(t @ t0)) / (np.linalg.norm(t) * np.linalg.norm(t0))
    return math.degrees(math.acos(min(c, 1.0)))
