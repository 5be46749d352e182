"""The rule of the translation averaging (include/sfm_hip.h, block "translation averaging") in NumPy float64, written from
the text of the rule, with a SETTLED flag per case, and the graphs the tests use.  Built like tests/_rotavg_reference.py.

A solve of step 3 goes by two routes: dense ``numpy.linalg.solve`` on the free unknowns, and block-Jacobi preconditioned
conjugate gradients (started at the standing positions, stopped at ``|r|^2 <= cg_tol^2 |b|^2`` or after ``cg_max``
iterations).  ``d_C`` is the largest disagreement of the two routes in any position, relative to the largest ``|c_v|``.
Every decision of steps 2 and 5 is also taken with ``cos_max`` moved by ``-+REL``.  A case is SETTLED iff every edge verdict
(after the rounds, of the polish, and the final one), every connectivity set and the stand decision are the same for both
routes and both moved thresholds (and the unmoved one).  The products are plain NumPy products, not the fused chains of the
header: a settled case has a margin of 1e-6 in ``cos_max`` on every decision, nine orders above the difference."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import _rotavg_reference as rr

NO_MODEL, KEPT_ROUNDS, CG_LIMIT = 1, 2, 4
NO_ROTATION, UNREACHED, HELD = 1, 2, 4
REL = 1e-6
CG_TOL = 1e-13
CG_MAX = 500
CHAIN_CG_MAX = 6000        # a chain of 300 at mu = 0.01 is the worst conditioned graph here: its CG needs thousands of iterations


# ---- step 1 --------------------------------------------------------------------------------------------------------------
def directions(R, edges, t, mask):
    """``(d (E, 3), used (E,))``: d = -R_j^T t normalised (zeros where the edge is not used)."""
    R = R.reshape(-1, 3, 3)
    i, j = edges[:, 0], edges[:, 1]
    has = np.any(R.reshape(-1, 9) != 0.0, axis=1)
    with np.errstate(all="ignore"):
        tt = np.sum(t * t, axis=1)
        used = has[i] & has[j] & np.isfinite(tt) & (tt > 0.0)
        if mask is not None:
            used &= np.asarray(mask).reshape(-1) != 0
        u = -np.einsum("eba,eb->ea", R[j], t)
        d = u / np.sqrt(np.sum(u * u, axis=1))[:, None]
    d[~used] = 0.0
    return d, used


# ---- step 2 --------------------------------------------------------------------------------------------------------------
def edge_terms(C, edges, d):
    with np.errstate(all="ignore"):
        v = C[edges[:, 1]] - C[edges[:, 0]]
        return np.sum(d * v, axis=1), np.sum(v * v, axis=1)


def inliers(dv, n2, cos_max):
    with np.errstate(all="ignore"):
        return np.isfinite(dv) & np.isfinite(n2) & (dv > 0.0) & (dv * dv >= (cos_max * cos_max) * n2)


def edge_cos(dv, n2, used):
    with np.errstate(all="ignore"):
        ok = used & np.isfinite(n2) & (n2 > 0.0)
        return np.where(ok, dv / np.sqrt(np.where(ok, n2, 1.0)), np.nan)


# ---- step 3 --------------------------------------------------------------------------------------------------------------
def connected(V, edges, live, root):
    """Depth from ``root`` over the edges named by ``live`` (-1: not joined)."""
    depth = np.full(V, -1, dtype=np.int64)
    depth[root] = 0
    i, j = edges[live, 0], edges[live, 1]
    for lev in range(1, V):
        new = np.concatenate([j[(depth[i] == lev - 1) & (depth[j] == -1)], i[(depth[j] == lev - 1) & (depth[i] == -1)]])
        if new.size == 0:
            break
        depth[new] = lev
    return depth


def apply_A(V, es, d, w, om, x):
    """A x over the edges ``es`` (those that take part): sum over the edges of a view of B_e (x_v - x_o)."""
    y = x[es[:, 1]] - x[es[:, 0]]
    z = w[:, None] * (y - om * d * np.sum(d * y, axis=1)[:, None])
    out = np.zeros((V, 3))
    np.add.at(out, es[:, 1], z)
    np.subtract.at(out, es[:, 0], z)
    return out


def rhs_and_blocks(V, es, d, w, l, mu):
    om = 1.0 - mu
    B = w[:, None, None] * (np.identity(3)[None] - om * d[:, :, None] * d[:, None, :])
    D = np.zeros((V, 3, 3))
    np.add.at(D, es[:, 0], B)
    np.add.at(D, es[:, 1], B)
    h = ((w * mu) * l)[:, None] * d
    b = np.zeros((V, 3))
    np.add.at(b, es[:, 1], h)
    np.subtract.at(b, es[:, 0], h)
    return b, D, B


def solve_dense(V, es, d, w, l, mu, free, C):
    b, D, B = rhs_and_blocks(V, es, d, w, l, mu)
    idx = np.nonzero(free)[0]
    pos = np.full(V, -1, dtype=np.int64)
    pos[idx] = np.arange(idx.size)
    n = idx.size
    A = np.zeros((n, 3, n, 3))
    A[np.arange(n), :, np.arange(n), :] = D[idx]
    rhs = b[idx].copy()
    for (i, j), Be in zip(es, B):
        pi, pj = pos[i], pos[j]
        if pi >= 0 and pj >= 0:
            A[pi, :, pj, :] -= Be
            A[pj, :, pi, :] -= Be
        elif pi >= 0:
            rhs[pi] += Be @ C[j]
        elif pj >= 0:
            rhs[pj] += Be @ C[i]
    x = np.linalg.solve(A.reshape(3 * n, 3 * n), rhs.reshape(3 * n)).reshape(n, 3)
    out = C.copy()
    out[idx] = x
    return out, 0, False


def solve_cg(V, es, d, w, l, mu, free, C, cg_tol, cg_max):
    om = 1.0 - mu
    b, D, _ = rhs_and_blocks(V, es, d, w, l, mu)
    b[~free] = 0.0
    Dinv = np.zeros((V, 3, 3))
    Dinv[free] = np.linalg.inv(D[free])
    x = C.copy()
    r = b - apply_A(V, es, d, w, om, x)
    r[~free] = 0.0
    z = np.einsum("vab,vb->va", Dinv, r)
    p = z.copy()
    bb, rz = float(np.sum(b * b)), float(np.sum(r * z))
    done = float(np.sum(r * r)) <= cg_tol * cg_tol * bb
    iters = 0
    while iters < cg_max and not done:
        q = apply_A(V, es, d, w, om, p)
        q[~free] = 0.0
        alpha = rz / float(np.sum(p * q))
        x = x + alpha * p
        r = r - alpha * q
        iters += 1
        if float(np.sum(r * r)) <= cg_tol * cg_tol * bb:
            done = True
            break
        z = np.einsum("vab,vb->va", Dinv, r)
        rz_new = float(np.sum(r * z))
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, iters, not done


def one_solve(V, edges, d, w, l, mu, root, C, route, cg_tol, cg_max):
    """``(positions, free, CG iterations, limit)`` of one solve from the standing positions C."""
    with np.errstate(all="ignore"):
        part = w > 0.0
    free = connected(V, edges, part, root) > 0
    es = edges[part]
    if route == "dense":
        x, iters, limit = solve_dense(V, es, d[part], w[part], l[part], mu, free, C)
    else:
        x, iters, limit = solve_cg(V, es, d[part], w[part], l[part], mu, free, C, cg_tol, cg_max)
    return x, free, iters, limit


def cost_of(dv, n2, w, l, mu):
    with np.errstate(all="ignore"):
        part = w > 0.0
        return float(np.sum(np.where(part, w * ((n2 - dv * dv) + mu * (dv - l) ** 2), 0.0)))


# ---- the rule ------------------------------------------------------------------------------------------------------------
def run(V, edges, R, t, mask=None, root=0, cos_max=1.0, mu=0.01, rounds=8, polish=1, route="dense", cos_shift=0.0, cg_tol=CG_TOL,
        cg_max=CG_MAX):
    """The rule, one graph.  Returns the outputs of step 6 and ``trace``: everything that was decided on the way.  The
    decisions are taken at ``cos_max + cos_shift``; the weights of step 4 at ``cos_max``."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    E = edges.shape[0]
    R = np.asarray(R, dtype=np.float64).reshape(V, 9)
    t = np.asarray(t, dtype=np.float64).reshape(E, 3)
    mu = 0.01 if mu == 0.0 else mu
    cm = min(1.0, cos_max + cos_shift)
    sigma2 = 2.0 - 2.0 * cos_max
    d, used = directions(R, edges, t, mask)
    norot = ~np.any(R != 0.0, axis=1)
    reach = connected(V, edges, used, root)
    log = np.zeros((rounds + 2, 4))
    trace = []
    status = 0
    C = np.zeros((V, 3))
    w, l = used.astype(np.float64), np.ones(E)
    model = bool(np.any(reach > 0))
    trace.append(("reach", tuple(reach >= 0)))
    verdict = np.zeros(E, dtype=bool)
    count = 0
    if model:
        for r in range(rounds + 1):
            C, free, iters, limit = one_solve(V, edges, d, w, l, mu, root, C, route, cg_tol, cg_max)
            status |= CG_LIMIT if limit else 0
            trace.append(("free", r, tuple(free)))
            if r == 0 and not np.all(np.isfinite(C[free])):
                model = False
                break
            dv, n2 = edge_terms(C, edges, d)
            verdict = used & inliers(dv, n2, cm)
            count = int(verdict.sum())
            log[r] = (count, iters, 1.0, cost_of(dv, n2, w, l, mu))
            trace.append(("verdict", r, tuple(verdict)))
            with np.errstate(all="ignore"):
                if r == rounds:
                    w = verdict.astype(np.float64)
                else:
                    ok = np.isfinite(n2) & (n2 > 0.0)
                    s2 = np.where(ok, 2.0 - 2.0 * (dv / np.sqrt(np.where(ok, n2, 1.0))), 2.0)
                    w = np.where(used, 1.0 / (1.0 + s2 / sigma2), 0.0)
                l = np.where(dv > 0.0, dv, 1.0)
    if model and polish:
        Cp, free, iters, limit = one_solve(V, edges, d, w, l, mu, root, C, route, cg_tol, cg_max)
        status |= CG_LIMIT if limit else 0
        dv, n2 = edge_terms(Cp, edges, d)
        vp = used & inliers(dv, n2, cm)
        stands = bool(np.all(np.isfinite(Cp[free]))) and int(vp.sum()) >= count
        log[rounds + 1] = (int(vp.sum()), iters, 1.0 if stands else 0.0, cost_of(dv, n2, w, l, mu))
        trace.append(("polish", tuple(free), tuple(vp), stands))
        if stands:
            C, verdict, count = Cp, vp, int(vp.sum())
        else:
            status |= KEPT_ROUNDS
    if not model:
        status, C, verdict, count = NO_MODEL, np.zeros((V, 3)), np.zeros(E, dtype=bool), 0
        log = np.zeros((rounds + 2, 4))
    conn = connected(V, edges, verdict, root)
    held = ~(model & (conn >= 0))
    has = model & (reach >= 0)
    C_out = np.where(has[:, None], C, 0.0)
    dv, n2 = edge_terms(C_out, edges, d)
    final = used & inliers(dv, n2, cm) & model
    trace.append(("final", model, tuple(final), tuple(held)))
    view_status = (norot * NO_ROTATION + (reach < 0) * UNREACHED + held * HELD).astype(np.int32)
    summary = np.array([has.sum(), norot.sum(), (reach < 0).sum(), held.sum(), final.sum(), (used & ~final).sum()], dtype=np.int64)
    return SimpleNamespace(C=C_out, edge_inlier=final.astype(np.uint8), edge_cos=edge_cos(dv, n2, used), edge_len=np.where(used, dv, np.nan),
                           view_status=view_status, n_inliers=int(final.sum()), status=status, summary=summary, log=log, trace=trace,
                           d=d, used=used)


def solve(case, **over):
    """The reference of a case: the dense route at the unmoved ``cos_max``, with ``settled``, ``d_C`` and ``bound``."""
    kw = dict(mask=case.mask, root=case.root, cos_max=case.cos_max, mu=case.mu, rounds=case.rounds, polish=case.polish,
              cg_tol=case.cg_tol, cg_max=case.cg_max)
    kw.update(over)
    ref = run(case.V, case.edges, case.R, case.t, **kw)
    other = run(case.V, case.edges, case.R, case.t, route="cg", **kw)
    moved = [run(case.V, case.edges, case.R, case.t, cos_shift=s, **kw) for s in (-REL, REL)]
    ref.settled = all(m.trace == ref.trace for m in [other] + moved) and other.status == ref.status
    ref.scale = float(np.max(np.sqrt(np.sum(ref.C * ref.C, axis=1))))
    ref.d_C = float(np.max(np.abs(other.C - ref.C))) / ref.scale if ref.scale > 0 else 0.0
    ref.bound = max(1e-9, 100.0 * ref.d_C)
    ref.cg_iters = other.log[:, 1].copy()
    return ref


# ---- the graphs ------------------------------------------------------------------------------------------------------------
def random_direction(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def turned(rng, d, lo_deg, hi_deg):
    """A unit vector at an angle in [lo_deg, hi_deg] from d, about a random axis."""
    a = math.radians(rng.uniform(lo_deg, hi_deg))
    n = np.cross(d, rng.standard_normal(3))
    n /= np.linalg.norm(n)
    return math.cos(a) * d + math.sin(a) * n


def make_case(name, V, pairs, seed, noise_deg=0.5, wrong_share=0.0, max_angle_deg=5.0, mu=0.01, rounds=8, polish=1, root=0,
              wrong=None, flipped=(), extra_views=0, centres=None, no_rotation=(), mask_off=(), spread=4.0, cg_max=CG_MAX):
    """Random rotations and centres per view; ``t_e = -R_j d`` with d the true direction from c_i to c_j turned by an angle
    of up to ``noise_deg`` and ``t_e`` scaled by a random length (the rule does not use it).  The edges named by ``wrong`` (or a
    share ``wrong_share`` of them, drawn) take a direction 30 .. 150 degrees from the true one; those in ``flipped`` have ``t``
    negated.  ``extra_views`` views carry no edge; ``no_rotation`` views have R = 0; ``mask_off`` edges are masked out."""
    rng = np.random.default_rng(seed)
    n = V + extra_views
    R = np.array([rr.random_rotation(rng) for _ in range(n)])
    c = rng.uniform(-spread, spread, (n, 3)) if centres is None else np.asarray(centres, dtype=np.float64)
    edges = np.array(pairs, dtype=np.int32).reshape(-1, 2)
    E = edges.shape[0]
    replaced = np.zeros(E, dtype=bool)
    if wrong is not None:
        replaced[list(wrong)] = True
    elif wrong_share > 0.0:
        replaced[rng.permutation(E)[:int(round(wrong_share * E))]] = True
    t = np.zeros((E, 3))
    for e, (i, j) in enumerate(edges):
        d = (c[j] - c[i]) / np.linalg.norm(c[j] - c[i])
        d = turned(rng, d, 30.0, 150.0) if replaced[e] else turned(rng, d, 0.0, noise_deg)
        t[e] = -(R[j] @ d) * rng.uniform(0.5, 2.0)
    for e in flipped:
        t[e] = -t[e]
    R = R.reshape(n, 9).copy()
    R[list(no_rotation)] = 0.0
    mask = None
    if len(mask_off):
        mask = np.ones(E, dtype=np.uint8)
        mask[list(mask_off)] = 0
    return SimpleNamespace(name=name, V=n, edges=edges, R=R, t=t, mask=mask, root=root, cos_max=math.cos(math.radians(max_angle_deg)),
                           max_angle_deg=max_angle_deg, mu=mu, rounds=rounds, polish=polish, centres=c, replaced=replaced,
                           flipped=tuple(flipped), seed=seed, cg_tol=CG_TOL, cg_max=cg_max)


def _size_case(V, E, seed, rounds=3):
    rng = np.random.default_rng(2000 + seed)
    if E < V - 1:                                  # fewer edges than a spanning tree: a random forest around the root
        pairs = rr.topo_random(V, rng, V - 1)[:E]
        if not any(0 in p for p in pairs):
            pairs[0] = (0, pairs[0][1] if pairs[0][1] != 0 else pairs[0][0])
    else:
        pairs = rr.topo_random(V, rng, E)
    return make_case("size_%d_%d" % (V, E), V, pairs, seed, wrong_share=0.1 if E >= 4 * V else 0.0, rounds=rounds)


def _chain(seed):
    """300 cameras one unit apart along a gently bending path: every baseline must come out at 1."""
    rng = np.random.default_rng(seed)
    steps = np.array([turned(rng, np.array([1.0, 0.0, 0.0]), 0.0, 20.0) for _ in range(299)])
    c = np.concatenate([np.zeros((1, 3)), np.cumsum(steps, axis=0)])
    return make_case("chain_300", 300, rr.topo_chain(300, None), seed, noise_deg=0.0, centres=c, rounds=2, cg_max=CHAIN_CG_MAX)


def _line(seed):
    """Nine cameras on one line, every pair joined: the directions fix no length, the mu term does."""
    c = np.outer(np.arange(9.0) * 0.7, np.array([0.6, 0.0, 0.8]))
    pairs = [(a, b) if (a + b) % 2 else (b, a) for a in range(9) for b in range(a + 1, 9)]
    return make_case("line_9", 9, pairs, seed, noise_deg=0.0, centres=c, rounds=2)


def _two_components(seed):
    rng = np.random.default_rng(seed)
    pairs = rr.topo_random(10, rng, 30) + [(a + 10, b + 10) for a, b in rr.topo_random(6, rng, 12)]
    return make_case("two_components", 16, pairs, seed, extra_views=1)


def _parallel(seed):
    """Six views; between 0 and 1 five parallel edges of which two disagree, between 2 and 3 two of which one is wrong."""
    pairs = [(0, 1)] * 5 + [(1, 2), (2, 3), (3, 2), (3, 4), (4, 5), (5, 0), (0, 2), (1, 3), (2, 4), (3, 5), (4, 0), (5, 1)]
    return make_case("parallel_edges", 6, pairs, seed, wrong=(1, 3, 7))


def _flipped(seed):
    rng = np.random.default_rng(seed)
    return make_case("flipped", 10, rr.topo_random(10, rng, 36), seed, flipped=(5,))


def _zero_R(seed):
    rng = np.random.default_rng(seed)
    return make_case("zero_R", 14, rr.topo_random(14, rng, 50), seed, no_rotation=(3, 9))


def _mask_cut(seed):
    """View 7's three edges are all masked out: it is unreached though the graph joins it."""
    rng = np.random.default_rng(seed)
    pairs = [p for p in rr.topo_random(12, rng, 40) if 7 not in p] + [(7, 1), (2, 7), (7, 5)]
    E = len(pairs)
    return make_case("mask_cut", 12, pairs, seed, mask_off=(E - 3, E - 2, E - 1))


def _root_masked(seed):
    rng = np.random.default_rng(seed)
    pairs = rr.topo_random(8, rng, 20)
    return make_case("root_masked", 8, pairs, seed, mask_off=[e for e, p in enumerate(pairs) if 0 in p])


def _held(seed):
    """View 9 hangs on the graph by two edges, both with t negated: their LINES still meet at its true position, where both
    point the wrong way.  Reached over used edges, cut off by the final verdicts."""
    rng = np.random.default_rng(seed)
    pairs = [p for p in rr.topo_random(9, rng, 30)] + [(9, 2), (4, 9)]
    return make_case("held", 10, pairs, seed, flipped=(30, 31))


def fan_case(name, angles_deg, seed=0, max_angle_deg=5.0, rounds=8, mu=0.01):
    """Two views and one parallel edge per entry of ``angles_deg``: the direction of edge k is the x axis turned by that angle
    in the x-y plane (R = I on both views)."""
    a = np.radians(np.asarray(angles_deg, dtype=np.float64))
    t = -np.stack([np.cos(a), np.sin(a), np.zeros_like(a)], axis=1)
    E = a.size
    return SimpleNamespace(name=name, V=2, edges=np.array([(0, 1)] * E, dtype=np.int32), R=np.tile(np.identity(3).reshape(9), (2, 1)), t=t,
                           mask=None, root=0, cos_max=math.cos(math.radians(max_angle_deg)), max_angle_deg=max_angle_deg, mu=mu,
                           rounds=rounds, polish=1, centres=None, replaced=np.zeros(E, dtype=bool), flipped=(), seed=seed, cg_tol=CG_TOL, cg_max=CG_MAX)


# Two views joined by nine parallel edges in one plane, five rounds.  The Cauchy rounds settle between the cluster around 0
# degrees and the one around +8, where six edges are admitted; the polish weighs those six alike, moves, and admits five.
# Found by scanning 3 000 random fans (4 .. 13 edges at -9 .. +9 degrees in steps of 0.1, 0 .. 8 rounds) with this file on the
# CPU for a polish that does not stand in a settled case; this was the second hit.
KEPT_FAN = (7.7, -1.1, 8.2, 0.0, -1.3, 2.2, 8.9, 8.1, -0.7)


def _kept(seed):
    """A polish that does not stand, see ``KEPT_FAN``."""
    return fan_case("kept", KEPT_FAN, rounds=5)


def tolerance_case(seed, share, V=40, E=200):
    """The graph of the tolerance record: every view of degree >= 4 (a leaf's single edge cannot be judged by anyone), 0.5
    degrees of noise, a share of the directions replaced by one 30 .. 150 degrees away."""
    rng = np.random.default_rng(seed)
    while True:
        pairs = rr.topo_random(V, rng, E)
        deg = np.bincount(np.array(pairs).reshape(-1), minlength=V)
        if deg.min() >= 4:
            break
    return make_case("tolerance_%d_%g" % (seed, share), V, pairs, seed, wrong_share=share, rounds=8, polish=1)


def aligned_error(C, truth):
    """The largest distance after the least-squares scale and shift of C onto truth, relative to the mean distance of truth
    from its centroid."""
    a, b = C - C.mean(axis=0), truth - truth.mean(axis=0)
    s = float(np.sum(a * b) / np.sum(a * a))
    return float(np.max(np.linalg.norm(s * a - b, axis=1)) / np.mean(np.linalg.norm(b, axis=1)))


CASES = {
    # V in {2, 3, 5, 64, 65, 257, 1 100} (the slices of a dot product: 64; the workgroup: 1 024) x E in {1, 3, 1 023, 1 025, 2 049}
    "size_2_1": lambda: _size_case(2, 1, 1),
    "size_3_3": lambda: _size_case(3, 3, 1),
    "size_5_3": lambda: _size_case(5, 3, 1),
    "size_64_1023": lambda: _size_case(64, 1023, 1),
    "size_65_1025": lambda: _size_case(65, 1025, 1),
    "size_257_2049": lambda: _size_case(257, 2049, 1),
    "size_1100_2049": lambda: _size_case(1100, 2049, 1, rounds=1),
    "chain_300": lambda: _chain(3),
    "star_201": lambda: make_case("star_201", 201, rr.topo_star(201, None), 4, wrong=(28, 29, 30, 31, 32), rounds=3),
    "complete_12": lambda: make_case("complete_12", 12, rr.topo_complete(12, None), 5, wrong_share=0.2),
    "line_9": lambda: _line(6),
    "two_components": lambda: _two_components(7),
    "zero_R": lambda: _zero_R(8),
    "mask_cut": lambda: _mask_cut(9),
    "parallel_edges": lambda: _parallel(10),
    "flipped": lambda: _flipped(11),
    "root_masked": lambda: _root_masked(12),
    "held": lambda: _held(13),
    "kept": lambda: _kept(0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c.ref = solve(c)
    return c


def end_to_end_case(seed=31, V=8, noise_deg=0.5, corrupted=(4, 17)):
    """Eight views, every pair posed: ``Rel_e = N R_j R_i^T`` with N a rotation by ``noise_deg``, ``t_e`` the unit translation of
    that pose with its direction turned by up to ``noise_deg``; the pairs named by ``corrupted`` carry a random rotation and a
    random direction.  Returns the graph with the true rotations and centres."""
    rng = np.random.default_rng(seed)
    R = np.array([rr.random_rotation(rng) for _ in range(V)])
    c = rng.uniform(-4.0, 4.0, (V, 3))
    edges = np.array(rr.topo_complete(V, None), dtype=np.int32)
    E = edges.shape[0]
    rel, t = np.zeros((E, 3, 3)), np.zeros((E, 3))
    for e, (i, j) in enumerate(edges):
        if e in corrupted:
            rel[e], t[e] = rr.random_rotation(rng), random_direction(rng)
            continue
        rel[e] = rr.noise_rotation(rng, noise_deg) @ R[j] @ R[i].T
        d = (c[j] - c[i]) / np.linalg.norm(c[j] - c[i])
        t[e] = -(R[j] @ turned(rng, d, 0.0, noise_deg))
    return SimpleNamespace(V=V, edges=edges, rel=rel.reshape(E, 9), t=t, R_true=R, centres=c, corrupted=tuple(corrupted))
