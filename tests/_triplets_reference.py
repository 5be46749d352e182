"""The rule of the view-triplet filter (include/sfm_hip.h, block "view triplets") in NumPy float64, written from the text of
the rule, with a SETTLED flag per case, and the graphs the tests use.  Built like tests/_rotavg_reference.py, whose graph
builders it shares.

Every decision is also taken with the threshold ``fma(2, cos_loop, 1)`` moved by ``-+REL`` relative.  A case is SETTLED iff
every triplet's verdict and every edge's verdict are the same for both moved thresholds and the unmoved one.  The products
are plain NumPy products, not the fused chains of the header: a settled case has a margin of 1e-6 on every decision, nine
orders above the difference.  Everything else in the rule is integer arithmetic, so the GPU tests compare exactly."""
import functools
import itertools
import math
from types import SimpleNamespace

import numpy as np

import _rotavg_reference as rr

REL = rr.REL
SUMMARY = ("triplets", "triplets_consistent", "edges_tested", "edges_kept", "edges_dropped", "edges_untested", "edges_masked",
           "largest_n_tri")


# ---- steps 1 and 2 -------------------------------------------------------------------------------------------------------
def oriented(edges, rel):
    """``(lo, hi, M)``: the ends of every edge in ascending order and M_e, frame lo -> frame hi."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    rel = np.asarray(rel, dtype=np.float64).reshape(-1, 3, 3)
    turn = edges[:, 0] > edges[:, 1]
    M = np.where(turn[:, None, None], rel.transpose(0, 2, 1), rel)
    return edges.min(axis=1), edges.max(axis=1), M


def triplets(V, edges, mask=None):
    """Every triplet ``(e_ab, e_bc, e_ac)`` of the unmasked edges, (T, 3) int64, by the sorted higher neighbours of every view."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    up = [dict() for _ in range(V)]                           # up[a][b] = the edges between a and b, a < b
    for e, (i, j) in enumerate(edges):
        if mask is not None and not mask[e]:
            continue
        up[min(i, j)].setdefault(max(i, j), []).append(e)
    out = []
    for a in range(V):
        for b, e_ab in up[a].items():
            for c, e_bc in up[b].items():
                e_ac = up[a].get(c)
                if e_ac is not None:
                    out.extend(itertools.product(e_ab, e_bc, e_ac))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def triplets_brute(V, edges, mask=None):
    """The same set by brute force: every three views, every three edges."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    out = []
    for a, b, c in itertools.combinations(range(V), 3):
        def between(p, q):
            return [e for e, (i, j) in enumerate(edges) if {int(i), int(j)} == {p, q} and (mask is None or mask[e])]
        out.extend(itertools.product(between(a, b), between(b, c), between(a, c)))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


# ---- step 3 ----------------------------------------------------------------------------------------------------------------
def triplet_lhs(M, trip):
    with np.errstate(all="ignore"):
        P = M[trip[:, 1]] @ M[trip[:, 0]]
        return np.sum(P * M[trip[:, 2]], axis=(1, 2))


# ---- steps 4 to 6 ------------------------------------------------------------------------------------------------------------
def run(V, edges, rel, mask=None, cos_loop=1.0, min_ok=1, min_pct=0, keep_untested=0, thr_scale=1.0, trip=None):
    """The rule, one graph.  Returns the outputs of step 6 and ``trip`` / ``ok``: every triplet and its verdict."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    E = edges.shape[0]
    live = np.ones(E, dtype=bool) if mask is None else np.asarray(mask).reshape(E) != 0
    _, _, M = oriented(edges, rel)
    if trip is None:
        trip = triplets(V, edges, live)
    thr = (2.0 * cos_loop + 1.0) * thr_scale
    lhs = triplet_lhs(M, trip)
    with np.errstate(all="ignore"):
        ok = np.isfinite(lhs) & (lhs >= thr)
    n_tri = np.bincount(trip.reshape(-1), minlength=E).astype(np.int64)
    n_ok = np.bincount(trip[ok].reshape(-1), minlength=E).astype(np.int64)
    need = max(int(min_ok), 1)
    tested = live & (n_tri > 0)
    keep = np.where(tested, (n_ok >= need) & (100 * n_ok >= int(min_pct) * n_tri), live & bool(keep_untested))
    summary = np.array([trip.shape[0], int(ok.sum()), int(tested.sum()), int(keep.sum()), int((tested & ~keep).sum()),
                        int((live & (n_tri == 0)).sum()), int((~live).sum()), int(n_tri.max())], dtype=np.int64)
    return SimpleNamespace(edge_keep=keep.astype(np.uint8), n_tri=n_tri, n_ok=n_ok, kept_idx=np.nonzero(keep)[0].astype(np.int32),
                           summary=summary, trip=trip, ok=ok, lhs=lhs)


def solve(case, **over):
    """The reference of a case at the unmoved threshold, with ``settled`` from the two moved ones."""
    kw = dict(mask=case.mask, cos_loop=case.cos_loop, min_ok=case.min_ok, min_pct=case.min_pct, keep_untested=case.keep_untested)
    kw.update(over)
    live = None if kw["mask"] is None else np.asarray(kw["mask"]) != 0
    trip = triplets(case.V, case.edges, live)
    ref = run(case.V, case.edges, case.rel, trip=trip, **kw)
    moved = [run(case.V, case.edges, case.rel, trip=trip, thr_scale=s, **kw) for s in (1.0 - REL, 1.0 + REL)]
    ref.settled = all(np.array_equal(m.ok, ref.ok) and np.array_equal(m.edge_keep, ref.edge_keep) for m in moved)
    return ref


# ---- the graphs ----------------------------------------------------------------------------------------------------------------
def topo_band(V, k, rng, n_edges=None):
    """View a joined to a + 1 .. a + k, orientations mixed: what the view graph of a sequence looks like."""
    pairs = [(a, b) for a in range(V) for b in range(a + 1, min(a + k, V - 1) + 1)]
    if n_edges is not None:
        pairs = pairs[:n_edges]
    return [(a, b) if rng.random() < 0.5 else (b, a) for a, b in pairs]


def topo_two_hubs(length, rng):
    """Views 0 and 1 joined to each other and to every spoke 2 .. length: both adjacencies hold `length` entries, so the edge
    (0, 1) strides over an adjacency of that length and searches one of that length."""
    pairs = [(0, 1)] + [(h, v) for v in range(2, length + 1) for h in (0, 1)]
    return [(a, b) if rng.random() < 0.5 else (b, a) for a, b in pairs]


def make_case(name, V, pairs, seed, mask=None, max_loop_deg=5.0, min_ok=1, min_pct=0, keep_untested=0, **kw):
    c = rr.make_case(name, V, pairs, seed, **kw)
    c.mask = None if mask is None else np.asarray(mask, dtype=np.uint8)
    c.cos_loop = math.cos(math.radians(max_loop_deg))
    c.max_loop_deg, c.min_ok, c.min_pct, c.keep_untested = max_loop_deg, min_ok, min_pct, keep_untested
    return c


def _triangle(signs, wrong):
    pairs = [(0, 1), (1, 2), (0, 2)]
    pairs = [(b, a) if signs >> k & 1 else (a, b) for k, (a, b) in enumerate(pairs)]
    return make_case("triangle_%d_%s" % (signs, wrong), 3, pairs, 30 + signs, wrong=wrong)


def _parallel():
    """Two parallel edges on each side of one triangle, about ONE world axis (the loop angles add: ab + bc - ac): the first
    edge of every side is off by 2 degrees in the direction that adds, so exactly the combination of the three first edges
    has a loop of 6 degrees and the seven others stay at 2 degrees or below 5."""
    rng = np.random.default_rng(41)
    truth = np.array([rr.random_rotation(rng) for _ in range(3)])
    x = np.array([1.0, 0.0, 0.0])
    spec = [(0, 1, 2.0, 0), (1, 2, 2.0, 1), (0, 2, -2.0, 0), (0, 1, 0.0, 1), (1, 2, 0.0, 0), (0, 2, 0.0, 1)]
    edges, rel = [], []
    for lo, hi, angle, turned in spec:
        M = truth[hi] @ rr.so3_exp(math.radians(angle) * x) @ truth[lo].T
        edges.append((hi, lo) if turned else (lo, hi))
        rel.append(M.T if turned else M)
    return SimpleNamespace(name="parallel_222", V=3, edges=np.array(edges, dtype=np.int32), rel=np.array(rel).reshape(-1, 9), mask=None,
                           cos_loop=math.cos(math.radians(5.0)), max_loop_deg=5.0, min_ok=1, min_pct=0, keep_untested=0, truth=truth,
                           replaced=np.zeros(6, dtype=bool), noise_deg=0.0, seed=41, root=0)


def _complete(V, seed, wrong, **kw):
    pairs = rr.topo_complete(V, None)
    index = {frozenset(p): e for e, p in enumerate(pairs)}
    return make_case("complete_%d" % V, V, pairs, seed, wrong=[index[frozenset(w)] for w in wrong], **kw)


def _two_components(seed):
    rng = np.random.default_rng(seed)
    a = topo_band(9, 3, rng)
    b = [(9 + i, 9 + j) for i, j in topo_band(6, 2, rng)]
    return make_case("two_components", 15, a + b, seed, wrong_share=0.15, extra_views=2)


def _band(V, k, seed, n_edges=None, share=0.1, **kw):
    return make_case("band_%d_%d" % (V, k), V, topo_band(V, k, np.random.default_rng(seed), n_edges), seed, wrong_share=share, **kw)


def _masked(seed):
    c = _complete(5, seed, [])
    c.mask = np.ones(c.edges.shape[0], dtype=np.uint8)
    c.mask[0] = 0
    return c


CASES = {
    "parallel_222": _parallel,
    "chain_10": lambda: make_case("chain_10", 10, rr.topo_chain(10, None), 3),
    "chain_10_keep": lambda: make_case("chain_10_keep", 10, rr.topo_chain(10, None), 3, keep_untested=1),
    "complete_12": lambda: _complete(12, 5, [(0, 1), (0, 2), (5, 6)]),
    "two_components": lambda: _two_components(6),
    # adjacency lengths around one group's stride, a hub beyond it and one beyond a workgroup's
    "hubs_63": lambda: make_case("hubs_63", 64, topo_two_hubs(63, np.random.default_rng(63)), 63, wrong_share=0.1),
    "hubs_64": lambda: make_case("hubs_64", 65, topo_two_hubs(64, np.random.default_rng(64)), 64, wrong_share=0.1),
    "hubs_65": lambda: make_case("hubs_65", 66, topo_two_hubs(65, np.random.default_rng(65)), 65, wrong_share=0.1),
    "hubs_200": lambda: make_case("hubs_200", 201, topo_two_hubs(200, np.random.default_rng(200)), 200, wrong_share=0.1),
    "hubs_1030": lambda: make_case("hubs_1030", 1031, topo_two_hubs(1030, np.random.default_rng(1030)), 1030, wrong_share=0.1),
    # E around the tile of the prefix sum, and past the threshold of the device-wide one (2^14)
    "band_E3": lambda: _band(3, 2, 71, share=0.0),
    "band_E1023": lambda: _band(180, 6, 72, 1023),
    "band_E1025": lambda: _band(180, 6, 73, 1025),
    "band_E2049": lambda: _band(350, 6, 74, 2049),
    "band_E16389": lambda: _band(2800, 6, 75, 16389),
    "masked_5": lambda: _masked(8),
    # K5 with (0, 1) and (0, 2) wrong: (0, 3) and (0, 4) have 1 of 3, (1, 2), (1, 3), (1, 4), (2, 3), (2, 4) 2 of 3, (3, 4) 3 of 3
    "k5_two_wrong": lambda: _complete(5, 9, [(0, 1), (0, 2)]),
    # the flagship setting of the tolerance record: 60 views on a band of k = 6, 30 % of the edges random
    "band_60_30": lambda: _band(60, 6, 11, share=0.3),
}
for _signs in range(8):
    for _wrong in (None, (1,)):
        CASES["triangle_%d_%s" % (_signs, "ok" if _wrong is None else "wrong")] = functools.partial(_triangle, _signs, _wrong)

VARIANTS = {"k5_two_wrong": [dict(min_ok=o, min_pct=p) for o in (1, 2) for p in (0, 50, 100)]}


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c.ref = solve(c)
    return c


@functools.lru_cache(maxsize=None)
def band_chain():
    """The chain ``average_rotations(triplets=...)`` runs, on the 30 % band: the filter, then the rotation averaging (128
    trees, 2 rounds of 2 steps) over the kept edges.  ``(case, rotation reference over the kept edges)``."""
    c = case("band_60_30")
    kept = c.ref.kept_idx
    sub = SimpleNamespace(V=c.V, edges=c.edges[kept], rel=c.rel[kept], root=0, cos_max=c.cos_max, max_hyp=128, iters=2, steps=2)
    return c, rr.solve(sub)


# ---- the tolerance record ----------------------------------------------------------------------------------------------------
def rotation_bound_deg(c, edges, inlier):
    """The bound of tests/test_rotavg_host.py on a view's error from the noise alone, over the edges given: to first order the
    refit returns w = L^-1 B^T n, so |w_v| <= noise sqrt(E_in (L^-1)_vv); ten per cent are added for the second order.  Views
    that the inlier edges do not join to the root get no bound (inf)."""
    V = c.V
    conn = rr.connected(V, np.asarray(edges, dtype=np.int64), inlier, c.root)
    L = np.zeros((V, V))
    for i, j in np.asarray(edges)[inlier]:
        L[i, i] += 1; L[j, j] += 1; L[i, j] -= 1; L[j, i] -= 1
    free = conn & (np.arange(V) != c.root)
    Linv = np.linalg.inv(L[np.ix_(free, free)])
    bound = np.full(V, np.inf)
    bound[c.root] = 0.0
    bound[free] = 1.1 * c.noise_deg * np.sqrt(int(inlier.sum()) * np.diag(Linv))
    return bound


def angle_deg(A, B):
    return math.degrees(math.acos(min(1.0, max(-1.0, 0.5 * (np.trace(A.T @ B) - 1.0)))))
