"""Host-side checks of the rotation averaging (no GPU): the spanning trees of sfm_rotation_tree against their defining
properties and the NumPy trees, every argument the library and ``check_rotation_graph`` refuse (before a device is looked
for, outputs untouched), sfm_rotation_edge_test against the reference, the so(3) helpers, the NumPy reference of
tests/_rotavg_reference.py on the graphs the GPU tests use -- EVERY case of tests/test_gpu_rotavg.py is settled, so the GPU
tests compare decisions exactly and leave nothing out -- and the reference's tolerance of wrong edges, recorded."""
import ctypes
import math

import numpy as np
import pytest

import _rotavg_reference as rr


# ---- the trees -----------------------------------------------------------------------------------------------------------
def _graphs():
    rng = np.random.default_rng(3)
    yield 2, np.array([[0, 1]]), 0
    yield 3, np.array([[0, 1], [1, 2], [0, 2]]), 0
    yield 12, np.array(rr.topo_complete(12, None)), 5
    yield 40, np.array(rr.topo_random(40, rng, 90)), 7
    two = rr.case("two_components")
    yield two.V, two.edges, 0
    par = rr.case("parallel_edges")
    yield par.V, par.edges, 3


@pytest.mark.parametrize("V,edges,root", list(_graphs()))
def test_the_tree_of_every_hypothesis(sfm, V, edges, root):
    native = sfm.native
    E = edges.shape[0]
    reach = rr.tree(V, edges, 0, root)[3] >= 0
    for h in (0, 1, 2, 17, 127, 4095, 65535):
        H, parent, depth = native.rotation_tree(V, edges, root, 65536, h)
        assert H == 65536
        want = rr.tree(V, edges, h, root)
        assert np.array_equal(parent, want[0]) and np.array_equal(depth, want[3]), h
        r0 = rr.tree_root(h, V, root)
        assert depth[r0] == 0 and parent[r0] == -1 and (h != 0 or r0 == root)
        for v in range(V):
            if depth[v] > 0:                                 # the parent edge joins v to a view one level up
                i, j = edges[parent[v]]
                other = j if i == v else i
                assert v in (i, j) and depth[other] == depth[v] - 1
                # ... and no edge reaches further up: breadth first
                for a, b in edges[(edges[:, 0] == v) | (edges[:, 1] == v)]:
                    assert depth[b if a == v else a] >= depth[v] - 1
        # it spans the component of its own root; that is the root's component iff it reaches `root`
        if depth[root] >= 0:
            assert np.array_equal(depth >= 0, reach)
        else:
            assert not np.any((depth >= 0) & reach)
    # h = 0: the lowest-numbered edge to the previous level
    H, parent, depth = native.rotation_tree(V, edges, root, 0, 0)
    assert H == 128
    for v in range(V):
        if depth[v] > 0:
            up = [e for e in range(E) if v in edges[e] and depth[edges[e][0] + edges[e][1] - v] == depth[v] - 1]
            assert parent[v] == min(up)
    assert native.rotation_tree(V, edges, root, 16, 16)[1].tolist() == [-1] * V         # h out of range: nothing is written
    for bad in ((1, edges, 0, 16), (V, edges, V, 16), (V, edges, -1, 16), (V, edges, root, -1), (V, edges, root, 65537),
                (V, np.array([[0, 0]]), 0, 16), (V, np.array([[0, V]]), 0, 16)):
        assert native.rotation_tree(bad[0], bad[1], bad[2], bad[3], 0)[0] == 0


def test_the_mixer_is_splitmix64():
    assert rr.mix(0) == 0xE220A8397B1DCDAF                    # splitmix64's first output from state 0
    z = np.array([0, 1, (5 << 32) | 7, (1 << 64) - 1], dtype=np.uint64)
    assert rr.mix_array(z).tolist() == [rr.mix(int(v)) for v in z]


# ---- the arguments -------------------------------------------------------------------------------------------------------
def _library_call(native, V, E, edges, rel, root, cos_max, max_hyp, iters, steps, cg_tol, cg_max, with_R=True):
    """sfm_rotation_average with every output present and filled with a mark: (status, the outputs)."""
    outs = dict(R=np.full((max(V, 1), 9), 7.0), edge_inlier=np.full(max(E, 1), 7, dtype=np.uint8), edge_cos=np.full(max(E, 1), 7.0),
                view_status=np.full(max(V, 1), -7, dtype=np.int32), small=np.full(3, -7, dtype=np.int32), summary=np.full(6, -7, dtype=np.int64))
    small = outs["small"].ctypes.data
    ip = ctypes.POINTER(ctypes.c_int)
    st = native.load().sfm_rotation_average(
        V, E, None if edges is None else native.iptr(edges), None if rel is None else native.dptr(rel), root, cos_max, max_hyp, iters,
        steps, cg_tol, cg_max, native.dptr(outs["R"]) if with_R else None, outs["edge_inlier"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        native.dptr(outs["edge_cos"]), native.iptr(outs["view_status"]), ctypes.cast(small, ip), ctypes.cast(small + 4, ip),
        ctypes.cast(small + 8, ip), outs["summary"].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return st, outs


def _untouched(outs):
    return (np.all(outs["R"] == 7.0) and np.all(outs["edge_inlier"] == 7) and np.all(outs["edge_cos"] == 7.0)
            and np.all(outs["view_status"] == -7) and np.all(outs["small"] == -7) and np.all(outs["summary"] == -7))


def test_every_bad_argument_is_refused_before_a_device_is_looked_for(sfm):
    native = sfm.native
    c = rr.case("complete_12")
    good = dict(V=c.V, E=c.edges.shape[0], edges=c.edges, rel=c.rel, root=0, cos_max=c.cos_max, max_hyp=16, iters=2, steps=2, cg_tol=1e-12,
                cg_max=100)
    nan = float("nan")
    loop, far, neg = c.edges.copy(), c.edges.copy(), c.edges.copy()
    loop[5] = (3, 3); far[7] = (0, c.V); neg[0] = (-1, 2)
    bad = [("V", 1, "sizes"), ("E", 0, "sizes"), ("root", -1, "root"), ("root", c.V, "root"), ("cos_max", nan, "cos_max"),
           ("cos_max", 0.0, "cos_max"), ("cos_max", 1.0000001, "cos_max"), ("cos_max", -0.5, "cos_max"), ("max_hyp", -1, "max_hyp"),
           ("max_hyp", 65537, "max_hyp"), ("iters", -1, "iters"), ("steps", 0, "steps"), ("cg_tol", 0.0, "cg_tol"), ("cg_tol", 1.0, "cg_tol"),
           ("cg_tol", nan, "cg_tol"), ("cg_max", 0, "cg_max"), ("edges", loop, "edge 5"), ("edges", far, "edge 7"), ("edges", neg, "edge 0"),
           ("edges", None, "null"), ("rel", None, "null")]
    for name, value, word in bad:
        kw = dict(good)
        kw[name] = value
        st, outs = _library_call(native, **kw)
        assert st == native.E_SHAPE and word in native.last_error() and _untouched(outs), (name, value, native.last_error())
        if name in ("V", "E") or value is None:
            continue
        py = {k: v for k, v in kw.items() if k not in ("V", "E")}
        with pytest.raises(ValueError, match=word):
            native.check_rotation_graph(kw["V"], **py)
    for V, edges in ((1, c.edges), (c.V, np.zeros((0, 2), dtype=np.int32))):
        with pytest.raises(ValueError, match="sizes"):
            native.check_rotation_graph(V, edges, c.rel[:edges.shape[0]])
    st, outs = _library_call(native, with_R=False, **good)
    assert st == native.E_SHAPE and "null" in native.last_error()                       # R_out is not optional
    # a Rel that is no rotation: the lowest such edge is named
    rel = c.rel.copy()
    rel[9] *= 1.01
    rel[4, 0] += 0.1
    kw = dict(good, rel=rel)
    st, outs = _library_call(native, **kw)
    assert st == native.E_BAD_ROTATION and "edge 4 " in native.last_error() and _untouched(outs)
    with pytest.raises(ValueError, match="edge 4 "):
        native.check_rotation_graph(c.V, c.edges, rel)
    # what passes the checks comes back converted
    V, edges, rel, root, cos_max, max_hyp, iters, steps, cg_tol, cg_max = native.check_rotation_graph(
        c.V, c.edges.tolist(), c.rel.reshape(-1, 3, 3), 3, 0.5, 0, 0, 1, 0.5, 1)
    assert edges.dtype == np.int32 and rel.shape == (c.edges.shape[0], 9) and (root, max_hyp, iters, steps, cg_max) == (3, 0, 0, 1, 1)
    assert native.rotation_plan(c.V, 0, 0) == (128, 1) and native.rotation_plan(1000, 65536, 0) == (3728, 18)
    assert native.rotation_plan(1000, 128, 1) == (1, 128)
    native.rotation_plan(c.V, 0, 0)
    for args in ((1, 16, 0), (12, -1, 0), (12, 65537, 0), (12, 16, -1)):
        with pytest.raises(ValueError):
            native.rotation_plan(*args)


def test_the_version(sfm):
    assert sfm.native.load().sfm_version() >= 107


# ---- the test of an edge -------------------------------------------------------------------------------------------------
def test_the_edge_test_against_the_reference(sfm):
    native = sfm.native
    rng = np.random.default_rng(2)
    for k in range(200):
        Ri, Rj = rr.random_rotation(rng), rr.random_rotation(rng)
        angle = (0.0, 1.0, 4.9, 5.1, 30.0, 179.0)[k % 6]
        rel = rr.noise_rotation(rng, angle) @ Rj @ Ri.T
        cos_max = math.cos(math.radians(5.0))
        inlier, lhs = native.rotation_edge_test(Ri, Rj, rel, cos_max)
        want = float(np.sum((rel @ Ri) * Rj))
        assert abs(lhs - want) <= 16 * np.finfo(float).eps * 3.0                        # nine products of entries below one
        assert abs(lhs - (1.0 + 2.0 * math.cos(math.radians(angle)))) < 1e-12
        assert inlier == (angle <= 5.0)
    eye = np.identity(3)
    assert native.rotation_edge_test(eye, eye, eye, 1.0) == (True, 3.0)
    bad = eye.copy(); bad[1, 1] = float("nan")
    assert native.rotation_edge_test(eye, bad, eye, 0.5)[0] is False and native.rotation_edge_test(bad, eye, eye, 0.5)[0] is False
    assert native.rotation_edge_test(eye, eye, np.full((3, 3), float("inf")), 0.5)[0] is False


def test_so3_log_and_exp(sfm):
    g = sfm.geometry
    rng = np.random.default_rng(4)
    for scale in (0.0, 1e-9, 1e-5, 0.9e-4, 1.1e-4, 1e-2, 1.0, 3.0):
        w = rng.standard_normal(3)
        w *= scale / np.linalg.norm(w)
        R = g.so3_exp(w)
        assert np.abs(R @ R.T - np.identity(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
        assert np.abs(R - rr.so3_exp(w)).max() < 1e-15
        if scale < math.pi / 2:                              # the log takes angles below a quarter turn exactly ...
            assert np.abs(g.so3_log(R) - w).max() <= 1e-14 * max(1.0, scale)
        assert np.abs(g.so3_exp(g.so3_log(R)) - R).max() < 1e-14                        # ... and below a half turn it still inverts
    Ri, rel = rr.random_rotation(rng), rr.random_rotation(rng)
    assert np.array_equal(g.compose_relative(Ri, rel.reshape(9)), rel @ Ri)


# ---- the reference on the cases of the GPU tests ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_every_case_is_settled(name):
    c = rr.case(name)
    assert c.ref.settled, name
    assert c.ref.d_R <= 1e-11, (name, c.ref.d_R)              # CG_TOL keeps the CG route this close to the dense one
    assert c.ref.cg_status == c.ref.status                   # ... and CG_MAX is never reached


def test_the_variants_of_the_gpu_tests_are_settled():
    c = rr.case("complete_12")
    for max_hyp in (1, 64, 65, 256):
        assert rr.solve(c, max_hyp=max_hyp).settled
    for iters, steps in ((0, 1), (3, 1), (3, 3), (1, 3)):
        for name in ("complete_12", "parallel_edges", "two_components"):
            ref = rr.solve(rr.case(name), iters=iters, steps=steps)
            assert ref.settled and ref.d_R <= 1e-11, (name, iters, steps)
    two = rr.case("two_components")
    none = rr.solve(two, root=two.V - 1)
    assert none.settled and none.status == rr.NO_MODEL and not none.R.any() and none.summary.tolist() == [0, two.V - 1, two.V, 0, 0, 0]


def test_the_cases_reach_what_they_are_there_for():
    assert rr.case("kept").ref.status == rr.KEPT_HYPOTHESIS and rr.case("kept").ref.summary[5] == 0
    held = rr.case("held").ref
    assert held.view_status.tolist() == [0, 0, rr.HELD] and held.summary[5] == 3 and held.status == 0
    two = rr.case("two_components").ref
    assert two.summary[1] == 8 and not two.R[two.view_status & rr.UNREACHED != 0].any() and np.isnan(two.edge_cos).sum() == 9
    tri = rr.case("triangle").ref
    assert tri.best_hyp == 0 and set(k for k in tri.counts if k >= 0) == {2}
    par = rr.case("parallel_edges")
    assert par.ref.edge_inlier[[18, 19]].tolist() == [0, 0] and par.ref.edge_inlier[20] == 1
    wrong = rr.case("root_wrong")
    # every tree joins the root to the rest along ONE of its wrong edges, an inlier by construction; the other two disagree with it
    assert wrong.ref.edge_inlier[[24, 25, 26]].sum() == 1 and wrong.ref.edge_inlier[:24].sum() >= 22
    assert rr.tree(300, rr.case("chain_300").edges, 0, 0)[3].max() == 299
    star = rr.case("star_201")
    assert np.bincount(star.edges.ravel())[0] == 200


# ---- the tolerance of wrong edges ----------------------------------------------------------------------------------------
def _angle(A, B):
    return math.degrees(math.acos(min(1.0, max(-1.0, 0.5 * (np.trace(A.T @ B) - 1.0)))))


def _outlier_run(share, seed, max_hyp=128, iters=2):
    """60 views, 240 edges (mean degree 8), 0.5 degrees of noise, `share` of the edges random, 5 degrees admitted."""
    c = rr.make_case("tolerance", 60, rr.topo_random(60, np.random.default_rng(60), 240), seed, wrong_share=share, max_hyp=max_hyp,
                     iters=iters)
    r = rr.run(c.V, c.edges, c.rel, 0, c.cos_max, max_hyp, iters, 2)
    G = c.truth @ c.truth[0].T                                # the truth in the gauge of the root
    residual = np.array([_angle(G[j], c.rel[e].reshape(3, 3) @ G[i]) for e, (i, j) in enumerate(c.edges)])
    return c, r, G, residual


def _rotation_bound_deg(c, inlier):
    """The bound on a view's error that follows from the noise alone.  To first order the refit returns w = L^-1 B^T n: B the
    incidence matrix of the inlier edges, L = B^T B with the root grounded, n_e the noise of edge e with |n_e| = 0.5 degrees.
    Row v of L^-1 B^T has sum of squares (L^-1 B^T B L^-1)_vv = (L^-1)_vv, the effective resistance between root and v, so by
    Cauchy-Schwarz |w_v| <= 0.5 sqrt(E_in (L^-1)_vv) degrees; ten per cent are added for the second order."""
    V = c.V
    L = np.zeros((V, V))
    for i, j in c.edges[inlier]:
        L[i, i] += 1; L[j, j] += 1; L[i, j] -= 1; L[j, i] -= 1
    keep = np.arange(V) != c.root
    Linv = np.linalg.inv(L[np.ix_(keep, keep)])
    bound = np.zeros(V)
    bound[keep] = 1.1 * c.noise_deg * np.sqrt(int(inlier.sum()) * np.diag(Linv))
    return bound


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_the_reference_tolerates_one_edge_in_twenty_being_wrong(seed):
    """The share the rule reaches in the planned setting (60 views, mean degree 8, 0.5 degrees, 5 degrees admitted, 128
    hypotheses, 2 rounds): at 5 % of the edges replaced by random rotations it flags exactly the replaced edges whose residual
    against the truth exceeds the threshold, no clean edge, and every rotation is within the bound of _rotation_bound_deg.
    Recorded: largest errors 0.75, 0.84, 0.61 degrees (seeds 11, 12, 13; 0.73, 0.83, 0.59 at 2 %); the plain h = 0 tree alone
    ends 173, 141 and 174 degrees off with 204, 213 and 151 of the 228 inliers, since its 59 edges hold a wrong one."""
    c, r, G, residual = _outlier_run(0.05, seed)
    assert np.array_equal(r.edge_inlier.astype(bool), residual <= c.max_angle_deg)
    assert not np.any(~r.edge_inlier.astype(bool) & ~c.replaced) and r.status == 0
    assert np.all(np.abs(residual - c.max_angle_deg) > 0.05)                            # no verdict hangs on the noise
    err = np.array([_angle(r.R[v], G[v]) for v in range(c.V)])
    bound = _rotation_bound_deg(c, r.edge_inlier.astype(bool))
    print("seed %d: max error %.3f degrees, smallest bound %.2f, largest %.2f" % (seed, err.max(), bound[1:].min(), bound.max()))
    assert np.all(err[1:] <= bound[1:]) and np.array_equal(r.R[0], np.identity(3))           # the root is the gauge, exactly
    tree0 = rr.run(c.V, c.edges, c.rel, 0, c.cos_max, 1, 0, 2)
    err0 = max(_angle(tree0.R[v], G[v]) for v in range(c.V))
    print("seed %d: the h = 0 tree alone: %d inliers, %.1f degrees" % (seed, tree0.n_inliers, err0))
    assert tree0.n_inliers < r.n_inliers and err0 > 100.0


def test_at_thirty_per_cent_no_spanning_tree_is_clean():
    """The setting first planned for this record, 30 % of the edges random: the rule does NOT reach it, and cannot.  A hypothesis is a
    spanning tree of 59 edges, every one of them an inlier by construction; it is free of wrong edges with probability
    0.7^59 = 7e-10, so none of 128 (or 65 536) trees is, the winner carries a wrong edge in its tree and the refit, which
    trusts the winner's inliers, keeps it.  Recorded over seeds 11, 12, 13: 115, 126 and 141 inliers where 168 edges are
    clean, 71, 54 and 35 clean edges flagged, largest errors 176, 180 and 164 degrees; at 10 % 8, 6 and 7 clean edges are
    flagged, at 20 % 34, 30 and 16.  DESIGN.md section 36 says so; the share the rule reaches is asserted above."""
    assert 65536 * 0.7 ** 59 < 1e-4
    c, r, G, residual = _outlier_run(0.30, 11)
    parent = rr.tree(c.V, c.edges, r.best_hyp, 0)[0]
    assert c.replaced[parent[parent >= 0]].any()              # the winning tree itself holds a replaced edge ...
    assert r.edge_inlier[parent[parent >= 0]].all()           # ... which stays an inlier to the end
    assert int((~r.edge_inlier.astype(bool) & ~c.replaced).sum()) > 0
