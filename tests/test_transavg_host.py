"""Host-side checks of the translation averaging (no GPU): every argument the library and ``check_translation_graph`` refuse
(before a device is looked for, outputs untouched), sfm_translation_edge_test at its boundaries, ``world_directions``, the
NumPy reference of tests/_transavg_reference.py on the graphs the GPU tests use -- EVERY case of tests/test_gpu_transavg.py
is settled, so the GPU tests compare decisions exactly and leave nothing out -- and the reference's tolerance of wrong
edges, recorded."""
import ctypes
import math

import numpy as np
import pytest

import _rotavg_reference as rr
import _transavg_reference as tr


# ---- the arguments -------------------------------------------------------------------------------------------------------
def _library_call(native, V, E, edges, R, t, mask, root, cos_max, mu, rounds, polish, cg_tol, cg_max, with_C=True):
    """sfm_translation_average with every output present and filled with a mark: (status, the outputs)."""
    n_v, n_e = max(V, 1), min(max(E, 1), 4096)          # the refused sizes write nothing: no need to hold 2^30 entries
    outs = dict(C=np.full((n_v, 3), 7.0), edge_inlier=np.full(n_e, 7, dtype=np.uint8), edge_cos=np.full(n_e, 7.0), edge_len=np.full(n_e, 7.0),
                view_status=np.full(n_v, -7, dtype=np.int32), small=np.full(2, -7, dtype=np.int32), summary=np.full(6, -7, dtype=np.int64),
                log=np.full((max(rounds, 0) + 2, 4), 7.0))
    small = outs["small"].ctypes.data
    ip, u8 = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint8)
    st = native.load().sfm_translation_average(
        V, E, None if edges is None else native.iptr(edges), None if R is None else native.dptr(R), None if t is None else native.dptr(t),
        None if mask is None else mask.ctypes.data_as(u8), root, cos_max, mu, rounds, polish, cg_tol, cg_max,
        native.dptr(outs["C"]) if with_C else None, outs["edge_inlier"].ctypes.data_as(u8), native.dptr(outs["edge_cos"]),
        native.dptr(outs["edge_len"]), native.iptr(outs["view_status"]), ctypes.cast(small, ip), ctypes.cast(small + 4, ip),
        outs["summary"].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), native.dptr(outs["log"]))
    return st, outs


def _untouched(outs):
    return (np.all(outs["C"] == 7.0) and np.all(outs["edge_inlier"] == 7) and np.all(outs["edge_cos"] == 7.0) and np.all(outs["edge_len"] == 7.0)
            and np.all(outs["view_status"] == -7) and np.all(outs["small"] == -7) and np.all(outs["summary"] == -7) and np.all(outs["log"] == 7.0))


def test_every_bad_argument_is_refused_before_a_device_is_looked_for(sfm):
    native = sfm.native
    c = tr.case("complete_12")
    good = dict(V=c.V, E=c.edges.shape[0], edges=c.edges, R=c.R, t=c.t, mask=None, root=0, cos_max=c.cos_max, mu=0.01, rounds=2, polish=1,
                cg_tol=1e-12, cg_max=100)
    nan = float("nan")
    loop, far, neg = c.edges.copy(), c.edges.copy(), c.edges.copy()
    loop[5] = (3, 3); far[7] = (0, c.V); neg[0] = (-1, 2)
    bad = [("V", 1, "sizes"), ("E", 0, "sizes"), ("E", 2 ** 30, "sizes"), ("root", -1, "root"), ("root", c.V, "root"), ("cos_max", nan, "cos_max"),
           ("cos_max", 0.0, "cos_max"), ("cos_max", 1.0000001, "cos_max"), ("cos_max", -0.5, "cos_max"), ("mu", nan, "mu"), ("mu", -0.1, "mu"),
           ("mu", 1.5, "mu"), ("rounds", -1, "rounds"), ("polish", 2, "polish"), ("polish", -1, "polish"), ("cg_tol", 0.0, "cg_tol"),
           ("cg_tol", 1.0, "cg_tol"), ("cg_tol", nan, "cg_tol"), ("cg_max", 0, "cg_max"), ("edges", loop, "edge 5"), ("edges", far, "edge 7"),
           ("edges", neg, "edge 0"), ("edges", None, "null"), ("R", None, "null"), ("t", None, "null")]
    for name, value, word in bad:
        kw = dict(good)
        kw[name] = value
        st, outs = _library_call(native, **kw)
        assert st == native.E_SHAPE and word in native.last_error() and _untouched(outs), (name, value, native.last_error())
        if name in ("V", "E") or value is None:
            continue
        py = {("edge_mask" if k == "mask" else k): v for k, v in kw.items() if k not in ("V", "E")}
        with pytest.raises(ValueError, match=word):
            native.check_translation_graph(kw["V"], **py)
    with pytest.raises(ValueError, match="sizes"):
        native.check_translation_graph(1, np.zeros((1, 2), dtype=np.int32), np.zeros((1, 9)), np.zeros((1, 3)))
    with pytest.raises(ValueError, match="sizes"):
        native.check_translation_graph(c.V, np.zeros((0, 2), dtype=np.int32), c.R, np.zeros((0, 3)))
    for kw in (dict(R=c.R[:5]), dict(t=c.t[:5]), dict(edge_mask=np.ones(3))):
        args = dict(edges=c.edges, R=c.R, t=c.t)
        args.update(kw)
        with pytest.raises(ValueError, match="must"):
            native.check_translation_graph(c.V, **args)
    st, outs = _library_call(native, with_C=False, **good)
    assert st == native.E_SHAPE and "null" in native.last_error()                       # C_out is not optional
    # a non-zero R that is no rotation: the lowest such view is named; nine zeros are no error
    R = c.R.copy()
    R[9] *= 1.01
    R[4, 0] += 0.1
    R[2] = 0.0
    st, outs = _library_call(native, **dict(good, R=R))
    assert st == native.E_BAD_ROTATION and "view 4 " in native.last_error() and _untouched(outs)
    with pytest.raises(ValueError, match="view 4 "):
        native.check_translation_graph(c.V, c.edges, R, c.t)
    # what passes the checks comes back converted
    V, edges, R2, t2, mask, root, cos_max, mu, rounds, polish, cg_tol, cg_max = native.check_translation_graph(
        c.V, c.edges.tolist(), c.R.reshape(-1, 3, 3), c.t.reshape(-1, 3, 1), [1, 0] * 33, 3, 0.5, 0.0, 0, False, 0.5, 1)
    assert edges.dtype == np.int32 and R2.shape == (c.V, 9) and t2.shape == (c.edges.shape[0], 3) and mask.dtype == np.uint8
    assert (root, mu, rounds, polish, cg_max) == (3, 0.0, 0, 0, 1) and mask.sum() == 33


def test_the_version(sfm):
    assert sfm.native.load().sfm_version() >= 108


# ---- the test of an edge -------------------------------------------------------------------------------------------------
def test_the_edge_test_at_its_boundaries(sfm):
    native = sfm.native
    nan, inf = float("nan"), float("inf")
    x, o = [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    assert native.translation_edge_test(x, o, [5.0, 0.0, 0.0], 1.0) == (True, 5.0, 25.0)          # exactly at cos_max = 1
    assert native.translation_edge_test(x, o, [5.0, 1e-7, 0.0], 1.0)[0] is False
    assert native.translation_edge_test(x, o, [0.0, 2.0, 0.0], 0.5) == (False, 0.0, 4.0)          # dv = 0
    assert native.translation_edge_test(x, o, o, 0.5) == (False, 0.0, 0.0)                        # n2 = 0
    assert native.translation_edge_test(x, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0], 1e-9)[0] is False
    assert native.translation_edge_test(x, o, [-1.0, 0.0, 0.0], 0.5)[0] is False                  # the wrong way: dv < 0
    assert native.translation_edge_test(x, o, [nan, 0.0, 0.0], 0.5)[0] is False
    assert native.translation_edge_test(x, [0.0, nan, 0.0], [1.0, 0.0, 0.0], 0.5)[0] is False
    assert native.translation_edge_test([nan, 0.0, 0.0], o, [1.0, 0.0, 0.0], 0.5)[0] is False
    assert native.translation_edge_test(x, o, [inf, 0.0, 0.0], 0.5)[0] is False
    assert native.translation_edge_test(x, o, [1e200, 1e200, 0.0], 0.5)[0] is False               # n2 overflows: not finite
    # exactly at cos_max: the 3-4-5 triangle at cos_max = 0.8, 0.6, and one step of cos_max to either side
    for v, cm in (([4.0, 3.0, 0.0], 0.8), ([3.0, 4.0, 0.0], 0.6), ([4.0, 0.0, 3.0], 0.8)):
        for cos_max in (cm, np.nextafter(cm, 0.0), np.nextafter(cm, 1.0), cm - 1e-6, cm + 1e-6):
            inlier, dv, n2 = native.translation_edge_test(x, o, v, cos_max)
            assert (dv, n2) == (v[0], 25.0) and inlier == (dv * dv >= (cos_max * cos_max) * n2), (v, cos_max)
        assert native.translation_edge_test(x, o, v, cm - 1e-6)[0] is True and native.translation_edge_test(x, o, v, cm + 1e-6)[0] is False
    # against the reference on random edges
    rng = np.random.default_rng(2)
    cos_max = math.cos(math.radians(5.0))
    for k in range(200):
        d = tr.random_direction(rng)
        angle = (0.0, 1.0, 4.9, 5.1, 30.0, 95.0, 179.0)[k % 7]
        ci = rng.uniform(-3, 3, 3)
        cj = ci + rng.uniform(0.1, 5.0) * tr.turned(rng, d, angle, angle)
        inlier, dv, n2 = native.translation_edge_test(d, ci, cj, cos_max)
        want_dv, want_n2 = tr.edge_terms(np.array([ci, cj]), np.array([[0, 1]]), d[None])
        assert abs(dv - want_dv[0]) <= 8 * np.finfo(float).eps * 10.0 and abs(n2 - want_n2[0]) <= 8 * np.finfo(float).eps * 100.0
        assert inlier == (angle <= 5.0) and inlier == bool(tr.inliers(want_dv, want_n2, cos_max)[0])


def test_world_directions(sfm):
    g = sfm.geometry
    rng = np.random.default_rng(4)
    R = np.array([rr.random_rotation(rng) for _ in range(6)])
    edges = np.array([(0, 1), (2, 1), (5, 3), (4, 0)])
    t = rng.standard_normal((4, 3)) * 3.0
    d = g.world_directions(R, edges, t)
    for e, (i, j) in enumerate(edges):
        want = -R[j].T @ t[e]
        assert np.abs(d[e] - want / np.linalg.norm(want)).max() <= 4 * np.finfo(float).eps
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 4 * np.finfo(float).eps
    # with R_j = Rel R_i and X_j = Rel X_i + t the baseline c_j - c_i is -R_j^T t
    c = rng.uniform(-2, 2, (6, 3))
    for i, j in edges:
        Rel = R[j] @ R[i].T
        t_true = -R[j] @ c[j] + Rel @ R[i] @ c[i]                 # X_j = R_j (X - c_j), X_i = R_i (X - c_i)
        got = g.world_directions(R, [(i, j)], t_true[None])[0]
        assert np.abs(got - (c[j] - c[i]) / np.linalg.norm(c[j] - c[i])).max() <= 1e-14
    assert np.array_equal(tr.directions(R.reshape(-1, 9), edges, t, None)[0], d)
    assert np.isnan(g.world_directions(R, edges[:1], np.zeros((1, 3)))).all()


# ---- the reference on the cases of the GPU tests ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_every_case_is_settled(name):
    c = tr.case(name)
    assert c.ref.settled, name
    assert c.ref.d_C <= 1e-10, (name, c.ref.d_C)              # CG_TOL keeps the CG route this close to the dense one
    assert not c.ref.status & tr.CG_LIMIT


def test_the_variants_of_the_gpu_tests_are_settled():
    for rounds in (0, 1, 8):
        for polish in (0, 1):
            for name in ("complete_12", "parallel_edges", "two_components", "size_65_1025"):
                ref = tr.solve(tr.case(name), rounds=rounds, polish=polish)
                assert ref.settled and ref.d_C <= 1e-10, (name, rounds, polish)
    for mu in (1.0, 0.1, 0.01, 0.0):
        for name in ("complete_12", "line_9", "star_201"):
            ref = tr.solve(tr.case(name), mu=mu)
            assert ref.settled and ref.d_C <= 1e-10, (name, mu)
    c = tr.case("complete_12")
    kw = dict(mask=c.mask, root=c.root, cos_max=c.cos_max, mu=c.mu, rounds=c.rounds, polish=c.polish, route="cg", cg_max=1)
    ref = tr.run(c.V, c.edges, c.R, c.t, **kw)
    assert ref.status & tr.CG_LIMIT and all(tr.run(c.V, c.edges, c.R, c.t, cos_shift=s, **kw).trace == ref.trace for s in (-tr.REL, tr.REL))
    c = tr.case("size_65_1025")
    mask = np.ones(c.edges.shape[0], dtype=np.uint8)
    mask[::17] = 0
    assert tr.solve(c, mask=mask).settled


def test_the_end_to_end_graph_is_settled_given_the_true_rotations():
    g = tr.end_to_end_case()
    mask = np.ones(g.edges.shape[0], dtype=np.uint8)
    mask[list(g.corrupted)] = 0
    c = tr.SimpleNamespace(V=g.V, edges=g.edges, R=(g.R_true @ g.R_true[0].T).reshape(-1, 9), t=g.t, mask=mask, root=0,
                           cos_max=math.cos(math.radians(5.0)), mu=0.01, rounds=8, polish=1, cg_tol=tr.CG_TOL, cg_max=tr.CG_MAX)
    ref = tr.solve(c)
    assert ref.settled and ref.status == 0 and ref.n_inliers == 26


def test_the_cases_reach_what_they_are_there_for():
    kept = tr.case("kept").ref
    assert kept.status == tr.KEPT_ROUNDS and kept.log[-1, 2] == 0.0 and kept.log[-1, 0] < kept.log[-2, 0] == kept.n_inliers
    held = tr.case("held").ref
    assert held.view_status[9] == tr.HELD and held.summary[3] == 1 and held.status == 0 and held.C[9].any()
    two = tr.case("two_components").ref
    assert two.summary[2] == 7 and not two.C[two.view_status & tr.UNREACHED != 0].any()
    zero = tr.case("zero_R").ref
    assert zero.summary[1] == 2 and np.isnan(zero.edge_len).sum() == int((~zero.used).sum()) > 0
    cut = tr.case("mask_cut").ref
    assert cut.view_status[7] == (tr.UNREACHED | tr.HELD) and cut.status == 0
    none = tr.case("root_masked").ref
    assert none.status == tr.NO_MODEL and not none.C.any() and not none.edge_inlier.any() and not none.log.any() and none.summary[3] == 8
    par = tr.case("parallel_edges")
    assert np.array_equal(~par.ref.edge_inlier.astype(bool), par.replaced)
    flipped = tr.case("flipped")
    assert flipped.ref.edge_inlier[5] == 0 and flipped.ref.edge_cos[5] < -0.99 and flipped.ref.n_inliers == 35
    chain = tr.case("chain_300").ref
    assert tr.connected(300, tr.case("chain_300").edges, chain.used, 0).max() == 299
    assert np.max(np.abs(chain.edge_len - 1.0)) / chain.scale <= chain.bound                   # every baseline comes out at 1
    line = tr.case("line_9").ref
    axis = np.array([0.6, 0.0, 0.8])
    assert np.max(np.abs(line.C - np.outer(line.C @ axis, axis))) / line.scale <= line.bound
    star = tr.case("star_201")
    assert np.bincount(star.edges.ravel())[0] == 200
    big = tr.case("size_1100_2049")
    assert big.V > 1024 and big.edges.shape[0] > 2048


# ---- the tolerance of wrong edges ----------------------------------------------------------------------------------------
def _tolerance_run(seed, share):
    c = tr.tolerance_case(seed, share)
    r = tr.run(c.V, c.edges, c.R, c.t, root=0, cos_max=c.cos_max, mu=0.01, rounds=8, polish=1)
    flagged = ~r.edge_inlier.astype(bool)
    return c, r, flagged


# measured with this file (40 views, 200 edges, every degree >= 4, 0.5 degrees of noise, 5 degrees admitted, mu = 0.01, 8 rounds,
# polish; seeds 11, 12, 13): per share, per seed (exactly the replaced edges flagged, clean edges flagged, replaced edges
# missed, largest position error in per cent of the mean distance from the centroid)
TOLERANCE_RECORD = {
    0.00: (("Y", 0, 0, 1.32), ("Y", 0, 0, 0.89), ("Y", 0, 0, 0.97)),
    0.05: (("Y", 0, 0, 1.43), ("Y", 0, 0, 0.97), ("Y", 0, 0, 0.81)),
    0.10: (("Y", 0, 0, 1.49), ("Y", 0, 0, 0.88), ("Y", 0, 0, 0.84)),
    0.20: (("n", 3, 0, 143.05), ("n", 3, 0, 154.92), ("Y", 0, 0, 1.55)),
    0.30: (("n", 3, 1, 154.58), ("n", 10, 4, 156.70), ("n", 4, 0, 149.60)),
}
TOLERATED_SHARE = 0.10


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_the_reference_tolerates_one_edge_in_ten_being_wrong(seed):
    """The largest share at which the reference flags exactly the replaced edges on all three seeds: 10 %.  (A throw-away
    generator had suggested 20 %; with the committed one two of the three seeds lose a view there, see TOLERANCE_RECORD and
    DESIGN.md section 37.)  The positions are then within 2 % of the scene's size of the truth; the bound is what the noise
    allows: a direction 0.5 degrees off moves the far end of a baseline by sin(0.5 degrees) = 0.9 % of its length, the longest
    baseline is below four times the mean distance from the centroid, and the estimator averages over at least four edges per
    view, which is not counted on."""
    c, r, flagged = _tolerance_run(seed, TOLERATED_SHARE)
    assert np.array_equal(flagged, c.replaced) and r.status == 0 and not r.view_status.any()
    err = tr.aligned_error(r.C, c.centres)
    span = np.mean(np.linalg.norm(c.centres - c.centres.mean(axis=0), axis=1))
    longest = max(np.linalg.norm(c.centres[j] - c.centres[i]) for i, j in c.edges) / span
    print("seed %d: largest position error %.2f %% (longest baseline %.2f spans)" % (seed, 100 * err, longest))
    assert longest < 4.0 and err <= 4.0 * math.sin(math.radians(0.5))


def test_the_tolerance_record():
    """The whole table, re-measured: the flags exactly, the errors to the digits recorded."""
    for share, rows in TOLERANCE_RECORD.items():
        for seed, (exact, clean, missed, err_pct) in zip((11, 12, 13), rows):
            c, r, flagged = _tolerance_run(seed, share)
            got = ("Y" if np.array_equal(flagged, c.replaced) else "n", int((flagged & ~c.replaced).sum()), int((~flagged & c.replaced).sum()))
            assert got == (exact, clean, missed), (share, seed, got)
            assert abs(100 * tr.aligned_error(r.C, c.centres) - err_pct) <= 0.05 * max(1.0, err_pct), (share, seed)
    first_loss = min(s for s, rows in TOLERANCE_RECORD.items() if any(row[0] != "Y" for row in rows))
    assert TOLERATED_SHARE == max(s for s in TOLERANCE_RECORD if s < first_loss)
