"""Matrix-free bundle adjustment of the resident scene (sfm_ba_iterate_pcg, ``BaProblem.iterate_pcg``,
``HipBaMixin.ba_solver = "pcg"``) against the NumPy reference of tests/_pcg_reference.py.

Norm: ``pr.rel``, the largest absolute difference over the largest absolute entry of the reference, cameras and points
separately.  Bound: 1e-9 against ``step_direct``, the project's parity bound; tests/test_pcg_host.py measures that the
reference's own PCG ends within 2e-13 of ``step_direct`` on every setting used here.  At low damping the bound is
``pr.tolerance`` of the disagreement of the two NumPy routes, measured here again."""
import numpy as np
import pytest

import _pcg_reference as pr

pytestmark = pytest.mark.gpu

TIGHT = 1e-13
GROUPS = (1, 4, 8, 16, 32, 64, 0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _problem(hip, c, loss="none"):
    prob = hip.BaProblem(c.n_cams, c.pt_ptr, c.cam_idx, c.uv)
    if loss != "none":
        prob.set_loss(loss, c.delta)
    return prob


def _check_step(hip, prob, c, lam, quirks, loss, which, where, group=0):
    mask = pr.free_mask(c.n_cams, which)
    b = pr.both_routes(c, lam, quirks, loss, which)
    prob.set_state(c.cams, c.pts)
    out = prob.iterate_pcg(lam, 1, quirks, mask, TIGHT, 0, group)
    cams, pts = prob.get_state()
    e_c, e_p = pr.rel(cams, b["direct"][0]), pr.rel(pts, b["direct"][1])
    e_cost = abs(out.cost[0] - b["cost"]) / b["cost"]
    print(where, "cameras %.2e points %.2e cost %.1e  cg %d (reference %d) rel %.1e" % (e_c, e_p, e_cost, out.cg_iters[0], b["count"],
                                                                                  out.cg_rel[0]))
    assert out.iters_done == 1 and out.cg_status[0] == hip.PCG_CONVERGED, where
    assert e_c <= 1e-9 and e_p <= 1e-9, where
    assert e_cost < 1e-11, where                           # a sum of M terms in another order
    assert out.cg_iters[0] <= b["count"] + 2 and out.cg_rel[0] <= TIGHT, where
    if mask is not None:
        held = np.flatnonzero(mask == 0)
        assert same_bits(cams[held], c.cams[held]), where
    return cams, pts


# ---- 1: one outer iteration against step_direct ---------------------------------------------------------------------
@pytest.mark.parametrize("loss", pr.LOSSES)
@pytest.mark.parametrize("name", pr.SCENES)
def test_step_parity(hip, sfm, oracle, name, loss):
    c = pr.case(sfm, name)
    with _problem(hip, c, loss) as prob:
        for lam in pr.LAMBDAS:
            for quirks in (oracle.QUIRKS_REFERENCE, 0):
                for which in pr.MASKS:
                    _check_step(hip, prob, c, lam, quirks, loss, which, (name, loss, lam, quirks, which))


# ---- 2: three outer iterations against the oracle and against the dense solver -----------------------------------------
@pytest.mark.parametrize("name", pr.SCENES)
def test_three_iterations(hip, sfm, oracle, name):
    c = pr.case(sfm, name)
    want_c, want_p = oracle.ba_sparse(c.cams, c.pts, c.cam_idx, c.pt_idx, c.uv, 5.0, 3)
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        out = prob.iterate_pcg(5.0, 3, tol=TIGHT)
        cams, pts = prob.get_state()
        prob.set_state(c.cams, c.pts)
        prob.iterate(5.0, 3)
        dense_c, dense_p = prob.get_state()
        dense_cost = prob.get_stats()
    print(name, "oracle %.2e %.2e  dense %.2e %.2e  cg" % (pr.rel(cams, want_c), pr.rel(pts, want_p), pr.rel(cams, dense_c),
                                                          pr.rel(pts, dense_p)), out.cg_iters)
    assert out.iters_done == 3 and not out.cg_status.any()
    assert pr.rel(cams, want_c) <= 1e-9 and pr.rel(pts, want_p) <= 1e-9
    assert pr.rel(cams, dense_c) <= 1e-9 and pr.rel(pts, dense_p) <= 1e-9
    assert pr.rel(out.cost, dense_cost) <= 1e-9


# ---- 3: low damping with the gauge held ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("6x300", "12x200_tracks"))
def test_low_damping_with_the_gauge_held(hip, sfm, oracle, name):
    c = pr.case(sfm, name)
    mask = pr.free_mask(c.n_cams, "held01")
    with _problem(hip, c) as prob:
        for lam in (1e-6, 0.0):
            q = oracle.QUIRKS_REFERENCE
            dc, dpts, _cost = pr.step_direct(c, c.cams, c.pts, lam, q, "none", mask, key="start")
            pc, ppts, _c, count, _status, _h = pr.step_pcg(c, c.cams, c.pts, lam, q, "none", mask, TIGHT, 500, key="start")
            bound = pr.tolerance(max(pr.rel(pc, dc), pr.rel(ppts, dpts)))
            prob.set_state(c.cams, c.pts)
            out = prob.iterate_pcg(lam, 1, q, mask, TIGHT, 500)
            cams, pts = prob.get_state()
            print(name, lam, "cameras %.2e points %.2e bound %.2e  cg %d (reference %d)" % (pr.rel(cams, dc), pr.rel(pts, dpts), bound,
                                                                                        out.cg_iters[0], count))
            assert out.cg_status[0] == hip.PCG_CONVERGED and out.cg_iters[0] <= count + 2
            assert pr.rel(cams, dc) <= bound and pr.rel(pts, dpts) <= bound
            assert same_bits(cams[:2], c.cams[:2]) and prob.info(hip.INFO_PCG_HELD_POINTS) == 0


# ---- 4: truncation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("12x200_tracks", "260"))
def test_truncation(hip, sfm, oracle, name):
    c = pr.case(sfm, name)
    want_c, want_p, _cost, count, status, _h = pr.step_pcg(c, c.cams, c.pts, 5.0, oracle.QUIRKS_REFERENCE, "none", None, TIGHT, 2,
                                                          key="start")
    full = pr.both_routes(c, 5.0, oracle.QUIRKS_REFERENCE, "none", "none")["direct"]
    assert count == 2 and status == pr.PCG_MAX_ITERS and pr.rel(want_c, full[0]) > 1e-8      # another step than the full one, by ten parity bounds at least
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        out = prob.iterate_pcg(5.0, 1, tol=TIGHT, max_cg=2)
        cams, pts = prob.get_state()
    assert out.iters_done == 1 and out.cg_status[0] == hip.PCG_MAX_ITERS and out.cg_iters[0] == 2 and 0 < out.cg_rel[0] < 1
    assert pr.rel(cams, want_c) <= 1e-9 and pr.rel(pts, want_p) <= 1e-9


# ---- 5: every group width -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name", ("hub70", "260"))
def test_group_widths(hip, sfm, oracle, name, group):
    c = pr.case(sfm, name)
    with _problem(hip, c) as prob:
        assert prob.info(hip.INFO_MAX_TRACK) >= 70
        for which in ("none", "held01"):
            _check_step(hip, prob, c, 5.0, oracle.QUIRKS_REFERENCE, "none", which, (name, group, which), group)
        with pytest.raises(ValueError):
            prob.iterate_pcg(5.0, 1, group=2)


# ---- 6: a block that does not factor ------------------------------------------------------------------------------
def test_singular_block(hip, sfm, oracle):
    """lambda = 0, no mask, on the scene with an empty camera: SFM_E_SINGULAR, the state untouched, the handle usable.
    Which camera is named: the lowest whose diagonal block does not factor.  NumPy (``pr.diagonal_block_pivots``) finds two
    such blocks on this scene: the empty camera's, which is zero, and camera 0's -- in a track-structured scene every
    point camera 0 sees is seen by camera 1 as well, and with the other cameras held camera 0 can still slide along the
    baseline and rescale its points, so its Schur complement has a null direction (smallest eigenvalue -7e-17 of 3e-3).
    So the unmasked call names camera 0, and the call with camera 0 held names the empty camera."""
    c = pr.case(sfm, "empty")
    assert np.bincount(c.cam_idx, minlength=c.n_cams)[pr.EMPTY_CAMERA] == 0
    pivots = pr.diagonal_block_pivots(c, 0.0, oracle.QUIRKS_REFERENCE)
    print("relative pivots of the diagonal blocks at lambda = 0:", pivots)
    assert np.flatnonzero(pivots <= 1e-9).tolist() == [0, pr.EMPTY_CAMERA] and np.all(np.delete(pivots, [0, pr.EMPTY_CAMERA]) > 1e-6)
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        for mask, want in ((None, 0), (np.arange(c.n_cams) != 0, pr.EMPTY_CAMERA)):
            with pytest.raises(hip.SfmSingularError) as err:
                prob.iterate_pcg(0.0, 2, mask=mask)
            assert err.value.camera == want and isinstance(err.value, hip.SfmHipError)
            cams, pts = prob.get_state()
            assert same_bits(cams, c.cams) and same_bits(pts, c.pts)
        # the same handle then runs a valid call
        b = pr.both_routes(c, 5.0, oracle.QUIRKS_REFERENCE, "none", "none")
        out = prob.iterate_pcg(5.0, 1, tol=TIGHT)
        cams, pts = prob.get_state()
        assert out.cg_status[0] == hip.PCG_CONVERGED
        assert pr.rel(cams, b["direct"][0]) <= 1e-9 and pr.rel(pts, b["direct"][1]) <= 1e-9
        assert np.array_equal(cams[pr.EMPTY_CAMERA, 0:3], c.cams[pr.EMPTY_CAMERA, 0:3])      # rhs = 0: only q is normalised


def test_argument_errors_and_noop(hip, sfm):
    c = pr.case(sfm, "6x300")
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        lib, h = prob._lib, prob._h
        for lam, iters, tol, max_cg, group in ((-1.0, 1, 1e-10, 0, 0), (float("nan"), 1, 1e-10, 0, 0), (float("inf"), 1, 1e-10, 0, 0),
                                               (5.0, -1, 1e-10, 0, 0), (5.0, 1, 0.0, 0, 0), (5.0, 1, 1.0, 0, 0), (5.0, 1, 1e-10, -1, 0),
                                               (5.0, 1, 1e-10, 0, 3)):
            assert lib.sfm_ba_iterate_pcg(h, lam, iters, 3, None, tol, max_cg, group, None, None, None, None, None, None) == hip.E_SHAPE
        out = prob.iterate_pcg(5.0, 0)
        assert out.iters_done == 0 and out.cost.shape == (0,)
        cams, pts = prob.get_state()
        assert same_bits(cams, c.cams) and same_bits(pts, c.pts)
        up = prob.upload_bytes
        prob.iterate_pcg(5.0, 1, mask=np.ones(c.n_cams))
        assert prob.upload_bytes == up + c.n_cams
        assert prob.pcg_times().shape == (5,) and prob.pcg_times()[4] > 0


# ---- 7: repeatability ---------------------------------------------------------------------------------------------
def _run(prob, c, cams, pts, mask=None, group=8):
    prob.set_state(cams, pts)
    out = prob.iterate_pcg(0.5, 2, mask=mask, tol=1e-10, group=group)
    return prob.get_state() + (out.cost, out.cg_iters, out.cg_rel)


def test_two_handles_two_streams_same_bits(hip, sfm):
    import torch
    c = pr.case(sfm, "tracks40")
    mask = pr.free_mask(c.n_cams, "held01")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with _problem(hip, c) as a, _problem(hip, c) as b:
        a.set_stream(s1.cuda_stream)
        b.set_stream(s2.cuda_stream)
        ra, rb = _run(a, c, c.cams, c.pts, mask), _run(b, c, c.cams, c.pts, mask)
        again = _run(a, c, c.cams, c.pts, mask)
        a.set_stream(None)
        b.set_stream(None)
    assert all(same_bits(x, y) for x, y in zip(ra, rb)) and all(same_bits(x, y) for x, y in zip(ra, again))


def test_a_grown_scene_gives_the_bits_of_the_whole_scene(hip, sfm):
    c = pr.case(sfm, "12x200_tracks")
    old = c.cam_idx < c.n_cams - 2
    ptr_old = np.zeros(c.n_pts + 1, dtype=np.int32)
    np.cumsum(np.bincount(c.pt_idx[old], minlength=c.n_pts), out=ptr_old[1:])
    with _problem(hip, c) as whole:
        want = _run(whole, c, c.cams, c.pts)
    with hip.BaProblem(c.n_cams - 2, ptr_old, c.cam_idx[old], np.ascontiguousarray(c.uv[:, old])) as prob:
        prob.set_state(c.cams[:-2], c.pts)
        prob.iterate_pcg(5.0, 1)                           # builds the lists of the old scene, then the scene grows
        prob.append(c.cams[-2:], np.zeros((3, 0)), c.cam_idx[~old], c.pt_idx[~old], np.ascontiguousarray(c.uv[:, ~old]))
        ptr, cam, uv = prob.structure()
        assert np.array_equal(ptr, c.pt_ptr) and np.array_equal(cam, c.cam_idx) and same_bits(uv, c.uv)
        got = _run(prob, c, c.cams, c.pts)
    assert all(same_bits(x, y) for x, y in zip(got, want))


def test_a_culled_scene_gives_the_bits_of_the_same_scene_created_whole(hip, sfm):
    c = pr.case(sfm, "6x300")
    with _problem(hip, c) as prob:
        prob.set_state(c.cams, c.pts)
        prob.iterate_pcg(5.0, 1)                           # builds the lists of the scene before the cull
        prob.set_state(c.cams, c.pts)
        err2 = prob.screen().err2
        report = prob.cull(float(np.quantile(err2, 0.9)), 1.0, 2)
        ptr, cam, uv = prob.structure()
        assert 0 < np.count_nonzero(report.obs_flags) < c.cam_idx.shape[0] // 5 and cam.shape[0] < c.cam_idx.shape[0]
        got = _run(prob, c, c.cams, c.pts)
    with hip.BaProblem(c.n_cams, ptr, cam, uv) as whole:
        want = _run(whole, c, c.cams, c.pts)
    assert all(same_bits(x, y) for x, y in zip(got, want))


# ---- 8: sfm_ba_iterate undisturbed --------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [0, 1])
def test_iterate_is_undisturbed(hip, sfm, oracle, graph):
    c = pr.case(sfm, "6x300")

    def fresh():
        p = hip.BaProblem(c.n_cams, c.pt_ptr, c.cam_idx, c.uv)
        p.set_option(hip.OPT_DETERMINISTIC, 1)
        p.set_option(hip.OPT_GRAPH, graph)
        return p

    with fresh() as prob, fresh() as other:
        other.set_state(c.cams, c.pts)
        other.iterate(5.0, 2)
        want = other.get_state() + (other.get_stats(),)
        prob.set_state(c.cams, c.pts)
        prob.iterate_pcg(5.0, 2, mask=pr.free_mask(c.n_cams, "held01"))
        prob.set_state(c.cams, c.pts)
        prob.iterate(5.0, 2)
        got = prob.get_state() + (prob.get_stats(),)
        assert all(same_bits(x, y) for x, y in zip(got, want))
        # iterate_pcg, then iterate, against the NumPy equivalent
        prob.set_state(c.cams, c.pts)
        prob.iterate_pcg(5.0, 1, tol=TIGHT)
        prob.iterate(5.0, 1)
        cams, pts = prob.get_state()
        assert prob.get_stats().shape[0] == 1              # the cost history restarted with the PCG call
    q = oracle.QUIRKS_REFERENCE
    mid_c, mid_p, _cost = pr.step_direct(c, c.cams, c.pts, 5.0, q)
    want_c, want_p = oracle.ba_sparse(mid_c, mid_p, c.cam_idx, c.pt_idx, c.uv, 5.0, 1)
    assert pr.rel(cams, want_c) <= 1e-9 and pr.rel(pts, want_p) <= 1e-9


# ---- 9: the drop-in -----------------------------------------------------------------------------------------------
class _KP:
    def __init__(self, x, y):
        self.pt = (float(x), float(y))


class _View:
    def __init__(self, rot, loc, k, key_pts):
        self.rot, self.loc, self.k, self.key_pts = rot, loc, k, key_pts

    def update_cam_pose(self, rot, loc):
        self.rot, self.loc = rot, loc


class _Holder:
    pass


def _drop_in(sfm, sc):
    vp, kt = _Holder(), _Holder()
    vp.view_list, kt.track_list = [], []
    tp = sfm.processors.HipTriangulationProcessor(0.5, 30)
    tp.tri_pts = np.vstack((sc.pts_init, np.ones((1, sc.n_pts))))
    bp = sfm.processors.HipBaProcessor(vp, kt, None, tp, None, iteration=3, damping_factor=5)
    bp.ba_verbose = False
    for c in range(sc.n_cams):
        sel = sc.cam_idx == c
        q = sc.cams_init[c, 3:7] / np.linalg.norm(sc.cams_init[c, 3:7])
        keys = [_KP(-1.0, -1.0)] + [_KP(x, y) for x, y in sc.uv_pix[:, sel].T]
        vp.view_list.append(_View(sfm.geometry.quaternion_to_rotation(q), sc.cams_init[c, 0:3].reshape(3, 1).copy(), sc.intrinsic.copy(), keys))
        track = _Holder()
        track.table = np.full((sc.n_cams, len(keys)), -1, dtype=int)
        track.table[c, 1:] = sc.pt_idx[sel]
        kt.track_list.append(track)
    return bp, vp, tp


def _poses(vp):
    return np.stack([v.rot for v in vp.view_list]), np.stack([np.asarray(v.loc).reshape(3) for v in vp.view_list])


def test_drop_in(hip, sfm):
    sc = sfm.scenes.make_scene(6, 300, 0.7, seed=21)
    results = {}
    for solver in ("dense", "pcg"):
        bp, vp, tp = _drop_in(sfm, sc)
        bp.ba_solver = solver
        try:
            bp.execute_bundle_adjustment()
        finally:
            bp.ba_release()
        results[solver] = _poses(vp) + (tp.tri_pts[0:3].copy(),)
        if solver == "pcg":
            last = bp.ba_pcg_last
            assert last.iters_done == 3 and not last.cg_status.any() and np.all(last.cg_rel <= 1e-10)
        else:
            assert bp.ba_pcg_last is None
    for got, want in zip(results["pcg"], results["dense"]):
        assert pr.rel(got, want) <= 1e-9
    # two views held: their rot / loc come back bit for bit, twice (the second call takes the resident scene up again)
    bp, vp, tp = _drop_in(sfm, sc)
    bp.ba_solver, bp.ba_hold_views = "pcg", (0, 1)
    rots0, locs0 = _poses(vp)
    try:
        for _ in range(2):
            bp.execute_bundle_adjustment()
            rots, locs = _poses(vp)
            assert same_bits(rots[:2], rots0[:2]) and same_bits(locs[:2], locs0[:2])
            assert not np.array_equal(rots[2:], rots0[2:])
    finally:
        bp.ba_release()
    # the two TypeError paths raise before anything is read
    bp, vp, tp = _drop_in(sfm, sc)
    bp.ba_hold_views = (0, 1)
    vp.view_list = None
    with pytest.raises(TypeError, match="ba_hold_views"):
        bp.execute_bundle_adjustment()
    bp.ba_hold_views, bp.ba_solver, bp.ba_resident = None, "pcg", False
    with pytest.raises(TypeError, match="ba_resident"):
        bp.execute_bundle_adjustment()
