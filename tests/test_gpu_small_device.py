"""Every launch plan that depends on the device's compute-unit count, run at small counts (sfm_set_cu_limit: 1, 2, 32, 33, 64 and
none): the persistent linearisation and back substitution with many trips per workgroup, the Schur plans and the decisions
that follow from them, the data-flow solve with few task workgroups (and the column steps where it cannot run), the split PnP
with one view per launch -- each against the reference and the tolerance of the module that owns the operation.  The limit
shapes the plans only: the workgroups still run on every compute unit of the device.

Also here, because it is the same kind of caller-told number: sfm_pnp_nonlinear_batch_dev told a max_view_points smaller than
its largest view."""
import gc
import time

import numpy as np
import pytest

import _cov_reference as cr
import _pcg_reference as pr
import _robust_reference as rr
import _tracks_reference as tr
from test_sharding_gloo import _pnp_case

pytestmark = pytest.mark.gpu

TOL = 1e-9                                # test_gpu_parity.py
LIMITS = (1, 2, 32, 33, 64, 0)            # 0: none
BA_SHAPES = [(9, 600, 0.8), (19, 900, 0.5), (37, 1500, 0.4), (74, 1200, 0.3)]      # 2, 5, 9 and 17 block columns
_CACHE = {}


@pytest.fixture(autouse=True)
def _limit_back_to_none(hip):
    gc.collect()                          # no handle of an earlier test waiting for the collector: the limit is refused while one lives
    yield
    gc.collect()
    hip.set_cu_limit(0)
    dev, eff = hip.cu_count()
    assert eff == dev


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ba_case(sfm, oracle, shape, seed_base=1100):
    """(scene, normalised keys, oracle cameras and points after 3 iterations at lambda = 5, the oracle's cost at the start of each),
    once per shape and left unchanged."""
    if shape not in _CACHE:
        sc = sfm.scenes.make_scene(*shape, seed=seed_base + shape[0])
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        trace = []
        want_c, want_p = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 5.0, 3, trace=trace)
        states = [(sc.cams_init, sc.pts_init)] + trace[:2]
        costs = np.array([float(np.sum(oracle.obs_terms_vec(c, p, sc.cam_idx, sc.pt_idx, uvn)[0] ** 2)) for c, p in states])
        for a in (uvn, want_c, want_p, costs):
            a.setflags(write=False)
        _CACHE[shape] = (sc, uvn, want_c, want_p, costs)
    return _CACHE[shape]


def _effective(hip, limit):
    dev = hip.cu_count()[0]
    return min(limit, dev) if limit else dev


# ---- bundle-adjustment iterations -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("shape", BA_SHAPES)
def test_ba_iterations_against_the_oracle(hip, oracle, sfm, shape, limit):
    """Every Schur kernel and the automatic choice, three iterations, against oracle.ba_sparse.  Under limit 1 the linearisation
    runs on 3 workgroups and the back substitution on 4 -- every scene here makes many trips per workgroup -- and the solve is the
    column steps; from 2 on it is the data-flow launch with 1, 31, 32 and 32 task workgroups at most."""
    sc, uvn, want_c, want_p, want_cost = _ba_case(sfm, oracle, shape)
    hip.set_cu_limit(limit)
    assert hip.cu_count()[1] == _effective(hip, limit)
    for mode in ("pairs", "mfma", "rows", "auto"):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_option(hip.OPT_SCHUR, {"pairs": hip.SCHUR_PAIRS, "mfma": hip.SCHUR_MFMA, "rows": hip.SCHUR_ROWS, "auto": hip.SCHUR_AUTO}[mode])
            path = prob.info(hip.INFO_SOLVE_PATH)
            assert path == (hip.SOLVE_STEPS if limit == 1 else hip.SOLVE_FLOW)
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(5.0, 3)
            cams, pts = prob.get_state()
            cost = prob.get_stats()
            in_solve = prob.info(hip.INFO_REDUCE_IN_SOLVE)
        print(shape, limit, mode, "cameras %.2e points %.2e cost %.2e reduce in solve %d" % (rel(cams, want_c), rel(pts, want_p), rel(cost, want_cost), in_solve))
        assert rel(cams, want_c) < TOL and rel(pts, want_p) < TOL, (shape, limit, mode)
        assert not (limit == 1 and in_solve)                  # no data-flow launch to take the reduce
        if limit == 1:
            # ba_linearize's per-workgroup cost slots (cost_ws) with 3 workgroups, summed by the reduce: as
            # test_ba_per_iteration_cost_statistics holds the full-size grid
            assert cost.shape == (3,) and rel(cost, want_cost) < 1e-10, (shape, mode)


def test_reduce_in_solve_is_decided_by_the_plan_of_the_count(hip, sfm):
    """ba_solve_can_defer_reduce follows the dense plan's slab counts, which follow the CU count: over the shapes where it can be
    chosen and all limits, some (shape, limit) leave the reduce to the solve's launch and some keep it a launch of its own.  (Both
    kinds are held against the oracle above: mode mfma.)"""
    seen = {}
    for shape in BA_SHAPES[2:]:
        sc = sfm.scenes.make_scene(*shape, seed=1100 + shape[0])
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        for limit in LIMITS:
            hip.set_cu_limit(limit)
            with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
                prob.set_option(hip.OPT_SCHUR, hip.SCHUR_MFMA)
                prob.set_state(sc.cams_init, sc.pts_init)
                prob.iterate(5.0, 1)
                prob.get_state()
                seen[(shape[0], limit)] = prob.info(hip.INFO_REDUCE_IN_SOLVE)
    print(seen)
    assert any(seen.values()) and not all(seen.values())
    assert not any(v for (_, limit), v in seen.items() if limit == 1)


# ---- the solve alone --------------------------------------------------------------------------------------------------------
def _solve_from_saved(hip, torch, sc, uvn, saved, debug=0):
    """One problem: linearise, replace [S | rhs] by `saved` (or save it), solve.  (cameras, saved, solve path, seconds of the solve)."""
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_option(hip.OPT_DEBUG, debug)
        _ptr, n, _ld = prob.reduced_buffer()
        buf = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        prob.bind_reduced_buffer(buf.data_ptr(), n)
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.linearize_reduce(5.0)
        hip.synchronize()
        if saved is None:
            saved = buf.clone()
        else:
            buf.copy_(saved)
        torch.cuda.synchronize()
        path = prob.info(hip.INFO_SOLVE_PATH)
        t0 = time.perf_counter()
        prob.solve_update(5.0)
        hip.synchronize()
        seconds = time.perf_counter() - t0
        cams, _pts = prob.get_state()
        prob.bind_reduced_buffer(0, 0)
    return cams, saved, path, seconds


@pytest.mark.parametrize("shape,limits", [((19, 900, 0.5), LIMITS), ((74, 1200, 0.3), LIMITS), ((237, 2500, 0.15), (33, 0, 2))])
def test_solve_is_the_same_bits_at_every_workgroup_count(hip, sfm, shape, limits):
    """sfm_ba_flow.h: every block is produced by one task in a fixed order, whatever the placement.  The same [S | rhs] solved by
    the launch of every count -- 1 + 1 workgroups under limit 2, the one task workgroup taking the whole table (2 650 tasks at 52
    block columns) -- gives the same cameras bit for bit, within 1e-11 of the column steps (the figure of
    test_ba_data_flow_solve_against_column_steps_and_oracle); under limit 1 the column steps themselves run."""
    import torch
    sc = sfm.scenes.make_scene(*shape, seed=500 + shape[0])
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    saved, flow = None, {}
    for limit in limits:
        hip.set_cu_limit(limit)
        cams, saved, path, seconds = _solve_from_saved(hip, torch, sc, uvn, saved)
        print(shape, "limit", limit, "path", path, "solve %.1f ms (host clock, first use of the kernel included)" % (1e3 * seconds))
        assert path == (hip.SOLVE_STEPS if limit == 1 else hip.SOLVE_FLOW)
        flow[limit] = cams
    hip.set_cu_limit(0)
    steps, _, path, _ = _solve_from_saved(hip, torch, sc, uvn, saved, debug=1024)
    assert path == hip.SOLVE_STEPS
    first = next(limit for limit in limits if limit != 1)
    for limit in limits:
        if limit == 1:
            assert same_bits(flow[limit], steps)
        else:
            assert same_bits(flow[limit], flow[first]), (shape, limit)
            assert rel(flow[limit], steps) < 1e-11, (shape, limit)


# ---- deterministic mode, graph replay -----------------------------------------------------------------------------------------
def test_deterministic_mode_under_limit_2(hip, oracle, sfm):
    sc = sfm.scenes.make_scene(40, 1500, 0.5, seed=71)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    hip.set_cu_limit(2)
    runs = []
    for rep in range(2):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_option(hip.OPT_DETERMINISTIC, 1)
            assert prob.info(hip.INFO_SCHUR_KERNEL) == hip.SCHUR_MFMA
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(5.0, 3)
            runs.append(prob.get_state())
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    ocams, opts = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 5.0, 3)
    assert rel(runs[0][0], ocams) < TOL and rel(runs[0][1], opts) < TOL


def test_graph_replay_equals_eager_launches_under_limit_32(hip, sfm):
    """test_ba_graph_replay_equals_eager_launches at its smallest shape: the captured body holds the grids of the limit."""
    sc = sfm.scenes.make_scene(6, 800, 1.0, seed=91)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    hip.set_cu_limit(32)
    for det in (1, 0):
        out, stats, replays = [], [], []
        for graph in (0, 1):
            with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
                prob.set_option(hip.OPT_DETERMINISTIC, det)
                prob.set_option(hip.OPT_GRAPH, graph)
                prob.set_state(sc.cams_init, sc.pts_init)
                prob.iterate(5.0, 6)
                prob.iterate(5.0, 2)
                prob.iterate(4.0, 3)
                stats.append(prob.get_stats())
                out.append(prob.get_state())
                replays.append(prob.info(hip.INFO_GRAPH_REPLAYS))
        assert replays[0] == 0 and replays[1] >= 4
        if det:
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
            assert np.array_equal(stats[0], stats[1])
        else:
            assert rel(out[0][0], out[1][0]) < 1e-12 and rel(out[0][1], out[1][1]) < 1e-12


# ---- the other operations on the resident scene -----------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [1, 32])
def test_refine_cameras(hip, sfm, oracle, limit):
    import test_gpu_refine_cameras as m
    sc, uvn, _uvo, _disp, _scale, _deltas = m._scene(sfm)
    lam, iters, quirks = 0.1, 5, oracle.QUIRKS_REFERENCE
    want_c, want_cost, want_st = m._reference(("parity", lam, iters, quirks, rr.LOSS_NONE), sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx,
                                              uvn, lam, iters, rr.LOSS_NONE, 1.0, quirks)
    hip.set_cu_limit(limit)
    cams, cost, status, pts = m._device(hip, sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, sc.cams_init, sc.pts_init, lam, iters, quirks)
    assert m.rel(cams, want_c) < 1e-9 and m.rel(cost, want_cost) < 1e-9
    assert np.array_equal(status, want_st) and not status.any() and same_bits(pts, sc.pts_init)


@pytest.mark.parametrize("limit", [1, 32])
def test_iterate_pcg(hip, sfm, oracle, limit):
    import test_gpu_pcg as m
    c = pr.case(sfm, "6x300")
    hip.set_cu_limit(limit)
    with m._problem(hip, c) as prob:
        m._check_step(hip, prob, c, 5.0, oracle.QUIRKS_REFERENCE, "none", "none", ("6x300", "limit", limit))


@pytest.mark.parametrize("limit", [1, 32])
def test_covariance(hip, sfm, oracle, limit):
    import test_gpu_covariance as m
    name, quirks = "6x300", oracle.QUIRKS_REFERENCE
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, name)
    lam, held = cr.settings(name)[2]                         # lambda = 1e-3, cameras 0 and 1 held
    mask = cr.free_mask(sc.n_cams, held)
    ab, want = cr.ab_disagreement((name, quirks, rr.LOSS_NONE, lam, held), cams, pts, sc.cam_idx, sc.pt_idx, uvn, lam, mask, rr.LOSS_NONE,
                                  5.0 / _scale, quirks)
    hip.set_cu_limit(limit)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_state(cams, pts)
        out = prob.covariance(lam, quirks, False, mask)
        m._check(out, want, ab, (name, "limit", limit))
        assert not out.cam_cov[list(held)].any() and not out.pt_status.any()


@pytest.mark.parametrize("limit", [1, 32])
def test_screen(hip, sfm, limit):
    import test_gpu_screen as m
    hip.set_cu_limit(limit)
    rs, prob = m._problem(hip, sfm)
    with prob:
        # the width `group` = 0 stands for moves with the count on this scene: 32 lanes per point on one CU, 64 from 32 CUs on
        assert hip.tracks_auto_group(rs.n_pts, rs.cam_idx.shape[0], int(rs.lengths.max())) == (32 if limit == 1 else 64)
        got = prob.screen()
        m._check_values(got, m._ref(sfm))
        m._check_flags(got, m._ref(sfm))


@pytest.mark.parametrize("limit", [1, 32])
def test_refine_points_with_the_automatic_group(hip, sfm, limit):
    """The ragged scene of the track tests as a resident problem, `group` = 0 (32 lanes under limit 1, 64 under 32), against the
    per-point NumPy reference of tests/_tracks_reference.py."""
    rs = tr.ragged_scene(sfm)
    want, want_cost = tr.ragged_reference(sfm, 5.0, 3)
    hip.set_cu_limit(limit)
    assert hip.tracks_auto_group(rs.n_pts, rs.cam_idx.shape[0], int(rs.lengths.max())) == (32 if limit == 1 else 64)
    with hip.BaProblem(rs.scene.n_cams, rs.pt_ptr, rs.cam_idx, rs.uv) as prob:
        prob.set_state(rs.scene.cams_true, rs.x_init[0:3])
        cost, status = prob.refine_points(5.0, 3, group=0)
        cams, pts = prob.get_state()
    assert same_bits(cams, rs.scene.cams_true)
    assert rel(pts, want[0:3]) < 1e-9
    for row in (0, 1):
        big = want_cost[row] > 1e-20
        assert np.max(np.abs(cost[row, big] - want_cost[row, big]) / want_cost[row, big]) < 1e-9, row
        assert np.all(np.abs(cost[row, ~big]) <= 1e-20), row
    assert not (status & (hip.TRACK_TOO_FEW | hip.TRACK_NONFINITE)).any()


# ---- split PnP ----------------------------------------------------------------------------------------------------------------
def test_split_pnp_one_view_per_launch(hip, sfm, oracle):
    """Under limit 1 a launch of the split class holds max(1, 2 / kmax) = 1 view: views 0 and 2 run in launches of their own, the
    3 and 4 slices of each resident together.  Bit for bit the unrestricted batch, and the oracle's result."""
    sizes = [3000, 40, 3073]
    offsets, uvp, xs, ks, r0, c0 = _pnp_case(sfm, sizes, seed=23)
    rot, loc, st = hip.pnp_nonlinear_batch(offsets, uvp, xs, ks, r0, c0, 5.0, 4)
    assert not st.any()
    hip.set_cu_limit(1)
    rot1, loc1, st1 = hip.pnp_nonlinear_batch(offsets, uvp, xs, ks, r0, c0, 5.0, 4)
    assert same_bits(rot1, rot) and same_bits(loc1, loc) and not st1.any()
    for v in range(len(sizes)):
        a, b = int(offsets[v]), int(offsets[v + 1])
        r_or, c_or = oracle.nonlinear_pnp(uvp[:, a:b], xs[:, a:b], ks[v], r0[v], c0[v].reshape(3, 1), 5.0, 4)
        assert rel(rot1[v], r_or) < 1e-9 and rel(loc1[v], c_or.reshape(3)) < 1e-9, v


# ---- the refusal --------------------------------------------------------------------------------------------------------------
def test_limit_is_refused_while_a_problem_lives(hip, sfm):
    sc = sfm.scenes.make_scene(6, 300, 0.6, seed=5)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    lib = hip.load()
    hip.set_cu_limit(64)
    before = hip.cu_count()
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        for n in (0, 1, 32):
            assert lib.sfm_set_cu_limit(n) == hip.E_SHAPE
            assert "sfm_ba_problem" in hip.last_error()
            assert hip.cu_count() == before
        with pytest.raises(ValueError):
            hip.set_cu_limit(2)
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.iterate(5.0, 1)                                 # still the problem it was
        prob.get_state()
    hip.set_cu_limit(2)                                      # destroyed: accepted
    assert hip.cu_count() == (before[0], 2)


# ---- max_view_points smaller than the largest view --------------------------------------------------------------------------------
SENTINEL = 0x5EED


def _pnp_dev(hip, torch, case, told, stream):
    """sfm_pnp_nonlinear_batch_dev told `told`: (R, C, status, seconds), outputs pre-set to NaN and status to a sentinel."""
    offsets, uvp, xs, ks, r0, c0 = case
    n_views = offsets.shape[0] - 1
    d = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to("cuda")      # noqa: E731
    t_off, t_uv, t_x, t_k, t_r0, t_c0 = d(offsets, np.int32), d(uvp), d(xs), d(ks.reshape(-1, 9)), d(r0.reshape(-1, 9)), d(c0)
    t_r, t_c = torch.full_like(t_r0, float("nan")), torch.full_like(t_c0, float("nan"))
    t_st = torch.full((n_views,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hip.pnp_nonlinear_batch_dev(n_views, t_off.data_ptr(), uvp.shape[1], t_uv.data_ptr(), t_x.data_ptr(), t_k.data_ptr(), t_r0.data_ptr(),
                                t_c0.data_ptr(), 5.0, 4, hip.QUIRKS_REFERENCE, t_r.data_ptr(), t_c.data_ptr(), t_st.data_ptr(), stream.cuda_stream,
                                max_view_points=told)
    stream.synchronize()
    seconds = time.perf_counter() - t0
    return t_r.cpu().numpy().reshape(-1, 3, 3), t_c.cpu().numpy(), t_st.cpu().numpy(), seconds


@pytest.mark.parametrize("sizes,told", [([300, 1500, 40], 1000), ([40, 3100], 1500), ([3000, 5000, 10], 3500), ([5000], 3500)])
def test_pnp_told_less_than_its_largest_view(hip, sfm, sizes, told):
    """A view larger than max_view_points is refined by no launch (include/sfm_hip.h): it comes back as R0, C0 with status
    SFM_E_SHAPE, at once -- no slice waits for a sibling that was not launched --, and every view within the told size is bit for
    bit what the truthful call gives."""
    import torch
    stream = torch.cuda.Stream()
    case = _pnp_case(sfm, sizes, seed=29)
    _offsets, _uvp, _xs, _ks, r0, c0 = case
    rot_t, loc_t, st_t, _ = _pnp_dev(hip, torch, case, max(sizes), stream)
    assert not st_t.any() and np.all(np.isfinite(rot_t)) and np.all(np.isfinite(loc_t))
    rot, loc, st, seconds = _pnp_dev(hip, torch, case, told, stream)
    print(sizes, told, "status", st, "%.1f ms" % (1e3 * seconds))
    assert seconds < 1.0
    assert SENTINEL not in st.tolist()
    assert any(n > told for n in sizes)
    for v, n in enumerate(sizes):
        if n <= told:
            assert st[v] == 0 and same_bits(rot[v], rot_t[v]) and same_bits(loc[v], loc_t[v]), v
        else:
            assert st[v] == hip.E_SHAPE and same_bits(rot[v], r0[v]) and same_bits(loc[v], c0[v]), v
