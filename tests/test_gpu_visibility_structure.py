"""Bundle adjustment on track-structured and degenerate visibility (scenes.Structure) against the CPU oracle.

Every other BA scene of the suite is Bernoulli visibility: tracks of about p V views, a dense reduced camera system S,
every camera well observed.  The reference's incremental loop (ba_processor.py:137-267) makes a different shape: a point
enters with its second view and is then seen by a run of consecutive views, so S is block-banded, most tracks have 2-4
views and a few are very long.  The scenes here have that shape, and the degenerate ones next to it: cameras without any
observation (their block row of S is exactly lambda I), points with one observation, disjoint camera clusters (S
block-diagonal), one camera that sees every point.

Camera counts straddle the code's own thresholds (8/9 small solve -> data-flow solve, 18/19 one dense product tile ->
several, 36/37 reduce inside the solve's launch, 102/103 fused linearise + back substitution -> separate launches, 151/152
ba_linearize LDS mode 2 -> 1, 234/235 LDS mode 1 -> 0 and the deterministic-mode limit, 237/238 data-flow solve -> column
steps); the rows kernel's LDS pitch changes at M / (N V) = 0.25.  Every oracle result is computed once per scene (module
cache).  Tolerances are the suite's: S 1e-11 and rhs 1e-10 relative, states 1e-9 relative max-norm."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9
MODES = ("pairs", "mfma", "rows", "auto")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def mode_id(hip, mode):
    return {"auto": hip.SCHUR_AUTO, "pairs": hip.SCHUR_PAIRS, "mfma": hip.SCHUR_MFMA, "rows": hip.SCHUR_ROWS}[mode]


def kernel_name(hip, k):
    return {hip.SCHUR_PAIRS: "pairs", hip.SCHUR_MFMA: "mfma", hip.SCHUR_ROWS: "rows"}.get(k, str(k))


# name -> (cameras, points, Structure arguments, seed); what each is meant to reach is in SCENE_PATHS
SCENES = {
    "empty_first_8": (8, 600, dict(mean_track=3.0, empty=(0,)), 1),
    "empty_mid_9": (9, 600, dict(mean_track=3.0, empty=(4,)), 2),
    "band_12": (12, 1500, dict(mean_track=4.0), 3),
    "empty_last_18": (18, 1500, dict(mean_track=3.0, empty=(17,)), 4),
    "heavy_19": (19, 2000, dict(mean_track=2.5, heavy=0.02), 5),
    "clusters3_36": (36, 2400, dict(mean_track=3.0, clusters=3), 6),
    "band_50": (50, 4000, dict(mean_track=4.0), 7),
    "empty_group_50": (50, 4000, dict(mean_track=4.0, empty=tuple(range(7, 14))), 8),
    "hub_50": (50, 3000, dict(mean_track=2.0, hub=(0,)), 9),
    "clusters2_60": (60, 3000, dict(mean_track=3.0, clusters=2), 10),
    "single_24": (24, 2000, dict(mean_track=3.0, single=0.15, empty=(11,)), 11),
}
SCENE_PATHS = {
    "empty_first_8": "P = 56: the single-launch small solve; camera 0 has no observation",
    "empty_mid_9": "P = 63: the data-flow solve; an empty camera inside the band",
    "band_12": "one dense product tile; M / (N V) = 0.29: rows kernel pitch 7",
    "empty_last_18": "the largest one-tile dense product; the last camera empty",
    "heavy_19": "several dense product tiles; a few tracks over every camera from their birth on",
    "clusters3_36": "block-diagonal S over three clusters; 36 cameras: the reduce stays its own launch",
    "band_50": "M / (N V) = 0.08: rows kernel pitch 8, R = 7 cameras per group",
    "empty_group_50": "cameras 7-13 = the whole second rows-kernel group without observations (one empty chunk)",
    "hub_50": "camera 0 sees every point, the rest two each: the rows kernel's most uneven camera split",
    "clusters2_60": "block-diagonal S over two clusters of 30 cameras",
    "single_24": "15 % of the points have one observation; camera 11 empty",
}
# heavy tails over the upper thresholds: mean track 2.3 plus 1 % of the tracks to the last camera keeps M / N <= 4, so
# ba_linearize's lane group is G = 4 and the long tracks loop V / 4 times
HEAVY = {v: (v, 3000, dict(mean_track=2.3, heavy=0.01), 100 + v) for v in (37, 102, 103, 151, 152, 234, 235, 237, 238, 240)}
HEAVY_PATHS = {
    37: "three dense tiles: the split-K reduce rides in the solve's launch (SFM_INFO_REDUCE_IN_SOLVE with the dense product)",
    102: "the last size with the fused linearise + back substitution", 103: "separate back substitution launch",
    151: "ba_linearize LDS mode 2 (last)", 152: "ba_linearize LDS mode 1",
    234: "LDS mode 1 (last); the deterministic-mode limit", 235: "LDS mode 0: global atomics",
    237: "the data-flow solve (last)", 238: "column steps of the reduced solve", 240: "column steps, LDS mode 0",
}
# lambda and iteration counts per scene for the iteration tests: every scene at both dampings
RUNS = {name: [(0.5, 2), (5.0, 1)] for name in SCENES}
RUNS.update({v: [(0.5, 2), (5.0, 3)] for v in HEAVY})
# the side of the rows kernel's pitch switch (ba_rows_plan: pitch 8 when M / (N V) <= 0.25) a scene is meant to sit on
PITCH8 = {"band_12": False, "band_50": True, "empty_group_50": True, "hub_50": True}

_cache = {}


def scene(sfm, key):
    if ("scene", key) not in _cache:
        nv, npt, kw, seed = HEAVY[key] if key in HEAVY else SCENES[key]
        sc = sfm.scenes.make_scene(nv, npt, seed=seed, structure=sfm.scenes.Structure(**kw))
        _cache[("scene", key)] = (sc, sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic), sfm.scenes.Structure(**kw))
    return _cache[("scene", key)]


def oracle_reduced(sfm, oracle, key, lam):
    if ("S", key, lam) not in _cache:
        sc, uvn, _ = scene(sfm, key)
        _cache[("S", key, lam)] = oracle.ba_reduced_system(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, lam)
    return _cache[("S", key, lam)]


def oracle_iterations(sfm, oracle, key, lam, iters):
    if ("it", key, lam, iters) not in _cache:
        sc, uvn, _ = scene(sfm, key)
        _cache[("it", key, lam, iters)] = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, lam, iters)
    return _cache[("it", key, lam, iters)]


def linked_cameras(n_cams, cam_idx, pt_idx, n_pts):
    """(V, V) bool: camera pairs that share a point -- every other 7 x 7 block of S is structurally zero."""
    vis = np.zeros((n_cams, n_pts), dtype=np.int64)
    vis[cam_idx, pt_idx] = 1
    return (vis @ vis.T) > 0


def assert_intended_regime(sc, name):
    """Hold a scene on the side of the rows kernel's pitch switch its SCENE_PATHS entry names."""
    if name in PITCH8:
        ratio = sc.n_obs / (sc.n_pts * sc.n_cams)
        assert (ratio <= 0.25) == PITCH8[name], "%s: M / (N V) = %.3f" % (name, ratio)


def assert_structural_zeros(s, linked, empty, lam_on_diagonal, what):
    """Blocks of S that no point touches are exactly 0.0; an empty camera's diagonal block is exactly lambda I (the
    packed buffer holds S before lambda: exactly 0 there)."""
    nv = linked.shape[0]
    blocks = np.asarray(s).reshape(nv, 7, nv, 7).transpose(0, 2, 1, 3)
    nz = np.any(blocks != 0.0, axis=(2, 3))
    off = ~linked & ~np.eye(nv, dtype=bool)
    bad = np.argwhere(off & nz)
    assert bad.shape[0] == 0, "%s: %d structurally zero blocks written, first %s" % (what, bad.shape[0], bad[:4].tolist())
    for c in empty:
        assert np.array_equal(blocks[c, c], lam_on_diagonal * np.eye(7)), "%s: empty camera %d diagonal" % (what, c)


def assert_empty_cameras_unmoved(cams, cams_init, empty, what):
    for c in empty:
        assert np.array_equal(cams[c, 0:3], cams_init[c, 0:3]), "%s: empty camera %d moved" % (what, c)
        assert np.max(np.abs(cams[c, 3:7] - cams_init[c, 3:7])) <= 1e-15, "%s: empty camera %d turned" % (what, c)


# ---- 1. the reduced system per Schur kernel ------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SCENES))
def test_reduced_system_on_structured_scenes(hip, sfm, oracle, name, mode):
    """sfm_ba_reduced_system (S with lambda, rhs) per Schur kernel against the oracle; structurally zero blocks exactly 0.0;
    an empty camera's block row exactly lambda I and its rhs exactly 0.  Path: SCENE_PATHS[name]."""
    sc, uvn, st = scene(sfm, name)
    assert_intended_regime(sc, name)
    lam = 0.5
    t = oracle_reduced(sfm, oracle, name, lam)
    s, rhs = hip.ba_reduced_system(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn, sc.cams_init, sc.pts_init, lam,
                                   schur_mode=mode_id(hip, mode))
    what = "%s / %s (%s)" % (name, mode, SCENE_PATHS[name])
    assert rel(s, t["S"]) < 1e-11, what
    assert rel(rhs, t["rhs"]) < 1e-10, what
    assert np.array_equal(s, s.T), what
    assert_structural_zeros(s, linked_cameras(sc.n_cams, sc.cam_idx, sc.pt_idx, sc.n_pts), st.empty, lam, what)
    for c in st.empty:
        assert not np.any(rhs[7 * c:7 * c + 7]), what


# ---- 2. iterations against the oracle (every Schur kernel, AUTO's pick recorded) -----------------------------------------


def run_modes(hip, sc, uvn, lam, iters, modes=MODES):
    out = {}
    for mode in modes:
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_option(hip.OPT_SCHUR, mode_id(hip, mode))
            prob.set_state(sc.cams_init, sc.pts_init)
            assert prob.info(hip.INFO_MAX_TRACK) == int(np.max(np.diff(sc.pt_ptr)))
            pick = prob.info(hip.INFO_SCHUR_KERNEL)
            prob.iterate(lam, iters)
            cams, pts = prob.get_state()
            out[mode] = dict(cams=cams, pts=pts, pick=pick, in_solve=prob.info(hip.INFO_REDUCE_IN_SOLVE),
                             cost=prob.get_stats())
    return out


def check_against_oracle(hip, res, want, sc, st, what):
    want_c, want_p = want
    for mode, r in res.items():
        w = "%s / %s (kernel run: %s)" % (what, mode, kernel_name(hip, r["pick"]))
        if mode != "auto":
            assert r["pick"] == mode_id(hip, mode), w
        assert rel(r["cams"], want_c) < TOL and rel(r["pts"], want_p) < TOL, w
        assert np.all(np.isfinite(r["cost"])) and np.all(r["cost"] > 0), w
        assert np.max(np.abs(np.linalg.norm(r["cams"][:, 3:7], axis=1) - 1.0)) < 1e-14, w
        assert_empty_cameras_unmoved(r["cams"], sc.cams_init, st.empty, w)


@pytest.mark.parametrize("name", list(SCENES))
def test_iterations_on_structured_scenes(hip, sfm, oracle, name):
    """1 and 2 iterations at lambda 0.5 and 5 through every Schur kernel against the oracle.  Path: SCENE_PATHS[name]."""
    sc, uvn, st = scene(sfm, name)
    assert_intended_regime(sc, name)
    for lam, iters in RUNS[name]:
        res = run_modes(hip, sc, uvn, lam, iters)
        check_against_oracle(hip, res, oracle_iterations(sfm, oracle, name, lam, iters), sc, st,
                             "%s lam %g x%d (%s)" % (name, lam, iters, SCENE_PATHS[name]))
        if name == "clusters3_36":
            assert res["mfma"]["in_solve"] == 0                 # two tiles: the reduce keeps its own launch


@pytest.mark.parametrize("n_cams", sorted(HEAVY))
def test_iterations_heavy_tail_across_thresholds(hip, sfm, oracle, n_cams):
    """Tracks of 2-3 views plus 1 % that run to the last camera: G = 4 lanes per point in ba_linearize, so those tracks go
    round its loop up to V / 4 times, and they fill the rows kernel's lanes.  Path: HEAVY_PATHS[n_cams]."""
    sc, uvn, st = scene(sfm, n_cams)
    assert sc.n_obs / sc.n_pts <= 4.0                          # pick_group: G = 4
    assert np.max(np.diff(sc.pt_ptr)) > n_cams // 2
    for lam, iters in RUNS[n_cams]:
        res = run_modes(hip, sc, uvn, lam, iters)
        check_against_oracle(hip, res, oracle_iterations(sfm, oracle, n_cams, lam, iters), sc, st,
                             "heavy %d lam %g x%d (%s)" % (n_cams, lam, iters, HEAVY_PATHS[n_cams]))
        if n_cams == 37:
            assert res["mfma"]["in_solve"] == 1


def test_iterations_reference_regime_c3_size(hip, sfm, oracle):
    """The C3 size (50 cameras x 20 000 points) with the reference's track shape (runs of mean length 4) instead of 60 %
    Bernoulli visibility: 3 iterations at lambda 0.5 and 2 at lambda 5 through every Schur kernel, AUTO's pick recorded.
    Two oracle runs (about 4 s on the CPU)."""
    sc = sfm.scenes.make_scene(50, 20000, seed=50, structure=sfm.scenes.Structure(mean_track=4.0))
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    for lam, iters in ((0.5, 3), (5.0, 2)):
        want = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, lam, iters)
        res = run_modes(hip, sc, uvn, lam, iters)
        check_against_oracle(hip, res, want, sc, sfm.scenes.Structure(), "C3-size tracks lam %g x%d" % (lam, iters))


# ---- 3. AUTO on track structure ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(SCENES) + sorted(HEAVY))
def test_auto_pick_matches_oracle(hip, sfm, oracle, name):
    """Whatever SFM_SCHUR_AUTO picks from its occupancy model (INFO_SCHUR_KERNEL, in the message), the iterations equal
    the oracle's.  Speed is not judged here."""
    sc, uvn, st = scene(sfm, name)
    lam, iters = RUNS[name][0]
    res = run_modes(hip, sc, uvn, lam, iters, modes=("auto",))
    assert res["auto"]["pick"] in (hip.SCHUR_PAIRS, hip.SCHUR_MFMA, hip.SCHUR_ROWS)
    check_against_oracle(hip, res, oracle_iterations(sfm, oracle, name, lam, iters), sc, st, "AUTO on %s" % name)


# ---- 4. growth in the reference's order ---------------------------------------------------------------------------------


GROW_V, GROW_N = 110, 2400
# after registering these views the packed reduced buffer is compared (20, 40 and 104 cameras)
GROW_CHECK = (19, 39, 103)


def growth_steps():
    """Registered views after each append: one at a time to 12 cameras, then four, then eight at a time."""
    steps = list(range(2, 12)) + list(range(12, 40, 4)) + list(range(40, GROW_V, 8)) + [GROW_V - 1]
    out = sorted(set(steps) | set(GROW_CHECK))
    return [v for v in out if v >= 1]


def grow_plan(sfm):
    """A tracks scene in the reference's order: a point enters when its second view registers (its birth + 1; points are
    numbered in birth order, so in order of entry); every later view of its run adds an observation to it."""
    if "grow" not in _cache:
        sc = sfm.scenes.make_scene(GROW_V, GROW_N, seed=77, structure=sfm.scenes.Structure(mean_track=3.0, heavy=0.01))
        uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
        entry = sc.cam_idx[sc.pt_ptr[:-1] + 1]                      # second view of every point
        assert np.all(np.diff(entry) >= 0)
        _cache["grow"] = (sc, uvn, entry)
    return _cache["grow"]


def grow_oracle(sfm, oracle, lam):
    """Oracle states after every step (2 iterations each), and the reduced system at the check points."""
    if ("grow_or", lam) not in _cache:
        sc, uvn, entry = grow_plan(sfm)
        cams, pts = sc.cams_init[:2].copy(), sc.pts_init[:, :0]
        states, reduced = {}, {}
        for v in [1] + growth_steps():
            n_now = int(np.sum(entry <= v))
            cams = np.vstack((cams, sc.cams_init[cams.shape[0]:v + 1]))
            pts = np.hstack((pts, sc.pts_init[:, pts.shape[1]:n_now]))
            act = np.flatnonzero((sc.cam_idx <= v) & (entry[sc.pt_idx] <= v))        # already sorted by (point, camera)
            if v in GROW_CHECK:
                reduced[v] = oracle.ba_reduced_system(cams, pts, sc.cam_idx[act], sc.pt_idx[act], uvn[:, act], lam)
            cams, pts = oracle.ba_sparse(cams, pts, sc.cam_idx[act], sc.pt_idx[act], uvn[:, act], lam, 2)
            states[v] = (cams, pts, act)
        _cache[("grow_or", lam)] = (states, reduced)
    return _cache[("grow_or", lam)]


@pytest.mark.parametrize("mode", MODES)
def test_growth_in_reference_order_matches_oracle(hip, sfm, oracle, mode):
    """View-by-view growth of a tracks scene through sfm_ba_append -- every new view extends the tracks of existing points
    and brings new ones -- with 2 iterations after every step, from 2 cameras past 9, 19, 37 and 103, against the oracle.
    At 20, 40 and 104 cameras, after earlier iterations and an append, the resident handle's packed reduced buffer (S before
    lambda, rhs) equals the oracle's and its structurally zero blocks are exactly 0.0: a dense-product Zd slot or a block of S
    left over from before the growth would show there."""
    import torch
    sh = sfm.sharding
    lam = 0.5
    sc, uvn, entry = grow_plan(sfm)
    states, reduced = grow_oracle(sfm, oracle, lam)
    act = np.flatnonzero((sc.cam_idx <= 1) & (entry[sc.pt_idx] <= 1))
    n1 = int(np.sum(entry <= 1))
    ptr = np.zeros(n1 + 1, dtype=np.int32)
    np.cumsum(np.bincount(sc.pt_idx[act], minlength=n1), out=ptr[1:])
    eng = sh.HipShardEngine(2, ptr, sc.cam_idx[act], uvn[:, act], torch.device("cuda", 0))
    try:
        eng.prob.set_option(hip.OPT_SCHUR, mode_id(hip, mode))
        eng.set_state(sc.cams_init[:2], sc.pts_init[:, :n1])
        have = np.zeros(sc.n_obs, dtype=bool); have[act] = True
        eng.iterate_local(lam, 2)
        n_pts = n1
        for v in growth_steps():
            now = (sc.cam_idx <= v) & (entry[sc.pt_idx] <= v)
            add = np.flatnonzero(now & ~have)
            n_now = int(np.sum(entry <= v))
            eng.append(sc.cams_init[eng.prob.n_cams:v + 1], sc.pts_init[:, n_pts:n_now], sc.cam_idx[add], sc.pt_idx[add],
                       uvn[:, add])
            have, n_pts = now, n_now
            what = "%s, %d cameras" % (mode, v + 1)
            assert eng.prob.info(hip.INFO_MAX_TRACK) == int(np.max(np.bincount(sc.pt_idx[have]))), what
            if v in GROW_CHECK:
                with eng.stream_context():
                    buf = eng.linearize_reduce(lam)
                torch.cuda.synchronize()
                host = buf.cpu().numpy()
                s_gpu, rhs_gpu = sh.unpack_reduced(host, v + 1)
                t = reduced[v]
                s_or = t["S"] - lam * np.eye(7 * (v + 1))
                assert np.max(np.abs(s_gpu - s_or)) < 1e-11 * np.max(np.abs(s_or)), what
                assert np.max(np.abs(rhs_gpu - t["rhs"])) < 1e-10 * np.max(np.abs(t["rhs"])), what
                idx = np.flatnonzero(have)
                assert_structural_zeros(s_gpu, linked_cameras(v + 1, sc.cam_idx[idx], sc.pt_idx[idx], n_now), (), 0.0, what)
                assert np.array_equal(sh.pack_reduced(s_gpu, rhs_gpu), host), what
                eng.solve_update(lam)
                eng.flush()
                eng.iterate_local(lam, 1)
            else:
                eng.iterate_local(lam, 2)
            cams, pts = eng.get_state()
            want_c, want_p, _ = states[v]
            assert rel(cams, want_c) < TOL and rel(pts, want_p) < TOL, what
    finally:
        eng.close()


# ---- 5. bitwise modes --------------------------------------------------------------------------------------------------


def test_graph_replay_bitwise_on_heavy_tail_with_empty_camera(hip, sfm, oracle):
    """SFM_OPT_GRAPH on a heavy-tail 60-camera scene with an empty camera (graphs need the fused linearisation: at most 102
    cameras), in the call pattern of test_ba_graph_replay_equals_eager_launches: the graph run replays (INFO_GRAPH_REPLAYS),
    the eager runs do not; with SFM_OPT_DETERMINISTIC two eager runs and the graph run are bit-identical, without it they
    agree to 1e-12; both match the oracle and leave the empty camera where it was."""
    sc = sfm.scenes.make_scene(60, 2400, seed=60, structure=sfm.scenes.Structure(mean_track=2.5, heavy=0.01, empty=(30,)))
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    want_c, want_p = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 5.0, 8)
    want_c, want_p = oracle.ba_sparse(want_c, want_p, sc.cam_idx, sc.pt_idx, uvn, 4.0, 3)
    for det in (1, 0):
        out, stats, replays = [], [], []
        for graph in ((0, 0, 1) if det else (0, 1)):
            with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
                prob.set_option(hip.OPT_DETERMINISTIC, det)
                prob.set_option(hip.OPT_GRAPH, graph)
                prob.set_state(sc.cams_init, sc.pts_init)
                prob.iterate(5.0, 6)
                prob.iterate(5.0, 2)                       # a second call: starts eagerly, then replays
                prob.iterate(4.0, 3)                       # another lambda: new graphs
                stats.append(prob.get_stats())
                out.append(prob.get_state())
                replays.append(prob.info(hip.INFO_GRAPH_REPLAYS))
        what = "deterministic" if det else "plain"
        assert all(r == 0 for r in replays[:-1]) and replays[-1] >= 4, (what, replays)
        for (cams, pts), cost in zip(out[1:], stats[1:]):
            if det:
                assert np.array_equal(cams, out[0][0]) and np.array_equal(pts, out[0][1]), what
                assert np.array_equal(cost, stats[0]), what
            else:
                assert rel(cams, out[0][0]) < 1e-12 and rel(pts, out[0][1]) < 1e-12, what
        for cams, pts in out:
            assert rel(cams, want_c) < TOL and rel(pts, want_p) < TOL, what
            assert_empty_cameras_unmoved(cams, sc.cams_init, (30,), what)


def test_deterministic_bitwise_on_heavy_tail_with_empty_camera(hip, sfm, oracle):
    """SFM_OPT_DETERMINISTIC on a heavy-tail 120-camera scene with an empty camera: two fresh runs are bit-identical and match
    the oracle.  A third run asks for SFM_OPT_GRAPH: above 102 cameras there is no fused linearisation to capture, so it
    launches eagerly (no replay) and gives the same bits."""
    sc = sfm.scenes.make_scene(120, 3000, seed=120,
                               structure=sfm.scenes.Structure(mean_track=2.5, heavy=0.01, empty=(60,)))
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    want_c, want_p = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 5.0, 3)
    out, stats = [], []
    for graph in (0, 0, 1):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_option(hip.OPT_DETERMINISTIC, 1)
            prob.set_option(hip.OPT_GRAPH, graph)
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(5.0, 3)
            out.append(prob.get_state())
            stats.append(prob.get_stats())
            assert prob.info(hip.INFO_GRAPH_REPLAYS) == 0
    for (cams, pts), cost in zip(out[1:], stats[1:]):
        assert np.array_equal(cams, out[0][0]) and np.array_equal(pts, out[0][1]) and np.array_equal(cost, stats[0])
    assert rel(out[0][0], want_c) < TOL and rel(out[0][1], want_p) < TOL
    assert_empty_cameras_unmoved(out[0][0], sc.cams_init, (60,), "deterministic")


def test_deterministic_mode_limit_on_heavy_tail(hip, sfm, oracle):
    """The deterministic mode's limit: 234 cameras run (two runs bit-identical, equal to the oracle), 235 are refused."""
    sc, uvn, st = scene(sfm, 234)
    lam, iters = RUNS[234][0]
    out = []
    for _ in range(2):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_option(hip.OPT_DETERMINISTIC, 1)
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(lam, iters)
            out.append(prob.get_state())
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    want_c, want_p = oracle_iterations(sfm, oracle, 234, lam, iters)
    assert rel(out[0][0], want_c) < TOL and rel(out[0][1], want_p) < TOL
    sc, uvn, st = scene(sfm, 235)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        with pytest.raises(ValueError):
            prob.set_option(hip.OPT_DETERMINISTIC, 1)
