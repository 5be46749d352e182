"""Property-based GPU parity (hypothesis): random small scenes -- camera count, point count, visibility, damping,
iteration count, quirk flags, Schur kernel, solve path -- through the C-ABI against the CPU oracle, plus the
size-independent properties the bundle-adjustment step has (cost history, idempotence of zero iterations, invariance
under the order in which the same observations are appended).  Sizes are kept to what the oracle does in
milliseconds; the example database is disabled so that a run never depends on local state."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

pytestmark = pytest.mark.gpu

import os

TOL = 1e-9
# The default run replays the same derandomised examples (a failure must reproduce on the next box).  Exploration runs:
# SFM_HYPOTHESIS_RANDOM=1 draws fresh examples, SFM_HYPOTHESIS_EXAMPLES=<n> sets how many of them per test
# (tools/gpu_explore.sh; SFM_TRACE_EXAMPLES keeps what was drawn).
_RANDOM = os.environ.get("SFM_HYPOTHESIS_RANDOM", "") not in ("", "0")
_EXAMPLES = int(os.environ.get("SFM_HYPOTHESIS_EXAMPLES", "0"))
SETTINGS = dict(max_examples=_EXAMPLES or 120, deadline=None, database=None, derandomize=not _RANDOM,
                suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])


def trace(*what):
    """SFM_TRACE_EXAMPLES=<file>: append every generated example before it runs (a GPU fault leaves no Python
    traceback of the example that caused it)."""
    import os
    f = os.environ.get("SFM_TRACE_EXAMPLES")
    if f:
        with open(f, "a") as fh:
            fh.write(repr(what) + "\n")


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


scene_args = st.tuples(st.integers(2, 64), st.integers(1, 400), st.sampled_from([0.25, 0.5, 0.8, 1.0]), st.integers(0, 10_000))


@settings(**SETTINGS)
@given(args=scene_args, lam=st.sampled_from([0.5, 5.0, 50.0]), iters=st.integers(1, 4),
       mode=st.sampled_from(["auto", "pairs", "mfma", "rows"]), debug=st.sampled_from([0, 16, 64, 256, 512, 1024, 16384]))
def test_ba_random_scene_matches_oracle(hip, oracle, sfm, args, lam, iters, mode, debug):
    n_cams, n_pts, vis, seed = args
    trace("ba", args, lam, iters, mode, debug)
    sc = sfm.scenes.make_scene(n_cams, n_pts, vis, seed=seed)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    want_c, want_p = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, lam, iters)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_option(hip.OPT_SCHUR, {"auto": hip.SCHUR_AUTO, "pairs": hip.SCHUR_PAIRS, "mfma": hip.SCHUR_MFMA, "rows": hip.SCHUR_ROWS}[mode])
        prob.set_option(hip.OPT_DEBUG, debug)          # result-preserving code-path switches only (include/sfm_hip.h)
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.iterate(lam, iters)
        cams, pts = prob.get_state()
        cost = prob.get_stats()
    assert rel(cams, want_c) < TOL and rel(pts, want_p) < TOL
    assert cost.shape == (iters,) and np.all(np.isfinite(cost)) and np.all(cost > 0)
    # quaternions stay unit (ba:388-392)
    assert np.max(np.abs(np.linalg.norm(cams[:, 3:7], axis=1) - 1.0)) < 1e-14


@settings(**{**SETTINGS, "max_examples": _EXAMPLES or 40})
@given(args=scene_args, split=st.floats(0.2, 0.8))
def test_ba_append_order_does_not_change_the_result(hip, sfm, args, split):
    """The same scene built in one piece and grown by an append (new points with their observations) iterates to the
    same state: the merged CSR equals the one-piece CSR."""
    n_cams, n_pts, vis, seed = args
    sc = sfm.scenes.make_scene(n_cams, n_pts, vis, seed=seed)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    n0 = max(1, min(n_pts - 1, int(split * n_pts)))
    m0 = int(sc.pt_ptr[n0])
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as whole:
        whole.set_state(sc.cams_init, sc.pts_init)
        whole.iterate(5.0, 2)
        want = whole.get_state()
    with hip.BaProblem(sc.n_cams, sc.pt_ptr[:n0 + 1], sc.cam_idx[:m0], uvn[:, :m0]) as grown:
        grown.set_state(sc.cams_init, sc.pts_init[:, :n0])
        grown.append(np.zeros((0, 7)), sc.pts_init[:, n0:], sc.cam_idx[m0:], sc.pt_idx[m0:], uvn[:, m0:])
        grown.iterate(5.0, 2)
        got = grown.get_state()
    assert rel(got[0], want[0]) < 1e-12 and rel(got[1], want[1]) < 1e-12


def _projections(sfm, sc, cams):
    projs = []
    for c in range(sc.n_cams):
        rot = sfm.geometry.quaternion_to_rotation(cams[c, 3:7])
        loc = cams[c, 0:3].reshape(3, 1)
        projs.append(sc.intrinsic @ np.hstack((rot.T, rot.T @ -loc)))
    return projs


@settings(**{**SETTINGS, "max_examples": (_EXAMPLES // 4) or 30})
@given(n_views=st.integers(2, 9), n_pts=st.integers(1, 700), seed=st.integers(0, 10_000), iters=st.integers(0, 25),
       lam=st.sampled_from([0.1, 0.5, 5.0]))
def test_nonlinear_triangulation_random_matches_oracle(hip, oracle, sfm, n_views, n_pts, seed, iters, lam):
    """tri:160-234 on random view counts / point counts / damping / iteration counts (0 iterations = identity)."""
    sc = sfm.scenes.make_scene(n_views, n_pts, 1.0, seed=seed)
    projs = _projections(sfm, sc, sc.cams_true)
    uv = [sc.uv_pix[:, sc.cam_idx == c] for c in range(n_views)]
    init = np.vstack((sc.pts_init, np.ones((1, sc.n_pts))))
    got = hip.tri_nonlinear(np.stack(projs), np.stack(uv), init, lam, iters)
    if iters == 0:
        assert np.array_equal(got, init)
        return
    want = oracle.nonlinear_triangulate_vec(init, projs, uv, lam, iters)
    assert rel(got, want) < TOL


@settings(**{**SETTINGS, "max_examples": (_EXAMPLES // 4) or 30})
@given(n_pts=st.integers(6, 500), seed=st.integers(0, 10_000), iters=st.integers(1, 30), quirks=st.sampled_from([0, 1, 2, 3]))
def test_nonlinear_pnp_random_matches_oracle(hip, oracle, sfm, n_pts, seed, iters, quirks):
    """campose:308-459 on random point counts / iteration counts / quirk flags: one view of a two-view scene, started
    from its perturbed pose."""
    sc = sfm.scenes.make_scene(2, n_pts, 1.0, seed=seed)
    sel = sc.cam_idx == 1
    ones = np.ones((1, int(sel.sum())))
    uv, x = np.vstack((sc.uv_pix[:, sel], ones)), np.vstack((sc.pts_true[:, sc.pt_idx[sel]], ones))      # homogeneous, as the reference passes them
    rot0 = sfm.geometry.quaternion_to_rotation(sc.cams_init[1, 3:7])
    loc0 = sc.cams_init[1, 0:3].reshape(3, 1)
    r, c = hip.pnp_nonlinear(uv, x, sc.intrinsic, rot0, loc0, 5, iters, quirks)
    ro, co = oracle.nonlinear_pnp(uv, x, sc.intrinsic, rot0, loc0, 5, iters, quirks)
    assert rel(r, ro) < TOL and rel(c, co) < TOL


@settings(**{**SETTINGS, "max_examples": (_EXAMPLES // 4) or 30})
@given(args=scene_args, iters=st.integers(2, 5), mode=st.sampled_from(["auto", "pairs", "mfma"]))
def test_ba_deterministic_graph_and_eager_agree_bitwise(hip, sfm, args, iters, mode):
    """SFM_OPT_DETERMINISTIC: two runs, and a hipGraph replay of the same run, give identical bits on random scenes."""
    n_cams, n_pts, vis, seed = args
    trace("det", args, iters, mode)
    sc = sfm.scenes.make_scene(n_cams, n_pts, vis, seed=seed)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    out = []
    for graph in (0, 0, 1):
        with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
            prob.set_option(hip.OPT_SCHUR, {"auto": hip.SCHUR_AUTO, "pairs": hip.SCHUR_PAIRS, "mfma": hip.SCHUR_MFMA}[mode])
            prob.set_option(hip.OPT_DETERMINISTIC, 1)
            prob.set_option(hip.OPT_GRAPH, graph)
            prob.set_state(sc.cams_init, sc.pts_init)
            prob.iterate(5.0, iters)
            out.append(prob.get_state())
    for cams, pts in out[1:]:
        assert np.array_equal(cams, out[0][0]) and np.array_equal(pts, out[0][1])


STRUCTURES = ("bernoulli", "tracks", "heavy", "clusters", "empty")


def structured_scene(sfm, n_cams, n_pts, structure, mean_track, seed):
    """A scene of one of STRUCTURES; settings a camera count cannot carry (clusters of fewer than two cameras, more empty
    cameras than leave two observed ones) fall back to the plain track structure."""
    St = sfm.scenes.Structure
    if structure == "bernoulli":
        return sfm.scenes.make_scene(n_cams, n_pts, min(1.0, mean_track / n_cams), seed=seed), St()
    st = St(mean_track=mean_track)
    if structure == "heavy":
        st = St(mean_track=mean_track, heavy=0.02)
    elif structure == "clusters" and n_cams >= 4:
        st = St(mean_track=mean_track, clusters=min(3, n_cams // 2))
    elif structure == "empty" and n_cams >= 5:
        st = St(mean_track=mean_track, empty=tuple(sorted({0, n_cams // 2, n_cams - 1})))
    return sfm.scenes.make_scene(n_cams, n_pts, seed=seed, structure=st), st


@settings(**{**SETTINGS, "max_examples": _EXAMPLES or 150})
@given(n_cams=st.integers(2, 240), n_pts=st.integers(20, 1500), structure=st.sampled_from(STRUCTURES),
       mean_track=st.sampled_from([2.0, 3.0, 4.0, 8.0]), seed=st.integers(0, 10_000), lam=st.sampled_from([0.5, 5.0]),
       iters=st.integers(1, 3), mode=st.sampled_from(["auto", "pairs", "mfma", "rows"]))
def test_ba_structured_scene_matches_oracle(hip, oracle, sfm, n_cams, n_pts, structure, mean_track, seed, lam, iters, mode):
    """Structured visibility (scenes.Structure: consecutive-view tracks, heavy tails, disjoint clusters, cameras without
    observations; Bernoulli at p = mean / V for comparison) over 2-240 cameras, the band test_ba_random_scene_matches_oracle
    does not reach: every threshold of the reduced solve and of ba_linearize's LDS modes.  150 examples; their scenes and
    oracle work took 9.5 s on a CPU host (8.1 s in oracle.ba_sparse)."""
    trace("structured", n_cams, n_pts, structure, mean_track, seed, lam, iters, mode)
    sc, stc = structured_scene(sfm, n_cams, n_pts, structure, mean_track, seed)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    want_c, want_p = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, lam, iters)
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_option(hip.OPT_SCHUR, {"auto": hip.SCHUR_AUTO, "pairs": hip.SCHUR_PAIRS, "mfma": hip.SCHUR_MFMA, "rows": hip.SCHUR_ROWS}[mode])
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.iterate(lam, iters)
        cams, pts = prob.get_state()
        pick = prob.info(hip.INFO_SCHUR_KERNEL)
    assert rel(cams, want_c) < TOL and rel(pts, want_p) < TOL, (structure, n_cams, mode, pick)
    for c in stc.empty:
        assert np.array_equal(cams[c, 0:3], sc.cams_init[c, 0:3])
        assert np.max(np.abs(cams[c, 3:7] - sc.cams_init[c, 3:7])) <= 1e-15
