"""The data-flow reduced solve with rows handed over through column i-2 (csrc/sfm_ba_flow.h): sfm_ba_iterate through the
data-flow launch against the column steps as separate launches (SFM_OPT_DEBUG bit 1024) and against the oracle, at the smallest
numbers of block columns where the hand-over level can go wrong, at full and at 60 % visibility, and at the largest size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9          # against the oracle, as test_ba_data_flow_solve_against_column_steps_and_oracle
TOL_PATHS = 1e-11   # between the two solve paths, as there

# cameras -> block columns: 2, 3 (no closer), 4 (first closer, only rows 1 / 2 of the chain before it), 5 (first closer that reads
# another closer's L[i-1][i-3] and finished block (i-1, i-2)), 6 (one row further), 52 (the largest table)
SHAPES = [(9, 300, 1.0), (9, 300, 0.6), (10, 300, 1.0), (10, 300, 0.6), (14, 400, 1.0), (14, 400, 0.6), (19, 400, 1.0), (19, 400, 0.6),
          (23, 400, 1.0), (23, 400, 0.6), (237, 600, 0.15)]


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


def _scene(sfm, n_cams, n_pts, vis):
    sc = sfm.scenes.make_scene(n_cams, n_pts, vis, seed=1300 + n_cams)
    return sc, sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)


def _iterate(hip, sc, uvn, dbg, want_path, deterministic=False):
    with hip.BaProblem(sc.n_cams, sc.pt_ptr, sc.cam_idx, uvn) as prob:
        prob.set_option(hip.OPT_DEBUG, dbg)
        if deterministic:
            prob.set_option(hip.OPT_DETERMINISTIC, 1)
        assert prob.info(hip.INFO_SOLVE_PATH) == want_path
        prob.set_state(sc.cams_init, sc.pts_init)
        prob.iterate(5.0, 3)
        return prob.get_state()


@pytest.mark.parametrize("n_cams,n_pts,vis", SHAPES)
def test_hand_over_through_column_i_minus_2_against_column_steps_and_oracle(hip, oracle, sfm, n_cams, n_pts, vis):
    sc, uvn = _scene(sfm, n_cams, n_pts, vis)
    assert (7 * n_cams + 31) // 32 == {9: 2, 10: 3, 14: 4, 19: 5, 23: 6, 237: 52}[n_cams]
    want_c, want_p = oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 5.0, 3)
    flow = _iterate(hip, sc, uvn, 0, hip.SOLVE_FLOW)
    steps = _iterate(hip, sc, uvn, 1024, hip.SOLVE_STEPS)
    for cams, pts in (flow, steps):
        print("vs oracle: cameras %.3e points %.3e" % (rel(cams, want_c), rel(pts, want_p)))
        assert rel(cams, want_c) < TOL and rel(pts, want_p) < TOL
    print("between the paths: cameras %.3e points %.3e" % (rel(flow[0], steps[0]), rel(flow[1], steps[1])))
    assert rel(flow[0], steps[0]) < TOL_PATHS and rel(flow[1], steps[1]) < TOL_PATHS


def test_two_runs_from_the_same_state_give_the_same_bits(hip, sfm):
    """19 cameras, 5 block columns: the closer of row 4 reads what the closer of row 3 delivered, whenever it arrives.  In
    deterministic mode, as test_ba_data_flow_solve_is_bitwise_repeatable: the kernels ahead of the solve keep a fixed order too."""
    sc, uvn = _scene(sfm, 19, 400, 0.6)
    a = _iterate(hip, sc, uvn, 0, hip.SOLVE_FLOW, deterministic=True)
    b = _iterate(hip, sc, uvn, 0, hip.SOLVE_FLOW, deterministic=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
