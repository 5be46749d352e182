"""Covariance of the resident scene, host side: the two NumPy routes of tests/_cov_reference.py against each other, the
closed-form cases, the degeneracy that makes the camera mask necessary, the sigma0 formula, and the C-ABI surface."""
import os
import re

import numpy as np
import pytest

import _cov_reference as cr
import _robust_reference as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", cr.SCENES)
def test_route_a_against_route_b(sfm, oracle, name):
    """The reference's own float64 error, per scene and setting: what the GPU test's tolerance is derived from
    (``cr.tolerance``).  Bound here: cond(H) eps is the forward error an inverse may carry; with the smallest
    eigenvalue of S_ff at 1e-5 .. 1e-4 (lambda = 0) or lambda (a free gauge) and entries of H up to ~1e4, cond(H) stays
    below 1e11, so the two routes must agree to 1e11 x 2.2e-16 ~ 2e-5 relative at the very worst; they are asserted to
    1e-6, and printed."""
    sc, uvn, cams, pts, scale = cr.scene(sfm, oracle, name)
    for quirks in (oracle.QUIRKS_REFERENCE, 0):
        for kind, delta in ((rr.LOSS_NONE, 1.0), (rr.LOSS_HUBER, 5.0 / scale)):
            for lam, held in cr.settings(name):
                (cam_ab, pt_ab, s_ab), _a = cr.ab_disagreement((name, quirks, kind, lam, held), cams, pts, sc.cam_idx, sc.pt_idx, uvn,
                                                               lam, cr.free_mask(sc.n_cams, held), kind, delta, quirks)
                print(name, "quirks", quirks, "loss", kind, "lambda", lam, "held", held, "cameras %.2e points %.2e" % (cam_ab, pt_ab))
                assert cam_ab < 1e-6 and pt_ab < 1e-6 and s_ab < 1e-12


def test_single_observations_undamped_is_the_limit(sfm, oracle):
    """lambda = 0 on the scene with single observations: the reference is the scene without those points
    (``cr.without_single_points``).  That this is the limit lambda -> 0 of the FULL scene is checked here: route A of the
    full scene converges to it linearly in lambda on the camera blocks and on the blocks of the other points (a single
    point's share of S is Jp^T (I - Jx (Jx^T Jx + lambda I)^-1 Jx^T) Jp = O(lambda / |Jx|^2); measured 9.5e-4 at 1e-9,
    9.5e-5 at 1e-10, 9.6e-6 at 1e-11), while keeping the single observations in U (their points as constants) changes the
    camera blocks by a quarter."""
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "single")
    mask = cr.free_mask(sc.n_cams, (0, 1))
    r_cam, r_pt, r_uv, _r_pts, kept = cr.without_single_points(sc.pt_ptr, sc.cam_idx, sc.pt_idx, uvn, pts)
    for quirks in (oracle.QUIRKS_REFERENCE, 0):
        (cam_ab, pt_ab), cam_cov, pt_cov, _s0, single = cr.single_undamped(sfm, oracle, quirks, rr.LOSS_NONE, 1.0, (0, 1))
        assert 10 < single.sum() < sc.n_pts and cam_ab < 1e-6 and pt_ab < 1e-6
        dist = {}
        for lam in (1e-9, 1e-10, 1e-11):
            near = cr.route_a(cams, pts, sc.cam_idx, sc.pt_idx, uvn, lam, mask, quirks=quirks)
            dist[lam] = max(cr.block_rel(near[0], cam_cov), cr.block_rel(near[1][~single], pt_cov[~single]))
        # the wrong limit: the single observations' Jp^T Jp kept in U
        s_wrong = oracle.ba_reduced_system(cams, pts[:, kept], r_cam, r_pt, r_uv, 0.0, quirks)["S"].copy()
        jp = oracle.obs_terms_vec(cams, pts, sc.cam_idx, sc.pt_idx, uvn, quirks)[1]
        for o in np.flatnonzero(single[sc.pt_idx]):
            c = sc.cam_idx[o]
            s_wrong[7 * c:7 * c + 7, 7 * c:7 * c + 7] += jp[o].T @ jp[o]
        wrong = np.linalg.inv(s_wrong[14:, 14:])
        d_wrong = cr.block_rel(np.stack([wrong[7 * k:7 * k + 7, 7 * k:7 * k + 7] for k in range(sc.n_cams - 2)]), cam_cov[2:])
        print(quirks, "full scene against the reduced one:", dist, "singles kept in U: %.2e" % d_wrong)
        assert dist[1e-11] < 1e-4 and 5 < dist[1e-9] / dist[1e-10] < 20 and 5 < dist[1e-10] / dist[1e-11] < 20
        assert d_wrong > 1e-2


def test_newton_step_confirms_route_b(sfm, oracle):
    """One Newton step in longdouble moves route B by no more than its distance from route A: neither route is off by more
    than the disagreement the tolerance is built on."""
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "6x300")
    mask = cr.free_mask(sc.n_cams, (0, 1))
    a = cr.route_a(cams, pts, sc.cam_idx, sc.pt_idx, uvn, 0.0, mask)
    b0 = cr.route_b(cams, pts, sc.cam_idx, sc.pt_idx, uvn, 0.0, mask, newton=False)
    b1 = cr.route_b(cams, pts, sc.cam_idx, sc.pt_idx, uvn, 0.0, mask, newton=True)
    print([cr.block_rel(x[0], y[0]) for x, y in ((a, b0), (a, b1), (b0, b1))], [cr.block_rel(x[1], y[1]) for x, y in ((a, b0), (a, b1), (b0, b1))])
    assert cr.block_rel(a[0], b1[0]) < 1e-9 and cr.block_rel(a[1], b1[1]) < 1e-9
    assert cr.block_rel(b0[0], b1[0]) < 1e-9 and cr.block_rel(b0[1], b1[1]) < 1e-9


def test_all_held_is_d_inverse_and_held_blocks_are_zero(sfm, oracle):
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "6x300")
    for lam in (0.0, 1e-3):
        cam_cov, pt_cov, _s0, t, _sigma = cr.route_a(cams, pts, sc.cam_idx, sc.pt_idx, uvn, lam, np.zeros(sc.n_cams, dtype=np.uint8),
                                                      want_parts=True)
        assert not cam_cov.any()
        assert np.array_equal(pt_cov, t["D_inv"][:, cr.PACK[0], cr.PACK[1]])
        cam_cov, pt_cov, _s0, t, _sigma = cr.route_a(cams, pts, sc.cam_idx, sc.pt_idx, uvn, lam, cr.free_mask(sc.n_cams, (0, 1)),
                                                      want_parts=True)
        assert not cam_cov[0:2].any() and all(cam_cov[c].any() for c in range(2, sc.n_cams))
        # a point seen by held cameras only gets exactly D^-1; every other point gains a positive semi-definite term
        seen_by = [set(sc.cam_idx[sc.pt_ptr[p]:sc.pt_ptr[p + 1]]) for p in range(sc.n_pts)]
        only_held = np.array([s <= {0, 1} for s in seen_by])
        dinv = t["D_inv"][:, cr.PACK[0], cr.PACK[1]]
        assert np.array_equal(pt_cov[only_held], dinv[only_held])
        gain = pt_cov[~only_held] - dinv[~only_held]
        assert np.all(gain[:, [0, 3, 5]] > 0)


def test_undamped_gauge_is_why_cameras_are_held(sfm, oracle):
    """With nothing held the smallest eigenvalue of S is lambda itself (the gauge): the 'covariance' of such a system is
    1 / lambda along those directions, whatever the data says."""
    sc, uvn, cams, pts, _scale = cr.scene(sfm, oracle, "6x300")
    for lam in (0.1, 1e-3):
        s = oracle.ba_reduced_system(cams, pts, sc.cam_idx, sc.pt_idx, uvn, lam)["S"]
        w = np.linalg.eigvalsh(0.5 * (s + s.T))
        print(lam, w[:9])
        assert abs(w[0] - lam) < 1e-6 * lam                # a null direction of J^T J: the 1 / lambda it gives says nothing about the data


def test_sigma0_formula(sfm, oracle):
    sc, uvn, cams, pts, scale = cr.scene(sfm, oracle, "single")
    n_observed = int(np.count_nonzero(np.diff(sc.pt_ptr)))
    for kind, delta in ((rr.LOSS_NONE, 1.0), (rr.LOSS_HUBER, 5.0 / scale)):
        cost = rr.state_cost(cams, pts, sc.cam_idx, sc.pt_idx, uvn, kind, delta)
        for held in ((0, 1), (0,), ()):
            got = cr.route_a(cams, pts, sc.cam_idx, sc.pt_idx, uvn, 1e-3, cr.free_mask(sc.n_cams, held), kind, delta)[2]
            want = cost / (2 * sc.n_obs - 7 * (sc.n_cams - len(held)) - 3 * n_observed)
            assert abs(got - want) <= 1e-15 * want
    assert cr.sigma0_sq(3.0, 5, 1, 1) == 0.0 and cr.sigma0_sq(3.0, 6, 1, 1) == 3.0 / 2


def test_abi_surface(sfm):
    n = sfm.native
    header = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    for name in ("sfm_ba_covariance", "sfm_ba_covariance_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header) and name in n.EXPORTS
    assert len(n.SIGNATURES["sfm_ba_covariance"]) == 11 and len(n.SIGNATURES["sfm_ba_covariance_plan"]) == 5
    for const, value in (("SFM_E_SINGULAR", n.E_SINGULAR), ("SFM_COV_CAM_HELD", n.COV_CAM_HELD), ("SFM_COV_CAM_PIVOT", n.COV_CAM_PIVOT),
                         ("SFM_COV_PT_EMPTY", n.COV_PT_EMPTY), ("SFM_COV_PT_SINGULAR", n.COV_PT_SINGULAR)):
        m = re.search(r"#define\s+%s\s+(-?\d+)" % const, header)
        assert m and int(m.group(1)) == value, const
    assert n.COV_CAM_HELD == n.CAM_HELD and n.COV_PT_EMPTY == n.PT_EMPTY
    assert hasattr(n.BaProblem, "covariance") and hasattr(sfm.processors.HipBaMixin, "structure_uncertainty")
    assert np.array_equal(n.sym3(np.arange(6.0)[None])[0], [[0, 1, 2], [1, 3, 4], [2, 4, 5]])


def test_plan_and_argument_checks_need_no_device(sfm):
    """The plan is host arithmetic; a bad handle and bad plan arguments are refused before anything touches a device."""
    n = sfm.native
    lib = n.load()
    block, blocks, launches, group_max = n.covariance_plan(6)
    assert block == 64 and blocks == 1 and launches == 3 and group_max == 64
    for v in (9, 10, 18, 19, 37, 238):
        b = n.covariance_plan(v)
        assert b[1] == -(-7 * v // block) and b[2] == 4 * b[1] - 1
    assert n.covariance_plan(9)[1] == 1 and n.covariance_plan(10)[1] == 2 and n.covariance_plan(18)[1] == 2 and n.covariance_plan(19)[1] == 3
    with pytest.raises(ValueError):
        n.covariance_plan(0)
    assert lib.sfm_ba_covariance(None, 0.0, 3, 0, None, 0, None, None, None, None, None) == n.E_HANDLE
