"""CPU checks of the float64 two-view references of tests/_twoview_cases.py (oracle.fund_eight_point,
essential_from_fundamental, pose_candidates) against a 50-digit mpmath SVD.

The GPU tests of tests/test_gpu_two_view_paths.py hold the kernels to err <= C u (condition numbers) against these
float64 references.  Here the float64 references themselves meet the same bound against the exact answer, so the
bound is one that any backward-stable float64 implementation meets, not one fitted to the kernel's errors."""
import mpmath
import numpy as np
import pytest

import _twoview_cases as tc

mp = mpmath.mp
DPS = 50


def _m(a):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(a)])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def _svd(a):
    """(U, S, V^T) of a square mp matrix, singular values descending."""
    return mp.svd_r(a)


@mp.workdps(DPS)
def mp_eight_point(pairs8):
    """Exact-to-50-digits epipolar:140-193: null vector of W (padded with a zero row, as the kernel does),
    rank-2 projection, / f2[2][2]."""
    w = np.vstack((tc.design_matrix(pairs8), np.zeros(9)))
    _, _, v = _svd(_m(w))
    f = mp.matrix(3, 3)
    for k in range(9):
        f[k // 3, k % 3] = v[8, k]
    u, s, v = _svd(f)
    f2 = u * mp.diag([s[0], s[1], 0]) * v
    return _np(f2 / f2[2, 2])


@mp.workdps(DPS)
def mp_essential(fund, kl, kr):
    e = _m(kr).T * _m(fund) * _m(kl)
    u, _, v = _svd(e)
    e = u * mp.diag([1, 1, 0]) * v
    return _np(e / e[2, 2])


@mp.workdps(DPS)
def mp_pose(esse):
    u, _, v = _svd(_m(esse))
    w = _m([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    r1, r2 = u * w * v, u * w.T * v
    r1 = r1 if mp.det(r1) > 0 else -r1
    r2 = r2 if mp.det(r2) > 0 else -r2
    return [_np(r1).T, _np(r2).T], np.array([float(u[i, 2]) for i in range(3)])


def test_eight_point_oracle_meets_the_bound():
    rng = np.random.default_rng(101)
    cases = tc.eight_point_cases(rng, 200, kinds=tuple(k for k in tc.KINDS if k != "repeat"))
    worst, checked, k_w_max, rho_max = 0.0, 0, 0.0, 0.0
    for c in cases:
        p8 = c["pairs"][c["sample"]]
        f_or, k_w, k_p, rho = tc.eight_point_ref(p8)
        bound = tc.eight_point_bound(k_w, k_p, rho)
        if not bound < 0.5:
            continue        # the first-order bound says nothing there
        err = tc.rel_err(f_or, mp_eight_point(p8))
        assert err <= bound, (c["kind"], c["param"], err, k_w, k_p, rho)
        worst = max(worst, err / (tc.U * k_w * k_p * rho))
        checked += 1
        k_w_max, rho_max = max(k_w_max, k_w), max(rho_max, rho)
    print("eight point: %d cases, max err/(u kW kP rho) = %.3g" % (checked, worst))
    assert checked >= 150 and k_w_max >= 1e6 and rho_max >= 1e3


def test_essential_oracle_meets_the_bound():
    rng = np.random.default_rng(102)
    worst, checked = 0.0, 0
    for e, _r, _t in tc.essential_cases(rng, 80):
        kl, kr = tc.random_intrinsic(rng), tc.random_intrinsic(rng)
        fund = tc.fund_from_essential(e + 1e-3 * np.max(np.abs(e)) * rng.normal(size=(3, 3)), kl, kr)
        e_or, mu, k_e, rho = tc.essential_ref(fund, kl, kr)
        bound = tc.C * tc.U * mu * k_e * rho
        err = tc.rel_err(e_or, mp_essential(fund, kl, kr))
        assert err <= bound, (err, mu, k_e, rho)
        worst = max(worst, err / (tc.U * mu * k_e * rho))
        checked += 1
    print("essential: %d cases, max err/(u mu kE rhoE) = %.3g" % (checked, worst))


def test_pose_oracle_meets_the_bound():
    rng = np.random.default_rng(103)
    cases = tc.essential_cases(rng, 80)
    for i, (e, _r, _t) in enumerate(cases):
        if i % 2:
            e = e + 1e-4 * np.max(np.abs(e)) * rng.normal(size=(3, 3))     # sigma0 != sigma1
        r_or, c_or, k_e = tc.pose_ref(e)
        r_mp, c_mp = mp_pose(e)
        assert tc.candidate_set_err(r_or, c_or, r_mp, c_mp) <= tc.C * tc.U * k_e, i


def test_pose_candidates_contain_the_true_pose():
    """The generator's E = [t]x R: R^T is one of the two candidate rotations, c = +-t/|t| up to the sign."""
    rng = np.random.default_rng(104)
    for e, rot, t in tc.essential_cases(rng, 40):
        (r1, r2), c1, _ = tc.pose_ref(e)
        assert min(np.max(np.abs(r1 - rot.T)), np.max(np.abs(r2 - rot.T))) < 1e-12
        tn = t / np.linalg.norm(t)
        assert min(np.max(np.abs(c1 - tn)), np.max(np.abs(c1 + tn))) < 1e-12


def test_generator_kinds():
    rng = np.random.default_rng(105)
    cases = tc.eight_point_cases(rng, 60)
    for c in cases:
        uniq = len(set(c["sample"].tolist()))
        assert uniq == (7 if c["kind"] == "repeat" else 8)
        if c["kind"] == "repeat":
            w = tc.design_matrix(c["pairs"][c["sample"]])
            assert np.linalg.matrix_rank(w) == 7
    es = tc.essential_cases(rng, 12)
    for axis in range(3):
        t = es[axis][2]
        assert np.count_nonzero(t) == 1 and t[axis] > 0
    small = [abs(e[2, 2]) / np.max(np.abs(e)) for e, _, _ in es[3::4]]
    assert all(0 < s < 1e-2 for s in small)
    sc = tc.two_view_scene(rng, 200, noise=0.5, outlier_frac=0.2)
    assert not np.allclose(sc["Kl"], sc["Kr"]) and sc["outliers"].size == 40
    z_r = (sc["R"] @ sc["X"] + sc["t"][:, None])[2]
    assert np.all(sc["X"][2] > 0) and np.all(z_r > 0)


@pytest.mark.parametrize("k", [-1000, -300, 0, 250, 900])
def test_oracle_pose_is_scale_free(k):
    """LAPACK scales internally: the float64 reference of the scale test gives the same candidates at 2^k E."""
    e = tc.essential_cases(np.random.default_rng(106), 5)[4][0]
    (r1, r2), c1, _ = tc.pose_ref(e)
    (s1, s2), d1, _ = tc.pose_ref(np.ldexp(e, k))
    assert tc.candidate_set_err([s1, s2], d1, [r1, r2], c1) < 1e-14
