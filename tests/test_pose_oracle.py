"""CPU checks of the float64 references of tests/_pose_cases.py (the DLT null vector over its W, the six-point pose,
the reprojection values) against 50-digit mpmath arithmetic.

The GPU tests of tests/test_gpu_pose_paths.py hold the kernels to err <= C u (condition numbers) against these float64
references.  Here the references themselves meet the same bounds against the exact answer, so a bound is one that any
backward-stable float64 implementation meets, not one fitted to the kernels' errors.  The conditions on the generators
are checked here too, on the CPU: among the kinds that do not repeat an index at most 10 % of the cases may be left out
because their first-order bound is vacuous, and the largest condition product actually checked must reach 1e6."""
import mpmath
import numpy as np
import pytest

import _pose_cases as pc

mp = mpmath.mp
DPS = 50


def _m(a):
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(a)])


def _vec(m, n):
    return np.array([float(m[i]) for i in range(n)])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


@mp.workdps(DPS)
def mp_dlt(projs, uv):
    """One track: the exact design matrix of the float64 projections and keys, its last right singular vector / its W."""
    k = projs.shape[0]
    a = mp.matrix(2 * k, 4)
    for v in range(k):
        p = _m(projs[v])
        for r in range(2):
            key = mp.mpf(float(uv[v, r, 0]))
            for j in range(4):
                a[2 * v + r, j] = key * p[2, j] - p[r, j]
    _, _, vt = mp.svd_r(a)
    return np.array([float(vt[3, j] / vt[3, 3]) for j in range(4)])


@mp.workdps(DPS)
def mp_six_point(key6, x6, kmat):
    """(R, C) of the six-point solve with the device's sign convention, from the float64 inputs."""
    p = mp.inverse(_m(kmat)) * _m(key6)
    w = mp.matrix(12, 12)
    for i in range(6):
        xh = [mp.mpf(float(x6[0, i])), mp.mpf(float(x6[1, i])), mp.mpf(float(x6[2, i])), mp.mpf(1)]
        for c in range(4):
            w[2 * i, c] = p[2, i] * xh[c]
            w[2 * i, 8 + c] = -p[0, i] * xh[c]
            w[2 * i + 1, 4 + c] = p[2, i] * xh[c]
            w[2 * i + 1, 8 + c] = -p[1, i] * xh[c]
    _, _, vt = mp.svd_r(w)
    m = mp.matrix(3, 3)
    m4 = mp.matrix(3, 1)
    for i in range(3):
        for j in range(3):
            m[i, j] = vt[11, 4 * i + j]
        m4[i] = vt[11, 4 * i + 3]
    uu, ss, vv = mp.svd_r(m)
    rot = (uu * vv).T
    loc = rot * (-m4) / ss[0]
    if mp.det(rot) < 0:
        rot = -rot
    return _np(rot), _vec(loc, 3)


def test_dlt_oracle_meets_the_bound():
    cases = pc.dlt_cases(np.random.default_rng(301), 210)
    worst = {}
    left_out, cond_max = 0, 0.0
    for c in cases:
        x, info = pc.dlt_ref(c["projs"], c["uv"])
        bound, cond = float(info["bound"][0]), float(info["kappa"][0] * info["rho"][0])
        if not bound < 0.5:
            left_out += 1
            continue
        err = pc.rel_err(x[:, 0], mp_dlt(c["projs"], c["uv"]))
        assert err <= bound, (c["kind"], c["k"], c["param"], err, bound)
        worst[c["kind"]] = max(worst.get(c["kind"], 0.0), err / (pc.U * cond))
        cond_max = max(cond_max, cond)
    print("DLT: %d cases, %.1f %% left out, largest kappa rho checked %.3g" % (len(cases), 100.0 * left_out / len(cases), cond_max))
    print("DLT: max err/(u kappa rho) per kind: " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    assert left_out <= 0.10 * len(cases) and cond_max >= 1e6
    assert set(worst) == set(pc.DLT_KINDS)


def test_six_point_oracle_meets_the_bound():
    rng = np.random.default_rng(302)
    kmat = pc.random_intrinsic(rng)
    kinds = tuple(k for k in pc.SIX_KINDS if k != "repeat")
    cases = pc.six_point_cases(rng, 150, kmat, kinds=kinds)
    worst_r, worst_c = {}, {}
    left_out, cond_max = 0, 0.0
    for c in cases:
        rot, loc, info = pc.six_point_ref(c["key"], c["X"], kmat)
        if not pc.six_point_checkable(info):
            left_out += 1
            continue
        r_mp, c_mp = mp_six_point(c["key"], c["X"], kmat)
        e_r, e_c = pc.rel_err(rot, r_mp), pc.rel_err(loc, c_mp)
        assert e_r <= info["bound_r"] and e_c <= info["bound_c"], (c["kind"], c["param"], e_r, e_c, info["bound_r"], info["bound_c"])
        worst_r[c["kind"]] = max(worst_r.get(c["kind"], 0.0), e_r / (pc.U * info["cond_r"]))
        worst_c[c["kind"]] = max(worst_c.get(c["kind"], 0.0), e_c / (pc.U * info["cond_c"]))
        cond_max = max(cond_max, info["cond_r"])
    print("six point: %d cases, %.1f %% left out, largest kW kP / s0(M) checked %.3g"
          % (len(cases), 100.0 * left_out / len(cases), cond_max))
    print("six point: max err/(u cond) per kind, rotation: " + ", ".join("%s %.3g" % kv for kv in sorted(worst_r.items())))
    print("six point: max err/(u cond) per kind, centre:   " + ", ".join("%s %.3g" % kv for kv in sorted(worst_c.items())))
    assert left_out <= 0.10 * len(cases) and cond_max >= 1e6
    assert set(worst_r) == set(kinds)


def test_six_point_reference_recovers_the_pose():
    """Noise-free cases: the reference returns the generator's (R, C) to its own bound (up to the point-set's conditioning)."""
    rng = np.random.default_rng(303)
    kmat = pc.random_intrinsic(rng)
    for c in pc.six_point_cases(rng, 40, kmat, kinds=("scene", "homog", "faraway")):
        rot, loc, info = pc.six_point_ref(c["key"], c["X"], kmat)
        if pc.six_point_checkable(info):
            # the generated keys are themselves rounded (relative u mu): the same first-order bound applies
            assert pc.rel_err(rot, c["R"]) <= info["bound_r"] and pc.rel_err(loc, c["C"]) <= info["bound_c"], c["kind"]


def test_generator_kinds():
    rng = np.random.default_rng(304)
    for c in pc.dlt_cases(rng, 84):
        a, _ = pc.dlt_design(c["projs"], c["uv"])
        assert a.shape == (1, 2 * c["k"], 4) and np.linalg.matrix_rank(a[0], tol=1e-13 * np.linalg.norm(a[0])) >= 3
        if c["kind"] == "dupview":
            i, j = c["param"]
            assert c["k"] >= 3 and np.array_equal(c["projs"][i], c["projs"][j]) and np.array_equal(c["uv"][i], c["uv"][j])
        if c["kind"] == "scaled":
            assert pc.SCALED_RANGE[0] <= c["param"] <= pc.SCALED_RANGE[1]
    assert {c["k"] for c in pc.dlt_cases(rng, 84)} == set(pc.DLT_VIEWS)
    kmat = pc.random_intrinsic(rng)
    for c in pc.six_point_cases(rng, 70, kmat):
        assert len(set(c["sample"].tolist())) == (5 if c["kind"] == "repeat" else 6)
        depth = (c["R"].T @ (c["X"][0:3] - c["C"][:, None]))[2]
        assert np.all(depth > 0)
        if c["kind"] == "homog":
            assert np.all(c["key"][2] != 1.0)
        if c["kind"] == "repeat":
            _, _, info = pc.six_point_ref(c["key"][:, c["sample"]], c["X"][:, c["sample"]], kmat)
            assert np.linalg.matrix_rank(info["W"]) <= 10


@pytest.mark.parametrize("kind", ["twin", "parallel", "twin_parallel"])
def test_planted_rank_deficient_tracks(kind):
    """What the GPU tests rely on: ``twin`` has rank 2; the W = 0 plants have an exactly zero third column, the
    reference's own division by W is then by an exact zero and its result is not finite."""
    d = pc.dlt_rank2(kind)
    a, _ = pc.dlt_design(d["projs"], d["uv"])
    assert np.linalg.matrix_rank(a[0]) == (3 if kind == "parallel" else 2)
    if d["w_zero"]:
        assert np.all(a[:, :, 2] == 0.0)
        x, info = pc.dlt_ref(d["projs"], d["uv"])
        if kind == "parallel":
            assert np.all(np.abs(info["v"][:, 2]) == 1.0) and not np.any(np.isfinite(x[2]))


def test_reprojection_bound_holds_for_the_float64_value():
    """The float64 value of reprojection_values against the same expression at 50 digits."""
    rng = np.random.default_rng(305)
    kmat = pc.random_intrinsic(rng)
    sc = pc.pnp_scene(rng, 60, kmat, noise=0.5, outlier_frac=0.2)
    proj, mag = pc.pose_projection(kmat, sc["R"], sc["C"])
    val, bound = pc.reprojection_values(proj, mag, sc["uv"], sc["X"])
    with mp.workdps(DPS):
        rt = mp.matrix(3, 4)
        r, cc = _m(sc["R"]), _m(sc["C"].reshape(3, 1))
        t = r.T * (-cc)
        for i in range(3):
            for j in range(3):
                rt[i, j] = r[j, i]
            rt[i, 3] = t[i]
        p = _m(kmat) * rt
        for i in range(60):
            s = p * _m(sc["X"][:, i:i + 1])
            e = [mp.mpf(float(sc["uv"][r_, i])) - s[r_] / s[2] for r_ in range(3)]
            exact = float(mp.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2))
            assert abs(val[i] - exact) <= bound[i], (i, val[i], exact, bound[i])
    assert np.all(bound < 1e-9)


@pytest.mark.parametrize("lam", [0.5, 1e-6, 0.0])
def test_tri_step_in_float64_meets_the_bound(lam):
    """The step of _pose_cases.tri_step in float64 against the same step in numpy.longdouble, from the float64 DLT result
    of the narrow / far / noisy geometry, as the GPU test runs it.  With damping the bound is C u (kappa |delta| + |x|); at
    lam = 0 that form is missed by this plain float64 evaluation on far points (printed), which is why the GPU test adds the
    rounding of the residuals there (tri_step_bound)."""
    rng = np.random.default_rng(306)
    worst_short = worst = 0.0
    total = left_out = 0
    for kind in ("narrow", "far", "noisy"):
        for k in (2, 3, 5):
            sc = pc.dlt_scene(rng, k, kind, 100)
            uv = sc["uv"] + 1e-4 * rng.normal(size=sc["uv"].shape)
            x0, _ = pc.dlt_ref(sc["projs"], uv)
            want, delta, a, beta = pc.tri_step(sc["projs"], uv, x0, lam)
            got = pc.tri_step(sc["projs"], uv, x0, lam, np.float64)[0]
            short, kappa = pc.tri_step_bound(x0, delta, a)
            bound, _ = pc.tri_step_bound(x0, delta, a, beta if lam == 0.0 else None)
            ok = pc.C * pc.U * kappa < 0.5
            err = np.linalg.norm((got - want)[0:3].astype(np.float64), axis=0)
            assert np.all(err[ok] <= bound[ok]), (kind, k, float(np.max(err[ok] / bound[ok])))
            worst, worst_short = max(worst, float(np.max(err[ok] / bound[ok]))), max(worst_short, float(np.max(err[ok] / short[ok])))
            total, left_out = total + ok.size, left_out + int((~ok).sum())
    print("lam = %g: %.1f %% left out, max err/bound %.3g (%.3g against the form without the residual term)"
          % (lam, 100.0 * left_out / total, worst, worst_short))
    if lam == 0.5:
        assert left_out <= 0.10 * total


@pytest.mark.parametrize("lam", [0.5, 1e-6, 0.0])
def test_pnp_step_reference_is_the_oracles_step(lam):
    """The longdouble PnP step of _pose_cases.pnp_step is the float64 oracle's first iteration (quirks Q1 and Q2 included):
    the two agree within the bound the GPU test holds the kernel to, and so does the same step taken in float64."""
    import sfm_oracle as oracle
    rng = np.random.default_rng(307)
    kmat = pc.random_intrinsic(rng)
    left_out = 0
    for name, uv, x, rot0, loc0 in pc.pnp_step_scenes(rng, kmat):
        if name == "split":
            continue                                   # the same arithmetic, only more of it
        rot, loc, delta, a, par = pc.pnp_step(uv, x, kmat, rot0, loc0, lam)
        bound, kappa = pc.pnp_step_bound(par, delta, a)
        if not pc.C * pc.U * kappa < 0.5:
            left_out += 1
            continue
        r_or, c_or = oracle.nonlinear_pnp(uv, x, kmat, rot0, loc0.reshape(3, 1), lam, 1)
        r_64, c_64 = pc.pnp_step(uv, x, kmat, rot0, loc0, lam, np.float64)[0:2]
        for r, c in ((r_or, c_or.ravel()), (r_64, c_64)):
            assert np.linalg.norm(c - loc.astype(np.float64)) <= bound, (name, lam)
            assert np.max(np.abs(r - rot.astype(np.float64))) <= 4 * bound, (name, lam)
    assert left_out == 0


def test_gap_threshold():
    val = np.array([0.1, 0.5, 0.5000001, 2.0, np.nan, np.inf])
    bound = np.array([1e-3, 1e-9, 1e-9, 0.3, 0.0, 0.0])
    t = pc.gap_threshold(val, bound, 0.5)
    assert t is not None and np.all(np.abs(val[:4] - t) > 2 * bound[:4]) and 0.5 < t < 0.5000001
    assert pc.gap_threshold(np.array([1.0, 1.0]), np.array([0.1, 0.1]), 1.0) is None
