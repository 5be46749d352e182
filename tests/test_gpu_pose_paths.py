"""The linear pose stage (csrc/sfm_core.hip, csrc/sfm_dlt.h, csrc/sfm_common.h) against the float64 references of
tests/_pose_cases.py, under bounds derived from condition numbers (u = 2^-53, C = 64; tests/test_pose_oracle.py shows the
float64 references meet the same bounds against 50-digit arithmetic):

* DLT, rectangular (tri_linear): one launch of 300 points per (k, kind), k in {2, 3, 4, 5, 9, 33}, seven kinds, every
  point within C u sqrt(2k) max(s0, mu) / (s2 - s3) rho; m across the 256-thread block edge; k across the 512-view LDS
  staging edge; W == 1.0 exactly; planted rank-deficient tracks by property; a NaN key poisons only its own point;
  power-of-two scalings of the design give equal bits while every intermediate stays normal;
* DLT, ragged (tri_tracks, linear mode): the same cases as tracks of mixed length in one call, within the same bounds;
  bit-equal to the rectangular kernel on rectangular tracks; SFM_TRACK_NONFINITE exactly on the planted W = 0 tracks
  and SFM_TRACK_TOO_FEW on lengths 0 and 1, the input point kept;
* six point (pnp_six_point_hypotheses): 2 100 hypotheses of seven kinds in one launch, rotation and centre within their
  per-hypothesis bounds; samples that repeat an index by property; the reference's own 300-hypothesis fixture within
  min(1e-7, bound) per hypothesis;
* scoring (pnp_inlier_mask, pnp_ransac_evaluate, pnp_linear_ransac): the threshold in a gap of the float64 values wider
  than twice their propagated rounding bounds (exact masks, counts and winner) and on a value (mask sum == count), n
  across the 256-thread edges, n_hyp in {1, 7, 300}, planted s2 = +-0 / NaN / inf * 0 points, a point behind the
  camera, a tie at the maximum, a threshold that nothing passes; values crowding the threshold through both the mask
  and the scoring kernel;
* one step of tri_nonlinear (NV = 2, 3, 4 and the generic path) from the DLT result of the narrow / far geometry and
  one step of pnp_nonlinear (its three size classes) from the six-point result, against numpy.longdouble steps.
"""
import numpy as np
import pytest

import _pose_cases as pc
from conftest import load_golden

pytestmark = pytest.mark.gpu

U, C = pc.U, pc.C
NARROW_E = (0.0, 1.0, 2.0, 3.0, 4.5, 6.0)          # one per entry of DLT_VIEWS
SCALED_J = (-400, -300, -200, -100, 100, 200)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------------------ DLT, rectangular
def _rect_scenes():
    """The (k, kind) launches: fixed scene, 300 points each."""
    rng = np.random.default_rng(401)
    out = []
    for kind in pc.DLT_KINDS:
        for i, k in enumerate(pc.DLT_VIEWS):
            param = NARROW_E[i] if kind == "narrow" else (SCALED_J[i] if kind == "scaled" else None)
            out.append(pc.dlt_scene(rng, max(k, 3) if kind == "dupview" else k, kind, 300, param))
    return out


@pytest.fixture(scope="module")
def rect_sweep(hip):
    scenes = _rect_scenes()
    return [(sc, hip.tri_linear(sc["projs"], sc["uv"]), pc.dlt_ref(sc["projs"], sc["uv"])) for sc in scenes]


def _tally(worst, kind, err, info, ok):
    cond = info["kappa"][ok] * info["rho"][ok]
    if ok.any():
        worst[kind] = max(worst.get(kind, 0.0), float(np.max(err[ok] / (U * cond))))
    return float(np.max(cond)) if ok.any() else 0.0


def test_tri_linear_every_kind_within_bound(rect_sweep):
    worst, total, left_out, cond_max = {}, 0, 0, 0.0
    for sc, got, (want, info) in rect_sweep:
        ok = info["bound"] < 0.5
        err = pc.rel_err_cols(got, want)
        bad = ok & ~(err <= info["bound"])
        assert not bad.any(), (sc["kind"], sc["k"], sc["param"], int(np.argmax(bad)), float(err[bad].max()),
                               float(info["bound"][bad].min()))
        assert np.all(got[3] == 1.0), (sc["kind"], sc["k"])
        cond_max = max(cond_max, _tally(worst, sc["kind"], err, info, ok))
        total, left_out = total + ok.size, left_out + int((~ok).sum())
    print("tri_linear: %d points, %.1f %% left out, largest kappa rho checked %.3g" % (total, 100.0 * left_out / total, cond_max))
    print("tri_linear: max err/(u kappa rho) per kind: " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    assert left_out <= 0.10 * total and cond_max >= 1e6 and set(worst) == set(pc.DLT_KINDS)
    assert max(worst.values()) < C


def test_tri_linear_power_of_two_scaling_keeps_the_bits(hip, rect_sweep):
    """|j| <= 200 keeps every intermediate of the QR and the Jacobi sweeps normal: 2^j commutes with every rounding."""
    seen = 0
    for sc, got, _ in rect_sweep:
        if sc["kind"] == "scaled" and abs(sc["param"]) <= 200:
            assert same_bits(got, hip.tri_linear(np.ldexp(sc["projs"], -sc["param"]), sc["uv"])), sc["param"]
            seen += 1
    assert seen == 4


@pytest.mark.parametrize("m", [1, 255, 256, 257, 1025])
def test_tri_linear_point_counts_across_the_block_edge(hip, m):
    sc = pc.dlt_scene(np.random.default_rng(410 + m), 3, "noisy", m)
    got = hip.tri_linear(sc["projs"], sc["uv"])
    want, info = pc.dlt_ref(sc["projs"], sc["uv"])
    assert got.shape == (4, m) and np.all(pc.rel_err_cols(got, want) <= info["bound"]) and np.all(got[3] == 1.0)
    assert np.all(info["bound"] < 1e-9)


@pytest.mark.parametrize("k", [2, 5, 512, 513])
def test_tri_linear_view_counts_across_the_lds_edge(hip, k):
    """512 views are staged in LDS, 513 are read from global memory."""
    sc = pc.dlt_scene(np.random.default_rng(420 + k), k, "noisy", 70)
    got = hip.tri_linear(sc["projs"], sc["uv"])
    want, info = pc.dlt_ref(sc["projs"], sc["uv"])
    err = pc.rel_err_cols(got, want)
    print("k = %d: max err/(u kappa rho) = %.3g" % (k, float(np.max(err / (U * info["kappa"] * info["rho"])))))
    assert np.all(err <= info["bound"]) and np.all(got[3] == 1.0) and np.all(info["bound"] < 1e-6)


def _null_space_property(projs, uv, x):
    """|A v| / s0(A) per point for v = x / |x|."""
    a, _ = pc.dlt_design(projs, uv)
    v = (x / np.linalg.norm(x, axis=0)).T
    return np.linalg.norm(np.einsum("mrc,mc->mr", a, v), axis=1) / np.linalg.svd(a, compute_uv=False)[:, 0]


@pytest.mark.parametrize("kind", ["twin", "parallel", "twin_parallel"])
def test_tri_linear_planted_rank_deficient_tracks(hip, kind):
    """twin: any unit v of the two-dimensional null space is right, the output is v / v[3].  parallel: the null vector is
    (0, 0, 1, 0) exactly, the division is by an exact zero as in the reference.  twin_parallel: the null space holds that
    W = 0 direction, so either outcome is consistent."""
    d = pc.dlt_rank2(kind)
    got = hip.tri_linear(d["projs"], d["uv"])
    finite = np.all(np.isfinite(got), axis=0)
    if kind == "parallel":
        want, _ = pc.dlt_ref(d["projs"], d["uv"])
        assert not np.any(np.all(np.isfinite(want), axis=0)) and not finite.any()
        assert np.all(np.isinf(got[2])) and np.all(np.isnan(got[3]))
    if kind == "twin":
        assert finite.all()
    if finite.any():
        x = got[:, finite]
        assert np.all(x[3] == 1.0)
        resid = _null_space_property(d["projs"], d["uv"][:, :, finite], x)
        assert np.all(resid <= C * U), resid


def test_tri_linear_nan_key_poisons_only_its_own_point(hip):
    sc = pc.dlt_scene(np.random.default_rng(430), 4, "noisy", 300)
    clean = hip.tri_linear(sc["projs"], sc["uv"])
    uv = sc["uv"].copy()
    uv[2, 1, 70] = np.nan
    uv[0, 0, 257] = np.inf
    got = hip.tri_linear(sc["projs"], uv)
    others = np.ones(300, dtype=bool)
    others[[70, 257]] = False
    assert same_bits(got[:, others], clean[:, others]) and np.all(np.isfinite(clean))
    assert not np.all(np.isfinite(got[:, 70])) and not np.all(np.isfinite(got[:, 257]))


# ------------------------------------------------------------------------------------------------ DLT, ragged
@pytest.fixture(scope="module")
def ragged(hip):
    """210 single tracks with their own projections, the W = 0 plants, a rank-2 twin and tracks of length 0 and 1, in
    one call.  The point order is shuffled so that neighbouring threads hold tracks of different lengths."""
    rng = np.random.default_rng(440)
    tracks = [dict(kind=c["kind"], k=c["k"], projs=c["projs"], uv=c["uv"][:, :, 0], case=c) for c in pc.dlt_cases(rng, 210)]
    for kind in ("parallel", "twin_parallel"):
        d = pc.dlt_rank2(kind, 1)
        tracks += [dict(kind=kind, k=d["projs"].shape[0], projs=d["projs"], uv=d["uv"][:, :, 0], case=None)] * 3
    d = pc.dlt_rank2("twin", 1)
    tracks.append(dict(kind="twin", k=2, projs=d["projs"], uv=d["uv"][:, :, 0], case=None))
    one = pc.dlt_scene(rng, 2, "scene", 1)
    tracks += [dict(kind="len1", k=1, projs=one["projs"][0:1], uv=one["uv"][0:1, :, 0], case=None)] * 3
    tracks += [dict(kind="len0", k=0, projs=np.zeros((0, 3, 4)), uv=np.zeros((0, 2)), case=None)] * 3
    order = rng.permutation(len(tracks))
    tracks = [tracks[i] for i in order]
    lengths = np.array([t["k"] for t in tracks])
    pt_ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    projs = np.concatenate([t["projs"] for t in tracks])
    cam_idx = np.arange(projs.shape[0], dtype=np.int32)
    uv = np.ascontiguousarray(np.concatenate([t["uv"] for t in tracks]).T)
    x_init = np.vstack((rng.normal(size=(3, len(tracks))), np.ones((1, len(tracks)))))
    got, _cost, status = hip.tri_tracks(pt_ptr, cam_idx, uv, projs, x_init, hip.TRACKS_LINEAR, 0.5, 0)
    return tracks, x_init, got, status


def test_tri_tracks_linear_every_kind_within_bound(ragged):
    tracks, _x_init, got, status = ragged
    worst, total, left_out, cond_max = {}, 0, 0, 0.0
    for p, t in enumerate(tracks):
        if t["case"] is None:
            continue
        want, info = pc.dlt_ref(t["case"]["projs"], t["case"]["uv"])
        total += 1
        if not info["bound"][0] < 0.5:
            left_out += 1
            continue
        err = pc.rel_err(got[:, p], want[:, 0])
        assert status[p] == 0 and got[3, p] == 1.0 and err <= info["bound"][0], (t["kind"], t["k"], t["case"]["param"], err, info["bound"][0])
        cond = float(info["kappa"][0] * info["rho"][0])
        worst[t["kind"]] = max(worst.get(t["kind"], 0.0), err / (U * cond))
        cond_max = max(cond_max, cond)
    print("tri_tracks linear: %d tracks, %.1f %% left out, largest kappa rho checked %.3g" % (total, 100.0 * left_out / total, cond_max))
    print("tri_tracks linear: max err/(u kappa rho) per kind: " + ", ".join("%s %.3g" % kv for kv in sorted(worst.items())))
    assert left_out <= 0.10 * total and cond_max >= 1e6 and set(worst) == set(pc.DLT_KINDS)
    assert max(worst.values()) < C


def test_tri_tracks_linear_status_of_the_planted_tracks(hip, ragged):
    tracks, x_init, got, status = ragged
    kinds = np.array([t["kind"] for t in tracks])
    few = np.isin(kinds, ("len0", "len1"))
    assert few.sum() == 6 and np.all(status[few] == hip.TRACK_TOO_FEW) and same_bits(got[:, few], x_init[:, few])
    zero = kinds == "parallel"
    assert zero.sum() == 3 and np.all(status[zero] == hip.TRACK_NONFINITE) and same_bits(got[:, zero], x_init[:, zero])
    # no other track is flagged, except that the twin with a W = 0 direction in its null space may be
    free = ~few & ~zero & (kinds != "twin_parallel")
    assert not status[free].any() and np.all(np.isfinite(got[:, free]))
    either = kinds == "twin_parallel"
    assert np.all((status[either] == 0) | (status[either] == hip.TRACK_NONFINITE))
    kept = either & (status == hip.TRACK_NONFINITE)
    assert same_bits(got[:, kept], x_init[:, kept])
    twin = int(np.flatnonzero(kinds == "twin")[0])
    d = pc.dlt_rank2("twin", 1)
    assert _null_space_property(d["projs"], d["uv"], got[:, twin:twin + 1])[0] <= C * U


def test_tri_tracks_linear_equals_the_rectangular_kernel_on_hard_geometry(hip, rect_sweep):
    """The shared solver of sfm_dlt.h behind both entries: equal bits for every kind at k = 2, 5 and 33."""
    for sc, rect, _ in rect_sweep:
        if sc["k"] not in (2, 5, 33) and not (sc["kind"] == "dupview" and sc["k"] == 3):
            continue
        k, m = sc["k"], sc["uv"].shape[2]
        pt_ptr = (k * np.arange(m + 1)).astype(np.int32)
        cam_idx = np.tile(np.arange(k, dtype=np.int32), m)
        uv = np.ascontiguousarray(sc["uv"].transpose(1, 2, 0).reshape(2, m * k))
        got, _cost, status = hip.tri_tracks(pt_ptr, cam_idx, uv, sc["projs"], None, hip.TRACKS_LINEAR, 0.5, 0)
        assert same_bits(got, rect) and not status.any(), (sc["kind"], k)


# ------------------------------------------------------------------------------------------------ six point
@pytest.fixture(scope="module")
def six_sweep(hip):
    rng = np.random.default_rng(450)
    kmat = pc.random_intrinsic(rng)
    cases = pc.six_point_cases(rng, 2100, kmat)
    uv, x, samples = pc.six_point_launch(cases)
    rot, loc, _cnt = hip.pnp_six_point_hypotheses(uv, x, kmat, samples, 2.0)
    return kmat, cases, rot, loc


def test_six_point_sweep_within_bound(six_sweep):
    kmat, cases, rot, loc = six_sweep
    worst_r, worst_c, total, left_out, cond_max = {}, {}, 0, 0, 0.0
    for h, c in enumerate(cases):
        if c["kind"] == "repeat":
            continue
        total += 1
        r_ref, c_ref, info = pc.six_point_ref(c["key"], c["X"], kmat)
        if not pc.six_point_checkable(info):
            left_out += 1
            continue
        e_r, e_c = pc.rel_err(rot[h], r_ref), pc.rel_err(loc[h], c_ref)
        assert e_r <= info["bound_r"] and e_c <= info["bound_c"], (h, c["kind"], c["param"], e_r, info["bound_r"], e_c, info["bound_c"])
        worst_r[c["kind"]] = max(worst_r.get(c["kind"], 0.0), e_r / (U * info["cond_r"]))
        worst_c[c["kind"]] = max(worst_c.get(c["kind"], 0.0), e_c / (U * info["cond_c"]))
        cond_max = max(cond_max, info["cond_r"])
    print("six point: %d hypotheses checked, %.1f %% left out, largest kW kP / s0(M) checked %.3g"
          % (total - left_out, 100.0 * left_out / total, cond_max))
    print("six point: max err/(u cond) per kind, rotation: " + ", ".join("%s %.3g" % kv for kv in sorted(worst_r.items())))
    print("six point: max err/(u cond) per kind, centre:   " + ", ".join("%s %.3g" % kv for kv in sorted(worst_c.items())))
    assert left_out <= 0.10 * total and cond_max >= 1e6 and len(worst_r) == len(pc.SIX_KINDS) - 1
    assert max(worst_r.values()) < C and max(worst_c.values()) < C


def test_six_point_repeated_index(six_sweep):
    """Rank-10 W: any unit vector of the two-dimensional null space is right.  The pose keeps R^T = polar(M) and
    C = R (-m4) / s0(M) of it, so some symmetric H and scale s make p = [R^T H | -s R^T C] a null vector of W
    (six_point_null_residual): |W p| <= C u kP s0(W) |p|, and R is orthonormal to C u kP."""
    kmat, cases, rot, loc = six_sweep
    seen = 0
    for h, c in enumerate(cases):
        if c["kind"] != "repeat":
            continue
        finite = np.all(np.isfinite(rot[h])), np.all(np.isfinite(loc[h]))
        assert finite[0] == finite[1], h
        key6, x6 = c["key"][:, c["sample"]], c["X"][:, c["sample"]]
        _, _, info = pc.six_point_ref(key6, x6, kmat)
        if not finite[0]:
            continue
        resid, k_p = pc.six_point_null_residual(info["W"], rot[h], loc[h])
        assert resid <= C * U * k_p, (h, resid, k_p)
        assert np.max(np.abs(rot[h] @ rot[h].T - np.eye(3))) <= C * U * k_p and np.linalg.det(rot[h]) > 0, h
        seen += 1
    assert seen >= 270


def test_six_point_reference_fixture_per_hypothesis(hip):
    """The reference's own 300 seeded hypotheses (tests/golden/g5_pnp_hypotheses.npz), each within min(1e-7, its own
    bound) of what the reference returned; where its det(rot) < 0 branch fired it returned -C (quirk Q13)."""
    g = load_golden("g5_pnp_hypotheses.npz")
    rot, loc, _cnt = hip.pnp_six_point_hypotheses(g["pts2d"], g["pts3d"], g["K"], g["samples"], float(g["threshold"]))
    branch = g["branch"].astype(bool)
    tight = 0
    for h in range(300):
        s = g["samples"][h]
        _, _, info = pc.six_point_ref(g["pts2d"][:, s], g["pts3d"][:, s], g["K"])
        c_want = -g["C"][h] if branch[h] else g["C"][h]
        e_r, e_c = pc.rel_err(rot[h], g["R"][h]), pc.rel_err(loc[h], c_want)
        assert e_r <= min(1e-7, info["bound_r"]) and e_c <= min(1e-7, info["bound_c"]), (h, e_r, e_c, info["bound_r"], info["bound_c"])
        tight += info["bound_c"] < 1e-7
    print("fixture: %d of 300 hypotheses held to their own bound below 1e-7" % tight)


# ------------------------------------------------------------------------------------------------ scoring and mask
THR = 2.0


def _mask_scene(seed, n):
    """A noisy view with gross outliers; a quarter of the keys are moved to THR (1 +- 10^-e), e in 3 .. 9, from their
    float64 projection, so that values crowd the threshold from both sides."""
    rng = np.random.default_rng(seed)
    kmat = pc.random_intrinsic(rng)
    sc = pc.pnp_scene(rng, n, kmat, noise=0.5, outlier_frac=0.2)
    proj, mag = pc.pose_projection(kmat, sc["R"], sc["C"])
    s = proj @ sc["X"]
    for i in rng.choice(n, max(1, n // 4), replace=False):
        ang = rng.uniform(0, 2 * np.pi)
        d = THR * (1.0 + rng.choice([-1.0, 1.0]) * 10.0 ** -rng.uniform(3, 9))
        sc["uv"][0:2, i] = s[0:2, i] / s[2, i] + d * np.array([np.cos(ang), np.sin(ang)])
    val, bound = pc.reprojection_values(proj, mag, sc["uv"], sc["X"])
    return kmat, sc, val, bound


@pytest.mark.parametrize("n", [6, 255, 256, 257, 1023, 1025])
def test_inlier_mask_with_the_threshold_in_a_gap(hip, n):
    kmat, sc, val, bound = _mask_scene(460 + n, n)
    thr = pc.gap_threshold(val, bound, THR)
    assert thr is not None and (n < 255 or abs(thr - THR) < 1e-3)
    near = np.abs(val - thr)
    print("n = %d: nearest value %.3g from the threshold, largest bound %.3g" % (n, near.min(), bound.max()))
    assert near.min() > 2 * bound.max() and (n < 255 or near.min() < 1e-6)
    got = hip.pnp_inlier_mask(sc["uv"], sc["X"], kmat, sc["R"], sc["C"], thr, as_array=True)
    assert np.array_equal(got, np.flatnonzero(val < thr))


def test_inlier_mask_planted_points(hip):
    """Identity pose, so s2 is the point's own Z: Z = +0, -0, a NaN and an inf * 0 coordinate are never inliers (the
    reference's `err < threshold` is false for NaN and inf); a point behind the camera that projects onto its key is
    one (the reference does not test the depth here)."""
    rng = np.random.default_rng(470)
    kmat = pc.random_intrinsic(rng)
    n = 300
    xc = np.vstack((rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(4, 15, n), np.ones(n)))
    proj, mag = pc.pose_projection(kmat, np.eye(3), np.zeros(3))
    assert np.array_equal(proj[:, 0:3], kmat) and not proj[:, 3].any()
    xc[2, 10], xc[2, 11] = 0.0, -0.0
    xc[0, 12] = np.nan
    xc[0, 13] = np.inf                       # times P[2][0] = 0
    xc[0:3, 14] = -xc[0:3, 14]               # behind the camera, the same image point
    xc[0:2, 15], xc[2, 15] = 0.0, 0.0        # 0 / 0
    uv = proj @ np.where(np.isfinite(xc), xc, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = uv / uv[2]
    uv[:, [10, 11, 15]] = [[kmat[0, 2]], [kmat[1, 2]], [1.0]]
    uv[0:2] += 0.5 * rng.normal(size=(2, n)) * (np.arange(n) >= 16)
    val, bound = pc.reprojection_values(proj, mag, uv, xc)
    assert not np.isfinite(val[[10, 11, 12, 13, 15]]).any() and val[14] < 1e-9 and xc[2, 14] < 0
    ok = np.isfinite(val)
    assert np.all(np.abs(val[ok] - THR) > 2 * bound[ok])
    want = np.flatnonzero(ok & (val < THR))
    assert 14 in want
    assert np.array_equal(hip.pnp_inlier_mask(uv, xc, kmat, np.eye(3), np.zeros(3), THR, as_array=True), want)
    # the same points through the hypothesis scoring: a sample of six clean points recovers the identity pose
    samples = np.array([[20, 40, 60, 80, 100, 120]], dtype=np.int32)
    _r, _c, inl, best = hip.pnp_linear_ransac(uv, xc, kmat, samples, 50.0, as_array=True)
    assert best == 0 and not np.isin([10, 11, 12, 13, 15], inl).any() and 14 in inl


def _ransac_case(seed, n, n_hyp):
    """A noise-free view with 25 % gross outliers (none at n = 6) and n_hyp six-point samples; per hypothesis the
    float64 pose, its bounds, every point's value under it and the value's bound (rounding + the pose's own bound)."""
    rng = np.random.default_rng(seed)
    kmat = pc.random_intrinsic(rng)
    sc = pc.pnp_scene(rng, n, kmat, noise=0.0, outlier_frac=0.25 if n > 6 else 0.0)
    samples = np.stack([rng.choice(n, 6, replace=False) for _ in range(n_hyp)]).astype(np.int32)
    clean = np.setdiff1d(np.arange(n), sc["outliers"])
    first = 2 if n_hyp >= 7 else 0
    samples[first] = rng.choice(clean, 6, replace=False)      # a sample without an outlier: it fits every clean point
    if n_hyp >= 7:
        samples[5] = samples[first]                  # and its copy: the tie sits at the maximum, the first one wins
    val, bound = np.empty((n_hyp, n)), np.empty((n_hyp, n))
    for h, s in enumerate(samples):
        rot, loc, info = pc.six_point_ref(sc["uv"][:, s], sc["X"][:, s], kmat)
        proj, mag = pc.pose_projection(kmat, rot, loc)
        dproj = pc.pose_uncertainty(kmat, loc, info["bound_r"], info["bound_c"])
        if np.all(np.isfinite(dproj)):
            val[h], bound[h] = pc.reprojection_values(proj, mag, sc["uv"], sc["X"], dproj)
        else:
            val[h], bound[h] = np.nan, np.inf
    return kmat, sc, samples, val, bound


def _counts_range(val, bound, thr):
    with np.errstate(invalid="ignore"):
        amb = ~(np.abs(val - thr) > 2 * bound)
        sure = (val < thr) & ~amb
    return sure, amb


@pytest.mark.parametrize("n,n_hyp", [(6, 1), (255, 7), (256, 300), (257, 7), (1023, 300), (1025, 7), (1025, 1)])
def test_ransac_counts_and_winner_with_the_threshold_in_a_gap(hip, n, n_hyp):
    kmat, sc, samples, val, bound = _ransac_case(480 + n + n_hyp, n, n_hyp)
    sure, amb = _counts_range(val, bound, THR)
    decided = ~amb.any(axis=1)
    lo, hi = sure.sum(axis=1), sure.sum(axis=1) + amb.sum(axis=1)
    print("n = %d, n_hyp = %d: %d hypotheses decided, largest bound among them %.3g" % (n, n_hyp, decided.sum(), bound[decided].max()))
    assert decided.sum() >= 0.9 * n_hyp
    rot, loc, cnt, _neg = hip.pnp_ransac_evaluate(sc["uv"], sc["X"], kmat, samples, THR)
    assert np.array_equal(cnt[decided], lo[decided]) and np.all((lo <= cnt) & (cnt <= hi))
    best = int(np.argmax(lo))
    assert decided[best] and lo[best] == n - sc["outliers"].size
    # the reference's rule: the first hypothesis with a strictly larger count; undecided ones cannot reach the winner
    assert np.all(hi[~decided] < lo[best])
    r, c, inl, got_best = hip.pnp_linear_ransac(sc["uv"], sc["X"], kmat, samples, THR, as_array=True)
    assert got_best == best and np.array_equal(inl, np.flatnonzero(sure[best]))
    assert same_bits(r, rot[best]) and same_bits(c.ravel(), loc[best])
    if n_hyp >= 7:
        assert best <= 2 and cnt[5] == cnt[2] == cnt[best] and same_bits(rot[5], rot[2])


@pytest.mark.parametrize("n,n_hyp", [(257, 1), (1025, 7)])
def test_score_kernel_with_values_crowding_the_threshold(hip, n, n_hyp):
    """pnp_score_kernel with values on both sides of the threshold at THR (1 +- 10^-e), e in 3 .. 6.  The pose is the
    device's own six-point solve of hypothesis 0, known to its bound: of 60 clean samples the best-conditioned one, a
    quarter of the keys are moved to crowd the threshold under its float64 pose, and the value bounds carry the pose's
    uncertainty.  The count of hypothesis 0 must be exact, and so must the mask of that pose."""
    rng = np.random.default_rng(485 + n)
    kmat = pc.random_intrinsic(rng)
    sc = pc.pnp_scene(rng, n, kmat, noise=0.5, outlier_frac=0.2)
    clean = np.setdiff1d(np.arange(n), sc["outliers"])
    draws = [rng.choice(clean, 6, replace=False) for _ in range(60)]
    refs = [pc.six_point_ref(sc["uv"][:, s], sc["X"][:, s], kmat) for s in draws]
    pick = int(np.argmin([r[2]["bound_c"] for r in refs]))
    rot, loc, info = refs[pick]
    proj, mag = pc.pose_projection(kmat, rot, loc)
    s = proj @ sc["X"]
    free = np.setdiff1d(np.arange(n), draws[pick])           # the sample's own keys stay: they define the pose
    for i in rng.choice(free, n // 4, replace=False):
        ang = rng.uniform(0, 2 * np.pi)
        d = THR * (1.0 + rng.choice([-1.0, 1.0]) * 10.0 ** -rng.uniform(3, 6))
        sc["uv"][0:2, i] = s[0:2, i] / s[2, i] + d * np.array([np.cos(ang), np.sin(ang)])
    val, bound = pc.reprojection_values(proj, mag, sc["uv"], sc["X"], pc.pose_uncertainty(kmat, loc, info["bound_r"], info["bound_c"]))
    thr = pc.gap_threshold(val, bound, THR)
    assert thr is not None
    near = np.abs(val - thr)
    print("n = %d: pose bounds %.3g / %.3g, nearest value %.3g from the threshold, largest bound %.3g"
          % (n, info["bound_r"], info["bound_c"], near.min(), bound.max()))
    assert near.min() > 2 * bound.max() and near.min() < 1e-5
    samples = np.stack([draws[pick]] + [rng.choice(n, 6, replace=False) for _ in range(n_hyp - 1)]).astype(np.int32)
    rots, locs, cnt, _neg = hip.pnp_ransac_evaluate(sc["uv"], sc["X"], kmat, samples, thr)
    want = np.flatnonzero(val < thr)
    assert cnt[0] == want.size
    assert np.array_equal(hip.pnp_inlier_mask(sc["uv"], sc["X"], kmat, rots[0], locs[0], thr, as_array=True), want)


@pytest.mark.parametrize("n,n_hyp", [(257, 7), (1023, 300)])
def test_ransac_threshold_on_a_value(hip, n, n_hyp):
    """The threshold equal to one point's float64 value under the winning hypothesis: that point may fall either way,
    but the winner's mask (pnp_inlier_mask_kernel) sums to the count that chose it (pnp_score_kernel)."""
    rng = np.random.default_rng(490 + n)
    kmat = pc.random_intrinsic(rng)
    sc = pc.pnp_scene(rng, n, kmat, noise=0.5, outlier_frac=0.2)
    samples = np.stack([rng.choice(n, 6, replace=False) for _ in range(n_hyp)]).astype(np.int32)
    _r0, _c0, cnt0, _ = hip.pnp_ransac_evaluate(sc["uv"], sc["X"], kmat, samples, THR)
    best0 = int(np.argmax(cnt0))
    rot, loc, info = pc.six_point_ref(sc["uv"][:, samples[best0]], sc["X"][:, samples[best0]], kmat)
    proj, mag = pc.pose_projection(kmat, rot, loc)
    val, _ = pc.reprojection_values(proj, mag, sc["uv"], sc["X"])
    thr = float(np.sort(val[val < THR])[-1])
    rots, locs, cnt, _ = hip.pnp_ransac_evaluate(sc["uv"], sc["X"], kmat, samples, thr)
    r, c, inl, best = hip.pnp_linear_ransac(sc["uv"], sc["X"], kmat, samples, thr, as_array=True)
    assert best == int(np.argmax(cnt)) and len(inl) == cnt[best] and cnt[best] > 6
    assert np.array_equal(inl, hip.pnp_inlier_mask(sc["uv"], sc["X"], kmat, rots[best], locs[best], thr, as_array=True))


def test_ransac_threshold_that_nothing_passes(hip):
    """include/sfm_hip.h: without an inlier the reference's initial identity pose comes back with best = -1."""
    kmat, sc, samples, _val, _bound = _ransac_case(499, 257, 7)
    for thr in (0.0, -1.0):
        r, c, inl, best = hip.pnp_linear_ransac(sc["uv"], sc["X"], kmat, samples, thr, as_array=True)
        assert best == -1 and inl.size == 0 and np.array_equal(r, np.eye(3)) and not c.any()
        _rot, _loc, cnt, cnt_neg = hip.pnp_ransac_evaluate(sc["uv"], sc["X"], kmat, samples, thr)
        assert not cnt.any() and not cnt_neg.any()


# ------------------------------------------------------------------------------------------------ one nonlinear step
def _step_scene(rng, k, kind):
    sc = pc.dlt_scene(rng, k, kind, 300)
    sc["uv"] = sc["uv"] + 1e-4 * rng.normal(size=sc["uv"].shape)
    x0, info = pc.dlt_ref(sc["projs"], sc["uv"])
    keep = info["bound"] < 0.5
    return sc["projs"], np.ascontiguousarray(sc["uv"][:, :, keep]), np.ascontiguousarray(x0[:, keep])


@pytest.mark.parametrize("lam", [0.5, 1e-6, 0.0])
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_tri_nonlinear_one_step_from_the_dlt_result(hip, k, lam):
    """One iteration from the float64 DLT result of the narrow and far geometry against a numpy.longdouble step:
    |x1 - x1_ref| <= C u (kappa(J^T J + lam I) |delta| + |x|); points whose C u kappa >= 0.5 are left out, at most 10 %
    of them at lam = 0.5.  At lam = 0 the share left out is only reported (a narrow track is legitimately singular), and
    the bound carries the rounding of the residuals as well (_pose_cases.tri_step_bound: a plain float64 evaluation
    misses the form without it there, tests/test_pose_oracle.py)."""
    rng = np.random.default_rng(500 + k)
    total = left_out = 0
    worst = 0.0
    for kind in ("narrow", "far", "noisy"):
        projs, uv, x0 = _step_scene(rng, k, kind)
        got = hip.tri_nonlinear(projs, uv, x0, lam, 1)
        want, delta, a, beta = pc.tri_step(projs, uv, x0, lam)
        bound, kappa = pc.tri_step_bound(x0, delta, a, beta if lam == 0.0 else None)
        ok = C * U * kappa < 0.5
        err = np.linalg.norm((got - want)[0:3].astype(np.float64), axis=0)
        ratio = err[ok] / bound[ok]
        print("k = %d, lam = %g, %s: %d points, %d left out, max err/bound %.3g, max kappa %.3g"
              % (k, lam, kind, ok.size, (~ok).sum(), ratio.max() if ok.any() else 0.0, kappa[ok].max() if ok.any() else 0.0))
        assert same_bits(got[3], x0[3])
        assert np.all(err[ok] <= bound[ok]), (kind, float(ratio.max()))
        total, left_out, worst = total + ok.size, left_out + int((~ok).sum()), max(worst, float(ratio.max()) if ok.any() else 0.0)
    print("k = %d, lam = %g: %.1f %% left out" % (k, lam, 100.0 * left_out / total))
    if lam == 0.5:
        assert left_out <= 0.10 * total


@pytest.mark.parametrize("lam", [0.5, 1e-6, 0.0])
def test_pnp_nonlinear_one_step_from_the_six_point_result(hip, lam):
    """One iteration from the float64 six-point pose of a noisy view (plain, far camera, near-coplanar points, and the
    kernel's three size classes) against a numpy.longdouble step: the parameters (C, q) within
    C u (kappa(J^T J + lam I) |delta| + |x|), so |C1 - C1_ref| within it and max|R1 - R1_ref| within four times it (R is
    quadratic in the unit quaternion).  A view whose C u kappa >= 0.5 is left out; none may be at lam = 0.5."""
    rng = np.random.default_rng(510)
    kmat = pc.random_intrinsic(rng)
    left_out = 0
    for name, uv, x, rot0, loc0 in pc.pnp_step_scenes(rng, kmat):
        want_r, want_c, delta, a, par = pc.pnp_step(uv, x, kmat, rot0, loc0, lam)
        bound, kappa = pc.pnp_step_bound(par, delta, a)
        if not C * U * kappa < 0.5:
            left_out += 1
            print("lam = %g, %s: left out (kappa %.3g)" % (lam, name, kappa))
            continue
        got_r, got_c = hip.pnp_nonlinear(uv, x, kmat, rot0, loc0, lam, 1)
        e_c = float(np.linalg.norm(got_c.ravel() - want_c.astype(np.float64)))
        e_r = float(np.max(np.abs(got_r - want_r.astype(np.float64)))) / 4
        print("lam = %g, %s (n = %d): kappa %.3g, |delta| %.3g, err/bound centre %.3g, rotation %.3g"
              % (lam, name, uv.shape[1], kappa, float(np.linalg.norm(delta.astype(np.float64))), e_c / bound, e_r / bound))
        assert e_c <= bound and e_r <= bound, (name, e_c, e_r, bound)
    print("lam = %g: %d of %d views left out" % (lam, left_out, len(pc.PNP_STEP_SCENES)))
    if lam == 0.5:
        assert left_out == 0
