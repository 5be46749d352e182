"""GPU tests of the translation averaging: sfm_translation_average, its _dev form and the Python entry points, against the
float64 NumPy reference of tests/_transavg_reference.py.

Decisions (status, n_inliers, every edge verdict, every view status, the summary, and per solve of the log its inlier count
and whether it stood) are compared EXACTLY: tests/test_transavg_host.py asserts that every case used here is settled in the
reference.  C_out, edge_cos and edge_len are compared at max(1e-9, 100 d_C) relative to the largest |c_v|, d_C being the
disagreement of the reference's own two routes: the bound comes from the reference alone.  The cost of a solve is a sum over
E terms w ((n2 - dv^2) + mu (dv - l)^2) whose v moves by at most 2 bound scale: it is held to 16 E scale^2 bound.  The device
runs with the reference's CG_TOL and the case's cg_max."""
import math

import numpy as np
import pytest

import _transavg_reference as tr
from _twoview_checks import same_bits

pytestmark = pytest.mark.gpu


def run(hip, c, **over):
    kw = dict(edge_mask=c.mask, root=c.root, cos_max=c.cos_max, mu=c.mu, rounds=c.rounds, polish=c.polish, cg_tol=c.cg_tol, cg_max=c.cg_max)
    kw.update(over)
    return hip.translation_average(c.V, c.edges, c.R, c.t, **kw)


def check_against(ref, got, where="", bound=None, cg_limit=False):
    C, edge_inlier, edge_cos, edge_len, view_status, n_inliers, status, summary, log = got
    bound = ref.bound if bound is None else bound
    assert ref.settled, where
    assert status == (ref.status | (tr.CG_LIMIT if cg_limit else 0)), where
    assert n_inliers == ref.n_inliers, where
    assert np.array_equal(edge_inlier, ref.edge_inlier), where
    assert np.array_equal(view_status, ref.view_status), where
    assert np.array_equal(summary, ref.summary), where
    assert np.array_equal(log[:, 0], ref.log[:, 0]) and np.array_equal(log[:, 2], ref.log[:, 2]), where
    scale = ref.scale if ref.scale > 0 else 1.0
    err_C = float(np.max(np.abs(C - ref.C))) / scale
    has = np.isfinite(ref.edge_cos)
    assert np.array_equal(np.isfinite(edge_cos), has), where
    assert np.array_equal(np.isfinite(edge_len), np.isfinite(ref.edge_len)), where
    err_c = float(np.max(np.abs(edge_cos[has] - ref.edge_cos[has]))) if has.any() else 0.0
    used = np.isfinite(ref.edge_len)
    err_l = float(np.max(np.abs(edge_len[used] - ref.edge_len[used]))) / scale if used.any() else 0.0
    err_cost = float(np.max(np.abs(log[:, 3] - ref.log[:, 3])))
    cost_bound = 16.0 * ref.edge_inlier.shape[0] * scale * scale * bound
    print("%s: |dC| %.3g |dcos| %.3g |dlen| %.3g bound %.3g d_C %.3g |dcost| %.3g (%.3g) CG %s" % (
        where, err_C, err_c, err_l, bound, ref.d_C, err_cost, cost_bound, log[:, 1].astype(int).tolist()))
    assert err_C <= bound and err_c <= bound and err_l <= bound and err_cost <= cost_bound, where


@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_case_matches_reference(hip, name):
    c = tr.case(name)
    check_against(c.ref, run(hip, c), name)


def test_chain_baselines_come_out_at_one(hip):
    c = tr.case("chain_300")
    got = run(hip, c)
    assert got[6] == 0 and got[1].all()
    err = float(np.max(np.abs(got[3] - 1.0))) / c.ref.scale
    print("chain: largest |len - 1| / scale %.3g (bound %.3g)" % (err, c.ref.bound))
    assert err <= c.ref.bound


def test_line_of_cameras(hip):
    """The directions of collinear cameras fix no length; the mu term does: every position is on the line."""
    c = tr.case("line_9")
    got = run(hip, c)
    assert got[6] == 0 and got[1].all()
    axis = np.array([0.6, 0.0, 0.8])
    off = got[0] - np.outer(got[0] @ axis, axis)
    assert float(np.max(np.abs(off))) / c.ref.scale <= c.ref.bound


def test_negated_translation_is_flagged(hip):
    c = tr.case("flipped")
    got = run(hip, c)
    for e in c.flipped:
        assert got[1][e] == 0 and got[2][e] < -math.cos(math.radians(c.max_angle_deg))
    assert got[1].sum() == c.edges.shape[0] - len(c.flipped)


def test_root_whose_edges_are_all_masked_has_no_model(hip):
    c = tr.case("root_masked")
    got = run(hip, c)
    assert got[6] == tr.NO_MODEL and not got[0].any() and not got[1].any() and np.all(got[4] & tr.HELD) and not got[8].any()
    assert got[7][0] == 0 and got[7][4] == 0
    check_against(c.ref, got, "root_masked")


def test_views_without_rotation_mask_and_components(hip):
    z = tr.case("zero_R")
    got = run(hip, z)
    assert np.all(got[4][[3, 9]] == (tr.NO_ROTATION | tr.UNREACHED | tr.HELD)) and not got[0][[3, 9]].any()
    m = tr.case("mask_cut")
    got = run(hip, m)
    assert got[4][7] == (tr.UNREACHED | tr.HELD) and not got[0][7].any() and np.isnan(got[3][-3:]).all()
    two = tr.case("two_components")
    got = run(hip, two)
    assert np.all(got[4][10:] == (tr.UNREACHED | tr.HELD)) and not got[0][10:].any() and not got[4][:10].any()
    h = tr.case("held")
    got = run(hip, h)
    assert got[4][9] == tr.HELD and got[0][9].any()          # reached, cut off by the verdicts: it keeps the position it had


@pytest.mark.parametrize("rounds", [0, 1, 8])
@pytest.mark.parametrize("polish", [0, 1])
def test_rounds_and_polish(hip, rounds, polish):
    for name in ("complete_12", "parallel_edges", "two_components", "size_65_1025"):
        c = tr.case(name)
        ref = tr.solve(c, rounds=rounds, polish=polish)
        check_against(ref, run(hip, c, rounds=rounds, polish=polish), "%s rounds=%d polish=%d" % (name, rounds, polish))


@pytest.mark.parametrize("mu", [1.0, 0.1, 0.01, 0.0])
def test_mu(hip, mu):
    """mu = 0 means 0.01."""
    for name in ("complete_12", "line_9", "star_201"):
        c = tr.case(name)
        ref = tr.solve(c, mu=mu)
        got = run(hip, c, mu=mu)
        check_against(ref, got, "%s mu=%g" % (name, mu))
        if mu == 0.0:
            assert all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(got, run(hip, c, mu=0.01)))


def test_polish_that_does_not_stand(hip):
    c = tr.case("kept")
    assert c.ref.status & tr.KEPT_ROUNDS and c.ref.log[-1, 2] == 0.0 and c.ref.log[-1, 0] < c.ref.log[-2, 0]
    check_against(c.ref, run(hip, c), "kept")


def test_cg_limit(hip):
    """cg_max = 1: the flag is set, the call succeeds, and the result is that of the reference's own CG route stopped after
    one iteration per solve (the dense route is no yardstick for an unconverged solve): decisions equal, values within 1e-9."""
    c = tr.case("complete_12")
    kw = dict(mask=c.mask, root=c.root, cos_max=c.cos_max, mu=c.mu, rounds=c.rounds, polish=c.polish, route="cg", cg_max=1)
    ref = tr.run(c.V, c.edges, c.R, c.t, **kw)
    moved = [tr.run(c.V, c.edges, c.R, c.t, cos_shift=s, **kw) for s in (-tr.REL, tr.REL)]
    ref.settled = all(m.trace == ref.trace for m in moved)
    ref.scale = float(np.max(np.sqrt(np.sum(ref.C * ref.C, axis=1))))
    ref.d_C = 0.0
    assert ref.status & tr.CG_LIMIT
    got = run(hip, c, cg_max=1)
    assert np.all(got[8][:, 1] == 1.0)
    check_against(ref, got, "cg_max=1", bound=1e-9)


def test_run_to_run_bits_and_absent_outputs(hip):
    c = tr.case("size_65_1025")
    a, b = run(hip, c), run(hip, c)
    assert all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
    only_C = run(hip, c, outputs=())
    assert same_bits(only_C[0], a[0]) and all(v is None for v in only_C[1:])
    some = run(hip, c, outputs=("edge_len", "summary"))
    assert same_bits(some[3], a[3]) and same_bits(some[7], a[7]) and some[1] is None and some[8] is None


def test_dev_form_matches_host_form(hip):
    import torch
    c = tr.case("size_65_1025")
    mask = np.ones(c.edges.shape[0], dtype=np.uint8)
    mask[::17] = 0
    host = run(hip, c, edge_mask=mask)
    dev = torch.device("cuda")
    E = c.edges.shape[0]
    d_R, d_t, d_mask = torch.from_numpy(c.R).to(dev), torch.from_numpy(c.t).to(dev), torch.from_numpy(mask).to(dev)
    d_C = torch.zeros(c.V, 3, dtype=torch.float64, device=dev)
    d_in = torch.zeros(E, dtype=torch.uint8, device=dev)
    d_cos = torch.zeros(E, dtype=torch.float64, device=dev)
    d_len = torch.zeros(E, dtype=torch.float64, device=dev)
    d_view = torch.zeros(c.V, dtype=torch.int32, device=dev)
    d_small = torch.zeros(2, dtype=torch.int32, device=dev)
    d_sum = torch.zeros(6, dtype=torch.int64, device=dev)
    d_log = torch.zeros(c.rounds + 2, 4, dtype=torch.float64, device=dev)
    kw = dict(root=c.root, cos_max=c.cos_max, mu=c.mu, rounds=c.rounds, polish=c.polish, cg_tol=c.cg_tol, cg_max=c.cg_max)
    torch.cuda.synchronize()
    hip.translation_average_dev(c.V, c.edges, d_R.data_ptr(), d_t.data_ptr(), d_mask.data_ptr(), d_C_out=d_C.data_ptr(),
                                d_edge_inlier=d_in.data_ptr(), d_edge_cos=d_cos.data_ptr(), d_edge_len=d_len.data_ptr(),
                                d_view_status=d_view.data_ptr(), d_n_inliers=d_small.data_ptr(), d_status=d_small.data_ptr() + 4,
                                d_summary=d_sum.data_ptr(), d_log=d_log.data_ptr(), **kw)
    assert same_bits(d_C.cpu().numpy(), host[0]) and same_bits(d_in.cpu().numpy(), host[1]) and same_bits(d_cos.cpu().numpy(), host[2])
    assert same_bits(d_len.cpu().numpy(), host[3]) and same_bits(d_view.cpu().numpy(), host[4])
    assert tuple(d_small.cpu().numpy().tolist()) == host[5:7] and same_bits(d_sum.cpu().numpy(), host[7]) and same_bits(d_log.cpu().numpy(), host[8])
    # only C_out, no mask; and an R that is no rotation is found on the device and named
    d_C2 = torch.zeros(c.V, 3, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    hip.translation_average_dev(c.V, c.edges, d_R.data_ptr(), d_t.data_ptr(), d_C_out=d_C2.data_ptr(), **kw)
    assert same_bits(d_C2.cpu().numpy(), run(hip, c)[0])
    bad = c.R.copy()
    bad[40] *= 1.01
    bad[12] *= 1.01
    d_bad = torch.from_numpy(bad).to(dev)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="view 12 "):
        hip.translation_average_dev(c.V, c.edges, d_bad.data_ptr(), d_t.data_ptr(), d_C_out=d_C2.data_ptr(), **kw)


def _angle_deg(a, b):
    c = float(a @ b) / (float(np.linalg.norm(a)) * float(np.linalg.norm(b)))
    return math.degrees(math.acos(min(1.0, max(-1.0, c))))


def test_average_translations_on_the_pose_pairs(hip, sfm):
    """The pairs of tests/_twoview_pose_reference.py as a view graph (tests/_rotavg_pairs.py): posed by ``initialise_pairs``,
    oriented by ``average_rotations``, placed by ``average_translations``.  The wrapper passes what ``native.translation_average``
    gets from the same arrays (bit for bit); the result agrees with the NumPy reference within its bound; and every edge's
    baseline lies within the admitted angle of the world direction of its pair."""
    import _rotavg_pairs as rp
    P = sfm.processors
    g = rp.pose_graph()
    ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
    out = ep.initialise_pairs(g.sets, g.K)
    for o, (ref, que) in zip(out, g.pairs):
        assert o["best_cand"] >= 0
        o["ref"], o["que"] = ref, que
    hopeless = dict(out[0], best_cand=-1, R=np.zeros((3, 3)))                             # a pair without a pose is skipped
    cp = P.HipCamposeProcessor(None, 5, 25)
    rots, rot_verdict = cp.average_rotations(out + [hopeless], g.n_views, root=0, max_angle_deg=g.max_angle_deg, max_hyp=16, iteration=2)
    assert rot_verdict["status"] == 0
    centres, verdict = cp.average_translations(out + [hopeless], rots, g.n_views, root=0, max_angle_deg=g.max_angle_deg, rounds=4,
                                               edge_mask=rot_verdict["edge_inlier"])
    assert verdict is cp.translation_last and verdict["pairs"] == [0, 1, 2, 3, 4]
    assert same_bits(centres[0], np.zeros((3, 1))) and all(c is not None and c.shape == (3, 1) for c in centres)
    edges = np.array(g.pairs, dtype=np.int32)
    R = np.array([r.T for r in rots])
    t = np.array([np.asarray(o["t"]).reshape(3) for o in out])
    direct = hip.translation_average(g.n_views, edges, R, t, edge_mask=rot_verdict["edge_inlier"], root=0, max_angle_deg=g.max_angle_deg,
                                     rounds=4, polish=1)
    assert same_bits(np.array(centres).reshape(-1, 3), direct[0]) and same_bits(verdict["edge_len"], direct[3])
    c = tr.SimpleNamespace(V=g.n_views, edges=edges, R=R.reshape(-1, 9), t=t, mask=rot_verdict["edge_inlier"].astype(np.uint8), root=0,
                           cos_max=float(np.cos(np.deg2rad(g.max_angle_deg))), mu=0.01, rounds=4, polish=1, cg_tol=1e-13, cg_max=500)
    ref = tr.solve(c)
    if ref.settled:
        check_against(ref, direct, "pose pairs")
    d = sfm.geometry.world_directions(R, edges, t)
    for e in np.flatnonzero(verdict["edge_inlier"]):
        i, j = edges[e]
        got = _angle_deg((centres[j] - centres[i]).reshape(3), d[e])
        print("edge %d: %.3f degrees from its direction (admitted %.2f)" % (e, got, g.max_angle_deg))
        assert got <= g.max_angle_deg * (1 + 1e-9)
    assert verdict["status"] == 0 and verdict["edge_inlier"].sum() >= 3 and not verdict["view_status"].any()
    quads = [(o["ref"], o["que"], o["R"], o["t"]) for o in out]
    again, _ = cp.average_translations(quads, R, g.n_views, root=0, max_angle_deg=g.max_angle_deg, rounds=4, edge_mask=rot_verdict["edge_inlier"])
    assert all(same_bits(a, b) for a, b in zip(again, centres))
    with pytest.raises(ValueError):
        cp.average_translations([hopeless], rots, g.n_views)


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def test_locate_views_on_a_device_tracker(hip, sfm):
    """Four views of ``scenes.make_descriptor_views`` through a ``HipDeviceKeyTracker``: five pairs verified, posed, oriented and
    placed.  View 0 is the gauge of both calls and sits at the world's origin with the identity, so the centres are the
    scene's up to scale.  The cameras stand nearly on a line, which fixes no ratio of baselines: directions are compared.  An
    inlier edge's baseline is within ``max_direction_deg`` of its direction d_e by the test itself; d_e is within PREMISE of the
    true direction (asserted as the premise); so the baseline is within their sum of the truth."""
    P = sfm.processors
    dv = sfm.scenes.make_descriptor_views(n_views=4, n_pts=200, seed=0)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(4)]
    K = np.asarray(sfm.scenes.UPENN_K, dtype=np.float64)
    kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
    pairs = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    try:
        for v in range(4):
            kt.add_new_view(views[v], views[:v])
        rots, centres, verdicts, poses = P.locate_views(kt, pairs, K, max_angle_deg=2.0, tree_hyp=8, rounds=2, max_direction_deg=5.0)
    finally:
        kt.kt_release()
    vt = verdicts["translation"]
    assert len(poses) == 5 and verdicts["rotation"]["status"] == 0 and vt["status"] == 0 and vt["pairs"] == [0, 1, 2, 3, 4]
    assert vt["edge_inlier"].all() and not vt["view_status"].any() and same_bits(centres[0], np.zeros((3, 1)))
    R = np.array([r.T for r in rots])
    d = sfm.geometry.world_directions(R, np.array(pairs), np.array([p["t"].reshape(3) for p in poses]))
    PREMISE = 5.0
    for e, (i, j) in enumerate(pairs):
        true = np.asarray(dv.locs[j]) - np.asarray(dv.locs[i])
        premise = _angle_deg(d[e], true)
        got = _angle_deg((centres[j] - centres[i]).reshape(3), true)
        print("pair %d-%d: direction %.3f, baseline %.3f degrees from the truth" % (i, j, premise, got))
        assert premise <= PREMISE and got <= PREMISE + 5.0


def test_end_to_end_rotations_then_positions(hip):
    """Eight views, all 28 pairs posed with 0.5 degrees of noise, two pairs corrupted: rotations, then positions with the rotation
    verdict as the mask, then the centres mapped onto the true ones by ``similarity_ransac``.  The bound is the largest residual
    of the NumPy reference's centres (from the same rotations) under the same map, times 1.1."""
    g = tr.end_to_end_case()
    R, rot_in, _, rot_view, _, _, rot_status, _ = hip.rotation_average(g.V, g.edges, g.rel, root=0, max_angle_deg=5.0, max_hyp=64, iters=2, steps=2)
    assert rot_status == 0 and not rot_view.any() and not rot_in[list(g.corrupted)].any()
    got = hip.translation_average(g.V, g.edges, R, g.t, edge_mask=rot_in, root=0, max_angle_deg=5.0, rounds=8, polish=1)
    c = tr.SimpleNamespace(V=g.V, edges=g.edges, R=R.reshape(-1, 9), t=g.t, mask=rot_in, root=0, cos_max=math.cos(math.radians(5.0)), mu=0.01,
                           rounds=8, polish=1, cg_tol=1e-13, cg_max=500)
    ref = tr.solve(c)
    check_against(ref, got, "end to end")
    assert got[6] == 0 and not got[4].any() and got[1].sum() == g.edges.shape[0] - len(g.corrupted)
    span = float(np.mean(np.linalg.norm(g.centres - g.centres.mean(axis=0), axis=1)))
    sim, inlier, _, _, status, _ = hip.similarity_ransac(np.array([0, g.V]), got[0].T.copy(), g.centres.T.copy(), (0.25 * span) ** 2, max_hyp=64, iters=2)
    assert status[0] == 0 and inlier.all()
    s, A, t = hip.split_similarity(sim[0])
    res_gpu = float(np.max(np.linalg.norm(s * got[0] @ A.T + t - g.centres, axis=1)))
    res_ref = float(np.max(np.linalg.norm(s * ref.C @ A.T + t - g.centres, axis=1)))
    print("end to end: largest residual %.4g (reference %.4g) = %.3g of the mean distance from the centroid" % (res_gpu, res_ref, res_gpu / span))
    assert res_gpu <= 1.1 * res_ref
