"""GPU tests of the rotation averaging: sfm_rotation_average, its _dev form and the Python entry points, against the float64
NumPy reference of tests/_rotavg_reference.py.

Decisions (status, best_hyp, n_inliers, every edge verdict, every view status, the summary -- and with it the number of rounds
that stood) are compared EXACTLY: tests/test_rotavg_host.py asserts that every case used here is settled in the reference.
R_out and edge_cos are compared at max(1e-9, 100 d_R), d_R being the disagreement of the reference's own two routes: the bound
comes from the reference alone.  The device runs with the reference's CG_TOL and CG_MAX."""
import math

import numpy as np
import pytest

import _rotavg_reference as rr
from _twoview_checks import same_bits

pytestmark = pytest.mark.gpu

KW = dict(cg_tol=rr.CG_TOL, cg_max=rr.CG_MAX)


def run(hip, c, **over):
    kw = dict(root=c.root, cos_max=c.cos_max, max_hyp=c.max_hyp, iters=c.iters, steps=c.steps)
    kw.update(KW)
    kw.update(over)
    return hip.rotation_average(c.V, c.edges, c.rel, **kw)


def check_against(ref, got, where="", bound=None, cg_limit=False):
    R, edge_inlier, edge_cos, view_status, n_inliers, best_hyp, status, summary = got
    bound = ref.bound if bound is None else bound
    assert ref.settled, where
    assert best_hyp == ref.best_hyp, where
    assert status == (ref.status | (rr.CG_LIMIT if cg_limit else 0)), where
    assert n_inliers == ref.n_inliers, where
    assert np.array_equal(edge_inlier, ref.edge_inlier), where
    assert np.array_equal(view_status, ref.view_status), where
    assert np.array_equal(summary, ref.summary), where
    err_R = float(np.max(np.abs(R - ref.R)))
    has = np.isfinite(ref.edge_cos)
    assert np.array_equal(np.isfinite(edge_cos), has), where
    err_c = float(np.max(np.abs(edge_cos[has] - ref.edge_cos[has]))) if has.any() else 0.0
    print("%s: |dR| %.3g |dcos| %.3g bound %.3g d_R %.3g" % (where, err_R, err_c, bound, ref.d_R))
    assert err_R <= bound and err_c <= bound, where


@pytest.mark.parametrize("name", sorted(rr.CASES))
def test_case_matches_reference(hip, name):
    c = rr.case(name)
    check_against(c.ref, run(hip, c), name)


@pytest.mark.parametrize("max_hyp", [1, 64, 65, 256])
def test_batches(hip, max_hyp):
    """A cap of 24 hypotheses' rotations per batch: 1, 3, 3 and 11 batches; the winner is carried across them."""
    c = rr.case("complete_12")
    ref = rr.solve(c, max_hyp=max_hyp)
    per = c.V * 72
    try:
        assert hip.rotation_plan(c.V, max_hyp, 24 * per) == (min(24, max_hyp), -(-max_hyp // 24))
        check_against(ref, run(hip, c, max_hyp=max_hyp), "max_hyp=%d" % max_hyp)
        capped = run(hip, c, max_hyp=max_hyp)
        hip.rotation_plan(c.V, max_hyp, 0)
        whole = run(hip, c, max_hyp=max_hyp)
        assert all(same_bits(np.asarray(a), np.asarray(b)) for a, b in zip(capped, whole))
    finally:
        hip.rotation_plan(c.V, max_hyp, 0)


@pytest.mark.parametrize("iters,steps", [(0, 1), (3, 1), (3, 3), (1, 3)])
def test_rounds_and_steps(hip, iters, steps):
    for name in ("complete_12", "parallel_edges", "two_components"):
        c = rr.case(name)
        ref = rr.solve(c, iters=iters, steps=steps)
        check_against(ref, run(hip, c, iters=iters, steps=steps), "%s iters=%d steps=%d" % (name, iters, steps))
        assert ref.summary[5] <= iters


def test_triangle_tie_goes_to_the_lower_hypothesis(hip):
    c = rr.case("triangle")
    assert len(set(k for k in c.ref.counts if k >= 0)) == 1 and c.ref.best_hyp == 0       # every tree counts 2: a tie
    got = run(hip, c)
    assert got[5] == 0 and got[4] == 2


def test_root_without_an_edge_has_no_model(hip):
    c = rr.case("two_components")
    lonely = c.V - 1                                         # a view that carries no edge
    ref = rr.solve(c, root=lonely)
    assert ref.status == rr.NO_MODEL and ref.settled
    got = run(hip, c, root=lonely)
    check_against(ref, got, "no model")
    assert not got[0].any() and got[5] == -1 and np.all(got[3] & rr.HELD)


def test_held_view(hip):
    c = rr.case("held")
    assert np.any(c.ref.view_status == rr.HELD)              # reached in the input graph, cut off by the final verdicts
    check_against(c.ref, run(hip, c), "held")


def test_round_that_does_not_stand(hip):
    c = rr.case("kept")
    assert c.ref.status & rr.KEPT_HYPOTHESIS
    check_against(c.ref, run(hip, c), "kept")


def test_cg_limit(hip):
    """cg_max = 1: the flag is set, the call succeeds, and the result is that of the reference's own CG route stopped after
    one iteration (the dense route is no yardstick for an unconverged solve): decisions equal, rotations within 1e-9."""
    c = rr.case("complete_12")
    ref = rr.run(c.V, c.edges, c.rel, c.root, c.cos_max, c.max_hyp, c.iters, c.steps, route="cg", cg_max=1)
    moved = [rr.run(c.V, c.edges, c.rel, c.root, c.cos_max, c.max_hyp, c.iters, c.steps, route="cg", cg_max=1, thr_scale=s)
             for s in (1 - rr.REL, 1 + rr.REL)]
    ref.settled = all(m.trace == ref.trace for m in moved)
    ref.d_R = 0.0
    assert ref.status & rr.CG_LIMIT
    check_against(ref, run(hip, c, cg_max=1), "cg_max=1", bound=1e-9)


def test_depths_in_global_memory(hip):
    """More views than the tree kernel keeps depths for in LDS (4 096)."""
    V = 4100
    rng = np.random.default_rng(5)
    c = rr.make_case("big", V, rr.topo_random(V, rng, 3 * V), 5, wrong_share=0.02, max_hyp=2, iters=1, steps=1)
    c.ref = rr.solve(c)
    check_against(c.ref, run(hip, c), "V=4100")


def test_permuted_embedding(hip):
    """The same graph with its views renumbered inside a larger numbering (the extra views carry no edge) and its edge ORDER
    kept, scored with the one hypothesis h = 0: the tree of h = 0 depends on edge numbers only, the products and the test are
    per edge, so R_out, edge_cos and every verdict are the permuted bits of the small call.  With iters = 0; the refit's sums
    run in view order and the other hypotheses draw their root from the view count, so nothing is claimed for them."""
    c = rr.case("complete_12")
    small = run(hip, c, max_hyp=1, iters=0)
    rng = np.random.default_rng(12)
    perm = rng.permutation(40)[:c.V]
    big = hip.rotation_average(40, perm[c.edges], c.rel, root=int(perm[c.root]), cos_max=c.cos_max, max_hyp=1, iters=0, steps=1, **KW)
    assert same_bits(big[0][perm], small[0]) and same_bits(big[1], small[1]) and same_bits(big[2], small[2])
    assert big[4:7] == small[4:7]
    rest = np.setdiff1d(np.arange(40), perm)
    assert not big[0][rest].any() and np.all(big[3][rest] == (rr.UNREACHED | rr.HELD)) and np.all(big[3][perm] == small[3])


def test_run_to_run_bits_and_absent_outputs(hip):
    c = rr.case("size_65_1025")
    a, b = run(hip, c), run(hip, c)
    assert all(same_bits(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
    kw = dict(root=c.root, cos_max=c.cos_max, max_hyp=c.max_hyp, iters=c.iters, steps=c.steps, **KW)
    only_R = hip.rotation_average(c.V, c.edges, c.rel, outputs=(), **kw)
    assert same_bits(only_R[0], a[0]) and all(v is None for v in only_R[1:])
    some = hip.rotation_average(c.V, c.edges, c.rel, outputs=("edge_cos", "summary"), **kw)
    assert same_bits(some[2], a[2]) and same_bits(some[7], a[7]) and some[1] is None and some[6] is None


def test_dev_form_matches_host_form(hip):
    import torch
    c = rr.case("size_65_1025")
    host = run(hip, c)
    dev = torch.device("cuda")
    E = c.edges.shape[0]
    d_rel = torch.from_numpy(c.rel).to(dev)
    d_R = torch.zeros(c.V, 9, dtype=torch.float64, device=dev)
    d_in = torch.zeros(E, dtype=torch.uint8, device=dev)
    d_cos = torch.zeros(E, dtype=torch.float64, device=dev)
    d_view = torch.zeros(c.V, dtype=torch.int32, device=dev)
    d_small = torch.zeros(3, dtype=torch.int32, device=dev)
    d_sum = torch.zeros(6, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    hip.rotation_average_dev(c.V, c.edges, d_rel.data_ptr(), root=c.root, cos_max=c.cos_max, max_hyp=c.max_hyp, iters=c.iters,
                             steps=c.steps, d_R_out=d_R.data_ptr(), d_edge_inlier=d_in.data_ptr(), d_edge_cos=d_cos.data_ptr(),
                             d_view_status=d_view.data_ptr(), d_n_inliers=d_small.data_ptr(), d_best_hyp=d_small.data_ptr() + 4,
                             d_status=d_small.data_ptr() + 8, d_summary=d_sum.data_ptr(), **KW)
    assert same_bits(d_R.cpu().numpy().reshape(c.V, 3, 3), host[0])
    assert same_bits(d_in.cpu().numpy(), host[1]) and same_bits(d_cos.cpu().numpy(), host[2]) and same_bits(d_view.cpu().numpy(), host[3])
    assert tuple(d_small.cpu().numpy().tolist()) == host[4:7] and same_bits(d_sum.cpu().numpy(), host[7])
    # only R_out; and a Rel that is no rotation is found on the device and named
    d_R2 = torch.zeros(c.V, 9, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    hip.rotation_average_dev(c.V, c.edges, d_rel.data_ptr(), root=c.root, cos_max=c.cos_max, max_hyp=c.max_hyp, iters=c.iters,
                             steps=c.steps, d_R_out=d_R2.data_ptr(), **KW)
    assert same_bits(d_R2.cpu().numpy(), d_R.cpu().numpy())
    bad = c.rel.copy()
    bad[7] *= 1.01
    bad[3] *= 1.01
    d_bad = torch.from_numpy(bad).to(dev)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="edge 3 "):
        hip.rotation_average_dev(c.V, c.edges, d_bad.data_ptr(), root=c.root, cos_max=c.cos_max, d_R_out=d_R2.data_ptr(), **KW)


def test_average_rotations_on_the_pose_pairs(hip, sfm):
    """The pairs of tests/_twoview_pose_reference.py as a view graph (tests/_rotavg_pairs.py): posed by ``initialise_pairs``,
    averaged by ``average_rotations``; every view is within depth x PAIR_DEG of its true rotation, the bound the pair poses
    themselves meet there, chained."""
    import _rotavg_pairs as rp
    P = sfm.processors
    g = rp.pose_graph()
    ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
    out = ep.initialise_pairs(g.sets, g.K)
    for o, (ref, que), R0 in zip(out, g.pairs, g.planted):
        assert o["best_cand"] >= 0 and np.abs(o["R"] - R0).max() < rp.PAIR_ENTRY         # the premise: what the pose tests assert
        o["ref"], o["que"] = ref, que
    hopeless = dict(out[0], best_cand=-1, R=np.zeros((3, 3)))                             # a pair without a pose is skipped
    cp = P.HipCamposeProcessor(None, 5, 25)
    rots, verdict = cp.average_rotations(out + [hopeless], g.n_views, root=0, max_angle_deg=g.max_angle_deg, max_hyp=16, iteration=2)
    assert verdict["pairs"] == [0, 1, 2, 3, 4] and verdict["status"] == 0 and verdict["edge_inlier"].all()
    assert np.array_equal(verdict["view_status"], np.zeros(4, dtype=np.int32)) and same_bits(rots[0], np.identity(3))
    for v in range(g.n_views):
        err = rp.angle_deg(rots[v].T, g.truth[v])
        print("view %d: %.3f degrees (bound %.2f)" % (v, err, g.depth[v] * g.pair_deg))
        assert err <= g.depth[v] * g.pair_deg
    triples = [(o["ref"], o["que"], o["R"]) for o in out]
    again, _ = cp.average_rotations(triples, g.n_views, root=0, max_angle_deg=g.max_angle_deg, max_hyp=16, iteration=2)
    assert all(same_bits(a, b) for a, b in zip(again, rots))
    with pytest.raises(ValueError):
        cp.average_rotations([hopeless], g.n_views)


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def test_orient_views_on_a_device_tracker(hip, sfm):
    """Four views of ``scenes.make_descriptor_views`` through a ``HipDeviceKeyTracker``: five pairs verified, posed and averaged.
    The keys are exact projections (six copies per view carry 0.5 px), the Sampson gate is 2 px at a focal length of 569 px,
    3.5e-3 rad = 0.2 degrees per match at the very most; a pose over more than a hundred such matches is held here to one
    degree per pair, and a view at tree depth d to d degrees."""
    P = sfm.processors
    dv = sfm.scenes.make_descriptor_views(n_views=4, n_pts=200, seed=0)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(4)]
    K = np.asarray(sfm.scenes.UPENN_K, dtype=np.float64)
    kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
    pairs = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    try:
        for v in range(4):
            kt.add_new_view(views[v], views[:v])
        rots, verdict, poses = P.orient_views(kt, pairs, K, max_angle_deg=2.0, tree_hyp=8, rounds=2)
    finally:
        kt.kt_release()
    assert len(poses) == 5 and all(p["R"] is not None for p in poses) and verdict["pairs"] == [0, 1, 2, 3, 4]
    assert verdict["status"] == 0 and verdict["edge_inlier"].all() and not verdict["view_status"].any()
    for v in range(4):
        want = np.asarray(dv.rots[v]) @ np.asarray(dv.rots[0]).T                        # view 0 is the gauge
        c = 0.5 * (np.trace(rots[v].T @ want) - 1.0)
        err = math.degrees(math.acos(min(1.0, c)))
        print("view %d: %.4f degrees" % (v, err))
        assert err <= 2.0                                                               # depth <= 2 from view 0
