"""GPU tests of the view-triplet filter: sfm_view_triplets, its _dev form and the Python entry points, against the float64
NumPy reference of tests/_triplets_reference.py.

Everything the call returns is an integer decision or an integer count (``lhs`` is no output), so every comparison here is
EXACT: tests/test_triplets_host.py asserts that every case used here is settled in the reference, a margin of 1e-6 relative
on every triplet where the fused products of the kernel differ from NumPy's by 1e-15."""
import gc
import math

import numpy as np
import pytest

import _rotavg_reference as rr
import _triplets_reference as tr
from _twoview_checks import same_bits

pytestmark = pytest.mark.gpu

GROUPS = (0, 1, 4, 8, 16, 32, 64)


def run(hip, c, **over):
    kw = dict(edge_mask=c.mask, cos_loop=c.cos_loop, min_ok=c.min_ok, min_pct=c.min_pct, keep_untested=c.keep_untested)
    kw.update(over)
    return hip.view_triplets(c.V, c.edges, c.rel, **kw)


def check_against(ref, got, where=""):
    edge_keep, n_tri, n_ok, kept_idx, summary = got
    assert ref.settled, where
    assert np.array_equal(n_tri, ref.n_tri), where
    assert np.array_equal(n_ok, ref.n_ok), where
    assert np.array_equal(edge_keep, ref.edge_keep), where
    assert kept_idx.dtype == np.int32 and np.array_equal(kept_idx, ref.kept_idx), where
    assert np.array_equal(summary, ref.summary), where


@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_case_matches_reference(hip, name):
    c = tr.case(name)
    check_against(c.ref, run(hip, c), name)


@pytest.mark.parametrize("name", ["parallel_222", "complete_12", "hubs_65", "hubs_1030", "band_E1025", "two_components", "masked_5"])
def test_every_group_width_gives_the_same_bits(hip, name):
    c = tr.case(name)
    for group in GROUPS:
        check_against(c.ref, run(hip, c, group=group), "%s group=%d" % (name, group))


@pytest.mark.parametrize("limit", [1, 32])
def test_small_devices_give_the_same_bits(hip, limit):
    """The grids are capped by the compute units the plans see (64 workgroups per unit for the enumeration, 4 for the
    summary): with one unit 16 389 edges at 64 lanes each are 65 turns of the enumeration's grid-stride loop, which the
    whole device never takes at these sizes."""
    gc.collect()                          # no handle of an earlier test waiting for the collector: the limit is refused while one lives
    try:
        hip.set_cu_limit(limit)
        for name, group in (("band_E16389", 64), ("band_E16389", 0), ("hubs_1030", 4), ("band_E2049", 1), ("complete_12", 64)):
            c = tr.case(name)
            check_against(c.ref, run(hip, c, group=group), "%s group=%d limit=%d" % (name, group, limit))
    finally:
        hip.set_cu_limit(0)
    dev, eff = hip.cu_count()
    assert eff == dev


def test_thresholds_of_the_verdict(hip):
    c = tr.case("k5_two_wrong")
    seen = set()
    for v in tr.VARIANTS["k5_two_wrong"]:
        ref = tr.solve(c, **v)
        check_against(ref, run(hip, c, **v), str(v))
        seen.add(tuple(ref.edge_keep.tolist()))
    assert len(seen) == 3                                     # the options differ on this case
    assert same_bits(run(hip, c, min_ok=0)[0], run(hip, c, min_ok=1)[0])               # 0 means 1


def test_edge_mask(hip):
    c = tr.case("masked_5")
    free = tr.solve(c, mask=None)
    check_against(free, run(hip, c, edge_mask=None), "no mask")
    got = run(hip, c)
    check_against(c.ref, got, "masked")
    assert got[0][0] == 0 and got[1][0] == 0 and got[4][6] == 1 and got[4][0] == free.summary[0] - 3
    everything = np.zeros(c.edges.shape[0], dtype=np.uint8)
    ref = tr.solve(c, mask=everything, keep_untested=1)
    check_against(ref, run(hip, c, edge_mask=everything, keep_untested=1), "all masked")
    assert ref.kept_idx.size == 0 and ref.summary.tolist() == [0, 0, 0, 0, 0, 0, 10, 0]


def test_run_to_run_bits_and_absent_outputs(hip):
    c = tr.case("band_E2049")
    a, b = run(hip, c), run(hip, c)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    none = run(hip, c, outputs=())
    assert all(v is None for v in none)
    some = run(hip, c, outputs=("kept_idx", "summary"))
    assert same_bits(some[3], a[3]) and same_bits(some[4], a[4]) and some[0] is None and some[1] is None and some[2] is None
    counts = run(hip, c, outputs=("n_ok",))
    assert same_bits(counts[2], a[2]) and counts[3] is None


def test_kept_idx_beyond_the_count_is_not_written(hip):
    c = tr.case("complete_12")
    lib = hip.load()
    E = c.edges.shape[0]
    kept = np.full(E, -7, dtype=np.int32)
    n_kept = np.zeros(1, dtype=np.int32)
    hip.check(lib.sfm_view_triplets(c.V, E, hip.iptr(c.edges), hip.dptr(c.rel), None, c.cos_loop, 1, 0, 0, 0, None, None, None,
                                    hip.iptr(kept), None, hip.iptr(n_kept)))
    n = int(n_kept[0])
    assert n == c.ref.kept_idx.size == E - 3 and np.array_equal(kept[:n], c.ref.kept_idx) and np.all(kept[n:] == -7)


@pytest.mark.parametrize("name", ["band_E1025", "band_E16389", "hubs_200"])
def test_dev_form_matches_host_form(hip, name):
    import torch
    c = tr.case(name)
    host = run(hip, c)
    check_against(c.ref, host, name)
    dev = torch.device("cuda")
    E = c.edges.shape[0]
    d_rel = torch.from_numpy(c.rel).to(dev)
    d_keep = torch.full((E,), 7, dtype=torch.uint8, device=dev)
    d_tri = torch.full((E,), -7, dtype=torch.int64, device=dev)
    d_ok = torch.full((E,), -7, dtype=torch.int64, device=dev)
    d_idx = torch.full((E,), -7, dtype=torch.int32, device=dev)
    d_sum = torch.full((8,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    n_kept = hip.view_triplets_dev(c.V, c.edges, d_rel.data_ptr(), cos_loop=c.cos_loop, d_edge_keep=d_keep.data_ptr(),
                                   d_n_tri=d_tri.data_ptr(), d_n_ok=d_ok.data_ptr(), d_kept_idx=d_idx.data_ptr(), d_summary=d_sum.data_ptr())
    assert n_kept == host[3].size
    assert same_bits(d_keep.cpu().numpy(), host[0]) and same_bits(d_tri.cpu().numpy(), host[1]) and same_bits(d_ok.cpu().numpy(), host[2])
    idx = d_idx.cpu().numpy()
    assert same_bits(idx[:n_kept], host[3]) and np.all(idx[n_kept:] == -7) and same_bits(d_sum.cpu().numpy(), host[4])
    # only kept_idx, with a mask on the device
    mask = np.ones(E, dtype=np.uint8)
    mask[::7] = 0
    ref = tr.solve(c, mask=mask)
    assert ref.settled
    d_mask = torch.from_numpy(mask).to(dev)
    d_idx2 = torch.full((E,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    n2 = hip.view_triplets_dev(c.V, c.edges, d_rel.data_ptr(), d_mask.data_ptr(), cos_loop=c.cos_loop, d_kept_idx=d_idx2.data_ptr())
    assert n2 == ref.kept_idx.size and np.array_equal(d_idx2.cpu().numpy()[:n2], ref.kept_idx)


def test_a_bad_rotation_is_found_on_the_device(hip):
    import torch
    c = tr.case("complete_12")
    dev = torch.device("cuda")
    bad = c.rel.copy()
    bad[7] *= 1.01
    bad[3] *= 1.01
    d_bad = torch.from_numpy(bad).to(dev)
    d_keep = torch.full((c.edges.shape[0],), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="edge 3 "):
        hip.view_triplets_dev(c.V, c.edges, d_bad.data_ptr(), cos_loop=c.cos_loop, d_edge_keep=d_keep.data_ptr())
    assert np.all(d_keep.cpu().numpy() == 7)                  # nothing else was launched
    with pytest.raises(ValueError, match="edge 3 "):
        hip.view_triplets(c.V, c.edges, bad)


def test_permuted_edges_and_views(hip):
    """The definition does not depend on order: the edges shuffled and the views renumbered give the permuted counts.  (A
    renumbering moves a, b, c of a triplet, so its products are formed in another order: the counts are equal because the case
    stays settled, which the reference confirms for the renumbered graph itself.)"""
    c = tr.case("complete_12")
    rng = np.random.default_rng(12)
    order, perm = rng.permutation(c.edges.shape[0]), rng.permutation(40)[:c.V]
    shuffled = hip.view_triplets(c.V, c.edges[order], c.rel[order], cos_loop=c.cos_loop)
    assert np.array_equal(shuffled[1], c.ref.n_tri[order]) and np.array_equal(shuffled[2], c.ref.n_ok[order])
    assert np.array_equal(shuffled[0], c.ref.edge_keep[order])
    big = SimpleCase(40, perm[c.edges].astype(np.int32), c.rel, c)
    ref = tr.solve(big)
    assert ref.settled and np.array_equal(ref.n_ok, c.ref.n_ok)
    check_against(ref, run(hip, big), "renumbered")


class SimpleCase:
    def __init__(self, V, edges, rel, like):
        self.V, self.edges, self.rel = V, edges, rel
        self.mask, self.cos_loop, self.min_ok, self.min_pct, self.keep_untested = like.mask, like.cos_loop, like.min_ok, like.min_pct, like.keep_untested


# ---- the route ---------------------------------------------------------------------------------------------------------------
def test_average_rotations_with_the_filter_equals_the_reference_chain(hip, sfm):
    P = sfm.processors
    c, rot = tr.band_chain()
    kept = c.ref.kept_idx
    triples = [(int(i), int(j), c.rel[e].reshape(3, 3)) for e, (i, j) in enumerate(c.edges)]
    hopeless = (0, 1, None)                                    # a pair without a pose is skipped, before the filter too
    cp = P.HipCamposeProcessor(None, 5, 25)
    rots, verdict = cp.average_rotations(triples[:5] + [hopeless] + triples[5:], c.V, root=0, max_angle_deg=c.max_angle_deg, max_hyp=128,
                                         iteration=2, triplets=dict(max_loop_deg=c.max_loop_deg, min_ok=1))
    E = c.edges.shape[0]
    assert verdict["pairs"] == list(range(5)) + list(range(6, E + 1))
    t = verdict["triplets"]
    assert t["pairs"] == verdict["pairs"] and np.array_equal(t["edge_keep"], c.ref.edge_keep.astype(bool))
    assert np.array_equal(t["n_tri"], c.ref.n_tri) and np.array_equal(t["n_ok"], c.ref.n_ok) and np.array_equal(t["kept_idx"], kept)
    assert [t["summary"][k] for k in sfm.native.TRIPLET_SUMMARY] == c.ref.summary.tolist()
    full = np.zeros(E, dtype=bool)
    full[kept] = rot.edge_inlier.astype(bool)
    assert rot.settled and np.array_equal(verdict["edge_inlier"], full)
    assert np.array_equal(full, ~c.replaced & c.ref.edge_keep.astype(bool))             # exactly the clean edges the filter kept
    assert np.array_equal(np.isfinite(verdict["edge_cos"]), c.ref.edge_keep.astype(bool))
    assert verdict["status"] == rot.status == 0 and verdict["best_hyp"] == rot.best_hyp and verdict["n_inliers"] == rot.n_inliers
    assert np.array_equal(verdict["view_status"], rot.view_status) and np.array_equal(verdict["summary"], rot.summary)
    err = max(float(np.max(np.abs(rots[v].T - rot.R[v]))) for v in range(c.V) if rots[v] is not None)
    print("|dR| %.3g bound %.3g" % (err, rot.bound))
    assert err <= rot.bound and [r is None for r in rots] == [bool(s & rr.UNREACHED) for s in rot.view_status]
    # filter_view_graph alone: keep per ENTRY
    keep, alone = cp.filter_view_graph(triples[:5] + [hopeless] + triples[5:], c.V, max_loop_deg=c.max_loop_deg)
    assert keep.shape == (E + 1,) and not keep[5] and np.array_equal(np.delete(keep, 5), c.ref.edge_keep.astype(bool))
    assert np.array_equal(alone["n_ok"], c.ref.n_ok) and cp.triplets_last is alone
    # without the filter the same call is the unfiltered averaging, which this graph defeats
    plain, plain_verdict = cp.average_rotations(triples, c.V, root=0, max_angle_deg=c.max_angle_deg, max_hyp=128, iteration=2)
    assert "triplets" not in plain_verdict and not np.array_equal(plain_verdict["edge_inlier"], ~c.replaced)
    with pytest.raises(ValueError, match="unknown"):
        cp.average_rotations(triples, c.V, triplets=dict(loop=5.0))


def test_triplets_none_is_the_call_without_the_argument(hip, sfm):
    P = sfm.processors
    c = rr.case("complete_12")
    triples = [(int(i), int(j), c.rel[e].reshape(3, 3)) for e, (i, j) in enumerate(c.edges)]
    cp = P.HipCamposeProcessor(None, 5, 25)
    a, va = cp.average_rotations(triples, c.V, root=0, max_angle_deg=c.max_angle_deg, max_hyp=16, iteration=2)
    b, vb = cp.average_rotations(triples, c.V, root=0, max_angle_deg=c.max_angle_deg, max_hyp=16, iteration=2, triplets=None)
    direct = hip.rotation_average(c.V, c.edges, c.rel, root=0, max_angle_deg=c.max_angle_deg, max_hyp=16, iters=2, steps=2)
    assert all(same_bits(x, y) and same_bits(x, R.T) for x, y, R in zip(a, b, direct[0]))
    assert sorted(va) == sorted(vb) and "triplets" not in vb
    for k in va:
        assert same_bits(np.asarray(va[k]), np.asarray(vb[k])), k
    assert same_bits(vb["edge_inlier"], direct[1].astype(bool)) and same_bits(vb["edge_cos"], direct[2])


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def test_orient_views_with_the_filter_on_a_device_tracker(hip, sfm):
    """The four views and five pairs of tests/test_gpu_rotavg.py's tracker: the pairs form the triangles (0, 1, 2) and
    (1, 2, 3), whose poses are held to a degree per pair, so a loop of 5 degrees keeps all five and the averaging behind the
    filter is the averaging without it, bit for bit; with one pair's pose replaced the filter drops what hangs on it."""
    P = sfm.processors
    dv = sfm.scenes.make_descriptor_views(n_views=4, n_pts=200, seed=0)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(4)]
    K = np.asarray(sfm.scenes.UPENN_K, dtype=np.float64)
    kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
    pairs = [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]
    try:
        for v in range(4):
            kt.add_new_view(views[v], views[:v])
        rots0, verdict0, poses0 = P.orient_views(kt, pairs, K, max_angle_deg=2.0, tree_hyp=8, rounds=2)
        rots, verdict, poses = P.orient_views(kt, pairs, K, max_angle_deg=2.0, tree_hyp=8, rounds=2, triplets=dict(max_loop_deg=5.0))
    finally:
        kt.kt_release()
    t = verdict["triplets"]
    assert t["edge_keep"].all() and t["n_tri"].tolist() == [1, 1, 2, 1, 1] and t["n_ok"].tolist() == [1, 1, 2, 1, 1]
    assert t["summary"]["triplets"] == 2 and t["summary"]["edges_kept"] == 5 and verdict["pairs"] == [0, 1, 2, 3, 4]
    assert verdict["status"] == 0 and verdict["edge_inlier"].all() and "triplets" not in verdict0
    assert all(same_bits(a, b) for a, b in zip(rots, rots0)) and same_bits(verdict["edge_cos"], verdict0["edge_cos"])
    # the poses the tracker gave, pair (1, 3) turned by 40 degrees: its triangle breaks, the other one stands
    triples = [(p["ref"], p["que"], p["R"]) for p in poses]
    triples[3] = (1, 3, rr.so3_exp(np.array([0.0, math.radians(40.0), 0.0])) @ triples[3][2])
    keep, broken = P.HipCamposeMixin().filter_view_graph(triples, 4, max_loop_deg=5.0)
    assert keep.tolist() == [True, True, True, False, False] and broken["n_ok"].tolist() == [1, 1, 1, 0, 0]
