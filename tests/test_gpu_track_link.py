"""Track linking on the device (csrc/sfm_track_link.hip) against the rule in NumPy (tests/_track_link_reference.py): every
output is an integer or a gathered bit pattern, so every comparison is exact.  The cases, and what each is there for, are
listed in the reference module; tests/test_track_link_host.py asserts that each is settled (two label routes agree)."""
import gc

import numpy as np
import pytest

import _track_link_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _limit_back_to_none(hip):
    gc.collect()                          # no handle of an earlier test waiting for the collector: the limit is refused while one lives
    yield
    gc.collect()
    hip.set_cu_limit(0)
    dev, eff = hip.cu_count()
    assert eff == dev


def run(hip, case, **kw):
    args = dict(mask=case.get("mask"), min_len=case.get("min_len", 2))
    args.update(kw)
    return hip.track_link(case["key_ptr"], case["pair_views"], case["pair_ptr"], case["a"], case["b"], **args)


def assert_same(got, want, what):
    for name in ref.OUTPUTS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_every_case_equals_the_rule(hip, name):
    case, want = ref.settled(name)
    assert_same(run(hip, case), want, name)


@pytest.mark.parametrize("name", ["tracks_1023", "tracks_1024", "tracks_1025", "tracks_2049", "keys_1023", "keys_1024", "keys_1025", "keys_2049",
                                  "scene_70_2", "m_65537"])
def test_both_scan_routes_give_the_same_bits(hip, name):
    case, want = ref.settled(name)
    K = int(case["key_ptr"][-1])
    for scan in (hip.LINK_SCAN_ONE_BLOCK, hip.LINK_SCAN_DEVICE):
        plan = hip.track_link_plan(case["key_ptr"].size - 1, K, int(case["pair_ptr"][-1]), scan=scan)
        assert plan["scan_keys"] == (scan if K > 1024 else 1) and plan["scan_components"] == (scan if K // 2 > 1024 else 1)
        assert_same(run(hip, case, scan=scan), want, (name, scan))


@pytest.mark.parametrize("name", ["scene_12_2", "scene_70_10", "through_65", "through_1100", "conflict_small", "min_len_3"])
def test_every_group_width_gives_the_same_bits(hip, name):
    case, want = ref.settled(name)
    for group in hip.TRACK_GROUPS[1:]:
        assert_same(run(hip, case, group=group), want, (name, group))


@pytest.mark.parametrize("limit", [1, 32])
def test_small_devices_give_the_same_bits(hip, limit):
    hip.set_cu_limit(limit)
    for name in ("scene_70_2", "m_65537", "conflict_by_counting", "through_1100", "tracks_2049"):
        case, want = ref.settled(name)
        plan = hip.track_link_plan(case["key_ptr"].size - 1, int(case["key_ptr"][-1]), int(case["pair_ptr"][-1]))
        assert plan["union_grid"] <= 16 * limit and plan["order_grid"] <= 32 * limit and plan["big_grid"] <= 4 * limit
        assert_same(run(hip, case), want, (name, limit))


def test_a_different_listing_gives_the_same_bits(hip):
    for name in ("scene_12_2", "scene_70_10", "duplicates", "mask_split"):
        case, want = ref.settled(name)
        for seed, kw in ((1, dict(pairs=False, orientation=False)), (2, dict(matches=False, orientation=False)),
                         (3, dict(matches=False, pairs=False)), (4, {})):
            assert_same(run(hip, ref.permuted(case, seed, **kw)), want, (name, seed))


def test_run_to_run_and_device_form_identity(hip):
    import torch
    case, want = ref.settled("scene_70_10")
    first = run(hip, case)
    for _ in range(3):
        assert_same(run(hip, case), first, "run to run")
    K, M = int(case["key_ptr"][-1]), int(case["pair_ptr"][-1])
    mask = (np.random.default_rng(5).random(M) < 0.8).astype(np.uint8)
    masked = dict(case, mask=mask)
    want_masked = ref.settle(masked)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_a, d_b, d_mask = dev(case["a"]), dev(case["b"]), dev(mask)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        outs = {name: torch.full((n,), -7, dtype=torch.int64 if name == "summary" else torch.int32, device="cuda")
                for name, n in (("key_track", K), ("pt_ptr", K // 2 + 2), ("cam_idx", K), ("key_idx", K), ("summary", 8), ("label", K))}
        stream.synchronize()
        n_tracks, n_obs = hip.track_link_dev(case["key_ptr"], case["pair_views"], case["pair_ptr"], d_a.data_ptr(), d_b.data_ptr(), d_mask.data_ptr(),
                                             d_key_track=outs["key_track"].data_ptr(), d_pt_ptr=outs["pt_ptr"].data_ptr(),
                                             d_cam_idx=outs["cam_idx"].data_ptr(), d_key_idx=outs["key_idx"].data_ptr(),
                                             d_summary=outs["summary"].data_ptr(), d_label=outs["label"].data_ptr(), stream=stream.cuda_stream)
    got = {name: t.cpu().numpy() for name, t in outs.items()}
    assert (n_tracks, n_obs) == (int(want_masked["summary"][2]), int(want_masked["summary"][5]))
    # what lies beyond the defined part is as the caller left it
    assert np.all(got["pt_ptr"][n_tracks + 1:] == -7) and np.all(got["cam_idx"][n_obs:] == -7) and np.all(got["key_idx"][n_obs:] == -7)
    got["pt_ptr"], got["cam_idx"], got["key_idx"] = got["pt_ptr"][:n_tracks + 1], got["cam_idx"][:n_obs], got["key_idx"][:n_obs]
    assert_same(got, want_masked, "device form")
    assert_same(run(hip, masked), want_masked, "host form, masked")
    # no mask, no outputs but the counts
    assert hip.track_link_dev(case["key_ptr"], case["pair_views"], case["pair_ptr"], d_a.data_ptr(), d_b.data_ptr()) == (
        int(want["summary"][2]), int(want["summary"][5]))


def test_absent_outputs(hip):
    case, want = ref.settled("scene_12_2")
    for outputs in (("key_track",), ("cam_idx",), ("pt_ptr", "key_idx"), ("label", "summary"), ()):
        got = run(hip, case, outputs=outputs)
        for name in ref.OUTPUTS:
            if name in outputs:
                assert np.array_equal(got[name], want[name]), (outputs, name)
            else:
                assert got[name] is None
    with pytest.raises(ValueError, match="outputs"):
        run(hip, case, outputs=("tracks",))


def test_the_device_form_names_the_lowest_bad_match_and_writes_nothing(hip):
    import torch
    case, _ = ref.settled("scene_12_2")
    K, M = int(case["key_ptr"][-1]), int(case["pair_ptr"][-1])
    n_keys = np.diff(case["key_ptr"])
    pair_of = np.repeat(np.arange(case["pair_views"].shape[0]), np.diff(case["pair_ptr"]))
    a, b = case["a"].copy(), case["b"].copy()
    lowest = 1500
    b[lowest] = n_keys[case["pair_views"][pair_of[lowest], 1]]               # one past the view
    a[lowest + 700] = -1
    a[M - 1] = n_keys[case["pair_views"][pair_of[M - 1], 0]] + 5
    mask = np.ones(M, dtype=np.uint8)
    mask[lowest] = 0                                                       # a masked match is checked like a used one
    d_a, d_b, d_mask = (torch.from_numpy(x).cuda() for x in (a, b, mask))
    outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for n in (K, K // 2 + 2, K, K, K)]
    d_sum = torch.full((8,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="match %d names a key outside its view" % lowest):
        hip.track_link_dev(case["key_ptr"], case["pair_views"], case["pair_ptr"], d_a.data_ptr(), d_b.data_ptr(), d_mask.data_ptr(),
                           d_key_track=outs[0].data_ptr(), d_pt_ptr=outs[1].data_ptr(), d_cam_idx=outs[2].data_ptr(),
                           d_key_idx=outs[3].data_ptr(), d_summary=d_sum.data_ptr(), d_label=outs[4].data_ptr())
    assert all(bool((t == -7).all()) for t in outs + [d_sum])
    with pytest.raises(ValueError, match="match %d " % lowest):
        hip.track_link(case["key_ptr"], case["pair_views"], case["pair_ptr"], a, b)


# ---- the store form ------------------------------------------------------------------------------------------------------
def _store_of(hip, case, seed):
    """A TrackStore holding the case's views (random coordinates) and its matches, one sfm_match_guided_set_pairs per pair: a
    key is kept once per pair, and a match with query key 0 is written but is no match (quirk Q3)."""
    rng = np.random.default_rng(seed)
    n_keys = np.diff(case["key_ptr"])
    store = hip.TrackStore()
    norm = []
    for n in n_keys:
        store.add_view(rng.uniform(0, 1000, (int(n), 2)))
        norm.append(rng.standard_normal((2, int(n))))
        store.set_normalised(store.n_views - 1, norm[-1])
    pairs = []
    for p, (r, q) in enumerate(case["pair_views"]):
        a, b = case["a"][case["pair_ptr"][p]:case["pair_ptr"][p + 1]], case["b"][case["pair_ptr"][p]:case["pair_ptr"][p + 1]]
        _, first_a = np.unique(a, return_index=True)
        keep = np.zeros(a.size, dtype=bool)
        keep[first_a] = True
        _, first_b = np.unique(np.where(keep, b, -1 - np.arange(b.size)), return_index=True)
        once = np.zeros(a.size, dtype=bool)
        once[first_b] = True
        keep &= once
        store.set_pairs(int(r), int(q), a[keep], b[keep])
        pairs.append((int(r), int(q)))
    return store, pairs, norm


def test_the_store_form_equals_the_array_form_and_feeds_the_bundle_adjustment(hip):
    import torch
    case, _ = ref.settled("scene_12_2")
    store, pairs, norm = _store_of(hip, case, 7)
    with store:
        rng = np.random.default_rng(8)
        total = int(case["key_ptr"][-1])
        for key_mask in (None, (rng.random(sum(store.n_keys(r) for r, _ in pairs)) < 0.85).astype(np.uint8)):
            # the array form fed from what sfm_track_pairs returns
            a, b, m, ptr, off = [], [], [], [0], 0
            for r, q in pairs:
                r_idx, q_idx, _, _ = store.pairs(r, q)
                a.append(r_idx); b.append(q_idx); ptr.append(ptr[-1] + r_idx.size)
                if key_mask is not None:
                    m.append(key_mask[off + r_idx])
                off += store.n_keys(r)
            fed = dict(key_ptr=case["key_ptr"], pair_views=np.array(pairs, dtype=np.int32), pair_ptr=np.array(ptr, dtype=np.int64),
                       a=np.concatenate(a), b=np.concatenate(b), mask=None if key_mask is None else np.concatenate(m), min_len=3)
            assert fed["a"].size < int(case["pair_ptr"][-1])                    # query key 0 and repeated keys are gone
            want = ref.settle(fed)
            assert_same(run(hip, fed), want, "array form")
            tables = [store.table(v).copy() for v in range(store.n_views)]
            d_track = torch.full((total,), -7, dtype=torch.int32, device="cuda")
            up = store.upload_bytes
            summary = store.link(pairs, key_mask, 3, d_track.data_ptr())
            assert store.upload_bytes - up == (0 if key_mask is None else key_mask.size)          # the mask is the only upload
            assert np.array_equal(summary, want["summary"]) and np.array_equal(d_track.cpu().numpy(), want["key_track"])
            assert all(np.array_equal(store.table(v), tables[v]) for v in range(store.n_views))   # no table is written
            n_tracks, n_obs = int(want["summary"][2]), int(want["summary"][5])
            assert (store.info(hip.TRACK_INFO_OBS_VIEWS), store.info(hip.TRACK_INFO_OBS_PTS), store.info(hip.TRACK_INFO_N_OBS)) == (
                store.n_views, n_tracks, n_obs)
            pt_ptr, cam, key, uv = store.observations()
            assert np.array_equal(pt_ptr, want["pt_ptr"]) and np.array_equal(cam, want["cam_idx"]) and np.array_equal(key, want["key_idx"])
            want_uv = np.stack([np.array([norm[c][0, k] for c, k in zip(cam, key)]), np.array([norm[c][1, k] for c, k in zip(cam, key)])])
            assert np.array_equal(uv.view(np.int64), want_uv.view(np.int64))                     # gathered bit patterns
            with hip.BaProblem.from_tracks(store) as prob:
                s_ptr, s_cam, s_uv = prob.structure()
                assert prob.info(hip.INFO_N_CAMS) == store.n_views
                assert np.array_equal(s_ptr, pt_ptr) and np.array_equal(s_cam, cam) and np.array_equal(s_uv.view(np.int64), uv.view(np.int64))
        # refusals leave the list as it is
        for bad, word in (([(0, 0)], "pair 0 "), ([(0, 99)], "view 99"), ([(-1, 2)], "view -1")):
            with pytest.raises(ValueError, match=word):
                store.link(bad)
        with pytest.raises(ValueError, match="min_len"):
            store.link(pairs, None, 1)
        with pytest.raises(ValueError, match="key_mask"):
            store.link(pairs, np.ones(3, dtype=np.uint8))
        assert store.info(hip.TRACK_INFO_OBS_PTS) == n_tracks and np.array_equal(store.observations()[1], cam)
        v = store.add_view(np.zeros((4, 2)))                                    # keys, but no normalised coordinates
        with pytest.raises(ValueError, match="view %d has no normalised" % v):
            store.link(pairs + [(0, v)])
        assert store.link(pairs, None, 3)[2] > 0                                # a view that no pair names needs none


# ---- end to end ----------------------------------------------------------------------------------------------------------
PIXEL_NOISE, FALSE_PER_PAIR, CORRUPTED = 0.5, 4, (4, 17)


def _eight_views(sfm, seed):
    """Eight views, all 28 pairs, two of them corrupted -- the graph of the translation averaging's end-to-end case, with keys.
    Its random rotations cannot look at one scene, so the eight views here stand on an arc and look at one cloud of 400
    points; the noise of the poses is what 0.5 px of key noise makes of them.  A view sees a point with 70 %; key 0 of every
    view and a tenth of the others see nothing.  A pair matches the points both views see with 90 % and carries four false
    matches between keys it does not use otherwise.  A corrupted pair matches its reference keys to EXTRA keys of its query
    view: the scene seen from a pose 20 degrees and a baseline away, keys that no other pair names -- a consistent and
    wrong relative pose, which is what the rotation averaging has to flag."""
    rng = np.random.default_rng(seed)
    from scipy.spatial.transform import Rotation
    K = np.asarray(sfm.scenes.UPENN_K, dtype=np.float64)
    V, N = 8, 400
    X = np.vstack((rng.uniform(-4, 4, N), rng.uniform(-3, 3, N), rng.uniform(9, 15, N)))
    locs = [np.array([6.0 * np.sin(t), rng.uniform(-1.0, 1.0), 6.0 - 6.0 * np.cos(t)]) for t in np.linspace(-0.6, 0.6, V)]
    locs[0], rots = np.zeros(3), []
    for v in range(V):
        z = np.array([0.0, 0.0, 12.0]) - locs[v]
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        look = np.stack((x, np.cross(z, x), z), axis=1)
        rots.append(np.identity(3) if v == 0 else look @ Rotation.from_rotvec(rng.normal(0.0, 0.03, 3)).as_matrix())

    def project(rot, loc, pts):
        cam = K @ (rot.T @ (pts - loc.reshape(3, 1)))
        return (cam[0:2] / cam[2:3]).T

    pairs = [(i, j) for i in range(V) for j in range(i + 1, V)]
    sees = rng.random((V, N)) < 0.7
    xy, key_point, key_of = [], [], []
    for v in range(V):
        pts = np.flatnonzero(sees[v])
        n = 1 + pts.size + pts.size // 10
        slot = 1 + rng.permutation(n - 1)[:pts.size]
        coords = rng.uniform(0, 1000, (n, 2))
        coords[slot] = project(rots[v], locs[v], X[:, pts]) + rng.normal(0.0, PIXEL_NOISE, (pts.size, 2))
        kp, ko = np.full(n, -1), np.full(N, -1)
        kp[slot], ko[pts] = pts, slot
        xy.append(coords); key_point.append(kp); key_of.append(ko)
    matches = []
    for p, (r, q) in enumerate(pairs):
        both = np.flatnonzero(sees[r] & sees[q])
        both = both[rng.random(both.size) < 0.9]
        a, b = key_of[r][both], key_of[q][both]
        if p in CORRUPTED:
            turn = Rotation.from_rotvec([0.0, np.radians(20.0), 0.0]).as_matrix()
            extra = project(rots[q] @ turn, locs[q] + np.array([0.0, 2.0, 1.0]), X[:, both]) + rng.normal(0.0, PIXEL_NOISE, (both.size, 2))
            b = xy[q].shape[0] + np.arange(both.size)
            xy[q] = np.vstack((xy[q], extra))
            key_point[q] = np.concatenate((key_point[q], np.full(both.size, -2)))
        matches.append([a, b])
    for p, (r, q) in enumerate(pairs):                                      # the false matches, once every view has all its keys
        a, b = matches[p]
        free_a = np.setdiff1d(np.arange(1, xy[r].shape[0]), a)
        free_b = np.setdiff1d(np.arange(1, xy[q].shape[0]), b)
        matches[p] = (np.concatenate((a, rng.choice(free_a, FALSE_PER_PAIR, replace=False))),
                      np.concatenate((b, rng.choice(free_b, FALSE_PER_PAIR, replace=False))))
    return dict(K=K, V=V, X=X, rots=rots, locs=locs, pairs=pairs, xy=xy, key_point=np.concatenate(key_point), matches=matches)


def _dlt(projs, uvs):
    rows = []
    for proj, (u, v) in zip(projs, uvs):
        rows += [u * proj[2] - proj[0], v * proj[2] - proj[1]]
    x = np.linalg.svd(np.array(rows))[2][-1]
    return (x / x[3]).reshape(4, 1)


def test_reconstruct_views_end_to_end(hip, sfm, oracle):
    """Matched views to an adjusted scene.  The two corrupted pairs are flagged, no kept track mixes two scene points (the
    generator's ground truth), and the reprojection RMSE over the kept observations is at most 1.1 x what the CPU route
    reaches on the same input: the NumPy reference linking, a DLT and oracle.nonlinear_triangulate per track and
    oracle.ba_sparse, from the same averaged rotations and centres, with the same damping and iteration count.  The 10 %
    cover the different-but-equivalent arithmetic of the two adjustment routes.  Measured on an MI355X: see the figures in
    DESIGN.md section 39."""
    P = sfm.processors
    g = _eight_views(sfm, 39)
    kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
    kt._store = hip.TrackStore()
    for v in range(g["V"]):
        kt._store.add_view(g["xy"][v])
        kt._xy.append(g["xy"][v]); kt._versions.append(0)
        kt.track_list.append(P.HipDeviceKeyTrack(kt, v, g["xy"][v].shape[0]))
    try:
        for (r, q), (a, b) in zip(g["pairs"], g["matches"]):
            kt._store.set_pairs(r, q, a, b)
        LAM, ITERS = 1.0, 10             # a fixed damping: at 5 the point blocks (of the order of 0.1 in normalised units) hardly move, below 0.1 the gauge drifts
        for v in range(g["V"]):
            kt._store.set_normalised(v, sfm.geometry.normalise_pixels(g["xy"][v].T, g["K"]))
        out = P.reconstruct_views(kt, g["pairs"], g["K"], lam=LAM, iters=ITERS, set_normalised=False, max_angle_deg=3.0, max_direction_deg=5.0)
        # the linking alone, once more: the per-key mask is the only upload, one byte per key of every pair's reference view
        up = kt._store.upload_bytes
        summary, key_track = P.link_views(kt, g["pairs"], [(e["r_idx"], e["inlier"]) for e in out["poses"]], out["pair_mask"])
        mask_bytes, n_ref_keys = kt._store.upload_bytes - up, sum(g["xy"][r].shape[0] for r, _ in g["pairs"])
        assert summary == out["summary"] and np.array_equal(key_track, out["key_track"])
        pt_ptr, cam_idx, key_idx, _ = kt._store.observations()
        again = P.reconstruct_views(kt, g["pairs"], g["K"], lam=LAM, iters=ITERS, solver="pcg", retriangulate_px=4.0, cull_px=4.0,
                                    set_normalised=False, max_angle_deg=3.0, max_direction_deg=5.0)
    finally:
        kt.kt_release()
    # the verdicts
    flagged = np.flatnonzero(~out["pair_mask"])
    print("pairs not admitted:", flagged.tolist(), "summary:", out["summary"], "cost:", out["cost"].tolist())
    assert set(CORRUPTED) <= set(flagged.tolist()) and not out["verdicts"]["rotation"]["edge_inlier"][list(CORRUPTED)].any()
    assert flagged.size <= len(CORRUPTED) + 2
    assert mask_bytes == n_ref_keys
    # no kept track mixes two scene points
    kept = out["key_track"] >= 0
    assert out["summary"]["tracks"] > 200 and not np.any(g["key_point"][kept] == -2)       # no key of a corrupted pair is in a track
    for t in range(out["summary"]["tracks"]):
        pts = g["key_point"][out["key_track"] == t]
        assert np.unique(pts[pts >= 0]).size <= 1, (t, pts)
    print("kept tracks that hold a key of no scene point:", sum(bool(np.any(g["key_point"][out["key_track"] == t] < 0)) for t in range(out["summary"]["tracks"])))
    # the CPU route on the same input
    fed = dict(key_ptr=np.concatenate(([0], np.cumsum([x.shape[0] for x in g["xy"]]))).astype(np.int32), pair_views=np.array(g["pairs"], dtype=np.int32),
               pair_ptr=np.concatenate(([0], np.cumsum([a.size for a, _ in g["matches"]]))).astype(np.int64), min_len=2)
    a_all, b_all, m_all = [], [], []
    for p, ((a, b), pose) in enumerate(zip(g["matches"], out["poses"])):
        order = np.argsort(a)                                               # the order of the table row
        assert np.array_equal(a[order], pose["r_idx"]) and np.array_equal(b[order], pose["q_idx"])
        a_all.append(a[order]); b_all.append(b[order]); m_all.append(pose["inlier"] & out["pair_mask"][p])
    fed.update(a=np.concatenate(a_all).astype(np.int32), b=np.concatenate(b_all).astype(np.int32), mask=np.concatenate(m_all).astype(np.uint8))
    want = ref.settle(fed)
    assert np.array_equal(want["key_track"], out["key_track"]) and np.array_equal(want["pt_ptr"], pt_ptr) and np.array_equal(want["cam_idx"], cam_idx)
    assert np.array_equal(want["key_idx"], key_idx) and np.array_equal(out["pt_ptr"], pt_ptr)
    uv_pix = np.array([g["xy"][c][k] for c, k in zip(cam_idx, key_idx)]).T
    uvn = sfm.geometry.normalise_pixels(uv_pix, g["K"])
    cams0 = sfm.geometry.pack_cameras(out["rots_averaged"], out["centres_averaged"])
    projs = [g["K"] @ np.hstack((r.T, -r.T @ c.reshape(3, 1))) for r, c in zip(out["rots_averaged"], out["centres_averaged"])]
    n_tracks = pt_ptr.size - 1
    pts0 = np.zeros((3, n_tracks))
    for t in range(n_tracks):
        obs = range(pt_ptr[t], pt_ptr[t + 1])
        pr, uv = [projs[cam_idx[o]] for o in obs], [uv_pix[:, o] for o in obs]
        x = oracle.nonlinear_triangulate(_dlt(pr, uv), pr, [u.reshape(2, 1) for u in uv], 0.5, 20)
        pts0[:, t] = x[0:3, 0]
    pt_idx = np.repeat(np.arange(n_tracks), np.diff(pt_ptr)).astype(np.int32)
    rmse0 = oracle.rmse_pixels(cams0, pts0, cam_idx, pt_idx, uv_pix, g["K"])
    trace = []
    cams_cpu, pts_cpu = oracle.ba_sparse(cams0, pts0, cam_idx, pt_idx, uvn, LAM, ITERS, trace=trace)
    steps_cpu = [oracle.rmse_pixels(c, p, cam_idx, pt_idx, uv_pix, g["K"]) for c, p in trace]
    rmse_cpu = oracle.rmse_pixels(cams_cpu, pts_cpu, cam_idx, pt_idx, uv_pix, g["K"])
    rmse_gpu = oracle.rmse_pixels(out["cameras"], out["points"], cam_idx, pt_idx, uv_pix, g["K"])
    print("reprojection RMSE over %d kept observations of %d tracks: before %.4f px, CPU route %.4f px, device route %.4f px"
          % (cam_idx.size, n_tracks, rmse0, rmse_cpu, rmse_gpu))
    print("CPU route per iteration:", ["%.3f" % r for r in steps_cpu])
    assert np.all(np.diff([rmse0] + steps_cpu) < 0)                          # the CPU route itself converges on this scene
    assert rmse_gpu <= 1.1 * rmse_cpu
    assert np.all(np.diff(out["cost"]) < 0)
    # the other route: PCG with two views held, after a robust re-triangulation and a cull at 4 px
    pt_idx2 = np.repeat(np.arange(again["pt_ptr"].size - 1), np.diff(again["pt_ptr"])).astype(np.int32)
    print("pcg route (adaptive damping, after retriangulation and a cull at 4 px): %d observations, cost %s" % (pt_idx2.size, again["cost"].tolist()))
    assert np.all(np.isfinite(again["cost"])) and again["cost"][-1] <= again["cost"][0] and np.array_equal(again["key_track"], out["key_track"])
