"""The device-resident key tracks (csrc/sfm_track.hip, native.TrackStore, HipDeviceKeyTracker) against the host path
that already exists (matching.py, HipKeyTracker, HipKeyTrack): everything is an integer or a copied coordinate, so every
check is exact equality.

1. synthetic neighbour arrays with dense duplicate train indices and tied distances, uploaded and handed straight to the
   store, in all three modes: kept lists, tables, inlier prefixes;
2. the ratio test one float32 step either side of 0.7 * d1;
3. quirk Q16: the reference's exceptions, at the same query, tables left as the host tracker leaves them;
4. five seeded views (SIFT-like L2 and ORB-like Hamming) through both trackers, all modes, with and without the
   fundamental-matrix inliers (same RNG stream);
5. generate_matched_pairs, update_usage, extract_*: shapes, dtypes, values; nothing uploaded twice."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1000, 20000)
DISTS = np.array([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 6.0], dtype=np.float32)


class View:
    def __init__(self, key_pts, key_descriptors):
        self.key_pts = key_pts
        self.key_descriptors = key_descriptors


def flags_of(hip, mode):
    """(is_knn_match, is_cross_check) of a device mode."""
    return {hip.MATCH_KNN2: (True, False), hip.MATCH_NN1: (False, False), hip.MATCH_MUTUAL: (False, True)}[mode]


def synthetic(rng, n_refs, nq, nt):
    """Neighbour arrays (n_refs, nq) whose train indices collide often and whose distances tie often."""
    bi = rng.integers(0, nt, (n_refs, nq)).astype(np.int32)
    bd = DISTS[rng.integers(0, DISTS.shape[0], (n_refs, nq))]
    si = rng.integers(0, nt, (n_refs, nq)).astype(np.int32)
    # exact float32 multiples: the ratio is 0.8, 2/3, 0.5 or 0.25, on both sides of 0.7
    sd = (bd * np.array([1.25, 1.5, 2.0, 4.0], dtype=np.float32)[rng.integers(0, 4, (n_refs, nq))]).astype(np.float32)
    mu = (rng.random((n_refs, nq)) < 0.7).astype(np.uint8)
    return bi, bd, si, sd, mu


def host_kept(sfm, hip, mode, nn, r):
    knn, cross = flags_of(hip, mode)
    q, t, d = sfm.matching.filter_matches(nn[0][r], nn[1][r], nn[2][r], nn[3][r], nn[4][r].astype(bool), knn, cross)
    kept = sfm.matching.dedup_kept(t, d)
    # does Q14's replacement rule pick an entry that is not the first appearance of its train index?
    _u, first = np.unique(t, return_index=True)
    replaced = int(np.sum(np.sort(kept) != np.sort(first))) if kept.shape[0] else 0
    return q[kept], t[kept], replaced


def make_store(hip, rng, n_refs, nq, nt):
    store = hip.TrackStore()
    xy = [rng.uniform(0, 1000, (nt, 2)).astype(np.float32).astype(np.float64) for _ in range(n_refs)]
    xy.append(rng.uniform(0, 1000, (nq, 2)).astype(np.float32).astype(np.float64))
    for v, a in enumerate(xy):
        assert store.add_view(a) == v
    return store, xy


def upload(torch, nn):
    bufs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in nn]
    torch.cuda.synchronize()
    return bufs


def host_tables(n_refs, nq, nt):
    return [np.full((n_refs + 1, nt), -1, dtype=np.int32) for _ in range(n_refs)] + [np.full((n_refs + 1, nq), -1, dtype=np.int32)]


def assert_tables(store, want, what):
    for v, w in enumerate(want):
        got = store.table(v)
        assert got.dtype == np.int32 and got.shape == w.shape, (what, v, got.shape, w.shape)
        np.testing.assert_array_equal(got, w, err_msg="%s table %d" % (what, v))


@pytest.mark.parametrize("mode_name", ("KNN2", "NN1", "MUTUAL"))
def test_synthetic_neighbours_filter_dedup_write(hip, sfm, mode_name):
    import torch
    mode = getattr(hip, "MATCH_" + mode_name)
    stream = torch.cuda.current_stream().cuda_stream
    replaced_total = 0
    for n_refs in (1, 9):
        for nq in SIZES:
            rng = np.random.default_rng(1000 * n_refs + nq)
            nt = max(2, nq // 16)                                   # far fewer train indices than queries
            nn = synthetic(rng, n_refs, nq, nt)
            want = [host_kept(sfm, hip, mode, nn, r) for r in range(n_refs)]
            replaced_total += sum(w[2] for w in want)
            bufs = upload(torch, nn)
            ptrs = [b.data_ptr() for b in bufs]

            # (a) one call: filter + dedup + write, nothing downloaded in between
            store, _xy = make_store(hip, rng, n_refs, nq, nt)
            try:
                down = store.download_bytes
                store.extend_dev(n_refs, n_refs, mode, *ptrs, stream=stream)
                assert store.download_bytes == down
                status, bad, n_kept = store.extend_status(n_refs)
                assert (status == hip.TRACK_OK).all() and (bad == -1).all()
                tables = host_tables(n_refs, nq, nt)
                for r in range(n_refs):
                    kq, kt, _ = want[r]
                    assert n_kept[r] == kq.shape[0], (n_refs, nq, r)
                    gq, gt = store.kept(r, int(n_kept[r]))
                    np.testing.assert_array_equal(gq, kq, err_msg="kept q %s" % ((n_refs, nq, r),))
                    np.testing.assert_array_equal(gt, kt, err_msg="kept t %s" % ((n_refs, nq, r),))
                    tables[r][n_refs, kt] = kq
                    tables[n_refs][r, kq] = kt
                assert_tables(store, tables, "extend %s" % ((n_refs, nq),))
            finally:
                store.close()

            # (b) filter + dedup, then the inlier prefixes (quirk Q15), cumulatively: 0, 1, len - 1, len
            store, _xy = make_store(hip, rng, n_refs, nq, nt)
            try:
                store.match_dedup_dev(n_refs, n_refs, mode, *ptrs, stream=stream)
                status, bad, n_kept = store.extend_status(n_refs)
                assert (status == hip.TRACK_OK).all()
                tables = host_tables(n_refs, nq, nt)
                assert_tables(store, tables, "dedup only %s" % ((n_refs, nq),))
                for step in range(4):
                    for r in range(n_refs):
                        kq, kt, _ = want[r]
                        ln = kq.shape[0]
                        n_in = (0, 1, ln - 1, ln)[step]
                        store.write_kept(r, n_in, stream=stream)
                        # a prefix outside [0, len] means the whole list (n < 0) -- the host slices the same way
                        n_eff = ln if (n_in < 0 or n_in > ln) else n_in
                        tables[r][n_refs, kt[:n_eff]] = kq[:n_eff]
                        tables[n_refs][r, kq[:n_eff]] = kt[:n_eff]
                    assert_tables(store, tables, "prefix step %d %s" % (step, (n_refs, nq)))
            finally:
                store.close()
    # the case set must exercise Q14's replacement rule: a kept entry that is not its train index's first appearance
    assert replaced_total > 0, mode_name


def test_q3_pairs_and_usage_on_synthetic_tables(hip, sfm):
    """Store level: query key 0 is matched and therefore never paired (Q3); usage lists with duplicate keys."""
    import torch
    rng = np.random.default_rng(7)
    n_refs, nq, nt = 2, 300, 40
    nn = list(synthetic(rng, n_refs, nq, nt))
    nn[0][:, 0] = 3                     # query 0 -> train 3, alone on it, so that it is kept
    for r in range(n_refs):
        clash = np.flatnonzero(nn[0][r] == 3)[1:]
        nn[0][r, clash] = 4
    want = [host_kept(sfm, hip, hip.MATCH_NN1, nn, r) for r in range(n_refs)]
    assert all(0 in w[0].tolist() for w in want)
    bufs = upload(torch, nn)
    store, xy = make_store(hip, rng, n_refs, nq, nt)
    try:
        store.extend_dev(n_refs, n_refs, hip.MATCH_NN1, *[b.data_ptr() for b in bufs], stream=torch.cuda.current_stream().cuda_stream)
        tables = host_tables(n_refs, nq, nt)
        for r in range(n_refs):
            kq, kt, _ = want[r]
            tables[r][n_refs, kt] = kq
            tables[n_refs][r, kq] = kt
        for ref in range(n_refs + 1):
            for que in range(n_refs + 1):
                row = tables[ref][que]
                r_idx = np.flatnonzero(row > 0)
                q_idx = row[r_idx]
                gr, gq, gref, gque = store.pairs(ref, que)
                np.testing.assert_array_equal(gr, r_idx)
                np.testing.assert_array_equal(gq, q_idx)
                assert gref.shape == gque.shape == (3, r_idx.shape[0]) and gref.dtype == gque.dtype == np.float64
                np.testing.assert_array_equal(gref, np.vstack((xy[ref][r_idx].T, np.ones((1, r_idx.shape[0])))))
                np.testing.assert_array_equal(gque, np.vstack((xy[que][q_idx].T, np.ones((1, q_idx.shape[0])))))
        assert (tables[0][n_refs] == 0).sum() == 1 and 3 not in store.pairs(0, n_refs)[0].tolist()      # Q3
        # usage: the last of a repeated key wins, as NumPy's fancy assignment
        keys = np.array([5, 9, 5, 17, 9, 5, 0], dtype=np.int32)
        tri = np.arange(100, 107, dtype=np.int32)
        store.update_usage(1, keys, tri)
        own = np.full(nt, -1, dtype=np.int32)
        own[keys] = tri
        np.testing.assert_array_equal(store.row(1, 1), own)
        k, t = store.constructed(1)
        np.testing.assert_array_equal(k, np.flatnonzero(own != -1))
        np.testing.assert_array_equal(t, own[own != -1])
        np.testing.assert_array_equal(store.unconstructed(1), np.flatnonzero(own == -1))
        with pytest.raises(ValueError):
            store.update_usage(1, np.array([nt], dtype=np.int32), np.array([1], dtype=np.int32))
        np.testing.assert_array_equal(store.row(1, 1), own)
        assert store.n_views == n_refs + 1 and store.n_keys(n_refs) == nq and store.n_rows(0) == n_refs + 1
    finally:
        store.close()


def test_tables_survive_more_views_than_spare_rows(hip):
    """Adding views beyond the spare row capacity moves the tables; their contents stay."""
    rng = np.random.default_rng(11)
    store = hip.TrackStore()
    try:
        n_views, n = 40, 7
        for v in range(n_views):
            store.add_view(rng.uniform(0, 10, (n, 2)))
            store.update_usage(v, np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32) + 10 * v)
        for v in range(n_views):
            t = store.table(v)
            assert t.shape == (n_views, n)
            want = np.full((n_views, n), -1, dtype=np.int32)
            want[v] = np.arange(n) + 10 * v
            np.testing.assert_array_equal(t, want)
    finally:
        store.close()


def test_ratio_boundary_equals_python_floats(hip):
    import torch
    rng = np.random.default_rng(5)
    d1 = np.concatenate((rng.uniform(1, 1000, 300), rng.uniform(1e-3, 1, 100), [10.0, 20.0, 100.0])).astype(np.float32)
    mid = (np.float32(0.7) * d1).astype(np.float32)
    d0 = np.concatenate((np.nextafter(mid, np.float32(0)), mid, np.nextafter(mid, np.float32(np.inf)),
                         (0.7 * d1.astype(np.float64)).astype(np.float32)))
    d1 = np.tile(d1, 4)
    nq = d0.shape[0]
    want = np.array([float(a) / float(b) < 0.7 for a, b in zip(d0, d1)])
    assert want.any() and (~want).any()
    bi = np.arange(nq, dtype=np.int32)[np.newaxis]                      # distinct train indices: nothing to deduplicate
    nn = (bi, d0[np.newaxis], bi.copy(), d1[np.newaxis], np.zeros((1, nq), dtype=np.uint8))
    bufs = upload(torch, nn)
    store = hip.TrackStore()
    try:
        store.add_view(np.zeros((nq, 2)))
        store.add_view(np.zeros((nq, 2)))
        store.match_dedup_dev(1, 1, hip.MATCH_KNN2, *[b.data_ptr() for b in bufs])
        status, _bad, n_kept = store.extend_status(1)
        assert status[0] == hip.TRACK_OK
        gq, gt = store.kept(0, int(n_kept[0]))
        np.testing.assert_array_equal(gq, np.flatnonzero(want))
        np.testing.assert_array_equal(gt, np.flatnonzero(want))
    finally:
        store.close()


def test_q16_status_on_mixed_synthetic_batch(hip, sfm):
    """One reference view whose knn result holds BOTH conditions: the status is what filter_matches raises, at the
    first offending query; the view after it does not write."""
    import torch
    rng = np.random.default_rng(9)
    n_refs, nq, nt = 3, 500, 50
    for first_kind in ("none", "zero"):
        nn = [a.copy() for a in synthetic(rng, n_refs, nq, nt)]
        no_second, zero = (130, 260) if first_kind == "none" else (260, 130)
        nn[2][1, [no_second, 400]] = -1
        nn[3][1, [no_second, 400]] = np.inf
        nn[3][1, [zero, 450]] = 0.0
        with pytest.raises(IndexError if first_kind == "none" else ZeroDivisionError):
            sfm.matching.filter_matches(nn[0][1], nn[1][1], nn[2][1], nn[3][1], nn[4][1].astype(bool), True, False)
        bufs = upload(torch, nn)
        store, _xy = make_store(hip, rng, n_refs, nq, nt)
        try:
            store.extend_dev(n_refs, n_refs, hip.MATCH_KNN2, *[b.data_ptr() for b in bufs])
            status, bad, n_kept = store.extend_status(n_refs)
            assert status.tolist() == [hip.TRACK_OK, hip.TRACK_NO_SECOND if first_kind == "none" else hip.TRACK_ZERO_SECOND, hip.TRACK_OK]
            assert bad.tolist() == [-1, 130, -1] and n_kept[1] == 0
            tables = host_tables(n_refs, nq, nt)
            kq, kt, _ = host_kept(sfm, hip, hip.MATCH_KNN2, nn, 0)
            tables[0][n_refs, kt] = kq                                   # only the view before the failing one wrote
            tables[n_refs][0, kq] = kt
            assert_tables(store, tables, "mixed batch " + first_kind)
        finally:
            store.close()


def int_rows(rng, n):
    base = rng.gamma(0.6, 1.0, (n, 128))
    return np.clip(np.rint(base / np.linalg.norm(base, axis=1, keepdims=True) * 512.0), 0, 255).astype(np.uint8)


def noisy(rng, rows):
    return np.clip(rows.astype(np.int64) + rng.integers(-2, 3, rows.shape), 0, 255).astype(np.uint8)


def q16_views(sfm, layout):
    """View 0 ordinary; then per layout entry a view with a single descriptor ('single': IndexError as a reference view)
    or with a row repeated that the last view also holds ('zero': both distances 0, ZeroDivisionError); last an ordinary
    view of noisy copies of view 0's rows."""
    rng = np.random.default_rng(31)
    special = int_rows(rng, 1)[0]
    descs = [int_rows(rng, 60)]
    for kind in layout:
        if kind == "single":
            descs.append(int_rows(rng, 1))
        else:
            d = int_rows(rng, 50)
            d[10] = d[11] = special
            descs.append(d)
    last = noisy(rng, descs[0])
    last[5] = special
    descs.append(last)
    return [View([sfm.scenes.KeyPoint(x, y) for x, y in rng.uniform(0, 900, (d.shape[0], 2))], d) for d in descs]


# (a view with a single descriptor can only be the LAST reference view: added earlier, the next view's own knn match
# against it raises; the order "no second neighbour first" inside one batch is in the synthetic test above)
@pytest.mark.parametrize("layout,exc", ((("single",), IndexError), (("zero",), ZeroDivisionError),
                                        (("zero", "single"), ZeroDivisionError)))
def test_q16_exceptions_and_tables_equal_the_host_tracker(hip, sfm, layout, exc):
    views = q16_views(sfm, layout)
    host = sfm.processors.HipKeyTracker("sift", False, True, False, None)
    dev = sfm.processors.HipDeviceKeyTracker("sift", False, True, False, None)
    try:
        for kt in (host, dev):
            for v in range(len(views) - 1):
                kt.add_new_view(views[v], views[:v])
            with pytest.raises(exc) as info:
                kt.add_new_view(views[-1], views[:-1])
            kt.message = str(info.value)
        assert host.message == dev.message
        assert len(host.track_list) == len(dev.track_list) == len(views) - 1
        wrote = False
        for v in range(len(host.track_list)):
            want = host.track_list[v].table
            got = dev.track_list[v].table
            assert got.dtype == want.dtype and got.shape == want.shape == (len(views), want.shape[1])
            np.testing.assert_array_equal(got, want, err_msg="table %d" % v)
            wrote = wrote or (want[len(views) - 1] >= 0).any()
        assert wrote                                  # view 0, before the failing one, got its pairs
    finally:
        host.kt_release()
        dev.kt_release()


def tracker_pair(sfm, key_type, cross, knn, fund, cfg):
    P = sfm.processors
    return P.HipKeyTracker(key_type, cross, knn, fund, cfg), P.HipDeviceKeyTracker(key_type, cross, knn, fund, cfg)


def assert_same_tables(host, dev, what):
    assert len(host.track_list) == len(dev.track_list)
    for v in range(len(host.track_list)):
        want, got = host.track_list[v].table, dev.track_list[v].table
        assert got.dtype == want.dtype and got.shape == want.shape, (what, v)
        np.testing.assert_array_equal(got, want, err_msg="%s view %d" % (what, v))
        assert dev.track_list[v].idx == host.track_list[v].idx and dev.track_list[v].key_num == host.track_list[v].key_num


@pytest.mark.parametrize("fund", (False, True))
@pytest.mark.parametrize("mode_name", ("knn", "match", "cross"))
@pytest.mark.parametrize("key_type", ("sift", "orb"))
def test_five_views_through_both_trackers(hip, sfm, key_type, mode_name, fund):
    dv = sfm.scenes.make_descriptor_views(n_views=5, n_pts=200, seed=0)
    desc = dv.sift if key_type == "sift" else dv.orb
    views = [View(dv.key_pts(v), desc[v]) for v in range(5)]
    cross, knn = mode_name == "cross", mode_name == "knn"
    cfg = sfm.processors.RansacConfig(2.0, 0.99, 0.75, 8, 100) if fund else None
    host, dev = tracker_pair(sfm, key_type, cross, knn, fund, cfg)
    try:
        snapshots = []
        for kt in (host, dev):
            random.seed(1234)
            for v in range(5):
                kt.add_new_view(views[v], views[:v])
                if kt is host:
                    snapshots.append([t.table.copy() for t in host.track_list])
                else:
                    # after EVERY added view every table equals the host tracker's at that point
                    for u in range(v + 1):
                        np.testing.assert_array_equal(dev.track_list[u].table, snapshots[v][u], err_msg="after view %d: table %d" % (v, u))
            kt.rng_state = random.getstate()
        assert host.rng_state == dev.rng_state
        assert_same_tables(host, dev, "%s %s fund=%s" % (key_type, mode_name, fund))
        assert (host.track_list[0].table[4] >= 0).sum() > 20
    finally:
        host.kt_release()
        dev.kt_release()


def test_pairs_usage_and_traffic_equal_the_host_tracker(hip, sfm, capsys):
    dv = sfm.scenes.make_descriptor_views(n_views=4, n_pts=300, seed=3, n_dup=20)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(4)]
    for v in views[:2]:                                # two views with the coordinate array, two read from key_pts
        v.key_xy = np.array([kp.pt for kp in v.key_pts])
    host, dev = tracker_pair(sfm, "sift", False, False, False, None)        # 1-NN: dense duplicates, key 0 is matched
    try:
        for kt in (host, dev):
            for v in range(4):
                kt.add_new_view(views[v], views[:v])
        assert_same_tables(host, dev, "pairs")
        assert any((host.track_list[r].table[q] == 0).any() for r in range(4) for q in range(4) if r != q)     # Q3 is exercised
        for ref in range(4):
            for que in range(4):
                want = host.generate_matched_pairs(ref, que, views)
                got = dev.generate_matched_pairs(ref, que, views)
                for w, g in zip((want[0][0], want[0][1], want[1], want[2]), (got[0][0], got[0][1], got[1], got[2])):
                    assert g.dtype == w.dtype and g.shape == w.shape, (ref, que)
                    np.testing.assert_array_equal(g, w, err_msg="pairs %d %d" % (ref, que))
                assert isinstance(got[0], list) and len(got[0]) == 2
        # a repeated call on unchanged tables uploads nothing again, and what comes down is the result alone (the count
        # and its flag, two index lists, two (3, n) double arrays): no table, no coordinates
        up, down = dev.kt_upload_bytes, dev.kt_download_bytes
        again = dev.generate_matched_pairs(0, 3, views)
        n03 = again[1].shape[1]
        assert n03 > 0
        assert dev.kt_upload_bytes == up and dev._store.upload_bytes + dev.__dict__.get("_hip_desc_bytes", 0) == up
        assert dev.kt_download_bytes - down == 8 + n03 * (4 + 4 + 24 + 24)
        np.testing.assert_array_equal(again[1], host.generate_matched_pairs(0, 3, views)[1])
        again[0][0][:] = -5.0                          # the caller's arrays are its own
        np.testing.assert_array_equal(dev.generate_matched_pairs(0, 3, views)[0][0], host.generate_matched_pairs(0, 3, views)[0][0])
        # invalid indices: the reference's line and None
        capsys.readouterr()
        assert dev.generate_matched_pairs(0, 4, views) is None and host.generate_matched_pairs(0, 4, views) is None
        lines = capsys.readouterr().out.splitlines()
        assert lines[0] == "HipDeviceKeyTracker:generate_matched_pairs - invalid ref_idx 0 or invalid que_idx 4"
        assert lines[1] == "HipKeyTracker:generate_matched_pairs - invalid ref_idx 0 or invalid que_idx 4"

        # usage: what BaProcessor.process does with the pairs of views 0 and 1, plus a repeated key
        pairs, r_idx, q_idx = host.generate_matched_pairs(0, 1, views)
        sel = np.arange(0, r_idx.shape[1], 2)[np.newaxis, :]
        tri = np.arange(sel.shape[1], dtype=int)[np.newaxis, :]
        for kt in (host, dev):
            kt.track_list[0].update_usage(np.take(r_idx, sel), tri)
            kt.track_list[1].update_usage(np.take(q_idx, sel), tri)
            kt.track_list[2].update_usage(np.array([[3, 8, 3, -1]]), np.array([[50, 51, 52, 53]]))
        assert_same_tables(host, dev, "usage")
        for v in range(4):
            wi, wv = host.track_list[v].extract_constructed_points()
            gi, gv = dev.track_list[v].extract_constructed_points()
            wu, gu = host.track_list[v].extract_unconstructed_points(), dev.track_list[v].extract_unconstructed_points()
            for w, g in ((wi, gi), (wv, gv), (wu, gu)):
                assert g.dtype == w.dtype and g.shape == w.shape, v
                np.testing.assert_array_equal(g, w)
        assert host.is_visible(0, 2) == dev.is_visible(0, 2) and host.is_visible(0, 10 ** 6) == dev.is_visible(0, 10 ** 6) == -1
        assert dev.find_best_view(3) == host.find_best_view(3) == 0
        # descriptors went up once per view, coordinates once per view (16 bytes a key), usage lists as int32 pairs
        desc_bytes = sum(v.key_descriptors.nbytes for v in views)
        assert host.kt_upload_bytes == desc_bytes
        assert dev.kt_upload_bytes == desc_bytes + 16 * sum(len(v.key_pts) for v in views) + 8 * (2 * sel.shape[1] + 4)
        dev.clear()
        assert dev.track_list == [] and dev.generate_matched_pairs(0, 0, views) is None
    finally:
        host.kt_release()
        dev.kt_release()


def test_new_view_without_keys_on_the_device_tracker(hip, sfm):
    dv = sfm.scenes.make_descriptor_views(n_views=2, n_pts=100, seed=4)
    views = [View(dv.key_pts(v), dv.sift[v]) for v in range(2)] + [View([], np.zeros((0, 128), dtype=np.uint8))]
    host, dev = tracker_pair(sfm, "sift", False, True, False, None)
    try:
        for kt in (host, dev):
            for v in range(3):
                kt.add_new_view(views[v], views[:v])
        assert_same_tables(host, dev, "empty view")
        assert dev.track_list[2].table.shape == (3, 0)
    finally:
        host.kt_release()
        dev.kt_release()
