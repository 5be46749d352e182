"""Guided matching on the MI355X against the NumPy reference of tests/_match_guided_reference.py.  Every row of every case is
settled in the reference (tests/test_match_guided_host.py asserts it), so all six outputs are compared exactly, the float
distances as bits; the shapes sit at the kernels' boundaries (the 128-row tile, the 16-column tile, the 1 024-column chunk)."""
import ctypes
import itertools

import numpy as np
import pytest

import _match_guided_reference as mg

pytestmark = pytest.mark.gpu

KINDS = {mg.FUNDAMENTAL: "F", mg.HOMOGRAPHY: "H"}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _metric(hip, sc):
    return hip.MATCH_HAMMING if sc.norm == mg.bf.NORM_HAMMING else hip.MATCH_L2


def _compare(got, ref, what):
    rows = ref["settled"]
    assert rows.all(), what                                  # the host conditions test says so; nothing is left out
    for name in mg.OUTPUTS:
        want = ref[name]
        assert got[name].dtype == want.dtype, (what, name)
        assert same_bits(got[name][rows], want[rows]), (what, name, np.flatnonzero(got[name] != want)[:8])


def _run_case(hip, sc, kind, max_err2=4.0, que_xy=None):
    with hip.DescriptorSet(_metric(hip, sc), sc.que_desc) as q, hip.DescriptorSet(_metric(hip, sc), sc.ref_desc) as r:
        out = hip.match_guided(q, sc.que_xy if que_xy is None else que_xy, [r], [sc.ref_xy], [kind], [mg.model_of(sc, kind)], max_err2)
        return {name: out[name][0] for name in mg.OUTPUTS}, (q.exact, r.exact)


# ---- parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [mg.FUNDAMENTAL, mg.HOMOGRAPHY], ids=lambda k: KINDS[k])
@pytest.mark.parametrize("nq,nt,dim", mg.PARITY_CASES, ids=lambda v: str(v))
def test_parity_on_the_exact_path(hip, nq, nt, dim, kind):
    sc, ref = mg.case(nq, nt, dim, kind)
    got, exact = _run_case(hip, sc, kind)
    assert exact == (True, True)
    _compare(got, ref, (nq, nt, dim, kind))


@pytest.mark.parametrize("kind", [mg.FUNDAMENTAL, mg.HOMOGRAPHY], ids=lambda k: KINDS[k])
@pytest.mark.parametrize("path", ["hamming", "float"])
def test_parity_on_the_hamming_and_general_float_paths(hip, path, kind):
    sc, ref = mg.case(mg.MID[0], mg.MID[1], 32, kind, metric="hamming" if path == "hamming" else "l2", float_rows=path == "float")
    got, exact = _run_case(hip, sc, kind)
    assert exact == (False, False)
    _compare(got, ref, (path, kind))


# ---- no gate: sfm_match bit for bit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["exact128", "exact200", "hamming", "float"])
def test_no_gate_equals_sfm_match(hip, path):
    dim = {"exact128": 128, "exact200": 200}.get(path, 32)
    a, _ = mg.case(129, 1025, dim, mg.FUNDAMENTAL, metric="hamming" if path == "hamming" else "l2", float_rows=path == "float")
    b, _ = mg.case(129, 17, dim, mg.FUNDAMENTAL, metric="hamming" if path == "hamming" else "l2", float_rows=path == "float")
    m = _metric(hip, a)
    with hip.DescriptorSet(m, a.que_desc) as q, hip.DescriptorSet(m, a.ref_desc) as r0, hip.DescriptorSet(m, b.ref_desc) as r1:
        want = hip.match(q, [r0, r1], hip.MATCH_MUTUAL)
        got = hip.match_guided(q, a.que_xy, [r0, r1], [None, b.ref_xy], ["none", "none"], [None, None], 4.0)
        for name, w in zip(mg.OUTPUTS[:5], want):
            assert same_bits(got[name], w), (path, name)
        assert want[4].any() and not want[4].all()
        assert np.array_equal(got["n_admitted"], np.repeat([[1025], [17]], 129, axis=1))
        # a NaN query coordinate is not looked at without a gate
        xy = a.que_xy.copy()
        xy[3] = np.nan
        again = hip.match_guided(q, xy, [r0, r1], [None, None], [0, 0], [None, None], 4.0)
        for name in mg.OUTPUTS:
            assert same_bits(again[name], got[name]), (path, name)


# ---- batch independence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("float_mixed", [False, True], ids=["exact", "exact+float"])
def test_one_launch_with_every_gate_equals_per_reference_calls(hip, float_mixed):
    sc = mg.batch_scene(float_mixed)
    q = hip.DescriptorSet(hip.MATCH_L2, sc.que_desc)
    refs = [hip.DescriptorSet(hip.MATCH_L2, desc) for _xy, desc, _k, _m in sc.refs]
    try:
        assert [r.exact for r in refs] == [True, not float_mixed, True, True] and q.exact
        xys, kinds, models = [r[0] for r in sc.refs], [r[2] for r in sc.refs], [r[3] for r in sc.refs]
        whole = hip.match_guided(q, sc.que_xy, refs, xys, kinds, models, 4.0)
        for r in range(len(refs)):
            alone = hip.match_guided(q, sc.que_xy, [refs[r]], [xys[r]], [kinds[r]], [models[r]], 4.0)
            for name in mg.OUTPUTS:
                assert same_bits(whole[name][r], alone[name][0]), (r, name)
            _compare({name: whole[name][r] for name in mg.OUTPUTS}, sc.out[r], ("batch", float_mixed, r))
        order = [3, 1, 0, 2]
        moved = hip.match_guided(q, sc.que_xy, [refs[r] for r in order], [xys[r] for r in order], [kinds[r] for r in order],
                                 [models[r] for r in order], 4.0)
        for i, r in enumerate(order):
            for name in mg.OUTPUTS:
                assert same_bits(moved[name][i], whole[name][r]), (r, name)
    finally:
        for s in refs + [q]:
            s.close()


# ---- a gate that admits nothing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [mg.FUNDAMENTAL, mg.HOMOGRAPHY], ids=lambda k: KINDS[k])
def test_a_gate_that_admits_nothing(hip, kind):
    sc, ref = mg.case(129, 1025, 128, kind)
    got, _ = _run_case(hip, sc, kind, max_err2=0.0)
    assert np.all(got["best_idx"] == -1) and np.all(got["second_idx"] == -1) and np.all(got["n_admitted"] == 0)
    assert np.all(np.isposinf(got["best_dist"])) and np.all(np.isposinf(got["second_dist"])) and not got["mutual"].any()
    xy = sc.que_xy.copy()
    xy[7, 0] = np.nan
    got, _ = _run_case(hip, sc, kind, que_xy=xy)
    assert got["best_idx"][7] == -1 and got["second_idx"][7] == -1 and got["n_admitted"][7] == 0 and not got["mutual"][7]
    assert np.isposinf(got["best_dist"][7]) and np.isposinf(got["second_dist"][7])
    keep = np.arange(129) != 7                              # the other rows: the best, second and count do not depend on row 7
    for name in ("best_idx", "best_dist", "second_idx", "second_dist", "n_admitted"):
        assert same_bits(got[name][keep], ref[name][keep]), name
    want = mg.reference(sc.norm, sc.que_desc, sc.ref_desc, xy, sc.ref_xy, kind, mg.model_of(sc, kind), 4.0)
    _compare(got, want, ("nan row", kind))


# ---- canonical ties -----------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_admitted_index(hip):
    t = mg.ties_scene()
    with hip.DescriptorSet(hip.MATCH_L2, t.que_desc) as q, hip.DescriptorSet(hip.MATCH_L2, t.ref_desc) as r:
        both = hip.match_guided(q, t.que_xy, [r], [t.ref_xy], ["homography"], [np.eye(3)], 4.0)
        assert both["best_idx"][0].tolist() == t.want_both_best and both["second_idx"][0].tolist() == t.want_both_second
        assert same_bits(both["best_dist"], both["second_dist"]) and both["n_admitted"][0].tolist() == [2, 2]
        moved = hip.match_guided(q, t.que_xy, [r], [t.ref_xy_lower_out], ["homography"], [np.eye(3)], 4.0)
        assert moved["best_idx"][0].tolist() == t.want_moved_best and moved["second_idx"][0].tolist() == [-1, -1]
        assert same_bits(moved["best_dist"], both["best_dist"]) and moved["n_admitted"][0].tolist() == t.want_moved_count
        assert moved["mutual"][0].tolist() == [True, True] and both["mutual"][0].tolist() == [True, True]


# ---- optional outputs, the _dev form ------------------------------------------------------------------------------------
def test_every_subset_of_the_optional_outputs(hip):
    sc, _ = mg.case(129, 1025, 128, mg.FUNDAMENTAL)
    with hip.DescriptorSet(hip.MATCH_L2, sc.que_desc) as q, hip.DescriptorSet(hip.MATCH_L2, sc.ref_desc) as r:
        args = (q, sc.que_xy, [r], [sc.ref_xy], [mg.FUNDAMENTAL], [sc.F], 4.0)
        full = hip.match_guided(*args)
        for k in range(len(mg.OUTPUTS) + 1):
            for subset in itertools.combinations(mg.OUTPUTS, k):
                got = hip.match_guided(*args, outputs=subset)
                assert sorted(got) == sorted(subset)
                for name in subset:
                    assert same_bits(got[name], full[name]), (subset, name)


def test_dev_form_on_a_callers_stream(hip):
    import torch
    sc, ref = mg.case(129, 1025, 128, mg.HOMOGRAPHY)
    stream = torch.cuda.Stream()
    with hip.DescriptorSet(hip.MATCH_L2, sc.que_desc) as q, hip.DescriptorSet(hip.MATCH_L2, sc.ref_desc) as r, \
            torch.cuda.stream(stream):
        d_q = torch.from_numpy(np.ascontiguousarray(sc.que_xy.T)).cuda()
        d_r = torch.from_numpy(np.ascontiguousarray(sc.ref_xy.T)).cuda()
        dt = (torch.int32, torch.float32, torch.int32, torch.float32, torch.uint8, torch.int32)
        outs = [torch.full((1, 129), 77, dtype=t, device="cuda") for t in dt]
        stream.synchronize()
        qxy, rxy = (d_q[0].data_ptr(), d_q[1].data_ptr()), (d_r[0].data_ptr(), d_r[1].data_ptr())
        # an empty query: nothing is written
        empty_h = hip.DescriptorSet(hip.MATCH_L2, np.zeros((0, 128), dtype=np.uint8))
        hip.match_guided_dev(empty_h, (0, 0), [r], [rxy], [mg.HOMOGRAPHY], [sc.H], 4.0, *[o.data_ptr() for o in outs],
                             stream=stream.cuda_stream)
        empty_h.close()
        for o in outs:
            assert bool((o.cpu() == 77).all())
        hip.match_guided_dev(q, qxy, [r], [rxy], [mg.HOMOGRAPHY], [sc.H], 4.0, *[o.data_ptr() for o in outs], stream=stream.cuda_stream)
        got = {name: o.cpu().numpy()[0] for name, o in zip(mg.OUTPUTS, outs)}
        got["mutual"] = got["mutual"].astype(bool)
        _compare(got, ref, "dev")
        # only the count asked for: the other buffers stay as they are
        cnt = torch.zeros((1, 129), dtype=torch.int32, device="cuda")
        stream.synchronize()
        hip.match_guided_dev(q, qxy, [r], [rxy], [mg.HOMOGRAPHY], [sc.H], 4.0, d_n_admitted=cnt.data_ptr(), stream=stream.cuda_stream)
        assert same_bits(cnt.cpu().numpy()[0], ref["n_admitted"])
        assert same_bits(d_q.cpu().numpy(), np.ascontiguousarray(sc.que_xy.T))


# ---- SFM_E_SHAPE from the library ---------------------------------------------------------------------------------------
def _raw(hip, q, refs, que_xy, ref_xys, kind, model, max_err2):
    """sfm_match_guided itself, past the Python checks: (status, the sentinel-filled best_idx)."""
    lib = hip.load()
    nr = len(refs)
    dp = ctypes.POINTER(ctypes.c_double)
    qx, qy = np.ascontiguousarray(que_xy[:, 0]), np.ascontiguousarray(que_xy[:, 1])
    keep = [np.ascontiguousarray(xy[:, i]) for xy in ref_xys for i in (0, 1)]
    rx = (dp * nr)(*[keep[2 * r].ctypes.data_as(dp) for r in range(nr)])
    ry = (dp * nr)(*[keep[2 * r + 1].ctypes.data_as(dp) for r in range(nr)])
    handles = (ctypes.c_void_p * nr)(*[r._h for r in refs])
    kind = np.asarray(kind, dtype=np.int32)
    model = np.ascontiguousarray(model, dtype=np.float64).reshape(nr, 9)
    best = np.full((nr, q.n), 77, dtype=np.int32)
    pp = ctypes.POINTER(ctypes.c_void_p)
    status = lib.sfm_match_guided(q._h, qx.ctypes.data_as(dp), qy.ctypes.data_as(dp), nr, handles, ctypes.cast(rx, pp),
                                  ctypes.cast(ry, pp), hip.iptr(kind), hip.dptr(model), float(max_err2),
                                  best.ctypes.data_as(ctypes.c_void_p), None, None, None, None, None)
    return status, best


def test_shape_errors_from_the_library(hip):
    sc, ref = mg.case(129, 17, 128, mg.FUNDAMENTAL)
    other, _ = mg.case(129, 17, 32, mg.FUNDAMENTAL)
    ham, _ = mg.case(mg.MID[0], mg.MID[1], 32, mg.FUNDAMENTAL, metric="hamming")
    F = sc.F
    with hip.DescriptorSet(hip.MATCH_L2, sc.que_desc) as q, hip.DescriptorSet(hip.MATCH_L2, sc.ref_desc) as r, \
            hip.DescriptorSet(hip.MATCH_L2, other.ref_desc) as r32, hip.DescriptorSet(hip.MATCH_HAMMING, ham.ref_desc) as rh, \
            hip.DescriptorSet(hip.MATCH_L2, np.zeros((0, 128), dtype=np.uint8)) as none:
        status, best = _raw(hip, q, [r], sc.que_xy, [sc.ref_xy], [1], F, 4.0)
        assert status == hip.OK and same_bits(best[0], ref["best_idx"])
        nan_model = F.copy(); nan_model[1, 1] = np.nan
        inf_model = F.copy(); inf_model[2, 0] = np.inf
        bad = {"nan max_err2": ([r], [sc.ref_xy], [1], F, float("nan")), "negative max_err2": ([r], [sc.ref_xy], [1], F, -1.0),
               "unknown kind": ([r], [sc.ref_xy], [3], F, 4.0), "negative kind": ([r], [sc.ref_xy], [-1], F, 4.0),
               "nan model": ([r], [sc.ref_xy], [1], nan_model, 4.0), "inf model": ([r], [sc.ref_xy], [2], inf_model, 4.0),
               "metric": ([rh], [ham.ref_xy], [1], F, 4.0), "dim": ([r32], [other.ref_xy], [1], F, 4.0),
               "empty reference": ([none], [np.zeros((0, 2))], [1], F, 4.0),
               "second reference bad": ([r, r], [sc.ref_xy, sc.ref_xy], [1, 7], np.stack((F, F)), 4.0)}
        for what, (refs, xys, kind, model, e2) in bad.items():
            status, best = _raw(hip, q, refs, sc.que_xy, xys, kind, model, e2)
            assert status == hip.E_SHAPE, what
            assert np.all(best == 77), what                  # nothing was launched
            assert hip.last_error(), what
        # the model of an ungated reference is not read
        status, best = _raw(hip, q, [r], sc.que_xy, [sc.ref_xy], [0], nan_model, 4.0)
        assert status == hip.OK and np.all(best >= 0)
        with pytest.raises(ValueError):
            hip.match_guided(q, sc.que_xy, [none], [np.zeros((0, 2))], [1], [F], 4.0)
        with pytest.raises(ValueError):
            hip.match_guided(q, sc.que_xy[:5], [r], [sc.ref_xy], [1], [F], 4.0)


# ---- the track store ----------------------------------------------------------------------------------------------------
def test_track_store_form_uploads_nothing(hip):
    import torch
    sc = mg.batch_scene(False)
    q = hip.DescriptorSet(hip.MATCH_L2, sc.que_desc)
    refs = [hip.DescriptorSet(hip.MATCH_L2, desc) for _xy, desc, _k, _m in sc.refs]
    try:
        xys, kinds, models = [r[0] for r in sc.refs], [r[2] for r in sc.refs], [r[3] for r in sc.refs]
        want = hip.match_guided(q, sc.que_xy, refs, xys, kinds, models, 4.0)
        with hip.TrackStore() as store:
            # views 0, 1, 3, 4 are the reference views, view 2 the query view; matched as references 4, 0, 3, 1
            layout = [xys[1], xys[3], sc.que_xy, xys[2], xys[0]]
            for xy in layout:
                store.add_view(xy)
            ref_views, pick = [4, 0, 3, 1], [0, 1, 2, 3]
            up = store.upload_bytes
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                dt = (torch.int32, torch.float32, torch.int32, torch.float32, torch.uint8, torch.int32)
                outs = [torch.full((4, q.n), 77, dtype=t, device="cuda") for t in dt]
                stream.synchronize()
                store.match_guided(2, q, ref_views, [refs[i] for i in pick], kinds, models, 4.0, *[o.data_ptr() for o in outs],
                                   stream=stream.cuda_stream)
                got = {name: o.cpu().numpy() for name, o in zip(mg.OUTPUTS, outs)}
            got["mutual"] = got["mutual"].astype(bool)
            assert store.upload_bytes == up and store.info(hip.TRACK_INFO_UPLOAD_BYTES) == up
            for name in mg.OUTPUTS:
                assert same_bits(got[name], want[name]), name
            with pytest.raises(ValueError):                 # a descriptor set that is not the view's
                store.match_guided(2, q, [0], [refs[0]], [1], [models[1]], 4.0, d_best_idx=outs[0].data_ptr())
            with pytest.raises(ValueError):
                store.match_guided(2, q, [9], [refs[0]], [1], [models[1]], 4.0, d_best_idx=outs[0].data_ptr())
    finally:
        for s in refs + [q]:
            s.close()


def test_set_pairs_writes_exactly_the_pairs(hip):
    rng = np.random.default_rng(8)
    sizes = (40, 25, 33)
    with hip.TrackStore() as store:
        for n in sizes:
            store.add_view(rng.uniform(0, 600, (n, 2)))
        # something in every row first, so that "the other rows keep their bits" says something
        store.set_pairs(0, 2, [1, 2, 3], [3, 2, 1])
        store.set_pairs(1, 2, [5, 6], [7, 8])
        store.set_pairs(0, 1, [30, 31, 32, 33], [20, 21, 22, 23])
        before = [store.table(v).copy() for v in range(3)]
        r_idx, q_idx = np.array([4, 0, 17, 39, 8]), np.array([9, 24, 3, 1, 12])
        store.set_pairs(0, 1, r_idx, q_idx)
        after = [store.table(v) for v in range(3)]
        want0 = np.full(sizes[0], -1); want0[r_idx] = q_idx
        want1 = np.full(sizes[1], -1); want1[q_idx] = r_idx
        assert np.array_equal(after[0][1], want0) and np.array_equal(after[1][0], want1)
        for v, rows in ((0, (0, 2)), (1, (1, 2)), (2, (0, 1, 2))):
            for row in rows:
                assert same_bits(after[v][row], before[v][row]), (v, row)
        r, q, rp, qp = store.pairs(0, 1)                        # entries > 0 only (quirk Q3): all five here
        order = np.argsort(r_idx)
        assert np.array_equal(r, r_idx[order]) and np.array_equal(q, q_idx[order])
        # bad indices change nothing
        now = [store.table(v).copy() for v in range(3)]
        for bad_r, bad_q in (([1, 40], [1, 2]), ([1, 2], [1, 25]), ([-1, 2], [1, 2]), ([1, 1], [1, 2]), ([1, 2], [3, 3])):
            with pytest.raises(ValueError):
                store.set_pairs(0, 1, bad_r, bad_q)
        for args in ((0, 0, [1], [1]), (0, 3, [1], [1]), (0, 1, [1, 2], [1])):
            with pytest.raises(ValueError):
                store.set_pairs(*args)
        for v in range(3):
            assert same_bits(store.table(v), now[v])
        store.set_pairs(0, 1, [], [])                           # no pairs: both rows empty
        assert np.all(store.table(0)[1] == -1) and np.all(store.table(1)[0] == -1) and same_bits(store.table(2), now[2])


# ---- the Python entry points --------------------------------------------------------------------------------------------
class View:
    def __init__(self, P, xy, descriptors):
        self.key_pts = [P.HipKeyPoint(float(x), float(y)) for x, y in xy]
        self.key_xy = np.ascontiguousarray(xy, dtype=np.float64)
        self.key_descriptors = descriptors


@pytest.mark.parametrize("planar", [False, True], ids=["general", "plane"])
def test_guided_pairs_on_the_twin_scene(hip, sfm, planar):
    P = sfm.processors
    sc = mg.twin_scene(planar)
    kind = mg.HOMOGRAPHY if planar else mg.FUNDAMENTAL
    model = ("homography", sc.H) if planar else ("fundamental", sc.F)
    ref = mg.reference(sc.norm, sc.que_desc, sc.ref_desc, sc.que_xy, sc.ref_xy, kind, model[1], 4.0)
    want_r, want_q = mg.pairs_of(ref)
    twinned = {(int(sc.true_ref[k]), int(sc.true_que[k])) for k in sc.twinned}
    views = [View(P, sc.ref_xy, sc.ref_desc), View(P, sc.que_xy, sc.que_desc)]
    kt = P.HipDeviceKeyTracker("sift", False, True, False, None)
    try:
        kt.add_new_view(views[0], [])
        kt.add_new_view(views[1], views[:1])
        _pairs, r0, q0 = kt.generate_matched_pairs(0, 1, views)
        assert not (set(zip(r0[0].tolist(), q0[0].tolist())) & twinned)       # the tables hold no twinned match
        up = kt.kt_upload_bytes
        r_idx, q_idx = P.guided_pairs(kt, 0, 1, 2.0, model=model)
        assert kt.kt_upload_bytes == up
        assert r_idx.shape == (1, want_r.shape[0]) and np.array_equal(r_idx[0], want_r) and np.array_equal(q_idx[0], want_q)
        got = set(zip(r_idx[0].tolist(), q_idx[0].tolist()))
        assert len(got & twinned) >= 0.85 * len(twinned)
        _pairs, r1, q1 = kt.generate_matched_pairs(0, 1, views)
        assert np.array_equal(r1, r0) and np.array_equal(q1, q0)              # nothing was written
        if not planar:
            # without a model: the fundamental matrix of verify_pairs over the pairs the tables hold
            auto = P.guided_pairs(kt, 0, 1, 2.0)
            assert auto is not None and kt.twoview_last["hypothesis"] >= 0
            again = P.guided_pairs(kt, 0, 1, 2.0, model=("fundamental", kt.twoview_last["fund_mat"]))
            assert np.array_equal(auto[0], again[0]) and np.array_equal(auto[1], again[1])
            found = set(zip(auto[0][0].tolist(), auto[1][0].tolist()))
            assert len(found & twinned) >= 0.8 * len(twinned)
        version = list(kt._versions)
        r_idx, q_idx = P.guided_pairs(kt, 0, 1, 2.0, model=model, write=True)
        assert kt._versions == [version[0] + 1, version[1] + 1]
        _pairs, r2, q2 = kt.generate_matched_pairs(0, 1, views)
        keep = want_q > 0                                                     # generate_matched_pairs never pairs query key 0 (Q3)
        assert np.array_equal(r2[0], want_r[keep]) and np.array_equal(q2[0], want_q[keep])
        assert np.array_equal(kt.track_list[0].table[1][want_r], want_q) and np.array_equal(kt.track_list[1].table[0][want_q], want_r)
        assert P.guided_pairs(kt, 0, 2) is None and P.guided_pairs(kt, 1, 1) is None
        with pytest.raises(ValueError):
            P.guided_pairs(kt, 0, 1, -1.0, model=model)
        with pytest.raises(ValueError):
            P.guided_pairs(kt, 0, 1, 2.0, model=("affine", sc.F))
    finally:
        kt.kt_release()


def test_guided_matches_over_host_arrays(hip, sfm):
    P = sfm.processors
    sc = mg.twin_scene(False)
    ref = mg.reference(sc.norm, sc.que_desc, sc.ref_desc, sc.que_xy, sc.ref_xy, mg.FUNDAMENTAL, sc.F, 4.0)
    want_r, want_q = mg.pairs_of(ref)
    ep = P.HipEpipolarProcessor(P.RansacConfig(0.01, 0.99, 0.75, 8, 128))
    r_idx, q_idx = ep.guided_matches(sc.que_desc, sc.que_xy, sc.ref_desc, sc.ref_xy, ("fundamental", sc.F))
    assert np.array_equal(r_idx[0], want_r) and np.array_equal(q_idx[0], want_q)
    assert same_bits(ep.guided_last["n_admitted"], ref["n_admitted"])
    with hip.DescriptorSet(hip.MATCH_L2, sc.que_desc) as q, hip.DescriptorSet(hip.MATCH_L2, sc.ref_desc) as r:
        again = ep.guided_matches(q, sc.que_xy, r, sc.ref_xy, ("fundamental", sc.F))
        assert np.array_equal(again[0], r_idx) and np.array_equal(again[1], q_idx) and q.n == sc.que_desc.shape[0]
