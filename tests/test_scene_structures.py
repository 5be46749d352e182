"""Track-structured scenes (scenes.Structure): the Bernoulli stream the goldens and the benchmark are built from is
unchanged, the generator keeps its invariants, and the oracle's block-sparse BA equals its line-faithful dense
restatement on these structures (every GPU assertion of tests/test_gpu_visibility_structure.py rests on it)."""
import numpy as np
import pytest

from conftest import load_golden

# tools/capture_goldens.py::g6_ba and g6_ba_c2
G6_CASES = [("3x50", 3, 50, 1.0, 11), ("5x200v80", 5, 200, 0.8, 12), ("6x120v60", 6, 120, 0.6, 13),
            ("8x300v50", 8, 300, 0.5, 14), ("C2", 5, 2000, 1.0, 0)]


@pytest.mark.parametrize("case", G6_CASES, ids=[c[0] for c in G6_CASES])
def test_bernoulli_stream_is_unchanged(sfm, case):
    name, nv, npt, vis, seed = case
    g = load_golden("g6_ba_%s.npz" % name)
    sc = sfm.scenes.make_scene(nv, npt, vis, seed=seed)
    for key in ("pt_ptr", "cam_idx", "pt_idx", "uv_pix", "cams_init", "pts_init"):
        assert np.array_equal(getattr(sc, key), g[key]), key


def _structures(st):
    return {
        "tracks": st(mean_track=3.0),
        "heavy": st(mean_track=2.5, heavy=0.05),
        "empty": st(mean_track=3.0, empty=(0, 4, 8)),
        "single": st(mean_track=3.0, single=0.2),
        "clusters": st(mean_track=3.0, clusters=3),
        "hub": st(mean_track=2.0, hub=(0,)),
    }


def _tracks(sc):
    return [sc.cam_idx[sc.pt_ptr[p]:sc.pt_ptr[p + 1]] for p in range(sc.n_pts)]


def _check_csr(sc):
    ptr = sc.pt_ptr
    assert ptr.dtype == np.int32 and sc.cam_idx.dtype == np.int32 and sc.pt_idx.dtype == np.int32
    assert ptr[0] == 0 and ptr[-1] == sc.n_obs and np.all(np.diff(ptr) >= 0)
    assert np.array_equal(sc.pt_idx, np.repeat(np.arange(sc.n_pts), np.diff(ptr)))
    key = sc.pt_idx.astype(np.int64) * sc.n_cams + sc.cam_idx
    assert np.all(np.diff(key) > 0)                   # sorted by (point, camera), no duplicate pair
    assert np.all((sc.cam_idx >= 0) & (sc.cam_idx < sc.n_cams))
    assert sc.uv_pix.shape == (2, sc.n_obs) and np.all(np.isfinite(sc.uv_pix))


@pytest.mark.parametrize("seed", [0, 1, 7])
@pytest.mark.parametrize("kind", ["tracks", "heavy", "empty", "single", "clusters", "hub"])
def test_structure_invariants(sfm, kind, seed):
    St = sfm.scenes.Structure
    st = _structures(St)[kind]
    nv, npt = 12, 400
    sc = sfm.scenes.make_scene(nv, npt, seed=seed, structure=st)
    again = sfm.scenes.make_scene(nv, npt, seed=seed, structure=st)
    for key in ("pt_ptr", "cam_idx", "uv_pix", "cams_init", "pts_init"):
        assert np.array_equal(getattr(sc, key), getattr(again, key)), key          # deterministic by seed
    _check_csr(sc)
    groups = st.groups(nv)
    where = {c: (g, i) for g, cams in enumerate(groups) for i, c in enumerate(cams)}
    births = []
    lens = np.diff(sc.pt_ptr)
    for p, cams in enumerate(_tracks(sc)):
        run = [c for c in cams if c not in st.hub]
        assert len(run) >= 1
        g, i0 = where[run[0]]
        # consecutive views of one group: a run of the group's camera list
        assert [where[c] for c in run] == [(g, i0 + k) for k in range(len(run))], (p, cams)
        births.append(run[0])
        assert all(c in cams for c in st.hub)
    assert np.all(np.diff(births) >= 0)                  # points numbered in birth order
    counts = np.bincount(sc.cam_idx, minlength=nv)
    for c in st.empty:
        assert counts[c] == 0
    if kind == "single":
        assert 0 < np.sum(lens == 1) < npt
        assert abs(np.mean(lens == 1) - st.single) < 0.07
    else:
        assert np.all(lens >= 2)
    if kind == "clusters":
        owner = np.full(npt, -1)
        for g, cams in enumerate(groups):
            seen = np.unique(sc.pt_idx[np.isin(sc.cam_idx, cams)])
            assert np.all(owner[seen] == -1)             # no point is shared by two clusters
            owner[seen] = g
        assert np.all(owner >= 0)
    if kind == "heavy":
        to_end = [p for p, cams in enumerate(_tracks(sc)) if cams[-1] == nv - 1 and len(cams) == nv - cams[0]]
        assert len(to_end) >= int(0.05 * npt)
    if kind == "hub":
        assert counts[0] == npt and np.all(lens >= 3)


def test_track_length_mean_follows_the_setting(sfm):
    """Far from the clip at the last view, the run length has the requested mean."""
    st = sfm.scenes.Structure(mean_track=4.0)
    sc = sfm.scenes.make_scene(400, 20000, seed=2, structure=st)
    lens = np.diff(sc.pt_ptr)
    assert abs(lens.mean() - 4.0) < 0.15 and lens.min() == 2


def test_empty_cameras_stay_empty_without_forced_observations(sfm):
    """The two-camera minimum of the Bernoulli path does not put observations back on an empty camera."""
    st = sfm.scenes.Structure(mean_track=2.0, empty=(0, 1, 3))
    sc = sfm.scenes.make_scene(5, 300, seed=4, structure=st)
    assert set(np.unique(sc.cam_idx)) == {2, 4}
    assert np.all(np.diff(sc.pt_ptr) == 2)


def test_structure_rejects_impossible_settings(sfm):
    St = sfm.scenes.Structure
    for st in (St(mean_track=1.5), St(empty=(0, 1, 2, 3, 4)), St(clusters=3, empty=(0,)), St(hub=(0,), single=0.1),
               St(heavy=0.7, single=0.5)):
        with pytest.raises(ValueError):
            sfm.scenes.make_scene(6, 50, seed=0, structure=st)


def _oracle_cases(St):
    return {
        "empty_first": (8, 120, St(mean_track=3.0, empty=(0,))),
        "empty_middle": (9, 120, St(mean_track=3.0, empty=(4,))),
        "empty_last": (10, 120, St(mean_track=3.0, empty=(9,))),
        "single": (8, 150, St(mean_track=3.0, single=0.2)),
        "two_clusters": (10, 140, St(mean_track=3.0, clusters=2)),
        "heavy_tail": (10, 150, St(mean_track=2.5, heavy=0.05)),
    }


@pytest.mark.parametrize("lam", [0.5, 5.0])
@pytest.mark.parametrize("case", ["empty_first", "empty_middle", "empty_last", "single", "two_clusters", "heavy_tail"])
def test_oracle_sparse_equals_dense_on_structures(sfm, oracle, case, lam):
    nv, npt, st = _oracle_cases(sfm.scenes.Structure)[case]
    sc = sfm.scenes.make_scene(nv, npt, seed=21, structure=st)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    tr_s, tr_d = [], []
    oracle.ba_sparse(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, lam, 3, trace=tr_s)
    oracle.ba_dense(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, lam, 3, trace=tr_d)
    for it, ((cs, ps), (cd, pd)) in enumerate(zip(tr_s, tr_d)):
        assert np.max(np.abs(cs - cd)) <= 1e-12 * np.max(np.abs(cd)), (case, it)
        assert np.max(np.abs(ps - pd)) <= 1e-12 * np.max(np.abs(pd)), (case, it)
        for c in st.empty:
            # a camera without observations: S's block row is lambda I, its rhs 0, so its position never moves and its
            # quaternion changes by no more than the renormalisation
            assert np.array_equal(cs[c, 0:3], sc.cams_init[c, 0:3])
            assert np.max(np.abs(cs[c, 3:7] - sc.cams_init[c, 3:7])) <= 1e-15


def test_oracle_reduced_system_structure(sfm, oracle):
    """The oracle's S has exact zero blocks where no point links two cameras, lambda I for an empty camera, and a
    block-diagonal shape over clusters."""
    St = sfm.scenes.Structure
    sc = sfm.scenes.make_scene(10, 200, seed=5, structure=St(mean_track=3.0, clusters=2, empty=(7,)))
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    t = oracle.ba_reduced_system(sc.cams_init, sc.pts_init, sc.cam_idx, sc.pt_idx, uvn, 0.5)
    linked = structural_blocks(sc)
    blocks = t["S"].reshape(10, 7, 10, 7).transpose(0, 2, 1, 3)
    for a in range(10):
        for b in range(10):
            if a != b and not linked[a, b]:
                assert not np.any(blocks[a, b]), (a, b)
    assert np.array_equal(blocks[7, 7], 0.5 * np.eye(7)) and not np.any(t["rhs"][49:56])
    assert not linked[:5, 5:].any()


def structural_blocks(sc):
    """(V, V) bool: camera pairs that share at least one point (the blocks of S that are not structurally zero)."""
    vis = np.zeros((sc.n_cams, sc.n_pts), dtype=np.int64)
    vis[sc.cam_idx, sc.pt_idx] = 1
    return (vis @ vis.T) > 0
