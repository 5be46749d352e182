"""CPU-side checks: the C-ABI library builds/loads and exports every symbol the header declares,
fails loudly without a GPU, and the host logic (observation adapter, geometry helpers, scene
generator) behaves like the reference.  No GPU compute here."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden


def test_header_symbols_match_exports(sfm):
    text = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    declared = set(re.findall(r"\b(sfm_[a-z0-9_]+)\s*\(", text))
    declared.discard("sfm_ba_problem")
    assert declared == set(sfm.native.EXPORTS)


def test_library_loads_and_exports_everything(sfm):
    if not os.path.exists(sfm.native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = sfm.native.load()
    for name in sfm.native.EXPORTS:
        assert hasattr(lib, name), name
    assert lib.sfm_version() >= 100


def test_signature_table_matches_the_header(sfm, monkeypatch):
    """native.SIGNATURES is the only place a C signature is written in Python: its keys are EXPORTS, load() alone sets
    argtypes on every symbol, and every argtypes list is as long as the header's parameter list."""
    native = sfm.native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert tuple(native.SIGNATURES) == native.EXPORTS and len(set(native.EXPORTS)) == len(native.EXPORTS)
    text = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    declared = {}
    for name, params in re.findall(r"\b(sfm_[a-z0-9_]+)\s*\(([^()]*)\)", text):
        params = params.strip()
        declared[name] = 0 if params in ("", "void") else params.count(",") + 1
    assert set(declared) == set(native.EXPORTS)
    monkeypatch.setattr(native, "_lib", None)      # a fresh CDLL: no wrapper has been called on its function objects
    lib = native.load()
    for name, n_params in declared.items():
        argtypes = getattr(lib, name).argtypes
        assert argtypes is not None, "%s: load() set no argtypes" % name
        assert len(argtypes) == n_params, "%s: header declares %d parameters, argtypes has %d" % (name, n_params, len(argtypes))
    assert lib.sfm_last_error.restype is ctypes.c_char_p


def test_no_cpu_fallback_without_gpu(sfm):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sfm.native.SfmHipError):
        sfm.native.init(0)
    sc = sfm.scenes.make_scene(3, 20, 1.0, seed=1)
    uvn = sfm.geometry.normalise_pixels(sc.uv_pix, sc.intrinsic)
    with pytest.raises(sfm.native.SfmHipError):
        sfm.native.ba_solve(3, sc.pt_ptr, sc.cam_idx, uvn, sc.cams_init, sc.pts_init, 5.0, 1)
    tp = sfm.processors.HipTriangulationProcessor()
    with pytest.raises(sfm.native.SfmHipError):
        tp.nonlinear_triangulate(np.ones((4, 3)), [np.eye(3, 4)] * 2, [np.ones((3, 3))] * 2)


def test_product_never_imports_oracle():
    pkg = os.path.join(REPO, "structure-from-motion_amd")
    for root, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(root, f)).read()
                assert "sfm_oracle" not in text, os.path.join(root, f)
                assert "import oracle" not in text and "from oracle" not in text, os.path.join(root, f)


def test_observation_adapter_matches_reference_triples(sfm):
    g = load_golden("g7_visible.npz")
    rows = [g["rows"][c, :n] for c, n in enumerate(g["row_len"])]
    pt_ptr, cam_idx, pt_idx, key_idx = sfm.observations.build_observations(rows, int(g["n_pts"]))
    got = np.stack((cam_idx, pt_idx, key_idx), axis=1)
    assert np.array_equal(got, g["triples"])
    assert pt_ptr[-1] == got.shape[0] and np.all(np.diff(pt_ptr) >= 0)
    for p in range(int(g["n_pts"])):
        assert np.all(pt_idx[pt_ptr[p]:pt_ptr[p + 1]] == p)


def test_observation_adapter_random_tables_vs_oracle(sfm, oracle):
    rng = np.random.default_rng(5)
    for trial in range(20):
        nv, npt = int(rng.integers(1, 6)), int(rng.integers(1, 30))
        rows = []
        for c in range(nv):
            nk = int(rng.integers(1, 40))
            row = rng.integers(-1, npt + 3, nk)          # includes ids >= n_pts and duplicates
            rows.append(row)
        pt_ptr, cam_idx, pt_idx, key_idx = sfm.observations.build_observations(rows, npt)
        oc, op, ok = oracle.observation_list(rows, npt)
        assert np.array_equal(cam_idx, oc) and np.array_equal(pt_idx, op) and np.array_equal(key_idx, ok)
    pt_ptr, cam_idx, pt_idx, key_idx = sfm.observations.build_observations([], 4)
    assert pt_ptr.tolist() == [0, 0, 0, 0, 0] and cam_idx.size == 0


def test_geometry_helpers_match_golden(sfm):
    g = load_golden("g3_quat.npz")
    geo = sfm.geometry
    for q, r, rb in zip(g["q"], g["R"], g["R_back"]):
        assert np.max(np.abs(geo.rotation_to_quaternion(r)[:, 0] - q)) < 1e-15
        assert np.max(np.abs(geo.quaternion_to_rotation(q) - rb)) < 1e-15
    got = np.array([geo.is_rotation(m) for m in g["verify_cases"]])
    assert np.array_equal(got, g["verify_verdict"])
    with pytest.raises(ValueError):
        geo.rotation_to_quaternion(np.eye(3) * 1.1)


def test_scene_generator_is_seeded_and_well_formed(sfm):
    a = sfm.scenes.make_scene(6, 200, 0.5, seed=9)
    b = sfm.scenes.make_scene(6, 200, 0.5, seed=9)
    assert np.array_equal(a.uv_pix, b.uv_pix) and np.array_equal(a.cam_idx, b.cam_idx)
    assert a.pt_ptr[0] == 0 and a.pt_ptr[-1] == a.n_obs
    assert np.all(np.diff(a.pt_ptr) >= 2)                       # every point in >= 2 cameras
    for p in range(a.n_pts):
        seg = a.cam_idx[a.pt_ptr[p]:a.pt_ptr[p + 1]]
        assert np.all(np.diff(seg) > 0)
    assert np.allclose(np.linalg.norm(a.cams_init[:, 3:7], axis=1), 1.0)
    r_true = sfm.scenes.reprojection_rmse(a.cams_true, a.pts_true, a)
    assert 0.55 < r_true < 0.85                                 # N(0, 0.5 px) per axis -> ~0.707 px
    c3 = sfm.scenes.CONFIGS["C3"]
    assert (c3["n_cams"], c3["n_pts"], c3["visibility"]) == (50, 20000, 0.6)


def test_observation_tracker_equals_full_rebuild(sfm):
    """The incremental observation diff of the drop-in (observations.ObservationTracker) against build_observations on
    random growing track tables: pure growth must give exactly the missing triples, anything else must ask for a rebuild
    -- including the Q3 corner cases (key index 0, a second key for an observed point) and ids that become valid only when
    the point count grows."""
    obs = sfm.observations
    rng = np.random.default_rng(11)
    rebuilds = grows = 0
    for trial in range(60):
        n_views, n_keys, n_pts = int(rng.integers(1, 4)), int(rng.integers(4, 40)), int(rng.integers(1, 25))
        rows = [np.full(n_keys, -1, dtype=np.int64) for _ in range(n_views)]
        for r in rows:
            k = rng.choice(np.arange(1, n_keys), size=min(n_keys - 1, int(rng.integers(0, n_keys))), replace=False)
            r[k] = rng.choice(n_pts + 5, size=k.shape[0], replace=False) if k.shape[0] <= n_pts + 5 else rng.integers(0, n_pts + 5, k.shape[0])
        tr = obs.ObservationTracker()
        _ptr, cam, pt, key = tr.reset(rows, n_pts)
        have = set(zip(cam.tolist(), pt.tolist(), key.tolist()))
        for step in range(6):
            kind = rng.integers(0, 6)
            rows = [r.copy() for r in rows]
            if kind <= 2:                                   # growth: new points, new entries on free keys, maybe a new view
                n_pts += int(rng.integers(0, 6))
                for r in rows:
                    free = np.flatnonzero(r == -1)
                    free = free[free > 0]
                    if free.size:
                        k = rng.choice(free, size=int(rng.integers(0, min(4, free.size) + 1)), replace=False)
                        r[k] = rng.integers(0, n_pts + 3, k.shape[0])
                if kind == 2:
                    new = np.full(int(rng.integers(3, 30)), -1, dtype=np.int64)
                    k = rng.choice(new.shape[0], size=int(rng.integers(1, new.shape[0])), replace=False)
                    new[k] = rng.integers(0, n_pts + 2, k.shape[0])
                    rows.append(new)
            elif kind == 3 and rows[0].shape[0] > 1:        # an existing entry is altered
                rows[0][int(rng.integers(1, rows[0].shape[0]))] = int(rng.integers(-1, n_pts))
            elif kind == 4:                                 # key index 0 gets an id
                rows[-1][0] = int(rng.integers(0, n_pts))
            else:                                           # nothing changes
                pass
            want = obs.build_observations(rows, n_pts)
            want_set = set(zip(want[1].tolist(), want[2].tolist(), want[3].tolist()))
            got = tr.diff(rows, n_pts)
            if got is None:
                rebuilds += 1
                _ptr, cam, pt, key = tr.reset(rows, n_pts)
                have = set(zip(cam.tolist(), pt.tolist(), key.tolist()))
            else:
                grows += 1
                new = set(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))
                assert len(new) == got[0].shape[0] and not (new & have)
                have |= new
            assert have == want_set, (trial, step, kind)
    assert rebuilds > 10 and grows > 100
    # the key cache returns what gather_normalised_keys returns
    class KP:
        def __init__(self, x, y):
            self.pt = (x, y)

    class V:
        pass
    views = []
    for c in range(3):
        v = V(); v.k = sfm.scenes.UPENN_K; v.key_pts = [KP(float(i + c), float(2 * i - c)) for i in range(50)]
        views.append(v)
    cam_idx = rng.integers(0, 3, 40).astype(np.int32); key_idx = rng.integers(0, 50, 40).astype(np.int32)
    assert np.array_equal(obs.KeyCache().gather_normalised(views, cam_idx, key_idx), obs.gather_normalised_keys(views, cam_idx, key_idx))


def test_observation_tracker_key_zero_then_second_key(sfm):
    """key 0 of a view maps to point X -- alone it is invisible (Q3: np.any tests the index VALUES,
    key_tracker.py:198-204) -- and after a reset a free key k > 0 of the same view is set to X.  The reference (and
    build_observations) now report the point through KEY 0 (key_idx[0][0]); the diff must not emit (cam, X, k)."""
    obs = sfm.observations
    row = np.full(8, -1, dtype=np.int64)
    row[0] = 3
    row[2] = 1
    tr = obs.ObservationTracker()
    _ptr, cam, pt, key = tr.reset([row], 5)
    assert list(zip(cam.tolist(), pt.tolist(), key.tolist())) == [(0, 1, 2)]          # key 0 -> point 3 is invisible
    grown = row.copy()
    grown[5] = 3
    want = obs.build_observations([grown], 5)
    assert sorted(zip(want[1].tolist(), want[2].tolist(), want[3].tolist())) == [(0, 1, 2), (0, 3, 0)]
    got = tr.diff([grown], 5)
    assert got is None                                                                # -> the caller rebuilds
    _ptr, cam, pt, key = tr.reset([grown], 5)
    assert sorted(zip(cam.tolist(), pt.tolist(), key.tolist())) == [(0, 1, 2), (0, 3, 0)]
    # the same with an id that only becomes a point when the point count grows (key 0 is a late id: also a rebuild),
    # and the harmless neighbour: a second key for a point key 0 does NOT map to is plain growth
    row2 = np.full(8, -1, dtype=np.int64)
    row2[0] = 6
    tr2 = obs.ObservationTracker()
    tr2.reset([row2], 5)
    g2 = row2.copy(); g2[4] = 6
    assert tr2.diff([g2], 7) is None
    tr3 = obs.ObservationTracker()
    tr3.reset([row], 5)
    g3 = row.copy(); g3[6] = 4
    got3 = tr3.diff([g3], 5)
    assert got3 is not None and list(zip(got3[0].tolist(), got3[1].tolist(), got3[2].tolist())) == [(0, 4, 6)]


def test_header_is_plain_c_and_links_from_a_c_program(sfm, tmp_path):
    """include/sfm_hip.h is the drop-in boundary: it must compile as C (no C++ types, no torch types) and a plain C program
    must be able to link libsfm_hip.so and call it.  Without a GPU the calls that need one fail with SFM_E_NO_DEVICE and a
    message -- loudly, never through a CPU path."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "sfm_hip.h"
int main(void) {
  double q[4] = {1, 0, 0, 0}, R[9];
  int st = 0;
  if (sfm_version() < 100) return 1;
  int rc = sfm_quat_to_rot(1, q, R, &st);           /* needs a device: SFM_OK on the GPU box, SFM_E_NO_DEVICE here */
  if (rc != SFM_OK && rc != SFM_E_NO_DEVICE) return 2;
  if (rc == SFM_E_NO_DEVICE && strlen(sfm_last_error()) == 0) return 3;
  if (rc == SFM_OK && (R[0] != 1.0 || R[4] != 1.0 || R[8] != 1.0 || st != SFM_OK)) return 4;
  sfm_ba_problem* p = 0;
  if (sfm_ba_destroy(p) != SFM_OK) return 5;         /* destroying a null handle is a no-op */
  /* the communicator API from plain C (round 4): without a device every call reports SFM_E_NO_DEVICE, with one
     sfm_comm_available says whether RCCL can be loaded; a one-rank communicator is then created and destroyed */
  char id[128];
  sfm_comm* comm = 0;
  int ra = sfm_comm_available();
  if (rc == SFM_E_NO_DEVICE && ra != SFM_E_NO_DEVICE) return 6;
  if (rc == SFM_OK && ra == SFM_OK) {
    if (sfm_comm_unique_id(id) != SFM_OK) return 7;
    if (sfm_comm_create(1, 0, id, &comm) != SFM_OK || comm == 0) return 8;
    sfm_comm* bad = 0;
    if (sfm_comm_create(2, 7, id, &bad) != SFM_E_SHAPE || bad != 0) return 9;      /* rank outside the world */
  }
  if (sfm_comm_destroy(comm) != SFM_OK) return 10;   /* null is a no-op as well */
  printf("abi ok rc=%d\n", rc);
  return 0;
}
''')
    exe = tmp_path / "abi"
    libdir = os.path.dirname(sfm.native.LIB_PATH)
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                         "-L", libdir, "-lsfm_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "abi ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-500:])


def test_key_cache_gathers_what_the_uncached_path_gathers(sfm):
    """observations.KeyCache keeps every view's keys (pixels and normalised) between BA calls: whatever order the
    observations come in, it must return gather_normalised_keys' values bit for bit, and notice a replaced key list or
    another intrinsic matrix."""
    obs = sfm.observations
    rng = np.random.default_rng(11)

    class KP:
        def __init__(self, x, y):
            self.pt = (x, y)

    class V:
        pass
    views = []
    for c in range(5):
        v = V()
        v.k = np.array([[800.0 + c, 0, 320], [0, 790.0, 240 + c], [0, 0, 1]])
        v.key_pts = [KP(float(x), float(y)) for x, y in rng.uniform(0, 640, (40, 2))]
        views.append(v)
    cache = obs.KeyCache()
    for order in ("by_point", "runs", "empty"):
        m = 0 if order == "empty" else 120
        cam = rng.integers(0, 5, m).astype(np.int32)
        key = rng.integers(0, 40, m).astype(np.int32)
        if order == "runs":
            cam = np.sort(cam)[::-1].copy()                      # a few runs, not ascending
        assert np.array_equal(cache.gather_normalised(views, cam, key), obs.gather_normalised_keys(views, cam, key))
    cam = np.repeat(np.arange(5, dtype=np.int32), 8); key = np.tile(np.arange(8, dtype=np.int32), 5)
    views[2].k = views[2].k * np.array([[1.01], [1.0], [1.0]])                     # another intrinsic matrix
    views[3].key_pts = [KP(p.pt[0] + 1.0, p.pt[1]) for p in views[3].key_pts]      # another key list
    assert np.array_equal(cache.gather_normalised(views, cam, key), obs.gather_normalised_keys(views, cam, key))


def test_bulk_ransac_samples_replay_random_sample_exactly(sfm):
    """sampling.sample_indices must return what ``[random.sample(range(n), k) for _ in range(count)]`` returns on the same
    generator AND leave the generator where that leaves it (the reference's later draws depend on it:
    campose_processor.py:531, epipolar_processor.py:225) -- populations with many duplicate re-draws, power-of-two
    boundaries, the small-population branch, the global generator."""
    import random
    sampling = sfm.sampling
    cases = [(5000, 6, 300), (86, 6, 300), (87, 8, 120), (128, 6, 100), (129, 6, 100), (255, 8, 64), (256, 8, 64), (4097, 6, 11),
             (40, 6, 50), (85, 6, 30), (8, 8, 20), (600, 6, 300), (2 ** 31 + 5, 6, 20), (2 ** 33, 6, 20), (1000, 6, 3)]
    for seed, (n, k, count) in enumerate(cases):
        a, b = random.Random(seed), random.Random(seed)
        got = sampling.sample_indices(n, k, count, rng=a)
        want = [b.sample(range(n), k) for _ in range(count)]
        assert got == want, (n, k, count)
        assert all(type(i) is int for i in got[0])
        assert a.getstate() == b.getstate(), (n, k, count)
    random.seed(-1)                                           # utils.py:129-174 seeds the global generator like this
    got = sampling.sample_indices(3000, 6, 300)
    after = random.random()
    random.seed(-1)
    want = [random.sample(range(3000), 6) for _ in range(300)]
    assert got == want and random.random() == after
    assert sampling._verified is True                         # the bulk path is what ran, not the fallback


def test_q13_sign_oracle_and_winner_rule_against_the_reference_chain(sfm, golden):
    """q13.det_branch_fires is the reference's det(rot) < 0 decision (campose_processor.py:629) for every one of the 3 600
    hypotheses of the captured per-view chains (g10: instrumented replay of the real RANSAC loop), and
    q13.reference_winner picks the hypothesis the reference kept -- also when scores tie, when the winner is itself a
    hypothesis whose branch fired (sequence 62, view 5), and when nothing has an inlier."""
    q13 = sfm.q13
    for seed in (61, 62, 63):
        g = golden("g10_incremental_%d.npz" % seed)
        kinv = np.linalg.inv(g["K"])
        for c in range(2, int(g["n_views"])):
            pre = "v%d_" % c
            fired, counts, samples, idx = g[pre + "hyp_fired"], g[pre + "hyp_counts"], g[pre + "hyp_samples"], g[pre + "pnp_index"]
            tri = g["v%d_ba_pts" % (c - 1)][:, idx]            # the points the view's PnP saw = the state after the previous BA
            key = g["uv"][c][:, idx]
            got = np.array([q13.det_branch_fires(kinv @ key[:, s.tolist()], tri[:, s.tolist()]) for s in samples])
            assert np.array_equal(got, fired), (seed, c)
            # the device's side of the bargain, emulated: a spared hypothesis scores `counts` under C, a fired one under -C;
            # give the other sign a LARGER count for every third hypothesis so that the lazy walk has to ask
            other = np.where(np.arange(counts.shape[0]) % 3 == 0, counts.max() + 5, 0)
            cpos = np.where(fired, other, counts); cneg = np.where(fired, counts, other)
            asked = []
            h, f = q13.reference_winner(cpos, cneg, lambda k: (asked.append(k), bool(fired[k]))[1])
            assert h == int(np.argmax(counts)) and f == bool(fired[h]), (seed, c)
            assert len(asked) < counts.shape[0]
    assert q13.reference_winner(np.zeros(5, int), np.zeros(5, int), lambda k: False) == (-1, False)
    # ties: the FIRST hypothesis with the best score wins (strict '>' in campose:554)
    assert q13.reference_winner(np.array([3, 7, 7, 2]), np.array([0, 0, 0, 9]), lambda k: False) == (1, False)
    assert q13.reference_winner(np.array([3, 7, 7, 2]), np.array([0, 0, 0, 9]), lambda k: k == 3) == (3, True)
    assert q13.reference_winner(np.array([3, 7, 7, 2]), np.array([0, 0, 7, 9]), lambda k: k == 1) == (2, False)


@pytest.mark.parametrize("nbk", [2, 3, 4, 5, 11, 16, 17, 44, 52])
def test_flow_task_table_is_complete_and_dependency_ordered(sfm, nbk):
    """The data-flow reduced solve (csrc/sfm_ba_flow.h) deals its tasks to the workgroups in table order and is deadlock-free only
    if every task comes after the tasks it waits for.  Restated here from the kernel's waits: a block of L / the rhs row / an
    identity row in column k needs the blocks of its own row and of row k left of k; the closer of row i needs the blocks of
    rows i-3, i-2, i through column i-4; the hand-over block (i, i-1) rows i-1 and i through column i-4.  Blocks within two
    block rows of the diagonal, W_k and X_k come from the chain workgroup, which waits only for hand-overs of earlier columns."""
    tab = sfm.native.flow_tasks(nbk)
    T1, CLOSER, H1, RHS, IDENT = 0, 1, 2, 3, 4
    pos = {}
    for n, (ty, i, k, key) in enumerate(tab.tolist()):
        name = {T1: ("L", i, k), CLOSER: ("L", i, i - 3), H1: ("H1", i), RHS: ("y", k), IDENT: ("X", i, k)}[ty]
        assert name not in pos
        pos[name] = n
    # completeness: every block the chain does not produce has exactly one task
    want = {("L", i, k) for i in range(3, nbk) for k in range(0, i - 2)} | {("H1", i) for i in range(3, nbk)}
    want |= {("y", k) for k in range(nbk)} | {("X", e, k) for e in range(nbk - 1) for k in range(e + 1, nbk)}
    assert set(pos) == want
    assert np.all(np.diff(tab[:, 3]) >= 0)

    def before(dep, n):          # dep produced by the chain, or by an earlier task
        assert dep not in pos or pos[dep] < n, (dep, n)

    for n, (ty, i, k, key) in enumerate(tab.tolist()):
        if ty == T1 or ty == CLOSER:
            k = k if ty == T1 else i - 3
            for m in range(k):
                before(("L", i, m), n); before(("L", k, m), n)
            if ty == CLOSER:
                for m in range(k):
                    before(("L", i - 2, m), n)
        elif ty == H1:
            for m in range(i - 3):
                before(("L", i, m), n); before(("L", i - 1, m), n)
        elif ty == RHS:
            for m in range(k):
                before(("y", m), n); before(("L", k, m), n)
        else:
            for m in range(i, k):
                before(("L", k, m), n)
                if m > i:
                    before(("X", i, m), n)
    assert sfm.native.flow_tasks(1).shape[0] == 0 and sfm.native.flow_tasks(53).shape[0] == 0


@pytest.mark.parametrize("n_cams", [10, 14, 37, 50, 74, 120, 237])
def test_flow_task_table_with_the_reduce_deferred_is_dependency_ordered(sfm, n_cams):
    """sfm_ba_iterate on one GPU leaves the split-K reduce of the dense product to the data-flow launch: the table then starts with
    one task per (camera, quarter of ba_linearize's accumulator rows) and one per 8 rows of every block of S but (0, 0), which the
    chain sums itself.  Restated from the kernel's waits: rows of S on a camera's own 7x7 block need that camera's four sums; a
    block of S is read by the chain (block rows 0-2), by the task of L[i][k] (k <= i-4), by the closer of row i (k = i-3, i-2, i)
    or by its hand-over task (k = i-1); a block of y needs the sums of the cameras in its rows.  Every reader comes after what it
    reads, and the rest of the table is the table of the plain solve in the same order."""
    nbk = (7 * n_cams + 31) // 32
    tab = sfm.native.flow_tasks_deferred(n_cams).tolist()
    T1, CLOSER, H1, RHS, IDENT, CAMSUM, SRED, COST = range(8)
    pos = {}
    for n, (ty, i, k, key) in enumerate(tab):
        name = {CAMSUM: ("cam", i, k), SRED: ("S", i, k, key & 3), COST: ("cost",)}.get(ty, (ty, i, k))
        assert name not in pos
        pos[name] = n
    assert {x for x in pos if x[0] == "cam"} == {("cam", c, part) for c in range(n_cams) for part in range(4)}
    assert {x for x in pos if x[0] == "S"} == {("S", i, k, q) for i in range(1, nbk) for k in range(i + 1) for q in range(4)}
    assert ("cost",) in pos
    plain = [r[:3] for r in sfm.native.flow_tasks(nbk).tolist()]
    assert [r[:3] for r in tab if r[0] < CAMSUM] == plain
    for n, (ty, i, k, key) in enumerate(tab):
        if ty == SRED and k >= i - 1:
            q = key & 3
            for c in range((32 * i + 8 * q) // 7, min(n_cams - 1, (32 * i + 8 * q + 7) // 7) + 1):
                for part in range(4):
                    assert pos[("cam", c, part)] < n
        reads = {T1: [(i, k)], H1: [(i, i - 1)], CLOSER: [(i, i - 3), (i, i - 2), (i, i)]}.get(ty, [])
        for (a, b) in reads:
            for q in range(4):
                assert pos[("S", a, b, q)] < n
        if ty == RHS:
            for c in range((32 * k) // 7, min(7 * n_cams - 1, 32 * k + 31) // 7 + 1):
                for part in range(4):
                    assert pos[("cam", c, part)] < n
    assert sfm.native.flow_tasks_deferred(4).shape[0] == 0 and sfm.native.flow_tasks_deferred(238).shape[0] == 0
