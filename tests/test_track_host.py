"""Host-side contract of the device-resident key tracks: the C ABI additions are exported, nothing works without a GPU,
the new classes carry the reference's signatures, and a full processor leaves everything alone.  No GPU compute."""
import inspect
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO

TRACK_SYMBOLS = {
    "sfm_track_create", "sfm_track_destroy", "sfm_track_info", "sfm_track_add_view", "sfm_track_drop_last_view",
    "sfm_track_match_dedup_dev", "sfm_track_extend_dev", "sfm_track_match_views", "sfm_track_extend_status",
    "sfm_track_kept_copy", "sfm_track_write_kept", "sfm_track_pairs_dev", "sfm_track_pairs", "sfm_track_update_usage",
    "sfm_track_constructed", "sfm_track_unconstructed", "sfm_track_copy_table", "sfm_track_copy_row",
}


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_track_header_symbols_equal_the_new_exports(sfm):
    text = open(os.path.join(REPO, "include", "sfm_hip.h")).read()
    declared = {s for s in re.findall(r"\b(sfm_[a-z0-9_]+)\s*\(", text) if s.startswith("sfm_track_")}
    exported = {s for s in sfm.native.EXPORTS if s.startswith("sfm_track_")}
    assert declared == exported == TRACK_SYMBOLS
    assert "typedef struct sfm_track_store sfm_track_store;" in text
    # the status and info constants of the binding are the header's
    for name in ("TRACK_INFO_N_VIEWS", "TRACK_INFO_N_KEYS", "TRACK_INFO_N_ROWS", "TRACK_INFO_UPLOAD_BYTES",
                 "TRACK_INFO_DOWNLOAD_BYTES", "TRACK_OK", "TRACK_NO_SECOND", "TRACK_ZERO_SECOND", "TRACK_BAD_TRAIN"):
        m = re.search(r"#define SFM_%s\s+(-?\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(sfm.native, name), name


def test_track_source_is_built_without_fast_math(sfm):
    mk = open(os.path.join(REPO, "structure-from-motion_amd", "csrc", "Makefile")).read()
    assert "sfm_track.hip" in mk and "fast-math" not in mk
    src = open(os.path.join(REPO, "structure-from-motion_amd", "csrc", "sfm_track.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    assert "asm" not in re.sub(r"//.*", "", src)


def test_track_store_and_device_tracker_need_a_gpu(sfm):
    if not _no_gpu():
        pytest.skip("GPU present")
    with pytest.raises(sfm.native.SfmHipError):
        sfm.native.TrackStore()
    kt = sfm.processors.HipDeviceKeyTracker("sift", False, True, False, None)

    class V:
        key_pts = [sfm.scenes.KeyPoint(1.0, 2.0)]
        key_descriptors = np.zeros((1, 128), dtype=np.uint8)
    with pytest.raises(sfm.native.SfmHipError):
        kt.add_new_view(V(), [])
    assert kt.track_list == []


def test_new_classes_carry_the_reference_signatures(sfm):
    P = sfm.processors
    with open(os.path.join(GOLDEN, "g11_reference_api.json")) as f:
        g11 = json.load(f)
    want = [name for name, _kind in g11["classes"]["BaProcessor"]["methods"]["process"]]
    assert want == ["self", "img", "k"]
    assert list(inspect.signature(P.HipBaProcessor.process).parameters) == want
    # KeyTracker's and KeyTrack's recorded parameter lists (the reference's key_tracker.py)
    with open(os.path.join(GOLDEN, "g12_keytracker_api.json")) as f:
        g12 = json.load(f)
    public = [n for n in g12["KeyTracker"] if not n.startswith("_KeyTracker__")]
    assert {"__init__", "add_new_view", "generate_matched_pairs", "find_best_view", "is_visible", "clear"} <= set(public)
    for name in public + ["_KeyTracker__extend_list"]:
        assert list(inspect.signature(getattr(P.HipDeviceKeyTracker, name)).parameters) == g12["KeyTracker"][name], name
        assert (list(inspect.signature(getattr(P.HipDeviceKeyTracker, name)).parameters)
                == list(inspect.signature(getattr(P.HipKeyTracker, name)).parameters)), name
    for name in ("update_usage", "extract_constructed_points", "extract_unconstructed_points"):
        assert list(inspect.signature(getattr(P.HipDeviceKeyTrack, name)).parameters) == g12["KeyTrack"][name], name
    # every other public method of the device tracker is an addition of this project, not a changed reference method
    extra = {n for n, _ in inspect.getmembers(P.HipDeviceKeyTracker, inspect.isfunction) if not n.startswith("_")} - set(public)
    assert extra == {"kt_release"}
    assert isinstance(P.HipDeviceKeyTracker.kt_upload_bytes, property)
    # defaults of add_new_view: None everywhere (quirk Q17 turns falsy values into the object's settings)
    sig = inspect.signature(P.HipDeviceKeyTracker.add_new_view)
    assert [p.default for p in list(sig.parameters.values())[3:]] == [None, None, None]


def test_device_tracker_falsy_flags_fall_back_to_the_object(sfm, monkeypatch):
    kt = sfm.processors.HipDeviceKeyTracker("sift", False, True, True, "cfg")
    seen = []
    monkeypatch.setattr(kt, "_KeyTracker__extend_list", lambda *a: seen.append(a[2:]))
    kt.track_list = [object()]                                # not the first view: goes to __extend_list
    kt.add_new_view(object(), [object()], False, False, None)
    assert seen == [(True, True, "cfg")]


def test_invalid_indices_print_the_reference_lines(sfm, capsys):
    kt = sfm.processors.HipDeviceKeyTracker("sift", False, True, False, None)
    assert kt.generate_matched_pairs(0, 1, []) is None
    assert kt.find_best_view(0) == -1
    out = capsys.readouterr().out.splitlines()
    assert out == ["HipDeviceKeyTracker:generate_matched_pairs - invalid ref_idx 0 or invalid que_idx 1",
                   "HipDeviceKeyTracker:find_best_view - invalid input_idx 0"]


def test_process_on_a_full_processor_touches_nothing(sfm, capsys):
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("process touched %s" % name)

    parts = [Untouchable() for _ in range(5)]
    bp = sfm.processors.HipBaProcessor(*parts, filter_size=3)
    bp.curr_data_idx = 3
    assert bp.process(np.zeros((4, 4), dtype=np.uint8), np.eye(3)) is None
    assert capsys.readouterr().out == "Bundle Adjustment processor is full\n"
    assert bp.curr_data_idx == 3
    bp.curr_data_idx = 7                                      # ">=", as in the reference
    assert bp.process(None, None) is None
    assert capsys.readouterr().out == "Bundle Adjustment processor is full\n"


def test_generated_views_carry_their_coordinates(sfm, monkeypatch):
    kp = {"x": np.array([1.5, 2.25], np.float32), "y": np.array([3.0, 0.1], np.float32),
          "size": np.ones(2, np.float32), "angle": np.zeros(2, np.float32), "response": np.ones(2, np.float32),
          "octave": np.zeros(2, np.int32), "descriptors": np.zeros((2, 128), np.float32)}
    monkeypatch.setattr(sfm.native, "sift_detect", lambda img, **kw: kp)
    vp = sfm.processors.HipViewProcessor("sift")
    view = vp.generate_view(np.zeros((8, 8), np.uint8), 0, np.eye(3))
    assert view.key_xy.dtype == np.float64 and view.key_xy.shape == (2, 2)
    assert view.key_xy.tolist() == [list(p.pt) for p in view.key_pts]
    assert sfm.processors.HipDeviceKeyTracker._key_xy(view) is not None
    # a view without the attribute: one pass over key_pts gives the same array
    del view.key_xy
    np.testing.assert_array_equal(sfm.processors.HipDeviceKeyTracker._key_xy(view),
                                  np.array([[1.5, 2.25], [3.0, np.float32(0.1)]]).T.reshape(2, 2))
