"""Host-side contract of the observation list built from device-resident key tracks: the switch on the BA drop-in, the
C ABI additions and the constants of the binding.  No GPU compute."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW_SYMBOLS = ("sfm_obs_set_normalised", "sfm_obs_build", "sfm_obs_copy",
               "sfm_ba_create_from_tracks", "sfm_ba_sync_tracks", "sfm_ba_get_structure")


def header():
    return open(os.path.join(REPO, "include", "sfm_hip.h")).read()


def test_device_tracks_switch_exists_and_is_off(sfm):
    P = sfm.processors
    assert P.HipBaMixin.ba_device_tracks is False
    assert P.HipBaProcessor.ba_device_tracks is False
    bp = P.HipBaProcessor(None, None, None, None, None)
    assert bp.ba_device_tracks is False and "ba_device_tracks" not in bp.__dict__
    assert "ba_device_tracks" in P.HipBaMixin.__doc__


def test_device_tracks_with_a_host_tracker_is_a_type_error(sfm):
    """The host tracker has no device tables to build from: the call says which attribute asked for them, before it
    touches a view, a point or the device."""
    P = sfm.processors

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("execute_bundle_adjustment touched %s" % name)

    for tracker in (P.HipKeyTracker("sift", False, True, False, None), object()):
        bp = P.HipBaProcessor(Untouchable(), tracker, None, Untouchable(), None)
        bp.ba_device_tracks = True
        with pytest.raises(TypeError, match="ba_device_tracks"):
            bp.execute_bundle_adjustment()
        with pytest.raises(TypeError, match="ba_device_tracks"):
            bp._BaProcessor__execute_bundle_adjustment()
        assert bp.ba_last_action is None and bp.ba_upload_bytes == 0
    # a device tracker passes the type check; without the resident problem there is nothing to keep in step
    bp = P.HipBaProcessor(Untouchable(), P.HipDeviceKeyTracker("sift", False, True, False, None), None, Untouchable(), None)
    bp.ba_device_tracks = True
    bp.ba_resident = False
    with pytest.raises(TypeError, match="ba_resident"):
        bp.execute_bundle_adjustment()


def test_header_declares_the_new_functions(sfm):
    text = header()
    declared = set(re.findall(r"\b(sfm_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in sfm.native.EXPORTS, name
        assert len(re.findall(r"^int %s\(" % name, text, flags=re.M)) == 1, name
    assert re.search(r"int sfm_obs_set_normalised\(sfm_track_store\* s, int view, int n, const double\* u, const double\* v\);", text)
    assert re.search(r"int sfm_obs_build\(sfm_track_store\* s, int n_views, int n_pts, int64_t\* n_obs\);", text)
    for method in ("set_normalised", "build_observations", "observations"):
        assert callable(getattr(sfm.native.TrackStore, method)), method
    for method in ("from_tracks", "sync_tracks", "structure"):
        assert callable(getattr(sfm.native.BaProblem, method)), method


def test_sync_constants_equal_the_header(sfm):
    text = header()
    values = {}
    for name in ("SYNC_REUSE", "SYNC_GROWN", "SYNC_REPLACED", "TRACK_INFO_OBS_VIEWS", "TRACK_INFO_OBS_PTS", "TRACK_INFO_N_OBS"):
        m = re.search(r"#define SFM_%s\s+(-?\d+)" % name, text)
        assert m, name
        values[name] = int(m.group(1))
        assert values[name] == getattr(sfm.native, name), name
    assert len({values[n] for n in ("SYNC_REUSE", "SYNC_GROWN", "SYNC_REPLACED")}) == 3


def test_library_exports_the_new_functions(sfm):
    lib = sfm.native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_host_reference_of_the_list_handles_the_edges(sfm):
    """What the GPU tests compare with: observations.build_observations on no views, no points, and quirk Q3."""
    B = sfm.observations.build_observations
    pt_ptr, cam, pt, key = B([], 0)
    assert pt_ptr.tolist() == [0] and cam.size == pt.size == key.size == 0
    pt_ptr, cam, pt, key = B([np.array([0, -1, 1, 1, 5])], 2)
    assert pt_ptr.tolist() == [0, 0, 1] and cam.tolist() == [0] and pt.tolist() == [1] and key.tolist() == [2]
    pt_ptr, cam, pt, key = B([np.array([1, -1, 1])], 2)                 # visible THROUGH key 0
    assert key.tolist() == [0]
