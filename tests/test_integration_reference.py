"""Check of INTEGRATION.md section 1: the HIP mixins placed IN FRONT OF the reference classes.  No GPU call is made --
this pins the Python-level contract (method resolution order, name mangling, signatures, the attributes the reference
constructors set and the mixins read).

The reference is not part of this repository, so its classes are described by data captured from it
(tests/golden/g11_reference_api.json, written by tools/capture_reference_api.py): per class the methods it defines
with their parameter lists, the class-private names ``BaProcessor.process`` calls, and the attributes the constructor
calls of ba_processor.py:463-488 leave on the instance.  The stand-in classes below are built from that record alone."""
import inspect
import json
import os
import types

import numpy as np
import pytest

API = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_reference_api.json")


def _stand_in(name, rec, instances):
    """A class with the reference class's name, methods (same parameter lists, bodies that refuse to run) and class
    attributes; its constructor leaves exactly the attributes the recorded constructor call left."""
    def method(mname, params):
        def fn(*args, **kwargs):
            raise NotImplementedError("stand-in for %s.%s" % (name, mname))
        fn.__name__, fn.__qualname__ = mname, "%s.%s" % (name, mname)
        fn.__signature__ = inspect.Signature([inspect.Parameter(p, getattr(inspect.Parameter, kind)) for p, kind in params])
        return fn

    ns = {m: method(m, params) for m, params in rec["methods"].items() if m != "__init__"}
    ns.update({a: None for a in rec["attributes"]})
    made = [i for i in instances if i["class"] == name]

    def __init__(self, *args):
        call = next(i for i in made if len(i["args"]) == len(args))
        for attr, enc in call["attrs"].items():
            if isinstance(enc, dict) and "arg" in enc:
                value = args[enc["arg"]]
            elif isinstance(enc, dict) and "array" in enc:
                value = np.array(enc["array"], dtype=enc["dtype"])
            else:
                value = enc
            setattr(self, attr, value)

    if "__init__" in rec["methods"]:
        ns["__init__"] = __init__
        __init__.__signature__ = inspect.Signature([inspect.Parameter(p, getattr(inspect.Parameter, kind))
                                                    for p, kind in rec["methods"]["__init__"]])
    return type(name, (), ns)


@pytest.fixture(scope="module")
def api():
    with open(API) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref(api):
    """The reference's modules as stand-ins: ref.ba.BaProcessor, ref.cam.CamposeProcessor, ref.epi.EpipolarProcessor,
    ref.tri.TriangulationProcessor, ref.utils.RansacConfig."""
    alias = {"ba_processor": "ba", "campose_processor": "cam", "epipolar_processor": "epi",
             "triangulation_processor": "tri", "utils": "utils"}
    mods = {short: types.SimpleNamespace() for short in alias.values()}
    for name, rec in api["classes"].items():
        setattr(mods[alias[rec["module"]]], name, _stand_in(name, rec, api["instances"]))
    return types.SimpleNamespace(**mods)


def _subclasses(sfm, ref):
    hip = sfm.processors

    class TriangulationProcessor(hip.HipTriangulationMixin, ref.tri.TriangulationProcessor):
        pass

    class CamposeProcessor(hip.HipCamposeMixin, ref.cam.CamposeProcessor):
        pass

    class BaProcessor(hip.HipBaMixin, ref.ba.BaProcessor):
        pass

    class EpipolarProcessor(hip.HipEpipolarMixin, ref.epi.EpipolarProcessor):
        pass

    return TriangulationProcessor, CamposeProcessor, BaProcessor, EpipolarProcessor


def test_mixins_override_the_hot_path_of_the_real_classes(sfm, ref, api):
    hip = sfm.processors
    tri_cls, cam_cls, ba_cls, epi_cls = _subclasses(sfm, ref)
    overrides = [
        (tri_cls, hip.HipTriangulationMixin, ref.tri.TriangulationProcessor,
         ["nonlinear_triangulate", "construct_jacobian_matrix", "triangulate", "linear_triangulate"]),
        (cam_cls, hip.HipCamposeMixin, ref.cam.CamposeProcessor,
         ["nonlinear_estimate_cam_pose_pnp", "construct_jacobian_matrix", "linear_estimate_cam_pose_pnp",
          "estimate_cam_pose_pnp", "extract_cam_pose_from_essential_mat", "evalulate_cam_pose_cheirality",
          "disambiguate_cam_pose_four"]),
        (epi_cls, hip.HipEpipolarMixin, ref.epi.EpipolarProcessor, ["determine_fundamental_mat", "extract_essential_mat"]),
    ]
    for cls, mixin, base, names in overrides:
        for name in names:
            assert getattr(cls, name) is getattr(mixin, name), (cls.__name__, name)       # the MRO picks the mixin
            assert hasattr(base, name), "the reference has no %s.%s to override" % (base.__name__, name)
            ours = list(inspect.signature(getattr(mixin, name)).parameters)
            theirs = list(inspect.signature(getattr(base, name)).parameters)
            assert ours == theirs, (name, ours, theirs)                                  # same argument names and order
    # the BA entry is a name-mangled private method: `process` calls self.__execute_bundle_adjustment(), which the
    # compiler spells _BaProcessor__execute_bundle_adjustment inside class BaProcessor (ba_processor.py:267)
    mangled = "_BaProcessor__execute_bundle_adjustment"
    assert mangled in api["private_calls"]["BaProcessor.process"]
    assert mangled in vars(ref.ba.BaProcessor)
    assert getattr(ba_cls, mangled) is getattr(hip.HipBaMixin, mangled)
    assert getattr(ba_cls, mangled) is hip.HipBaMixin.execute_bundle_adjustment
    # everything else stays the reference's
    assert ba_cls.process is ref.ba.BaProcessor.process
    assert tri_cls.add_tri_pt is ref.tri.TriangulationProcessor.add_tri_pt


def test_reference_constructors_provide_what_the_mixins_read(sfm, ref, capsys):
    tri_cls, cam_cls, ba_cls, epi_cls = _subclasses(sfm, ref)
    ransac = ref.utils.RansacConfig(8.0, 0.99, 0.75, 6, 300)                      # ba_processor.py:463-480
    tp = tri_cls()                                                                # ba_processor.py:485
    cp = cam_cls(ransac, 5, 300)                                                  # ba_processor.py:486
    ep = epi_cls(ransac)                                                          # ba_processor.py:484
    bp = ba_cls(None, None, ep, tp, cp)                                           # ba_processor.py:487-488
    capsys.readouterr()
    assert (tp.damping_factor, tp.iteration) == (0.5, 100)                        # tri:12 defaults the mixin falls back to
    assert (cp.damping_factor, cp.iteration) == (5, 300) and cp.ransac_config is ransac
    assert ep.ransac is ransac and ep.fund_mat.shape == (3, 3)
    assert (bp.iteration, bp.damping_factor) == (3, 5)                            # ba:24 defaults
    for attr in ("view_processor", "key_tracker", "tri_processor", "campose_processor"):
        assert hasattr(bp, attr)
    assert bp.tri_processor is tp
    # the drop-in's own RansacConfig mirrors the reference's field for field
    ours = sfm.processors.RansacConfig(8.0, 0.99, 0.75, 6, 300)
    capsys.readouterr()
    for field in ("inlier_threshold", "subset_confidence", "sample_confidence", "sample_num", "iteration", "random_seed"):
        assert getattr(ours, field) == getattr(ransac, field), field
    # class-level switches of the mixins do not collide with reference attributes
    for name in ("ba_quirk_flags", "ba_verbose", "ba_resident", "ba_last_action"):
        assert not hasattr(ref.ba.BaProcessor, name)
    assert not hasattr(ref.cam.CamposeProcessor, "quirk_flags")
