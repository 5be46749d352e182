#!/usr/bin/env python3
"""Record the Python-level API of the reference's processor classes as data (tests/golden/g11_reference_api.json).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/capture_reference_api.py REFERENCE_DIR

REFERENCE_DIR is a checkout of willSapgreen/structure-from-motion (read-only; nothing of it is copied).  The fixture
holds, per class, the names and parameter lists of the methods the class defines, the class-private (name-mangled)
names the compiled body of ``BaProcessor.process`` calls, and the attributes a few constructor calls leave on the
instance (the calls of ba_processor.py:463-488).  tests/test_integration_reference.py builds stand-in base classes
from it, so that the check of INTEGRATION.md section 1 runs without the reference on the machine.
"""
import argparse
import contextlib
import inspect
import io
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "g11_reference_api.json")
CLASSES = (("triangulation_processor", "TriangulationProcessor"), ("campose_processor", "CamposeProcessor"),
           ("epipolar_processor", "EpipolarProcessor"), ("ba_processor", "BaProcessor"), ("utils", "RansacConfig"))


def class_record(module, cls):
    methods, attributes = {}, {}
    for name, value in vars(cls).items():
        if name in ("__module__", "__doc__", "__dict__", "__weakref__", "__qualname__"):
            continue
        if inspect.isfunction(value):
            methods[name] = [[p.name, p.kind.name] for p in inspect.signature(value).parameters.values()]
        else:
            attributes[name] = type(value).__name__
    return {"module": module, "methods": methods, "attributes": attributes}


def encode(value, args):
    """JSON form of one instance attribute: a constructor argument by position, a plain value, or an array."""
    if not isinstance(value, (bool, int, float, str, type(None))):
        for i, a in enumerate(args):
            if value is a:
                return {"arg": i}
    if isinstance(value, np.ndarray):
        return {"array": value.tolist(), "dtype": str(value.dtype)}
    if isinstance(value, (bool, int, float, str, type(None))):
        return value
    return {"type": type(value).__name__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference project")
    ref = os.path.abspath(ap.parse_args().reference)
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))     # placeholder: imported at module scope, never called here
    mods = {m: __import__(m) for m, _ in CLASSES}
    cls = {c: getattr(mods[m], c) for m, c in CLASSES}

    out = {"classes": {c: class_record(m, cls[c]) for m, c in CLASSES},
           "private_calls": {"BaProcessor.process": [n for n in cls["BaProcessor"].process.__code__.co_names
                                                     if n.startswith("_BaProcessor__")]},
           "instances": []}

    made = {}

    def construct(name, cname, *args):
        with contextlib.redirect_stdout(io.StringIO()):            # some constructors print
            obj = cls[cname](*args)
        arg_json = [{"instance": next(k for k, v in made.items() if v is a)} if any(a is v for v in made.values()) else a
                    for a in args]
        out["instances"].append({"name": name, "class": cname, "args": arg_json,
                                 "attrs": {k: encode(v, args) for k, v in vars(obj).items()}})
        made[name] = obj

    # the calls of ba_processor.py:463-488
    construct("ransac", "RansacConfig", 8.0, 0.99, 0.75, 6, 300)
    construct("tp", "TriangulationProcessor")
    construct("cp", "CamposeProcessor", made["ransac"], 5, 300)
    construct("ep", "EpipolarProcessor", made["ransac"])
    construct("bp", "BaProcessor", None, None, made["ep"], made["tp"], made["cp"])

    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
