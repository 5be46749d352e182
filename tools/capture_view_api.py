"""Record the signatures and constructor fields of the reference's View and ViewProcessor (view_processor.py) into
tests/golden/g13_view_api.json, with a placeholder cv2 module, as tools/capture_keytracker_goldens.py does for
KeyTracker.

    python tools/capture_view_api.py /path/to/reference"""
import inspect
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(ref):
    cv = types.ModuleType("cv2")
    cv.SIFT_create = lambda *a, **k: object()
    sys.modules["cv2"] = cv
    sys.path.insert(0, ref)
    import view_processor as vp
    out = {}
    for cls in (vp.View, vp.ViewProcessor):
        methods = {}
        for name, fn in inspect.getmembers(cls, inspect.isfunction):
            if name.startswith("__") and name != "__init__":
                continue
            methods[name] = str(inspect.signature(fn))
        out[cls.__name__] = {"methods": methods}
    view = vp.View(np.zeros((2, 2), np.uint8), 0, np.eye(3), [], None)
    out["View"]["fields"] = sorted(vars(view))
    proc = vp.ViewProcessor('sift')
    out["ViewProcessor"]["fields"] = sorted(vars(proc))
    path = os.path.join(REPO, "tests", "golden", "g13_view_api.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(path)


if __name__ == "__main__":
    main(sys.argv[1])
