"""Write the g13 SIFT fixtures: upenn frames 1-3 as 640 x 480 gray uint8, plus the reference's recorded poses.

    python tools/capture_sift_fixtures.py /path/to/reference/test_dataset/upenn

Each frame is read with PIL, converted to gray by cvtColor's BGR2GRAY fixed-point rule
((1868 b + 9617 g + 4899 r + 8192) >> 14), and halved by rounded 2 x 2 means ((sum + 2) // 4).  Every file also holds
K (the intrinsics the reference uses for upenn, for the full-size frame) and the reference's recorded result for views
0-2 (results/view_pose.pkl: camera centres and rotations).  The fixtures are data only; the GPU tests read them and
never the reference tree."""
import os
import pickle
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[568.996140852, 0, 643.21055941], [0, 568.988362396, 477.982801038], [0, 0, 1]])


def gray_half(path):
    rgb = np.asarray(Image.open(path).convert("RGB")).astype(np.int32)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    gray = (1868 * b + 9617 * g + 4899 * r + 8192) >> 14
    h, w = gray.shape
    s = gray[:h // 2 * 2, :w // 2 * 2].reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3))
    return ((s + 2) // 4).astype(np.uint8)


def main(upenn):
    with open(os.path.join(upenn, "results", "view_pose.pkl"), "rb") as f:
        locs, rots = pickle.load(f)
    for n in (1, 2, 3):
        img = gray_half(os.path.join(upenn, "image%07d.bmp" % n))
        out = os.path.join(REPO, "tests", "golden", "g13_upenn_%d.npz" % n)
        np.savez_compressed(out, image=img, K=K, centres=np.asarray(locs)[:3], rotations=np.asarray(rots)[:3])
        print(out, img.shape, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
