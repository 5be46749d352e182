#!/usr/bin/env python3
"""kernel_resources.py CSRC_DIR OUT.txt -- registers, scratch, occupancy and LDS of every kernel of the resident-scene files
(sfm_ba_cov, sfm_ba_pcg, sfm_ba_motion, the linearise and backsub kernels of sfm_ba, the shared cost reduction), from
-Rpass-analysis=kernel-resource-usage for gfx950; no GPU needed.  Run it on two checkouts and diff the tables
(profiles/resident_ops/).  File names after OUT.txt replace that list: `... OUT.txt sfm_tri_ransac.hip` gives the table
of the robust triangulation's kernels (profiles/track_ops/)."""
import os
import re
import subprocess
import sys

csrc, out = sys.argv[1], sys.argv[2]
FILES = sys.argv[3:] or ["sfm_ba_cov.hip", "sfm_ba_pcg.hip", "sfm_ba_motion.hip", "sfm_ba.hip", "sfm_ba_host.hip"]
KEEP_BA = ("ba_linearize_kernel", "ba_backsub_kernel")
rows = []
for f in FILES:
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", f, "-o", "/dev/null"],
                       cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        sys.exit(1)
    cur = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1), "file": f}
            rows.append(cur)
            continue
        if cur is None:
            continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r"SGPRs: (\d+)"),
                         ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m and key not in cur:
                cur[key] = int(m.group(1))
names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True,
                       text=True).stdout.splitlines()
lines = []
for r, n in zip(rows, names):
    n = re.sub(r"^void ", "", n).replace("(anonymous namespace)::", "")
    n = re.sub(r"\(.*$", "", n).replace("sfm::", "")
    if r["file"] == "sfm_ba.hip" and not n.startswith(KEEP_BA):
        continue
    if r["file"] == "sfm_ba_host.hip" and not n.startswith("ba_point_cost_reduce_kernel"):
        continue
    lines.append("%-72s %5d %5d %5d %8d %4d %7d %6d" % (n, r.get("vgpr", -1), r.get("agpr", -1), r.get("sgpr", -1),
                                                        r.get("scratch", -1), r.get("occ", -1), r.get("lds", -1),
                                                        r.get("vspill", -1)))
lines.sort()
with open(out, "w") as fh:
    fh.write("%-72s %5s %5s %5s %8s %4s %7s %6s\n" % ("kernel", "VGPR", "AGPR", "SGPR", "scratch", "occ", "LDS B", "vspill"))
    fh.write("\n".join(lines) + "\n")
print(len(lines), "kernels ->", out)
