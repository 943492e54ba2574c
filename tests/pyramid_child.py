"""Builds the pyramids of every row of tests/pyramid_cases.py through api.ImagePyramid / api.DepthPyramid, smoothed and not, and writes
every level to an .npz: `python tests/pyramid_child.py OUT.npz [group ...]`. tests/test_gpu_pyramid_cases.py runs it in fresh processes
with ODO_PYR_UNFUSED / ODO_PYR_WIDE_FROM set — the library reads the two once per process — and calls build_levels() itself for the
default path. Nothing is judged here: the parent compares."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import pyramid_cases as PC  # noqa: E402


def build_levels(api, rows):
    """{pyramid_cases.key(row, smooth, level): the level as the GPU library returns it}."""
    out = {}
    for r in rows:
        img = PC.image(r)
        for smooth in PC.SMOOTH:
            if r["kind"] == "image":
                p = api.ImagePyramid(r["levels"], img, smooth)
                get = p.GetPyramidImage
            else:
                p = api.DepthPyramid(r["levels"], img, smooth)
                get = p.GetPyramidDepth
            for l in range(r["levels"]):
                out[PC.key(r, smooth, l)] = get(l)
            p.close()
    return out


def main(argv):
    from odometry_amd import api
    groups = argv[2:] or PC.GROUPS
    rows = [r for r in PC.TABLE if r["group"] in groups]
    np.savez(argv[1], **build_levels(api, rows))
    api.default_context().close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
