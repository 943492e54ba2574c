"""The keyframe point-cloud map without a GPU: its C ABI is declared, exported and bound; the odo_math.h world-point and voxel-key
functions the kernels run equal numpy float32 in the stated operation order, bit for bit; the PLY writer's layout; the insertion
kernels in the gfx950 code object (no spills, no private segment)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_SYMBOLS = ["odo_map_create", "odo_map_insert_dev", "odo_map_size", "odo_map_download", "odo_map_stats", "odo_map_keyframe_pose",
               "odo_map_clear", "odo_map_destroy", "odo_tracker_attach_map"]
MAP_KERNELS = ["map_claim_kernel", "map_count_kernel", "map_scan_kernel", "map_scatter_kernel"]


def test_map_symbols_are_declared_exported_and_bound():
    from odometry_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "odometry_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for n in MAP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), f"{n} is not declared in include/odometry_hip.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert "typedef struct odo_map odo_map;" in txt
    from odometry_amd import api
    assert hasattr(api, "PointMap") and hasattr(api.Tracker, "attach_map")


HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include "odo_math.h"
// in:  n, then n x (X, Y, Z, A[16]) and n x (v, size) as float32;  out: n x (xw, yw, zw) float32, n x (ok, k) int32
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  int n = 0;
  if (fread(&n, 4, 1, f) != 1) return 1;
  float* in = (float*)malloc(sizeof(float) * 19 * (size_t)n);
  float* vk = (float*)malloc(sizeof(float) * 2 * (size_t)n);
  if (fread(in, sizeof(float), 19 * (size_t)n, f) != 19 * (size_t)n || fread(vk, sizeof(float), 2 * (size_t)n, f) != 2 * (size_t)n) return 1;
  fclose(f);
  float* w = (float*)malloc(sizeof(float) * 3 * (size_t)n);
  int* k = (int*)malloc(sizeof(int) * 2 * (size_t)n);
  for (int i = 0; i < n; i++) {
    const float* r = in + 19 * (size_t)i;
    odo::world_point(r[0], r[1], r[2], r + 3, &w[3 * i], &w[3 * i + 1], &w[3 * i + 2]);
    int q = 0;
    k[2 * i] = odo::voxel_index(vk[2 * i], vk[2 * i + 1], &q) ? 1 : 0;
    k[2 * i + 1] = k[2 * i] ? q : 0;
  }
  f = fopen(argv[2], "wb");
  fwrite(w, sizeof(float), 3 * (size_t)n, f);
  fwrite(k, sizeof(int), 2 * (size_t)n, f);
  fclose(f);
  return 0;
}
"""


def np_world(X, Y, Z, A):
    """world_point in numpy float32, the stated order: ((a0 X + a4 Y) + a8 Z) + a12, one rounding per operation."""
    A = A.astype(np.float32)
    out = []
    for r in range(3):
        out.append(((A[:, r] * X + A[:, 4 + r] * Y) + A[:, 8 + r] * Z) + A[:, 12 + r])
    return out


def np_voxel(v, size):
    q = np.floor(v.astype(np.float32) / size.astype(np.float32))
    ok = np.abs(q) < np.float32(2 ** 20)
    return ok, np.where(ok, q, 0).astype(np.int32)


def test_world_point_and_voxel_key_match_numpy_float32_bit_for_bit():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no host C++ compiler")
    rng = np.random.default_rng(7)
    n = 100_000
    X = (rng.standard_normal(n) * 10).astype(np.float32)
    Y = (rng.standard_normal(n) * 3).astype(np.float32)
    Z = rng.uniform(0.1, 60, n).astype(np.float32)
    A = (rng.standard_normal((n, 16)) * rng.choice([1e-3, 1.0, 50.0, 1e4], (n, 1))).astype(np.float32)
    A[:, [3, 7, 11]] = 0
    A[:, 15] = 1
    size = rng.choice(np.float32([0.1, 0.05, 0.25, 1.0, 0.3, 1e-3]), n).astype(np.float32)
    v = (rng.standard_normal(n) * rng.choice([1.0, 100.0, 1e4, 1e6], n)).astype(np.float32)
    # values on voxel boundaries and at +-2^20 voxels: exact multiples (power-of-two sizes), float multiples (0.1), and their neighbours
    m = n // 4
    kk = rng.integers(-2 ** 20 - 3, 2 ** 20 + 3, m)
    kk[:16] = [2 ** 20, -2 ** 20, 2 ** 20 - 1, -2 ** 20 + 1, 2 ** 20 + 1, -2 ** 20 - 1, 0, -1, 1, 2 ** 19, -2 ** 19, 3, -3, 2 ** 20, -2 ** 20, 0]
    size[:m] = rng.choice(np.float32([0.25, 0.5, 0.125, 0.1, 0.05]), m)
    v[:m] = (kk.astype(np.float64) * size[:m].astype(np.float64)).astype(np.float32)
    v[m:2 * m] = np.nextafter(v[:m], np.float32(np.inf))
    size[m:2 * m] = size[:m]
    v[2 * m:3 * m] = np.nextafter(v[:m], np.float32(-np.inf))
    size[2 * m:3 * m] = size[:m]
    inp = np.concatenate([X[:, None], Y[:, None], Z[:, None], A], axis=1).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "h.cpp"), os.path.join(td, "h")
        open(src, "w").write(HARNESS)
        subprocess.run([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "odometry_amd", "csrc"),
                        "-o", exe, src], check=True)
        fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.int32(n).tobytes())
            f.write(inp.tobytes())
            f.write(np.stack([v, size], axis=1).astype(np.float32).tobytes())
        subprocess.run([exe, fin, fout], check=True)
        raw = open(fout, "rb").read()
    w = np.frombuffer(raw[:12 * n], np.float32).reshape(n, 3)
    k = np.frombuffer(raw[12 * n:], np.int32).reshape(n, 2)
    ref = np_world(X, Y, Z, A)
    for r in range(3):
        assert np.array_equal(w[:, r].view(np.uint32), ref[r].view(np.uint32)), f"world coordinate {r} differs"
    ok, q = np_voxel(v, size)
    assert np.array_equal(k[:, 0].astype(bool), ok)
    assert np.array_equal(k[:, 1], q)
    # the boundary rows do exercise both sides of the range test and exact multiples
    assert ok[:m].sum() < m and (~ok[:m]).sum() >= 4
    exact = (size[:m] == np.float32(0.25)) & (np.abs(kk) < 2 ** 20)
    assert np.array_equal(q[:m][exact], kk[exact])


def parse_ply(path):
    """Minimal binary little-endian PLY reader: (header lines, structured vertex array)."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    types = {"float": "<f4", "uchar": "u1"}
    fields = [(l.split()[2], types[l.split()[1]]) for l in lines if l.startswith("property")]
    data = np.frombuffer(blob[end:], np.dtype(fields))
    assert len(data) == n
    return lines, data


def test_save_ply_round_trips_with_an_exact_header():
    from odometry_amd import api
    xyzi = np.array([[1.5, -2.0, 3.25, 17.6], [0.0, 1e6, -1e-3, -5.0], [7.0, 8.0, 9.0, 300.0], [1, 2, 3, np.nan]], np.float32)
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "m.ply")
        api.write_ply(p, xyzi)
        lines, data = parse_ply(p)
        assert os.path.getsize(p) == len("\n".join(lines)) + 1 + 4 * 15
    assert lines == ["ply", "format binary_little_endian 1.0", "element vertex 4", "property float x", "property float y",
                     "property float z", "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    for i, c in enumerate("xyz"):
        assert np.array_equal(data[c], xyzi[:, i])
    grey = np.array([17, 0, 255, 0], np.uint8)
    for c in ("red", "green", "blue"):
        assert np.array_equal(data[c], grey)


def test_map_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
    from odometry_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools here")
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "lib.so")
        shutil.copy(_lib.LIB_PATH, so)
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        notes = ""
        for f in sorted(os.listdir(td)):
            if "gfx950" in f:
                notes += subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(td, f)], check=True,
                                        capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        for k in MAP_KERNELS:
            if k in name:
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert sorted(found) == sorted(MAP_KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found
