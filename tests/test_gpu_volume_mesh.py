"""The TSDF volume's triangle mesh on the GPU (odo_volume_mesh, odo_volume_upload, api.TsdfVolume.mesh / upload / save_mesh_ply)
against the numpy model of tests/test_volume_mesh_cpu.py: upload against download and the point extraction, vertices, normals and
indices bit for bit on integrated and uploaded grids and across the launch geometries, capacities, and the volume's state and
lifecycle round a mesh call."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_volume import _K, _grid_equal, _points_equal, _tracker, _volume, second_rig
from test_rgbd_cpu import drive
from test_volume_cpu import bits, empty_grid, extract_model, integrate_model, params
from test_volume_mesh_cpu import grid_params, mesh_model, pattern_grid, random_grid, read_ply_mesh, tiny_grids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seq():
    return drive()


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _mesh_equal(got, want, tag):
    assert len(got[0]) == len(want[0]) and len(got[2]) == len(want[2]), \
        f"{tag}: {len(got[0])} vertices / {len(got[2])} triangles, the model has {len(want[0])} / {len(want[2])}"
    assert np.array_equal(bits(got[0]), bits(want[0])), f"{tag}: positions differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{tag}: normals / weights differ"
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), f"{tag}: indices differ"


def _uploaded(ctx, p, q, w):
    vol = _volume(ctx, p)
    vol.upload(q, w)
    return vol


def _check_uploaded(ctx, p, q, w, tag):
    vol = _uploaded(ctx, p, q, w)
    want = mesh_model(q, w, p)
    _mesh_equal(vol.mesh(), want, tag)
    vol.close()
    return want


# ---- upload ------------------------------------------------------------------------------------------------------------------------
def test_upload_round_trips_and_feeds_the_extraction(ctx):
    dims = (37, 21, 13)
    p = grid_params(dims)
    q, w = random_grid(dims, 3, holes=0.1, zeros=0.05)
    vol = _volume(ctx, p)
    raw = np.full(p["size"], 900, np.uint16)
    vol.integrate(raw, np.eye(4))
    before = vol.stats()
    assert before["frames"] == 1
    vol.upload(q, w)
    _grid_equal(vol, q, w, "uploaded")
    assert vol.stats() == before                                   # the counters are left as they are
    want = extract_model(q, w, p)
    _points_equal(vol.extract(len(want[0]) + 10), want, "extraction of an uploaded grid")
    assert len(want[0]) > 1000
    assert vol.lib.odo_volume_upload(vol.h, None, None) == -1
    _grid_equal(vol, q, w, "after a refused upload")
    vol.integrate(raw, np.eye(4))                                  # an integration behind an upload works on the uploaded grid
    q2, w2, upd, _ = integrate_model(q, w, raw, np.eye(4), p)
    _grid_equal(vol, q2, w2, "upload + 1 integration")
    assert vol.stats()["frames"] == 2 and vol.stats()["updated"] == upd
    vol.close()


def test_upload_is_refused_while_attached(seq):
    from odometry_amd import _lib as L
    p = params(seq, dims=(32, 16, 24), vs=0.08, origin=(-1.28, 0.9, 3.6))
    trk = _tracker(seq)
    vol = _volume(trk, p)
    q, w = random_grid(p["dims"], 4)
    trk.attach_volume(vol)
    with pytest.raises(L.OdoError, match="attached"):
        vol.upload(q, w)
    _grid_equal(vol, *empty_grid(p), "after the refused upload")
    trk.attach_volume(None)
    vol.upload(q, w)
    _grid_equal(vol, q, w, "detached")
    vol.close()
    trk.close()


# ---- the mesh against the model ----------------------------------------------------------------------------------------------------
def test_pinned_case_matches_the_model_bit_for_bit(ctx, seq):
    p = params(seq)
    vol = _volume(ctx, p)
    q, w = empty_grid(p)
    assert vol.mesh(with_counts=True)[3] == (0, 0, 0, 0)                   # an empty volume
    for n in range(10):
        vol.integrate(seq["depth"][n], seq["poses"][n])
        q, w, _, _ = integrate_model(q, w, seq["depth"][n], seq["poses"][n], p)
        if n + 1 in (1, 10):
            before = vol.stats(), vol.grid()
            want = mesh_model(q, w, p)
            got = vol.mesh()
            print(f"pinned after {n + 1}: {len(got[0])} vertices, {len(got[2])} triangles")
            _mesh_equal(got, want, f"pinned after {n + 1} integrations")
            after = vol.stats(), vol.grid()
            assert before[0] == after[0] and np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
    _points_equal(vol.extract(1 << 20), extract_model(q, w, p), "the point extraction after the mesh")
    vol.clear()
    assert vol.mesh(with_counts=True)[3] == (0, 0, 0, 0)                   # and after clear()
    vol.close()


def test_second_rig_matches_the_model_bit_for_bit(ctx):
    p, frames = second_rig()
    vol = _volume(ctx, p)
    q, w = empty_grid(p)
    for raw, A in frames:
        vol.integrate(raw, A)
        q, w, _, _ = integrate_model(q, w, raw, A, p)
    want = mesh_model(q, w, p)
    assert len(want[0]) > 3000 and len(want[2]) > 3000
    _mesh_equal(vol.mesh(), want, "second rig")
    vol.close()


def test_tiny_cases_match_the_model_bit_for_bit(ctx):
    total = 0
    for n, (p, q, w) in enumerate(tiny_grids()):
        total += len(_check_uploaded(ctx, p, q, w, f"tiny {n}")[2])
    assert total > 100


def test_every_sign_pattern_of_a_cell(ctx):
    q, w = pattern_grid()
    want = _check_uploaded(ctx, grid_params((48, 48, 2)), q, w, "256 patterns")
    assert (len(want[0]), len(want[2])) == (2432, 1920)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_grids_with_holes_and_zeros(ctx, seed):
    dims = [(45, 31, 19), (70, 9, 40)][seed]
    q, w = random_grid(dims, 50 + seed, holes=0.08, zeros=0.05)
    want = _check_uploaded(ctx, grid_params(dims), q, w, f"random {dims}")
    assert len(want[2]) > 10_000 and len(np.unique(bits(want[0])[:, :3], axis=0)) < len(want[0])   # coincident vertices are kept


# The mesh kernels' blocks are 1 024 voxels and the scan walks 1 024 blocks at a time, as the point extraction's do: its rows serve.
GEOMETRIES = {
    "2x2x2": ((2, 2, 2), 0.5),          # one cell, 8 of 1 024 lanes
    "65x5x2": ((65, 5, 2), 0.5),        # one voxel past a wave on x, not a whole block
    "3x85x2": ((3, 85, 2), 0.5),        # rows of 3: every wave holds 21 of them, cells straddle waves
    "1024x32x32": ((1024, 32, 32), 0.03),   # 1 024 blocks: exactly one full scan chunk
    "1025x32x32": ((1025, 32, 32), 0.03),   # 1 025 blocks: one block into the second chunk, rows no multiple of a wave
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_launch_geometries(ctx, name):
    dims, negative = GEOMETRIES[name]
    q, w = random_grid(dims, 7, holes=0.02, zeros=0.01, negative=negative)
    want = _check_uploaded(ctx, grid_params(dims, vs=0.01), q, w, name)
    print(f"{name}: {len(want[0])} vertices, {len(want[2])} triangles")
    assert len(want[2]) > 0


# ---- capacities ----------------------------------------------------------------------------------------------------------------------
def test_capacities(ctx):
    dims = (40, 30, 20)
    p = grid_params(dims)
    q, w = random_grid(dims, 9, holes=0.05, zeros=0.02)
    X, N, T, vkeys, tkeys = mesh_model(q, w, p, detail=True)
    nv, nt = len(X), len(T)
    vol = _uploaded(ctx, p, q, w)
    counts = (C.c_long * 4)(-1, -1, -1, -1)
    assert vol.lib.odo_volume_mesh(vol.h, 0, 0, None, None, None, counts) == 0 and tuple(counts) == (0, nv, 0, nt)
    assert vol.mesh_counts() == (nv, nt)
    vox, first = np.unique(vkeys // 7, return_index=True)
    many = np.nonzero(np.diff(np.append(first, nv)) >= 2)[0]
    v_cut = int(first[many[len(many) // 2]]) + 1                           # the first vertex of a voxel with >= 2, the rest cut off
    cell, first = np.unique(tkeys // 12, return_index=True)
    many = np.nonzero(np.diff(np.append(first, nt)) >= 2)[0]
    t_cut = int(first[many[len(many) // 2]]) + 1                           # the first triangle of a cell with >= 2
    assert 0 < v_cut < nv and 0 < t_cut < nt
    for vc, tc in ((nv - 1, nt), (nv, nt - 1), (v_cut, nt), (nv, t_cut), (v_cut, t_cut), (0, nt), (nv, 0), (nv + 5, nt + 7), (nv, nt)):
        got = vol.mesh(vc, tc, with_counts=True)
        tag = f"capacities {vc} / {tc}"
        assert got[3] == (min(vc, nv), nv - min(vc, nv), min(tc, nt), nt - min(tc, nt)), (tag, got[3])
        _mesh_equal(got[:3], (X[:vc], N[:vc], T[:tc]), tag)               # the prefixes, indices never remapped
    vol.close()


# ---- volume and lifecycle ----------------------------------------------------------------------------------------------------------
def test_mesh_of_an_attached_volume_mid_drive(seq):
    p = params(seq)
    trk = _tracker(seq)
    vol = _volume(trk, p)
    trk.attach_volume(vol)
    dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"][:6], seq["depth"][:6])]
    trk.init(*dev[0])
    for k in range(1, 4):
        assert trk.track(*dev[k])["solve_status"] == 0
    got = vol.mesh()                                                       # waits for the pending integrations
    st = vol.stats()
    assert st["frames"] == 4
    q, w = vol.grid()
    _mesh_equal(got, mesh_model(q, w, p), "attached, after 4 frames")
    for k in range(4, 6):
        assert trk.track(*dev[k])["solve_status"] == 0
    assert vol.stats()["frames"] == 6
    q, w = vol.grid()
    _mesh_equal(vol.mesh(), mesh_model(q, w, p), "attached, after 6 frames")
    vol.close()
    trk.close()


def test_save_mesh_ply(ctx, tmp_path):
    dims = (24, 20, 16)
    p = grid_params(dims)
    q, w = random_grid(dims, 12, holes=0.05)
    vol = _uploaded(ctx, p, q, w)
    path = str(tmp_path / "mesh.ply")
    vol.save_mesh_ply(path)
    vert, face = read_ply_mesh(path)
    X, N, T = mesh_model(q, w, p)
    assert len(face) == len(T) > 0 and face.min() >= 0 and face.max() < len(vert) == len(X)
    assert np.array_equal(bits(vert[:, :3]), bits(X[:, :3])) and np.array_equal(face, T)
    vol.close()
