"""The C-ABI library loads and exports every symbol include/odometry_hip.h declares (no compute without a GPU)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(odo_[a-z_0-9]+)\s*\(", txt)))


def test_header_symbols_are_exported_and_bound():
    from odometry_amd import _lib
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/odometry_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert sorted(_lib.SIGNATURES) == names
    assert lib.odo_version() >= 100


def test_the_plan_report_is_declared_bound_and_refuses_null():
    """odo_lm_last_plan: which path an optimiser's last Solve took (tests/test_gpu_batch_chain_cases.py reads every route from it)."""
    from odometry_amd import _lib, api
    lib = _lib.load()
    assert "odo_lm_last_plan" in declared_symbols() and hasattr(api.LevenbergMarquardtOptimizer, "last_plan")
    restype, argtypes = _lib.SIGNATURES["odo_lm_last_plan"]
    assert restype is C.c_int and len(argtypes) == 2
    out = (C.c_int * 6)(*[7] * 6)
    assert lib.odo_lm_last_plan(None, out) == -1 and "odo_lm_last_plan" in _lib.last_error()
    assert list(out) == [7] * 6


def test_library_is_in_tree_and_has_gfx950_code():
    from odometry_amd import _lib
    assert _lib.LIB_PATH.startswith(ROOT)
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for k in (b"lm_residual_dense_kernel", b"depth_disparity_kernel", b"pyrdown_kernel"):
        assert k in blob


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from odometry_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.odo_ctx_create(0, C.byref(h)) == -1
    assert "no HIP device" in _lib.last_error() or "failed" in _lib.last_error()
    from odometry_amd import api
    with pytest.raises(_lib.OdoError):
        api.Context(0)


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "odometry_amd")
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith((".py", ".h", ".hip", ".hpp", ".cpp")):
                src = open(os.path.join(dp, fn)).read()
                assert "oracle" not in src.replace("the oracle", "").replace("against the oracle", "") or fn == "odo_math.h", \
                    f"{fn} mentions the oracle"


def test_kernel_register_budgets():
    """Register budgets that are part of how the kernels share the chip (read from the built code object's metadata; no GPU needed).
    lm_fine_kernel's 32 workgroups hold one CU each of an XCD for a whole Solve while the depth stream's kernels run on the same CUs:
    at <= 208 VGPRs (two waves per SIMD = 416 of 512) the depth stream's 256-thread blocks still fit beside a workgroup; a build that
    drifted to 247 had nothing left and the depth job of the next frame slowed from ~200 to ~400 us, past the frame time
    (DESIGN.md section 5.1). No kernel may spill."""
    import re
    import shutil
    import subprocess
    import tempfile
    from odometry_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools here")
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        so = os.path.join(td, "lib.so")
        shutil.copy(_lib.LIB_PATH, so)
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        notes = ""
        for f in sorted(os.listdir(td)):
            if "gfx950" in f:
                notes += subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(td, f)], check=True,
                                        capture_output=True, text=True).stdout
    kernels = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and vg and sp and ps:
            kernels[name.group(1)] = (int(vg.group(1)), int(sp.group(1)), int(ps.group(1)))
    assert len(kernels) > 40
    spilling = {k: v for k, v in kernels.items() if v[1] > 0}
    assert not spilling, spilling
    fine = {k: v for k, v in kernels.items() if "lm_fine_kernel" in k}
    assert len(fine) == 2, fine      # the single tracker's and the batched tracker's
    for k, v in fine.items():
        # (batched twin: 229 since the ILP-first scheduler, 233 with round 6's branch-free quadrant selects: the allocation granule is 8 —
        #  240 either way from 233, and two waves per SIMD up to 256)
        assert v[0] <= (240 if "batch" in k else 208), (k, v)
    # depth_lm_persistent_kernel: its 80 workgroups of 512 threads wait for each other, so ALL must be resident on the 32 CUs of one
    # XCD at once: 640 waves / 128 SIMDs = 5 waves per SIMD -> at most 512 / 5 = 102 -> 96 VGPRs (allocation granule 8)
    dp = [v for k, v in kernels.items() if "depth_lm_persistent_kernel" in k]
    assert len(dp) == 1 and dp[0][0] <= 96, dp
    # Scratch memory: a by-value kernel argument whose address escapes (a pointer select between it and global memory is enough) is
    # mirrored in scratch by every lane — round 4 shipped lm_step_kernel that way for a few commits (1 032 B per lane, launches
    # 7.8 -> 18 us, the dense 1080p stream 1 550 -> 1 100 frames/s) and no spill count showed it. No kernel of the hot path may own
    # more than a few dozen bytes of private segment, the LM / depth-LM evaluation kernels none.
    big = {k: v for k, v in kernels.items() if v[2] > 64}
    assert not big, big
    for key in ("lm_step_kernel", "lm_fine_kernel", "lm_fine_tdist_kernel", "depth_lm_persistent_kernel", "depth_lm_step_kernel",
                "lm_dense_eval", "depth_disparity_kernel"):
        hit = {k: v for k, v in kernels.items() if key in k}
        assert hit and all(v[2] == 0 for v in hit.values()), hit
    # lm_fine_tdist_kernel (t-distribution weights, configs[0]'s parameter set) is a build of its own so that the scale loop's
    # registers do not count against lm_fine_kernel's budget
    assert any("lm_fine_tdist_kernel" in k for k in kernels)
