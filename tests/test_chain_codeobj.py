"""The LM chain unit's code object (odometry_amd/csrc/lm_chain_kernels.hip), cross-compiled as odometry_amd/build.py compiles it
and read from the assembly's metadata: no GPU needed.

The chain kernels are one latency-bound wave each for most of their time, so what the compiler sets up around them is part of their
speed: a private segment makes every dispatch ask for scratch memory (lm_coarse_kernel once carried 36 bytes of it that no
instruction touched — a spill slot left behind by an eight-dword kernel-argument load that lived across the evaluation loop), a
VGPR spill is a trip to memory inside the evaluation, and lm_fine_kernel's scalar spills are v_writelane / v_readlane pairs in its
loop."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_FINE_SGPR_SPILLS = 50   # lm_fine_kernel's sgpr_spill_count before the evaluation head was reworked, with this compiler


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    from odometry_amd import build as b
    if not os.path.exists(b.HIPCC):
        pytest.skip("no hipcc here")
    out = os.path.join(str(tmp_path_factory.mktemp("chain_codeobj")), "chain.s")
    subprocess.run([b.HIPCC] + b._flags_for(b.SRC_CHAIN, b.FLAGS) + ["-S", "--cuda-device-only", "-o", out, b.SRC_CHAIN],
                   check=True, capture_output=True)
    text = open(out).read()
    found = {}
    for blk in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        field = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
        found[field("name")] = {k: int(field(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    return found


def _one(kernels, name):
    hit = [v for k, v in kernels.items() if re.search(r"\d+%s[A-Z]" % name, k)]
    assert len(hit) == 1, (name, sorted(kernels))
    return hit[0]


def test_the_unit_holds_the_chain_kernels(kernels):
    for name in ("lm_coarse_kernel", "lm_coarse_armed_kernel", "lm_coarse_full_kernel", "lm_fine_kernel", "lm_fine_trace_kernel",
                 "lm_fine_tdist_kernel"):
        _one(kernels, name)


def test_no_kernel_of_the_chain_owns_private_memory_or_spills_vector_registers(kernels):
    bad = {k: v for k, v in kernels.items() if v["private_segment_fixed_size"] != 0 or v["vgpr_spill_count"] != 0}
    assert not bad, bad


def test_fine_kernel_spills_no_more_scalars_than_before(kernels):
    assert _one(kernels, "lm_fine_kernel")["sgpr_spill_count"] <= PARENT_FINE_SGPR_SPILLS
