"""The evaluation loop of the pose LM's chain kernels in the assembly (odometry_amd/csrc/lm_chain_kernels.hip cross-compiled as
odometry_amd/build.py compiles it; tests/chain_asm.py finds the loop): no GPU needed.

One wave runs the loop's state machine and issues one instruction per four to five cycles whatever its EXEC mask (DESIGN.md
section 5.1), so the loop's instruction count is its time. lm_state_machine_hot takes wave 0's branch on scalar conditions; what it
must not bring back is what the compiler made of a divergent `threadIdx.x < 64`: exec-mask nests for the accept, lambda and
max_iters tests and the level walk, and register copies into and out of temporaries at their merges. The counts of the commit before
that change, with this compiler, are the bounds here (profiles/state_machine_uniform_ab.md, section 2): the whole text of the
kernel's last depth-1 loop — also the rarely taken blocks the layout moves behind the kernel's exit.

lm_fine_kernel's loop read ten spilled scalar pairs before, all of them lane masks that the compiler had hoisted out of the loop:
the solve's six per-column masks, the masks of its matrix load and of its reciprocal pivots, sincos_pair_lanes' lane-group select and
the mask of the lanes that publish a row. Each is now one compare, where it is used, on a per-lane register the compiler cannot see
through (an empty asm): the kernel has 25 scalar spills against 50 and none of them is read inside the loop."""
import os

import pytest

import chain_asm

# (total instructions, v_mov_b32 + v_mov_b64, *saveexec*) inside the evaluation loop, parent build
PARENT_LOOP = {
    "lm_coarse_kernel": (2002, 188, 46),
    "lm_coarse_armed_kernel": (2006, 188, 46),
    "lm_fine_kernel": (2137, 286, 39),
}


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    from odometry_amd import build as b
    if not os.path.exists(b.HIPCC):
        pytest.skip("no hipcc here")
    return chain_asm.compile_chain(os.path.join(str(tmp_path_factory.mktemp("chain_sm")), "chain.s"))


@pytest.mark.parametrize("kernel", list(PARENT_LOOP))
def test_the_loop_is_no_longer_than_before(text, kernel):
    c = chain_asm.counts(chain_asm.loop_instructions(text, kernel))
    print(kernel, c)
    assert c["barriers"] >= 2, "not the evaluation loop"
    total, v_mov, saveexec = PARENT_LOOP[kernel]
    assert c["total"] <= total
    assert c["v_mov"] <= v_mov
    assert c["saveexec"] <= saveexec


def test_fine_kernel_reloads_no_spilled_scalar_in_the_loop(text):
    reloads = chain_asm.spill_reloads_in_loop(text, "lm_fine_kernel")
    print(len(reloads), "reloads of", sorted(chain_asm.spill_registers(text, "lm_fine_kernel")))
    assert not reloads, reloads
