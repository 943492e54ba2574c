"""Reading the LM chain unit's assembly (odometry_amd/csrc/lm_chain_kernels.hip compiled with -S --cuda-device-only): the text of
one kernel, the blocks of its evaluation loop, instruction counts. Shared by tests/test_chain_statemachine_codeobj.py and by
whoever fills in profiles/state_machine_uniform_ab.md (python tests/chain_asm.py chain.s). No GPU needed.

The evaluation loop is the kernel's LAST loop of depth 1 (the loops in front of it are the prologue's polls and copies). The
compiler marks every block of a loop in the block's comment ("in Loop: Header=BBn_m Depth=1", or "Parent Loop BBn_m Depth=1" on the
loops nested in it), so the loop's text is: the header block and every later block that carries the header's label in such a
comment — also the rarely taken blocks the layout moves behind the kernel's exit."""
import re

KERNELS = ("lm_coarse_kernel", "lm_coarse_armed_kernel", "lm_coarse_full_kernel", "lm_fine_kernel", "lm_fine_trace_kernel",
           "lm_fine_tdist_kernel")
_INSN = re.compile(r"^\t([a-z][a-z0-9_]+)(?:\s|$)")


def compile_chain(out):
    """The chain unit's assembly with odometry_amd/build.py's own flags, written to `out`; returns its text."""
    import subprocess
    from odometry_amd import build as b
    subprocess.run([b.HIPCC] + b._flags_for(b.SRC_CHAIN, b.FLAGS) + ["-S", "--cuda-device-only", "-o", out, b.SRC_CHAIN],
                   check=True, capture_output=True)
    return open(out).read()


def meta(text):
    """{kernel name: {vgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size}} from the code object's metadata."""
    found = {}
    for blk in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        field = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
        vals = {k: int(field(k)) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
        for name in KERNELS:
            if re.search(r"\d+%s[A-Z]" % name, field("name")):
                found[name] = vals
    return found


def kernel_body(text, name):
    """The lines of one kernel, from its label to the end of the function."""
    m = re.search(r"^(_Z\w*\d+%s[A-Z]\w*):" % name, text, re.M)
    assert m, name
    end = text.index(".Lfunc_end", m.end())
    return text[m.end():end].split("\n")


def blocks(lines):
    """[(label or None, [lines])]: a block starts at a .LBBn_m label (a label's own line carries the first loop comment)."""
    out = [(None, [])]
    for ln in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            out.append((m.group(1), [ln]))
        else:
            out[-1][1].append(ln)
    return out


def loop_blocks(lines):
    """The blocks of the kernel's last depth-1 loop (see the module's docstring)."""
    bl = blocks(lines)
    heads = [i for i, (lab, ls) in enumerate(bl) if lab and any(re.search(r"=>This (Inner )?Loop Header: Depth=1\b", l) for l in ls[:4])]
    assert heads, "no depth-1 loop"
    h = heads[-1]
    tag = bl[h][0][2:]   # BBn_m
    mine = re.compile(r"(Header=%s Depth=1\b|Parent Loop %s Depth=1\b)" % (tag, tag))
    out = [bl[h]]
    for lab, ls in bl[h + 1:]:
        if any(mine.search(l) for l in ls if ";" in l):
            out.append((lab, ls))
    return out


def instructions(lines):
    """[(mnemonic, whole line)] of the machine instructions among `lines` (directives, labels and comments left out)."""
    out = []
    for ln in lines:
        m = _INSN.match(ln)
        if m and not m.group(1).startswith("."):
            out.append((m.group(1), ln))
    return out


def loop_instructions(text, name):
    return [i for _, ls in loop_blocks(kernel_body(text, name)) for i in instructions(ls)]


def counts(insns):
    mn = [m for m, _ in insns]
    return {"total": len(mn),
            "v_mov": sum(1 for m in mn if m.startswith("v_mov_b32") or m.startswith("v_mov_b64")),
            "saveexec": sum(1 for m in mn if "saveexec" in m),
            "exec_branch": sum(1 for m in mn if m.startswith("s_cbranch_exec")),
            "s_nop": sum(1 for m in mn if m == "s_nop"),
            "v_readlane": sum(1 for m in mn if m.startswith("v_readlane")),
            "barriers": sum(1 for m in mn if m == "s_barrier")}


def spill_registers(text, name):
    """The VGPRs the kernel keeps spilled scalars in: the destinations of its v_writelane_b32 (the chain's source writes no lane
    itself: every v_writelane in these kernels is the register allocator's)."""
    regs = set()
    for m, ln in instructions(kernel_body(text, name)):
        if m.startswith("v_writelane"):
            regs.add(re.search(r"v_writelane_b32\s+(v\d+)", ln).group(1))
    return regs


def spill_reloads_in_loop(text, name):
    """v_readlane_b32 instructions inside the evaluation loop that read a spill register (the solve's own v_readlane read the
    system's registers, which no v_writelane targets)."""
    regs = spill_registers(text, name)
    out = []
    for m, ln in loop_instructions(text, name):
        if m.startswith("v_readlane"):
            src = re.search(r"v_readlane_b32\s+s\d+,\s*(v\d+)", ln)
            if src and src.group(1) in regs:
                out.append(ln.strip())
    return out


if __name__ == "__main__":
    import sys
    for path in sys.argv[1:]:
        text = open(path).read()
        md = meta(text)
        for name in KERNELS:
            print(path, name, md[name], counts(loop_instructions(text, name)), "spill reloads in loop:", len(spill_reloads_in_loop(text, name)))
