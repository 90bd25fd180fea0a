"""The vector-ALU work of a sample-loop step and of a colour unit, counted in the ISA the compiler emitted (tools/isa_valu_count.py):
dividing the views' per-ray arithmetic between the two lane halves (gpnerf_kernels.hip view_axes_halved) has to show as fewer non-MFMA
vector instructions around the same MFMAs, without new scratch.  CPU only: it disassembles the built library."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gp-nerf_amd", "csrc", "libgpnerf_hip.so")

# render_fused_kernel<form, Loop, Colour> by number (tests/test_isa_gathers.py): <0,0,3> = <FORM_F32, PLAIN, UNIFIED>, the headline
HEADLINE, UNITS = "render_fused_kernel<0,0,3>", "colour_units_kernel<0>"
UNIT_MFMAS, STEP_MFMAS = 436, 312      # the colour branch of one 32-entry unit; the density branch of one 32-sample step
# Measured with this tool on the parent commit dca59c8 (same compiler, same flags): non-MFMA v_* instructions of the basic block that
# holds a colour unit's MFMAs, the same over every block of the sample loop (the narrowest loop with a step's MFMAs), scratch B / lane
PARENT = {
    HEADLINE: {"unit": 2090, "step": 2758, "scratch": 44},
    UNITS: {"unit": 1917, "scratch": 0},
}


def _tool():
    spec = importlib.util.spec_from_file_location("isa_valu_count", os.path.join(ROOT, "tools", "isa_valu_count.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _need_objdump():
    if not (shutil.which("llvm-objdump") or os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")):
        pytest.skip("llvm-objdump not available")


_SCAN = {}


def _scan():
    if not _SCAN:
        _SCAN.update(_tool().scan(LIB, ("render_fused_kernelILi0ELNS_4LoopE0ELNS_6ColourE3E", "colour_units_kernelILi0E")))
    return _SCAN


@pytest.mark.parametrize("kernel", [HEADLINE, UNITS])
def test_a_colour_unit_issues_fewer_vector_instructions_around_the_same_mfmas(kernel):
    _need_objdump()
    tool, c = _tool(), _scan()[kernel]
    units = tool.block_with(c, UNIT_MFMAS)
    print(kernel, "blocks with", UNIT_MFMAS, "MFMAs:", units, "parent:", PARENT[kernel]["unit"])
    assert len(units) == 1, c["blocks"]
    assert units[0] < PARENT[kernel]["unit"]


def test_a_sample_loop_step_issues_fewer_vector_instructions_around_the_same_mfmas():
    _need_objdump()
    step = _tool().loop_with(_scan()[HEADLINE], STEP_MFMAS)
    print(HEADLINE, "sample loop (MFMAs, other vector instructions):", step, "parent:", PARENT[HEADLINE]["step"])
    assert step is not None, _scan()[HEADLINE]["loops"]
    assert step[0] == STEP_MFMAS and step[1] < PARENT[HEADLINE]["step"]


@pytest.mark.parametrize("kernel", [HEADLINE, UNITS])
def test_scratch_is_not_above_the_parents(kernel):
    _need_objdump()
    c = _scan()[kernel]
    print(kernel, c["vgpr"], "VGPRs,", c["scratch"], "B scratch per lane; parent:", PARENT[kernel]["scratch"])
    assert c["vgpr"] is not None and c["vgpr"] <= 256
    assert c["scratch"] is not None and c["scratch"] <= PARENT[kernel]["scratch"]


def test_the_counter_cuts_blocks_at_branches_and_their_targets():
    """the tool itself, on a hand-written disassembly: a loop of two blocks (one with MFMAs) behind a prologue"""
    rows = ["\tv_mov_b32_e32 v0, 0                                    // 000000001000: 7E000280",
            "\tv_add_f32_e32 v1, v0, v0                               // 000000001004: 02020100",
            "\tv_mfma_f32_32x32x2_f32 v[0:15], v16, v17, v[0:15]      // 000000001008: D3C00000 04022310",
            "\tv_mul_f32_e32 v2, v1, v1                               // 000000001010: 0A040301",
            "\ts_cbranch_scc1 1                                       // 000000001014: BF850001",
            "\tv_sub_f32_e32 v2, v2, v1                               // 000000001018: 08040302",
            "\tv_mfma_f32_32x32x2_f32 v[0:15], v16, v17, v[0:15]      // 00000000101C: D3C00000 04022310",
            "\ts_cbranch_vccnz 65527                                  // 000000001024: BF87FFF7",
            "\ts_endpgm                                               // 000000001028: BF810000"]
    c = _tool().count(list(enumerate(rows, 1)))
    # the backward branch at 0x1024 goes to 0x1024 + 4 - 9 * 4 = 0x1004; the forward one at 0x1014 to 0x101c
    assert c["blocks"] == [(0x1004, 1, 2), (0x101c, 1, 0)], c["blocks"]
    assert c["loops"] == [(0x1004, 0x1024, 2, 3)], c["loops"]
