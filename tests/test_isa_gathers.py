"""The fused render kernels' gathers issue each batch of taps in one memory round trip: a gate on the ISA the compiler emitted
(tools/isa_gather_waits.py).  CPU only: it disassembles the built library."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gp-nerf_amd", "csrc", "libgpnerf_hip.so")


def _tool():
    spec = importlib.util.spec_from_file_location("isa_gather_waits", os.path.join(ROOT, "tools", "isa_gather_waits.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _need_objdump():
    if not (shutil.which("llvm-objdump") or os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump")):
        pytest.skip("llvm-objdump not available")


_SCAN = {}


def _scan():
    if not _SCAN:
        _SCAN.update(_tool().scan(LIB))
    return _SCAN


# render_fused_kernel<form, Loop, Colour> by number: forms F32 = 0, SPLIT = 1, SPLIT_GUARD = 2, F32_FIXUP = 3, F32_FOLD = 4; Loop PLAIN = 0,
# CHAINED = 1, CULLED = 2; Colour STEP = 0, WAVE = 1, LIST = 2, UNIFIED = 3
CLEAN = ["render_fused_kernel<0,0,2>", "render_fused_kernel<0,0,3>", "render_fused_kernel<4,0,2>", "render_fused_kernel<4,0,3>",
         "colour_units_kernel<0>", "colour_units_kernel<4>"]

# waits inside a gather group per variant in the build BEFORE gather_view pinned its tap offsets (the parent commit of this test,
# same compiler flags): no variant may hold more than it did then
BEFORE = {
    "render_fused_kernel<0,0,0>": 9, "render_fused_kernel<0,0,1>": 21, "render_fused_kernel<0,1,0>": 34, "render_fused_kernel<0,1,1>": 43,
    "render_fused_kernel<0,1,2>": 35, "render_fused_kernel<0,1,3>": 59, "render_fused_kernel<0,2,0>": 12, "render_fused_kernel<0,2,1>": 18,
    "render_fused_kernel<1,0,0>": 5, "render_fused_kernel<1,0,1>": 9, "render_fused_kernel<1,1,0>": 15, "render_fused_kernel<1,1,1>": 27,
    "render_fused_kernel<1,2,0>": 6, "render_fused_kernel<1,2,1>": 7, "render_fused_kernel<2,0,0>": 5, "render_fused_kernel<2,0,1>": 4,
    "render_fused_kernel<2,1,0>": 20, "render_fused_kernel<2,1,1>": 12, "render_fused_kernel<2,2,0>": 6, "render_fused_kernel<2,2,1>": 5,
    "render_fused_kernel<3,0,0>": 9, "render_fused_kernel<3,2,0>": 12, "render_fused_kernel<4,0,0>": 14, "render_fused_kernel<4,0,1>": 19,
    "render_fused_kernel<4,1,0>": 53, "render_fused_kernel<4,1,1>": 47, "render_fused_kernel<4,1,2>": 35, "render_fused_kernel<4,1,3>": 51,
    "render_fused_kernel<4,2,0>": 14, "render_fused_kernel<4,2,1>": 19,
}


def test_the_scan_finds_every_variant():
    _need_objdump()
    res = _scan()
    assert sorted(res) == sorted(CLEAN + list(BEFORE)), sorted(res)
    assert all(loads >= 60 for loads, _ in res.values()), {k: v[0] for k, v in res.items()}


@pytest.mark.parametrize("kernel", CLEAN)
def test_no_wait_stands_inside_a_gather_of_the_list_forms(kernel):
    """(a) The fp32 forms' plain sample loop with frame-level deferral (LIST, UNIFIED: the headline launch among them) and the list's own
    kernel: every gather's loads issue back to back."""
    _need_objdump()
    loads, bad = _scan()[kernel]
    print(kernel, loads, "loads,", len(bad), "waits inside a gather group")
    assert not bad, bad[:4]


def test_the_checker_flags_a_split_batch_and_passes_a_whole_one():
    """(b) The checker itself, on the listing the compiler produced for one view before the fix (a later tap's address computed INTO a
    register of a load in flight: the hardware drains the load first) and on the same gather with its offsets final beforehand."""
    tool = _tool()
    bad = ["global_load_dwordx4 v[18:21], v18, s[42:43]",
           "global_load_dwordx4 v[22:25], v22, s[42:43]",
           "s_waitcnt vmcnt(1)",
           "v_mad_u32_u24 v21, v26, s39, v27",
           "s_waitcnt vmcnt(0)",
           "v_mad_u32_u24 v25, v26, s39, v28",
           "global_load_dwordx4 v[26:29], v21, s[42:43]",
           "global_load_dwordx4 v[30:33], v25, s[42:43]",
           "s_waitcnt vmcnt(0)",
           "v_pk_fma_f32 v[40:41], v[18:19], v[50:51], v[40:41] op_sel_hi:[1,0,1]"]
    good = ["v_mad_u32_u24 v34, v26, s39, v27",
            "v_mad_u32_u24 v35, v26, s39, v28",
            "global_load_dwordx4 v[18:21], v18, s[42:43]",
            "global_load_dwordx4 v[22:25], v22, s[42:43]",
            "global_load_dwordx4 v[26:29], v34, s[42:43]",
            "global_load_dwordx4 v[30:33], v35, s[42:43]",
            "s_waitcnt vmcnt(3)",
            "v_pk_fma_f32 v[40:41], v[18:19], v[50:51], v[40:41] op_sel_hi:[1,0,1]",
            "s_waitcnt vmcnt(0)",
            "v_pk_fma_f32 v[40:41], v[30:31], v[50:51], v[40:41] op_sel_hi:[1,0,1]",
            "global_load_dwordx4 v[18:21], v60, s[42:43]"]
    rows = lambda ls: list(enumerate(ls, 1))
    loads, found = tool.check(rows(bad))
    assert loads == 4 and [ln for ln, _, _ in found] == [3, 5], found
    assert tool.check(rows(good)) == (5, [])
    # a dependent load (pointer chase: the address IS a loaded value) is a consumer, not a split batch
    chase = ["global_load_dwordx4 v[4:7], v1, s[2:3]", "s_waitcnt vmcnt(0)", "v_lshlrev_b32_e32 v8, 5, v4", "global_load_dwordx4 v[10:13], v8, s[4:5]"]
    assert tool.check(rows(chase)) == (2, [])
    # ... and a sched_barrier (assembly listings) ends a group
    fenced = ["global_load_dwordx4 v[4:7], v1, s[2:3]", "s_waitcnt vmcnt(0)", "; sched_barrier mask(0x00000000)", "global_load_dwordx4 v[10:13], v8, s[4:5]"]
    assert tool.check(rows(fenced)) == (2, [])


@pytest.mark.parametrize("kernel", sorted(BEFORE))
def test_no_other_variant_holds_more_such_waits_than_before(kernel):
    """(c) The variants the change does not clean completely (the split forms' non-batched view gather walks its taps on purpose; the
    chained and culled loops): at most what they held before."""
    _need_objdump()
    loads, bad = _scan()[kernel]
    print(kernel, loads, "loads,", len(bad), "waits inside a gather group; before:", BEFORE[kernel])
    assert len(bad) <= BEFORE[kernel], (len(bad), BEFORE[kernel], bad[:4])
