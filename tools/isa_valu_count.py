"""Static count of the vector-ALU work of the fused render kernels, from the ISA of the built library: on gfx950 the fp32 MFMA and the
vector ALU do not overlap on a SIMD, so what a sample-loop step or a colour unit costs beside its MFMAs is the number
of other `v_*` instructions it issues.  The listing is obtained as tools/isa_gather_waits.py obtains it (llvm-objdump on the library's
gfx950 code object, or a `hipcc -S` listing) and cut into basic blocks: a block starts at the kernel's entry, at every branch target
and behind every branch.  Reported per kernel:

  * every basic block that contains MFMAs: its MFMA count and its count of non-MFMA `v_*` instructions;
  * every loop that contains MFMAs -- the address span [target, branch] of a backward branch, the widest span per target -- with the
    same two counts over ALL blocks of the span (a sample-loop step is several blocks: the levels' empty-space exits, the list flush,
    the flipped order's second look at the images; blocks a given step does not take are counted too, so the figure is an upper
    bound of one step that moves exactly with the instructions taken out of the step's own blocks);
  * the kernel's VGPR count and scratch bytes per lane (the code object's metadata; a listing carries them as directives).

It looks at instruction classes and counts, nothing else.

usage: isa_valu_count.py lib.so|file.s [kernel substring ...]"""
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

_HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ("render_fused_kernel", "colour_units_kernel")
_BRANCH = ("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def instructions(rows):
    """rows: [(line number, text)] of one kernel -> ([(position, op, branch target position or None)], {label: position}).
    A disassembly gives every instruction's address in its trailing comment and a branch's target as a signed count of dwords
    behind the branch; a listing names labels.  Positions are addresses (disassembly) or instruction ordinals (listing)."""
    out, labels, pending = [], {}, []
    for _, l in rows:
        m = re.match(r"^(\.L\w+):", l.strip())
        if m:
            pending.append(m.group(1))
            continue
        t = l.split("//")[0].split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":") or re.match(r"^[0-9a-f]{8,16} <", t):
            continue
        parts = t.split()
        op = parts[0]
        am = re.search(r"//\s*([0-9A-Fa-f]{6,16}):", l)
        pos = int(am.group(1), 16) if am else len(out)
        for lb in pending:
            labels[lb] = pos
        pending = []
        target = None
        if op.startswith(("s_cbranch", "s_branch")) and len(parts) > 1:
            arg = parts[1].rstrip(",")
            if re.match(r"^-?\d+$", arg) and am:
                d = int(arg) & 0xffff
                target = pos + 4 + 4 * (d - 0x10000 if d & 0x8000 else d)
            else:
                target = arg                                    # a label, resolved below
        out.append((pos, op, target))
    out = [(p, op, labels.get(t) if isinstance(t, str) else t) for p, op, t in out]
    return out, labels


def count(rows):
    """-> {"blocks": [(start, mfma, valu)] for blocks with MFMAs, "loops": [(start, end, mfma, valu)] for loops with MFMAs}"""
    ins, _ = instructions(rows)
    leaders = {ins[0][0]} if ins else set()
    for i, (p, op, tgt) in enumerate(ins):
        if op.startswith(_BRANCH):
            if tgt is not None:
                leaders.add(tgt)
            if i + 1 < len(ins):
                leaders.add(ins[i + 1][0])
    is_mfma = lambda op: op.startswith(("v_mfma", "v_smfma"))
    blocks, cur = [], None
    for p, op, _ in ins:
        if p in leaders or cur is None:
            cur = [p, 0, 0]
            blocks.append(cur)
        if is_mfma(op):
            cur[1] += 1
        elif op.startswith("v_"):
            cur[2] += 1
    spans = {}
    for p, op, tgt in ins:
        if op.startswith(("s_cbranch", "s_branch")) and tgt is not None and tgt <= p:
            spans[tgt] = max(spans.get(tgt, p), p)
    loops = []
    for s, e in sorted(spans.items()):
        mf = sum(1 for p, op, _ in ins if s <= p <= e and is_mfma(op))
        va = sum(1 for p, op, _ in ins if s <= p <= e and op.startswith("v_") and not is_mfma(op))
        if mf:
            loops.append((s, e, mf, va))
    return {"blocks": [tuple(b) for b in blocks if b[1]], "loops": loops}


def resources(path):
    """{mangled kernel name: (VGPRs, scratch bytes per lane)} of a library's gfx950 code object or of a listing"""
    out = {}
    if path.endswith((".s", ".S", ".asm")):
        text = open(path).read()
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
            v = re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2))
            s = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
            out[m.group(1)] = (int(v.group(1)) if v else None, int(s.group(1)) if s else None)
        return out
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = shutil.which("llvm-readelf") or os.path.join(os.path.dirname(objdump), "llvm-readelf")
    tmp = tempfile.mkdtemp(prefix="gpnerf_isa_")
    try:
        lib = os.path.join(tmp, "x.so")
        shutil.copy(path, lib)
        subprocess.run([objdump, "--offloading", lib], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        for co in sorted(glob.glob(lib + ".*gfx950*")):
            notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
            for entry in re.split(r"\n\s*- ", notes):
                n = re.search(r"\.name:\s+(\S+)", entry)
                v = re.search(r"\.vgpr_count:\s+(\d+)", entry)
                s = re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry)
                if n and v and s:
                    out[n.group(1).strip("'\"")] = (int(v.group(1)), int(s.group(1)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return out


def scan(path, wants=KERNELS):
    """{short name: {"blocks", "loops", "vgpr", "scratch"}}"""
    gw = _load("isa_gather_waits")
    rows = _load("isa_mfma_hazards").listing_of(path)
    res = resources(path)
    out = {}
    for name, body in gw.kernels_of(rows, wants).items():
        c = count(body)
        c["vgpr"], c["scratch"] = res.get(name, (None, None))
        out[gw.short_name(name)] = c
    return out


def block_with(c, mfma):
    """the non-MFMA vector instructions of the blocks that hold exactly `mfma` MFMAs"""
    return [va for _, mf, va in c["blocks"] if mf == mfma]


def loop_with(c, mfma):
    """(MFMAs, non-MFMA vector instructions) of the narrowest loop that holds exactly `mfma` MFMAs, or None"""
    hits = sorted((e - s, mf, va) for s, e, mf, va in c["loops"] if mf == mfma)
    return hits[0][1:] if hits else None


def main():
    res = scan(sys.argv[1], tuple(sys.argv[2:]) or KERNELS)
    for name in sorted(res):
        c = res[name]
        print(f"{name}: {c['vgpr']} VGPRs, {c['scratch']} B scratch per lane")
        for s, mf, va in c["blocks"]:
            print(f"    block {s:#x}: {mf} MFMAs, {va} other vector instructions")
        for s, e, mf, va in c["loops"]:
            print(f"    loop {s:#x}..{e:#x}: {mf} MFMAs, {va} other vector instructions")


if __name__ == "__main__":
    main()
