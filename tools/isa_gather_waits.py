"""Static check of the built library's ISA for the fused render kernels' gathers (gp-nerf_amd/csrc/gpnerf_kernels.hip: gather_view,
the volume gathers): a gather is written as ONE batch of `global_load_dwordx4` -- every tap's address final before the first load,
one memory round trip -- and the compiler may still split it.  When the register allocator computes a later tap's address into a
register that an earlier load of the same batch is still writing, the hardware has to drain that load first: an
`s_waitcnt vmcnt(N)` appears between two loads of the batch, and the batch runs as two or three dependent round trips.  Nothing
computes a different bit, so no golden vector sees it; hence a gate on the code the compiler actually emitted.

The listing is walked linearly per kernel.  A gather group opens at a `global_load_dwordx4` and holds the registers its loads
write.  It closes at the first consumer (an instruction that READS one of those registers -- a dependent load's address
included), at a `; sched_barrier` comment (assembly listings only), a label, a branch, an s_barrier or the kernel's end.  An
instruction that overwrites a group register takes it out of the group (that is the allocator's reuse, not a consumer).  An
`s_waitcnt` with a vmcnt field met while a group is open is remembered; if the next thing that touches the group is another
`global_load_dwordx4` and not a consumer, the wait stood inside the batch: a violation.  (A wait followed by a consumer of an
EARLIER batch's registers is that batch's: software pipelining -- level l reduced while level l + 1 is in flight -- is no violation.)

usage: isa_gather_waits.py lib.so|file.s [kernel substring ...]     exit code 1 if a wait inside a gather group is found"""
import importlib.util
import os
import re
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ("render_fused_kernel", "colour_units_kernel")

_REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
_NO_DST = ("global_store", "scratch_store", "buffer_store", "flat_store", "ds_write", "ds_store", "v_cmpx", "exp", "global_atomic")


def _hazards():
    spec = importlib.util.spec_from_file_location("isa_mfma_hazards", os.path.join(_HERE, "isa_mfma_hazards.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _regs(operand):
    out = set()
    for m in _REG.finditer(operand):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def _split(t):
    """'op a, b, c mods' -> (op, [operands])"""
    parts = t.split(None, 1)
    ops = [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []
    return parts[0], ops


def check(rows):
    """rows: [(line number, text)] of one kernel -> (gather loads seen, [(line, text, why)])"""
    group, x4_in_group, waits = set(), 0, []
    older = set()                                           # registers of closed groups' loads, possibly not consumed yet
    loads, bad = 0, []

    def close(hard=True):
        nonlocal x4_in_group
        if hard:
            older.clear()
        else:
            older.update(group)
        group.clear()
        waits.clear()
        x4_in_group = 0

    for ln, l in rows:
        if "sched_barrier" in l:
            close()
            continue
        t = l.split("//")[0].split(";")[0].strip()
        if re.match(r"^[0-9a-f]+:\s", t):                  # (objdump with --show-raw-insn or addresses in front)
            t = t.split(":", 1)[1].strip()
        if not t or t.startswith("."):
            if re.match(r"^\.L\w+:", t):
                close()
            continue
        if t.endswith(":") or re.match(r"^[0-9a-f]{8,16} <", t):
            close()
            continue
        op, ops = _split(t)
        if op.startswith(("s_cbranch", "s_branch", "s_barrier", "s_endpgm", "s_setpc", "s_swappc")):
            close()
            continue
        if op == "s_waitcnt":
            if group and re.search(r"vmcnt\(\d+\)", t):
                waits.append((ln, t))
            continue
        if op.startswith("s_"):
            continue
        has_dst = not op.startswith(_NO_DST)
        dst = _regs(ops[0]) if (has_dst and ops) else set()
        src = set().union(*[_regs(o) for o in (ops[1:] if has_dst else ops)]) if ops else set()
        if op.startswith(("v_fmac", "v_mac", "v_pk_fmac", "v_dot")):
            src |= dst                                      # accumulating forms read their destination
        if src & group:                                     # a consumer: the batch is over, whatever was waited for was due
            close(hard=False)
        if src & older:                                     # ... or it was due for an EARLIER batch, reduced while this one is in flight
            waits.clear()
        older.difference_update(dst)
        if op == "global_load_dwordx4":
            loads += 1
            if waits and x4_in_group:
                for wl, wt in waits:
                    bad.append((wl, wt, f"between two global_load_dwordx4 of one gather group (next load at line {ln}: `{t}`)"))
            waits.clear()
            x4_in_group += 1
            group |= dst
        elif op.startswith("global_load") or op.startswith("scratch_load") or op.startswith("buffer_load"):
            group -= dst
            if x4_in_group:
                group |= dst                                # (a narrower load inside a batch belongs to it)
        else:
            group -= dst
    return loads, bad


def kernels_of(rows, wants=KERNELS):
    """{mangled name: [(line, text)]} for every kernel whose name contains one of `wants`"""
    hdr = re.compile(r"^(?:[0-9a-f]{8,16} <(_Z\w+)>:|(_Z\w*):)")
    starts = [(i, (m.group(1) or m.group(2))) for i, l in enumerate(rows) for m in [hdr.match(l)] if m]
    out = {}
    for j, (s, name) in enumerate(starts):
        if not any(w in name for w in wants):
            continue
        e = starts[j + 1][0] if j + 1 < len(starts) else len(rows)
        e = next((i for i in range(s, e) if rows[i].startswith(".Lfunc_end")), e)
        out[name] = [(i + 1, rows[i]) for i in range(s + 1, e)]
    return out


def short_name(mangled):
    """render_fused_kernel<4,0,3> / colour_units_kernel<0> from the mangled name (form, Loop, Colour as numbers)"""
    m = re.search(r"render_fused_kernelILi(\d+)ELNS\w*?4LoopE(\d+)ELNS\w*?6ColourE(\d+)E", mangled)
    if m:
        return "render_fused_kernel<%s,%s,%s>" % m.groups()
    m = re.search(r"colour_units_kernelILi(\d+)E", mangled)
    if m:
        return "colour_units_kernel<%s>" % m.group(1)
    return mangled


def scan(path, wants=KERNELS):
    """{short name: (gather loads, violations)}"""
    rows = _hazards().listing_of(path)
    return {short_name(n): check(body) for n, body in kernels_of(rows, wants).items()}


def main():
    total = 0
    res = scan(sys.argv[1], tuple(sys.argv[2:]) or KERNELS)
    for name in sorted(res):
        loads, bad = res[name]
        print(f"{name}: {loads} global_load_dwordx4, {len(bad)} wait(s) inside a gather group")
        for ln, t, why in bad:
            print(f"    line {ln}: `{t}`: {why}")
        total += len(bad)
    sys.exit(1 if total else 0)


if __name__ == "__main__":
    main()
