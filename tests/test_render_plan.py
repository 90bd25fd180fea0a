"""CPU: the launch planner of gpnerf_render_fused, seen through gpnerf_render_plan (host arithmetic, no device).

plan_render() chooses among dozens of launch sequences and lays six regions out in the bytes a caller lends; the kernels trust
both.  This file sweeps the planner's inputs -- ray counts on both sides of every threshold it tests, sample counts at the limits
of the list / mask / split rules, the CU counts GPNERF_FLAG_RESERVE_CUS leaves, every flag and output the planner reads, and
workspaces from nothing to four times the documented size -- and holds every plan to the invariants a kernel needs: regions
aligned, inside the bytes lent and disjoint; a grid that covers the frame; a colour mode the kernel's static_asserts allow.  The
set of (shape, colour, arithmetic) triples the sweep reaches is written down below: a planner change that makes one appear or
vanish has to edit it in the open.

The cross product of the grid is ~10^8 points; the sweep keeps every ray count, sample count, CU count and workspace size and thins
the product (see `points()`), to about a minute of host time."""
import ctypes as C
import importlib
import itertools
import struct
import time

import pytest

L = importlib.import_module("gp-nerf_amd._lib")

SHAPES, COLOURS, SELS = L.SHAPE_NAMES, L.COLOUR_NAMES, L.SEL_NAMES
STATIC, QUEUE, QUEUE_REMAINDER, REMAINDER_UNITS, CHAINED = range(5)
STEP, WAVE, LIST, UNIFIED = range(4)
REF, FOLD, SPLIT, GUARD = range(4)
QUEUE_BYTES = 256
S_LIST = (1, 7, 8, 16, 33, 64, 128, 129, 256, 257, 4000)
CUS_LIST = (256, 248, 192, 56, 8, 4, 7)          # the chip, what GPNERF_FLAG_RESERVE_CUS(8 / 64 / 200 / 248) leaves, and below 8
OUT_NONE, OUT_WEIGHTS, OUT_RAW, OUT_DONE = range(4)
OUT_FACTS = (0, L.PLAN_WEIGHTS, L.PLAN_RAW, L.PLAN_SAMPLES_DONE)

# A call's settings as the planner reads them: (split, early, occ, no_exits, shared, ref_order, folded, out)
#   split: 0 fp32 forms, 1 GPNERF_FLAG_SPLIT_F16, 2 with GPNERF_FLAG_SPLIT_GUARD; occ: 0 off, 1 GPNERF_FLAG_OCC_CULL on a frame
#   without an occupancy volume, 2 with one; out: none / weights / raw / samples_done
FACTORS = (3, 2, 3, 2, 2, 2, 2, 4)
ALL_COMBOS = tuple(itertools.product(*[range(k) for k in FACTORS]))
# every combination that differs from the default call in at most two settings: covers every pair of settings
PAIR_COMBOS = tuple(c for c in ALL_COMBOS if sum(1 for v in c if v) <= 2)


def flags_of(c):
    split, early, occ, no_exits, shared, ref_order, folded, out = c
    fl = (L.FLAG_SPLIT_F16 if split else 0) | (L.FLAG_SPLIT_GUARD if split == 2 else 0) | (L.FLAG_EARLY_TERM if early else 0)
    fl |= (L.FLAG_OCC_CULL if occ else 0) | (L.FLAG_NO_EXITS if no_exits else 0) | (L.FLAG_SHARED_DEVICE if shared else 0)
    fl |= L.FLAG_REF_ORDER if ref_order else 0
    return fl, OUT_FACTS[out] | (L.PLAN_FOLDED if folded else 0) | (L.PLAN_OCC if occ == 2 else 0)


def ray_counts(n_cus, S):
    """1, 31..33; +-1 ray and +-1 tile around every ray count at which a threshold of plan_render flips for this chip (one, 1 1/8,
    1 1/4, two, 2 1/8, four and 4 1/8 rounds of wavefronts: tiles == slots, tiles > slots, rem_tiles * 8 <= slots, tiles < 2 * slots,
    tiles * 4 >= slots * 5); 131072 +- 1 (the size function stops reserving the split partials); 512 x 512, 1024 x 1024; the
    2^26-sample edge of the list for this S."""
    slots = n_cus * 8
    ns = {1, 31, 32, 33, 131071, 131072, 131073, 512 * 512, 1024 * 1024}
    for t in (slots, slots + slots // 8, slots + slots // 8 + 1, (slots * 5) // 4, (slots * 5 + 3) // 4, 2 * slots, 2 * slots + slots // 8,
              4 * slots, 4 * slots + slots // 8):
        for d in (-32, -1, 0, 1, 32, 33):
            ns.add(t * 32 + d)
    if S <= 256:
        ns.update(((1 << 26) // S, (1 << 26) // S + 1))
    return sorted(n for n in ns if n >= 1)


def workspaces(W):
    """nothing, less than / exactly the queue's counters, the documented size and its neighbours, fractions of it (the 48 MB cap of
    tests/test_gpu_parity.py among them), four times it"""
    return (0, 255, 256, W, max(W - 256, 0), W + 256, W // 2, W // 4, W // 16, (W * 3) // 4, min(W, 48 << 20), 4 * W)


def points():
    """(n_cus, n_rays, S, combo, workspace index).  The thinning keeps every value of every axis and
       * every (n_cus, n_rays, S) with every PAIR_COMBOS setting at the documented workspace size (index 3: invariant 7 compares
         it with four times that) and at three more sizes that rotate through the list;
       * at 256 and 8 CUs every (n_rays, combo) of the FULL flag x output product, at two (S, workspace) pairs that rotate."""
    for n_cus in CUS_LIST:
        for si, S in enumerate(S_LIST):
            for ni, n in enumerate(ray_counts(n_cus, S)):
                for ci, c in enumerate(PAIR_COMBOS):
                    yield n_cus, n, S, c, 3
                    r = ni * 5 + ci * 3 + si
                    for k in range(3):
                        yield n_cus, n, S, c, (r + 4 * k) % 12
    for n_cus in (256, 8):
        for ni, n in enumerate(ray_counts(n_cus, 257)):         # (the 2^26 edge is S's own: covered above)
            for ci, c in enumerate(ALL_COMBOS):
                if sum(1 for v in c if v) <= 2:
                    continue
                for k in range(2):
                    r = ni * 7 + ci + k * 5
                    yield n_cus, n, S_LIST[r % 11], c, (r // 11 + 6 * k) % 12


def align256(v):
    return (v + 255) & ~255


def list_bytes(n, S):
    """the colour list's block (include/gpnerf_hip.h `workspace`): a 256-byte head, a count per ray, a flag per unit, a 16-byte entry
    per sample + a padded unit per visit of a work unit, a 16-byte result per sample"""
    entries = n * S + (((n + 31) // 32) * 8 + 64) * 32
    return 256 + align256(n * 4) + align256((entries // 32 + 64) * 4) + entries * 16 + n * S * 16


class Planner:
    FMT = "<5iI2i2q22Q"

    def __init__(self):
        self.lib = L.lib()
        self.plan = L.GpnerfRenderPlan()
        assert struct.calcsize(self.FMT) == C.sizeof(self.plan)
        self.ref = C.byref(self.plan)
        self.buf = (C.c_char * C.sizeof(self.plan)).from_buffer(self.plan)
        self.calls = 0

    def __call__(self, n, S, flags, n_cus, facts, ws):
        self.calls += 1
        rc = self.lib.gpnerf_render_plan(n, S, flags, n_cus, facts, ws, self.ref)
        return rc, struct.unpack_from(self.FMT, self.buf)


def check(pt, rc, p, guard_bytes, lbytes):
    """Invariants 1-5 of one plan.  p: the unpacked GpnerfRenderPlan; returns nothing, asserts with the point in the message."""
    n_cus, n, S, c, ws = pt
    split16, early, occ, no_exits, shared, ref_order, folded, out = c
    if split16 == 2 and ws < QUEUE_BYTES + guard_bytes:
        assert rc == -1, ("a guarded call without room for the queue's counters and the guard is refused", pt)
        return
    assert rc == 0, (rc, pt)
    sel, colour, shape, waves, split, grid, cus, _, tiles, main_rays = p[:10]
    reg = p[10:22]          # queue, part, chain, list, mask, guard: off, bytes
    clr = p[22:32]
    q_off, q_b, part_off, part_b, ch_off, ch_b, l_off, l_b, m_off, m_b, g_off, g_b = reg
    assert sel == (GUARD if split16 == 2 else SPLIT if split16 else FOLD if folded and not ref_order else REF), pt
    assert cus == n_cus and tiles == (n + 31) // 32 and 1 <= waves <= 8 and split in (1, 2, 4, 8), (pt, p)
    # 1. regions: aligned, inside the bytes lent, disjoint
    spans = []
    for i in range(0, 12, 2):
        off, b = reg[i], reg[i + 1]
        if b:
            assert off % 256 == 0 and off + b <= ws, ("region misaligned or beyond the workspace", i // 2, pt, p)
            spans.append((off, off + b, i // 2))
    spans.sort()
    for a, b in zip(spans, spans[1:]):
        if a[1] > b[0]:
            # the one documented overlap: under CHAINED the queue's counters are the first control words of the chain block
            assert shape == CHAINED and {a[2], b[2]} == {0, 2} and q_off == ch_off == 0 and q_b <= clr[5], ("regions overlap", pt, p)
    assert not (part_b and l_b), ("split partials and a list share the bytes behind the queue's counters", pt, p)
    for i in range(0, 10, 2):
        off, b = clr[i], clr[i + 1]
        if b:
            assert any(lo <= off and off + b <= hi for lo, hi, _ in spans), ("a cleared range outside every region", i // 2, pt, p)
    # 2. without a workspace
    if ws == 0:
        assert shape == STATIC and split == 1 and not spans and colour in (STEP, WAVE), (pt, p)
    # 3. the guard is where frame.render_fused reads guard_tiles from
    if sel == GUARD:
        assert g_b == guard_bytes and g_off == ((ws - guard_bytes) // 256) * 256, (pt, p)
    else:
        assert g_b == 0, (pt, p)
    # 4. grid and coverage
    rnd = n_cus * 8 * 32
    assert grid >= 1, (pt, p)
    if shape == STATIC:
        assert grid * waves >= tiles * split, ("a static grid that does not cover the frame", pt, p)
    else:
        assert grid <= n_cus and split == 1 and (waves == 8 or shape == QUEUE) and q_b + ch_b > 0, (pt, p)
    if shape == QUEUE_REMAINDER:
        assert main_rays > 0 and main_rays % rnd == 0 and 0 < n - main_rays <= rnd // 8, (pt, p)
    else:
        assert main_rays == n, (pt, p)
    if split > 1:
        assert S // split >= 8 and shape == STATIC and part_b == n * split * 64, (pt, p)
    else:
        assert part_b == 0, (pt, p)
    assert (ch_b > 0) == (shape == CHAINED), (pt, p)
    if shape in (QUEUE_REMAINDER, REMAINDER_UNITS):
        assert q_b == QUEUE_BYTES and S >= 8 and n_cus >= 8 and not early and not occ, (pt, p)       # (both launches' counters: words 0..15)
    if shape == CHAINED:
        assert early and n_cus >= 8 and tiles >= n_cus * 8, (pt, p)
    # 5. the colour mode against what the kernels can do (variant_ok() in gpnerf_kernels.hip, which render_fused_kernel asserts and the variant table is built from)
    assert (colour == STEP) == bool(no_exits or out == OUT_RAW), (pt, p)
    assert (l_b > 0) == (colour in (LIST, UNIFIED)), (pt, p)
    if l_b:
        assert sel in (REF, FOLD) and not occ and l_b == lbytes and shape != STATIC, (pt, p)
        assert S <= 256 and n * S <= 1 << 26, ("a list beyond 2^26 samples", pt, p)
    if colour == UNIFIED:
        assert not shared and shape in (QUEUE, REMAINDER_UNITS), (pt, p)
    if m_b:
        assert S <= 128 and occ == 2 and out not in (OUT_WEIGHTS, OUT_RAW) and shape in (STATIC, QUEUE), (pt, p)
        assert m_b == align256(n * 16) + 2 * align256(tiles * 4), (pt, p)


def key(p):
    """what two plans of one frame have in common when only the diagnostics differ: shape, geometry, grid, main_rays"""
    return (p[2], p[3], p[4], p[5], p[9])


def cannot_list(n, S, c):
    return S > 256 or n * S > 1 << 26 or c[2] != 0


def test_every_plan_of_the_sweep_keeps_the_planners_invariants():
    plan = Planner()
    lib = plan.lib
    reached, examples = set(), {}
    n_points, kinds = 0, {"a": 0, "b": 0}
    t0 = time.time()
    cache_key, W, gb, lb, wss = None, 0, 0, 0, ()
    for pt5 in points():
        n_cus, n, S, c, wi = pt5
        if cache_key != (n, S):
            cache_key = (n, S)
            W, gb, lb = int(lib.gpnerf_render_workspace_bytes(n, S)), int(lib.gpnerf_render_guard_bytes(n)), list_bytes(n, S)
            wss = workspaces(W)
        ws = wss[wi]
        flags, facts = flags_of(c)
        pt = (n_cus, n, S, c, ws)
        rc, p = plan(n, S, flags, n_cus, facts, ws)
        check(pt, rc, p, gb, lb)
        n_points += 1
        if rc:
            continue
        t = (p[2], p[1], p[0])
        if t not in reached:
            reached.add(t)
            examples[t] = pt
        # 6. a plan is a function of the frame and the workspace, not of the diagnostics: the same cut with GPNERF_FLAG_NO_EXITS,
        #    and with a `raw` or a `weights` output -- culled frames included, whose launches then do without the mask (the planner
        #    sets the mask's bytes aside all the same, so that the split partials find the same room)
        if not c[3]:
            rc2, p2 = plan(n, S, flags | L.FLAG_NO_EXITS, n_cus, facts, ws)
            assert rc2 == 0 and key(p2) == key(p), ("GPNERF_FLAG_NO_EXITS changes the plan", pt, p, p2)
        if c[7] == OUT_NONE:
            for twin, name in ((L.PLAN_RAW, "raw"), (L.PLAN_WEIGHTS, "weights")):
                rc2, p2 = plan(n, S, flags, n_cus, facts | twin, ws)
                assert rc2 == 0 and key(p2) == key(p), (f"a {name} output changes the cut of the frame", pt, p, p2)
                assert p2[0] == p[0] and (p2[1] == p[1] or twin == L.PLAN_RAW) and p2[19] == 0, (name, pt, p, p2)     # (no mask with it)
        # 7. the documented size suffices: four times the bytes buy no other plan, except
        #    (a) launches of more than 131072 rays -- for which gpnerf_render_workspace_bytes reserves no split partials, two rounds
        #        of a 256-CU chip -- that cannot list their colour work (S > 256, more than 2^26 samples, GPNERF_FLAG_OCC_CULL): the
        #        size holds no list for them either, and with more bytes choose_geometry may split a tile's samples (the split-
        #        precision forms, which never list, find room for the partials in the bytes the size counts for the list);
        #    (b) chips of at most 8 CUs with launches of at most 32 * 8 * 8 rays, below which the size function reserves no list
        #        (a round of full workgroups on the 8 CUs GPNERF_FLAG_RESERVE_CUS leaves at least): with more bytes they list.
        #    Inside (a) and (b) the smaller workspace's plan is still a valid one: it has just passed invariants 1-6.
        if wi == 3:
            rc4, p4 = plan(n, S, flags, n_cus, facts, 4 * W)
            assert rc4 == 0
            if (p4[0], p4[1]) + key(p4) != (p[0], p[1]) + key(p):
                a = n > 131072 and cannot_list(n, S, c)
                b = n_cus <= 8 and n <= 32 * 8 * 8
                assert a or b, ("the documented workspace size buys a different plan than four times it", pt, p, p4)
                kinds["a" if a else "b"] += 1
    dt = time.time() - t0
    print(f"\nrender plan sweep: {n_points} points ({plan.calls} plans) in {dt:.1f} s; {len(reached)} (shape, colour, sel) triples; "
          f"documented size != 4x: {kinds['a']} of kind (a), {kinds['b']} of kind (b)")
    names = {(SHAPES[s], COLOURS[co], SELS[se]) for s, co, se in reached}
    missing, extra = REACHABLE - names, names - REACHABLE
    assert not missing and not extra, (sorted(missing), {t: examples[(SHAPES.index(t[0]), COLOURS.index(t[1]), SELS.index(t[2]))] for t in extra})
    assert {t[0] for t in names} == set(SHAPES) and {t[1] for t in names} == set(COLOURS) and {t[2] for t in names} == set(SELS)


FORMS4 = ("REF", "FOLD", "SPLIT", "GUARD")
FP32 = ("REF", "FOLD")
# The launch sequences a caller can reach, by plan_render's rules: every shape runs every arithmetic with the colour branch in the
# step (diagnostics) or in the wavefronts' own queues; only the fp32 forms list, only persistent launches do, and only a launch
# that is alone on the list (QUEUE, REMAINDER_UNITS) evaluates it itself (UNIFIED).
REACHABLE = (
    {("STATIC", co, f) for co in ("STEP", "WAVE") for f in FORMS4}
    | {("QUEUE", co, f) for co in ("STEP", "WAVE") for f in FORMS4} | {("QUEUE", co, f) for co in ("LIST", "UNIFIED") for f in FP32}
    | {("QUEUE_REMAINDER", co, f) for co in ("STEP", "WAVE") for f in FORMS4} | {("QUEUE_REMAINDER", "LIST", f) for f in FP32}
    | {("REMAINDER_UNITS", co, f) for co in ("STEP", "WAVE") for f in FORMS4} | {("REMAINDER_UNITS", co, f) for co in ("LIST", "UNIFIED") for f in FP32}
    | {("CHAINED", co, f) for co in ("STEP", "WAVE") for f in FORMS4} | {("CHAINED", "LIST", f) for f in FP32}
)


def test_the_sample_order_and_the_front_test_change_no_plan():
    """GPNERF_FLAG_NEG_RAY | GPNERF_FLAG_FLIP_SAMPLES (the dense renderer on THuman data) is kernel arithmetic only: for every
    reachable (shape, colour, arithmetic) triple the planner returns the same plan -- triple, geometry, grid, main_rays, every
    region and every cleared range -- with the two flags as without, and with either alone.  tests/test_gpu_plans.py relies on it:
    its direction axis renders the forward order's candidate calls flipped and expects the forward order's plans.

    Points: the chip and the 8 CUs GPNERF_FLAG_RESERVE_CUS leaves at least, every ray count and sample count of the sweep above,
    every PAIR_COMBOS setting and every early-terminated launch without exits that differs in one more (the chained launches with the
    colour branch in the step, in the folded and the split forms), at the documented workspace size and at the 48 MB cap that takes
    a frame's list away."""
    plan = Planner()
    lib = plan.lib
    both = L.FLAG_NEG_RAY | L.FLAG_FLIP_SAMPLES
    reached, n_points = set(), 0
    combos = PAIR_COMBOS + tuple(c for c in ALL_COMBOS if c[1] and c[3] and sum(1 for v in c if v) == 3)
    for n_cus in (256, 8):
        for S in S_LIST:
            for n in ray_counts(n_cus, S):
                W = int(lib.gpnerf_render_workspace_bytes(n, S))
                for c in combos:
                    flags, facts = flags_of(c)
                    for ws in (W, min(W, 48 << 20)):
                        rc, p = plan(n, S, flags, n_cus, facts, ws)
                        for extra in (both, L.FLAG_NEG_RAY, L.FLAG_FLIP_SAMPLES):
                            assert plan(n, S, flags | extra, n_cus, facts, ws) == (rc, p), ("the direction changes the plan", extra, (n_cus, n, S, c, ws), p)
                        n_points += 1
                        if rc == 0:
                            reached.add((SHAPES[p[2]], COLOURS[p[1]], SELS[p[0]]))
    print(f"\ndirection sweep: {n_points} points, {len(reached)} triples")
    assert reached == REACHABLE, (sorted(REACHABLE - reached), sorted(reached - REACHABLE))


def test_reserved_cus_plan_as_the_smaller_chip():
    """GPNERF_FLAG_RESERVE_CUS(n) on a chip is the plan of a chip with n fewer CUs (whole XCD rounds of 8, at least 8 stay)."""
    plan = Planner()
    for n_cus, reserve, left in ((256, 8, 248), (256, 64, 192), (256, 200, 56), (256, 255, 8), (256, 7, 256), (304, 48, 256), (8, 8, 8), (4, 8, 4)):
        for n, S in ((70000, 48), (288 * 288, 48), (512 * 512, 64), (2047, 33)):
            for c in ((0, 0, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 0), (2, 0, 0, 0, 0, 0, 0, 0)):
                flags, facts = flags_of(c)
                W = int(plan.lib.gpnerf_render_workspace_bytes(n, S))
                a = plan(n, S, flags | (reserve << 24), n_cus, facts, W)
                b = plan(n, S, flags, left, facts, W)
                assert a == b and a[0] == 0 and a[1][6] == left, (n_cus, reserve, n, S, c)


def test_the_plan_refuses_what_the_render_call_refuses():
    plan = Planner()
    assert plan(64, 0, 0, 256, 0, 0)[0] == -1 and plan(-1, 8, 0, 256, 0, 0)[0] == -1 and plan(1 << 31, 8, 0, 256, 0, 1 << 20)[0] == -1
    assert plan(64, 8, 0, 0, 0, 0)[0] == -1
    assert plan.lib.gpnerf_render_plan(64, 8, 0, 256, 0, 0, None) == -1
    rc, p = plan(0, 8, 0, 256, 0, 1 << 20)
    assert rc == 0 and not any(p), "an empty ray list launches nothing"
    gb = int(plan.lib.gpnerf_render_guard_bytes(64))
    g = L.FLAG_SPLIT_F16 | L.FLAG_SPLIT_GUARD
    assert plan(64, 8, g, 256, 0, QUEUE_BYTES + gb - 1)[0] == -1 and plan(64, 8, g, 256, 0, QUEUE_BYTES + gb)[0] == 0


def test_render_plan_takes_render_fuseds_keywords():
    """frame.render_plan derives flags, wanted outputs and workspace bytes through the code render_fused uses."""
    import inspect
    fm = importlib.import_module("gp-nerf_amd.frame")
    a, b = inspect.signature(fm.render_fused).parameters, inspect.signature(fm.render_plan).parameters
    assert list(b)[:len(a)] == list(a) and list(b)[len(a):] == ["n_cus"]
    assert all(a[k].default == b[k].default for k in a)
    p = fm.render_plan(None, 512 * 512, 64, n_cus=256)
    assert p.triple() == ("QUEUE", "UNIFIED", "REF") and p.regions()["list"][0] == QUEUE_BYTES
    assert fm.render_plan(None, 512 * 512, 64, n_cus=256, workspace_cap=48 << 20).triple() == ("QUEUE", "WAVE", "REF")
    assert fm.render_plan(None, 512 * 512, 64, n_cus=256, load_balance=False).triple() == ("STATIC", "WAVE", "REF")
    assert fm.render_plan(None, 512 * 512, 128, n_cus=256, early_term=True, fold=True, shared_device=True).triple() == ("CHAINED", "LIST", "FOLD")
    assert fm.render_plan(None, 70000, 48, n_cus=256, split_f16=True).triple() == ("REMAINDER_UNITS", "WAVE", "GUARD")
    assert fm.render_plan(None, 70000, 48, n_cus=256, split_f16=True, want=("samples_done",), exits=False).triple() == ("QUEUE_REMAINDER", "STEP", "GUARD")
    assert fm.render_plan(None, 70000, 48, n_cus=256, reserve_cus=200).n_cus == 56
    with pytest.raises(L.GpnerfError):
        fm.render_plan(None, 4096, 8, n_cus=256, split_f16=True, guard=True, load_balance=False)
