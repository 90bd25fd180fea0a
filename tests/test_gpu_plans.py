"""GPU: every launch plan of gpnerf_render_fused, run on purpose.

plan_render() (gp-nerf_amd/csrc/gpnerf_kernels.hip) picks one of dozens of launch sequences from the ray count, the sample count,
the flags, the outputs, the device's CU count and the bytes of workspace; tests/test_render_plan.py holds the planner's arithmetic to
its invariants on the host.  Here each reachable plan is rendered: a helper asks frame.render_plan for the plan a candidate call
gets on THIS device (sizes are multiples of its round of wavefronts, not of 256 CUs), every test asserts the plan before it renders
and prints it (-s), and a test that cannot find its plan fails.

Frames are a 64 x 64 synthetic scene's rays repeated modulo the frame, so one oracle render of the 4096 base rays serves every ray of
every case: all rays are compared, which includes the first tile, the last whole tile, the ragged last tile and everything behind
main_rays / in the last partial round."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4          # north_star: max-abs on the maps against the reference CPU path
S = 32
EPS = 1e-5
KEYS = ("rgb_map", "depth_map", "acc_map", "weights", "rgb_in_map")
WANT = ("weights", "z_vals", "rgb_in", "ray_mask")


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module("gp-nerf_amd.frame")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def build_frame(fm, sc):
    return fm.Frame(to_dev(sc["src_imgs"][0]), to_dev(sc["featmaps"]), [to_dev(v) for v in sc["volumes"]], to_dev(sc["src_Ks"][0]),
                    to_dev(sc["src_poses"][0]), sc["Rh"][0], sc["Th"][0], sc["bounds"][0, 0], sc["voxel_size"], sc["out_sh"][0],
                    fm.pack_head(sc["head"], torch.device("cuda:0")))


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ragged(rounds, tiles=0):
    """a ray count: `rounds` rounds of wavefronts of this device + `tiles` 32-ray tiles + a ragged tile of 17 rays"""
    return lambda cus: int(rounds * cus * 8) * 32 + tiles * 32 + 17


SMALL = 48 << 20    # a workspace with room for the tile queue and the chain block, not for a frame's colour list
# Candidate calls per launch shape, cheapest first: (ray count, keyword arguments).  The colour mode and the arithmetic come from
# MODES / FORMS below; the first candidate whose plan on this device is the wanted one is rendered.
SHAPE_CALLS = {
    "STATIC": [(ragged(0.5), {}), (ragged(0.25), {}), (ragged(0, 40), {})],
    # two rounds less a few tiles: more than 1 1/4 rounds, and too large a last round for a remainder launch
    "QUEUE": [(ragged(2, -4), {}), (ragged(1.75), {}), (ragged(2.5), {})],
    # whole rounds + a few tiles: two launches where samples_done is asked for, and from two rounds on
    "QUEUE_REMAINDER": [(ragged(1, 5), {"want": WANT + ("samples_done",)}), (ragged(2, 5), {})],
    "REMAINDER_UNITS": [(ragged(1, 5), {}), (ragged(1, 4), {})],
    "CHAINED": [(ragged(1, 5), {"early_term": True, "term_eps": EPS}), (ragged(2, -4), {"early_term": True, "term_eps": EPS})],
}
MODES = {
    "STEP": [{"exits": False}],
    "WAVE": [{"workspace_cap": SMALL}, {"workspace_cap": 1 << 20}, {"workspace_cap": 4 << 20}, {}],
    "LIST": [{"shared_device": True}, {}],
    "UNIFIED": [{}],
}
FORMS = {"REF": {}, "FOLD": {"fold": True}, "SPLIT": {"split_f16": True, "guard": False}, "GUARD": {"split_f16": True, "guard": True}}
# tests/test_render_plan.py REACHABLE, reference-order form: 16 (shape, colour) pairs
REF_PAIRS = [(sh, co) for sh in SHAPE_CALLS for co in MODES if co in ("STEP", "WAVE") or (co == "LIST" and sh != "STATIC") or
             (co == "UNIFIED" and sh in ("QUEUE", "REMAINDER_UNITS"))]


def find_plan(fm, shape, colour, sel, extra=None, modes=None):
    """(n_rays, kwargs, plan) of the first candidate call whose plan on this device is (shape, colour, sel); colour may be a tuple:
    any of them.  modes: the keyword arguments to try instead of MODES[colour].  Fails, with what every candidate got instead, when
    there is none."""
    colours = (colour,) if isinstance(colour, str) else colour
    extra = dict(extra or {})
    tried = []
    for n_of, kw_shape in SHAPE_CALLS[shape]:
        for kw_mode in (modes if modes is not None else [m for co in colours for m in MODES[co]]):
            kw = dict(kw_shape, **kw_mode, **FORMS[sel])
            kw.update({k: v for k, v in extra.items() if k != "want"})
            want = tuple(dict.fromkeys(kw_shape.get("want", WANT) + extra.get("want", ())))
            kw["want"] = tuple(w for w in want if not w.startswith("-") and "-" + w not in want)      # ("-weights": without them)
            n = n_of(n_cus())
            plan = fm.render_plan(None, n, S, **kw)
            t = plan.triple()
            if t[0] == shape and t[1] in colours and t[2] == sel:
                print(f"\n  plan: n_rays={n} S={S} {kw} -> {plan}")
                return n, kw, plan
            tried.append((n, kw, t))
    pytest.fail(f"no candidate call gets the plan {(shape, colour, sel)} on {n_cus()} CUs: {tried}")


class Scene:
    """a 64 x 64 scene on the device, its base rays, and the oracle's render of them (cached per termination setting)"""

    def __init__(self, fm, oracle, sc):
        self.fm, self.oracle, self.sc = fm, oracle, sc
        self.fr = build_frame(fm, sc)
        self.rays_h = oracle.rays_of(sc)
        self.base = to_dev(self.rays_h)
        self._ref = None

    def rays(self, n):
        return self.base[torch.arange(n, device=self.base.device) % self.base.shape[0]].contiguous()

    def ref(self):
        if self._ref is None:
            self._ref = self.oracle.render(self.sc, S)
        return self._ref


@pytest.fixture(scope="module")
def scene(fm, syn, oracle):
    sc = syn.make_scene(H=64, W=64, seed=9, fill="full", pose="identity", sigma_bias=1.0)
    s = Scene(fm, oracle, sc)
    assert float(s.rays_h[:, 7].max()) * EPS < 5e-5      # early termination drops at most term_eps * far of the depth
    return s


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def against_the_oracle(scene, n, kw, plan):
    """render the call; every ray against the oracle's render of its base ray (early-terminated plans against the UNTERMINATED
    oracle: rgb / acc lose at most T_stop <= term_eps, depth at most term_eps * far -- tests/test_gpu_configs.py config 3)"""
    fm = scene.fm
    rays = scene.rays(n)
    got = fm.render_fused(scene.fr, rays, S, **kw)
    ref = scene.ref()
    rows = np.arange(n) % scene.rays_h.shape[0]
    for k in KEYS:
        err = float(np.abs(got[k].cpu().numpy() - ref[k][rows]).max())
        print(f"    {k}: max error against the oracle {err:.3g}")
        assert err < TOL, (k, err, str(plan))
    # the tail the remainder shapes exist for: at least 128 rays behind main_rays / in the last partial round, and something is
    # rendered there at all
    slots = plan.n_cus * 8
    if plan.triple()[0] == "QUEUE_REMAINDER":
        assert 128 <= n - plan.main_rays, str(plan)
    if plan.triple()[0] == "REMAINDER_UNITS":
        assert 128 <= n - plan.tiles // slots * slots * 32 <= slots * 4, str(plan)
    tail = plan.main_rays if plan.main_rays < n else n - 128
    assert float(got["acc_map"][tail:].max()) > 0.1
    # One wavefront per whole tile, fp32: the bits do not depend on the launch (include/gpnerf_hip.h `workspace`).  Not the chained
    # launches, which stop a ray where a launch without a workspace stops its 32-ray tile.
    if plan.split == 1 and plan.triple()[2] in ("REF", "FOLD") and not kw.get("early_term"):
        whole = fm.render_fused(scene.fr, rays, S, load_balance=False, **{k: v for k, v in kw.items() if k != "workspace_cap"})
        for k in got:
            assert torch.equal(bits(got[k]), bits(whole[k])), (k, str(plan))
    return got


@pytest.mark.parametrize("shape,colour", REF_PAIRS, ids=[f"{s}-{c}" for s, c in REF_PAIRS])
def test_every_reachable_plan_of_the_reference_order_form_against_the_oracle(shape, colour, fm, scene):
    n, kw, plan = find_plan(fm, shape, colour, "REF")
    assert plan.triple() == (shape, colour, "REF")
    if shape == "STATIC":
        assert plan.split > 1, "the static candidates are frames that split a tile's samples"
    against_the_oracle(scene, n, kw, plan)


@pytest.mark.parametrize("sel", ["FOLD", "SPLIT"])
@pytest.mark.parametrize("shape", list(SHAPE_CALLS))
def test_the_folded_and_the_split_form_on_every_launch_shape_against_the_oracle(shape, sel, fm, scene):
    n, kw, plan = find_plan(fm, shape, ("UNIFIED", "LIST", "WAVE"), sel, modes=[{}])
    assert plan.triple()[0] == shape and plan.triple()[2] == sel
    against_the_oracle(scene, n, kw, plan)


def overflow_scene(syn):
    """tests/test_gpu_guard.py's overflow data, both kinds at once: huge source-view features in the left third of the views and a
    huge volume level in a corner -- MFMA operands of the split form leave the f16 range in part of the image.  Wrong VALUES in the
    unguarded split form (inf / NaN in registers), never an address."""
    sc = dict(syn.make_scene(H=64, W=64, seed=5, fill="full", pose="identity"))
    f = sc["featmaps"].copy()
    f[:, :, : f.shape[2] // 3] *= 3.0e5
    sc["featmaps"] = f
    v = [a.copy() for a in sc["volumes"]]
    v[1][..., : v[1].shape[-2] // 3, : v[1].shape[-1] // 3] *= 2.0e5
    sc["volumes"] = v
    return sc


@pytest.fixture(scope="module")
def overflow(fm, syn, oracle):
    return Scene(fm, oracle, overflow_scene(syn))


GUARD_CASES = [("STATIC", {}), ("QUEUE", {}), ("QUEUE_REMAINDER", {}), ("REMAINDER_UNITS", {}), ("CHAINED", {}),
               ("QUEUE", {"ray_order": True}), ("QUEUE", {"occ_cull": True})]


@pytest.mark.parametrize("shape,how", GUARD_CASES, ids=[s + "".join("-" + k for k in h) for s, h in GUARD_CASES])
def test_the_guard_with_tiles_flagged_on_every_launch_shape(shape, how, fm, overflow):
    """GPNERF_FLAG_SPLIT_GUARD's one promise -- the result never depends on the range of the data -- on every launch shape, with
    flagged tiles in the first round, the last whole round and the remainder (the scene's rays repeat every 4096), in a random ray
    order, and under the occupancy cull's mask and tile order (the fix-up launch has an instantiation of its own for it).

    The fix-up launch has to walk every tile of the call whatever the render launches' cut into rounds and a remainder: under
    QUEUE_REMAINDER the second launch flags its tiles by their slot in the whole call, behind main_rays."""
    extra = {"want": ("guard_tiles",)}
    if how.get("occ_cull"):
        extra.update(occ_cull=True, want=("guard_tiles", "-weights"))
    n, kw, plan = find_plan(fm, shape, "WAVE", "GUARD", extra=extra, modes=[{}])
    assert plan.triple() == (shape, "WAVE", "GUARD") and plan.regions().get("guard"), str(plan)
    assert (plan.split > 1) == (shape == "STATIC") and bool(plan.regions().get("mask")) == bool(how.get("occ_cull")), str(plan)
    kw = {k: v for k, v in kw.items() if k not in ("split_f16", "guard")}
    rays = overflow.rays(n)
    if how.get("ray_order"):
        kw["ray_order"] = torch.randperm(n, generator=torch.Generator().manual_seed(3)).int().cuda()
    fr = overflow.fr
    ref = fm.render_fused(fr, rays, S, fold=False, **kw)                               # the fp32 form as the fix-up launch runs it
    bad = fm.render_fused(fr, rays, S, split_f16=True, guard=False, **kw)
    got = fm.render_fused(fr, rays, S, split_f16=True, guard=True, **kw)
    flagged = int(got["guard_tiles"])
    # the last partial round (QUEUE_REMAINDER: what the second launch renders)
    slots = plan.n_cus * 8
    tail = int(plan.main_rays) if shape == "QUEUE_REMAINDER" else (plan.tiles - 1) // slots * slots * 32
    assert n - tail >= 128
    keys = [k for k in KEYS if k in got]
    err_bad = {where: float((bad["rgb_map"][sl] - ref["rgb_map"][sl]).abs().nan_to_num(nan=1e9).max())
               for where, sl in (("first tiles", slice(0, 4096)), ("tail", slice(tail, n)))}
    err = {k: float((got[k] - ref[k]).abs().nan_to_num(nan=1e9).max()) for k in keys}
    err_tail = {k: float((got[k][tail:] - ref[k][tail:]).abs().nan_to_num(nan=1e9).max()) for k in keys}
    print(f"    guard_tiles={flagged} of {plan.tiles}; unguarded split form off by {err_bad}; guarded: max error {err}; behind ray {tail}: {err_tail}")
    assert 0 < flagged <= plan.tiles, (flagged, plan.tiles)
    assert int(ref["guard_tiles"]) == 0 and int(bad["guard_tiles"]) == 0
    # without the guard the split form is simply wrong on this data, in the first round and in the tail
    assert err_bad["first tiles"] > 1e-2 and err_bad["tail"] > 1e-2, err_bad
    for k in keys:
        assert err[k] < TOL, (k, err[k], "behind main_rays / in the last partial round:", err_tail[k], "guard_tiles", flagged, str(plan))
    assert torch.equal(got["z_vals"], ref["z_vals"])
    if kw.get("early_term"):
        return      # the fix-up launch terminates per tile, the chained launch per ray: equal to the bound above, not to the bit
    # the flagged tiles ARE the fp32 form's, bit for bit: the fix-up launch runs the same code on the same 32 rays of a launch slot
    whole = fm.render_fused(fr, rays, S, load_balance=False, fold=False, **{k: v for k, v in kw.items() if k != "want"})
    diff = (got["rgb_map"] != whole["rgb_map"]).any(1)
    if "ray_order" in kw:
        diff = diff[kw["ray_order"].long()]
    pad = torch.zeros(plan.tiles * 32, dtype=torch.bool, device=diff.device)
    pad[: diff.numel()] = diff
    assert int((~pad.view(plan.tiles, 32).any(1)).sum()) >= flagged


def test_a_captured_guarded_call_clears_the_previous_replays_flags(fm, overflow):
    """The guarded split form on overflow data, a frame with a remainder launch, captured into a HIP graph: three replays give the
    same bits and the same positive guard_tiles.  Before every replay the test sets every tile's flag word in the guard region (at
    the offset render_plan reports, in the module's cached workspace of the capture stream): a replay that did not clear them would
    count every tile."""
    n, kw, plan = find_plan(fm, "QUEUE_REMAINDER", "WAVE", "GUARD", extra={"want": ("guard_tiles",)}, modes=[{}])
    assert plan.triple() == ("QUEUE_REMAINDER", "WAVE", "GUARD") and plan.main_rays < n, str(plan)
    g_off, g_bytes = plan.regions()["guard"]
    rays = overflow.rays(n)
    ref = fm.render_fused(overflow.fr, rays, S, **kw)
    flagged = int(ref["guard_tiles"])
    assert 0 < flagged < plan.tiles
    fp32 = fm.render_fused(overflow.fr, rays, S, fold=False, **{k: v for k, v in kw.items() if k not in ("split_f16", "guard")})
    for k in KEYS:              # (the replays below are held to ref's bits: ref itself is the fp32 form's to the usual bound, remainder included)
        assert float((ref[k] - fp32[k]).abs().nan_to_num(nan=1e9).max()) < TOL, k
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fm.render_fused(overflow.fr, rays, S, **kw)              # warm-up on the capture stream (allocator pool, kernel attributes)
        ws = fm._workspace(rays.device, 0)                       # the capture stream's cached workspace
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = fm.render_fused(overflow.fr, rays, S, **kw)
    with torch.cuda.stream(s):
        assert fm._workspace(rays.device, 0).data_ptr() == ws.data_ptr() and ws.numel() >= g_off + g_bytes
    words = ws[g_off:g_off + g_bytes].view(torch.int32)
    assert 64 + plan.tiles <= words.numel()
    for i in range(3):
        for v in out.values():
            v.zero_()
        words[64:64 + plan.tiles] = 1                           # (word 0: the count; words 64..: one flag per tile)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(out["guard_tiles"]) == flagged, (i, int(out["guard_tiles"]), flagged)
        for k in ref:
            assert torch.equal(bits(out[k]), bits(ref[k])), (i, k)
