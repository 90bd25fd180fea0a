"""GPU: every launch variant of the encoder's convolutions (tests/conv_cases.py: kernel family x COT x RW x KSPLIT x concatenation,
at ragged, tiny and many-tile shapes) against float64 torch on the CPU, and the operators beside them (InstanceNorm, table
apply, bilinear x2) at channel counts and sizes off the encoder's path.  The bounds are those of tests/test_gpu_conv.py.

Every launch goes through the C entry points with `y` and `tile_stats` placed inside larger buffers whose margins must come back
untouched.  Each case prints its largest error; with GPNERF_CONV_VARIANT_ERRORS set to a path, the worst error per variant and
arithmetic form is written there as JSON lines."""
import copy
import importlib
import json
import os

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 4096            # floats on either side of y and tile_stats
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def enc():
    return importlib.import_module("gp-nerf_amd.encoder")


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("gp-nerf_amd._lib")


@pytest.fixture(params=["fp32", "split"])
def form(request, enc):
    """both arithmetic forms of the convolutions, as in tests/test_gpu_conv.py (requested by every convolution test)"""
    with enc._form(request.param == "fp32"):
        yield request.param


@pytest.fixture(scope="module")
def errors():
    """(variant, form, check) -> the worst (error, bound, case)"""
    worst = {}

    def note(case, form, check, err, bound):
        print(f"{case.name} [{form}] {check}: {err:.3e} (bound {bound:.3e})")
        key = ("/".join(str(v) for v in case.variant), form, check)
        if key not in worst or err / bound > worst[key][0] / worst[key][1]:
            worst[key] = (err, bound, case.name)

    yield note
    path = os.environ.get("GPNERF_CONV_VARIANT_ERRORS")
    if path:
        with open(path, "w") as f:
            for (variant, form, check), (err, bound, name) in sorted(worst.items()):
                f.write(json.dumps({"variant": variant, "form": form, "check": check, "worst_error": err, "bound": bound, "case": name}) + "\n")


def _mk_conv(c, gen, bias=None, weight_scale=1.0):
    cin = c.cin + c.cin_b
    conv = torch.nn.Conv2d(cin, c.cout, c.ks, stride=c.stride, padding=c.ks // 2, bias=c.bias if bias is None else bias, padding_mode="reflect")
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / (cin * c.ks * c.ks)) ** 0.5 * weight_scale)
        if conv.bias is not None:
            conv.bias.copy_(torch.randn(c.cout, generator=gen) * 0.1)
    return conv


def _mk_norm(ch, gen):
    norm = torch.nn.InstanceNorm2d(ch, track_running_stats=False, affine=True)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.2 * torch.randn(ch, generator=gen))
        norm.bias.copy_(0.2 * torch.randn(ch, generator=gen))
    return norm


def _ref64(conv, x):
    """float64 nn.Conv2d(padding_mode='reflect') on the CPU, returned in float32"""
    with torch.no_grad():
        c64 = torch.nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, stride=conv.stride, padding=conv.padding,
                              bias=conv.bias is not None, padding_mode="reflect").double()
        c64.weight.copy_(conv.weight.detach().cpu().double())
        if conv.bias is not None:
            c64.bias.copy_(conv.bias.detach().cpu().double())
        return c64(x.detach().cpu().double()).float()


_DATA = {}


def _data(c):
    """the case's convolution, input and float64 results (ordinary operands, and operands scaled by 1e4), made once"""
    if c.name not in _DATA:
        gen = torch.Generator().manual_seed(1000 + cc.CASES.index(c))
        conv = _mk_conv(c, gen)
        x = torch.randn((c.n, c.cin + c.cin_b, c.h, c.w), generator=gen) * 2.0 + 0.3
        x_big = x * 1e4
        _DATA[c.name] = (conv, x, _ref64(conv, x), x_big, _ref64(conv, x_big))
    return _DATA[c.name]


def _variant(L, c):
    return L.conv_variant(c.n, c.h, c.w, c.cin, c.cin_b, c.cout, c.ks, c.stride)


def _framed(numel):
    buf = torch.full((numel + 2 * MARGIN,), SENTINEL, device=DEV, dtype=torch.float32)
    return buf, buf[MARGIN:MARGIN + numel]


def _margins_untouched(buf):
    edge = torch.full((MARGIN,), SENTINEL, device=DEV, dtype=torch.float32)
    return torch.equal(buf[:MARGIN], edge) and torch.equal(buf[-MARGIN:], edge)


def _launch(enc, L, c, conv, x, in_tab=None, in_act=0, norm=None):
    """One call of gpnerf_conv2d_norm_nhwc (gpnerf_conv2d_norm_cat_nhwc for a concatenating case) on the device tensor x [N, cin
    (+ cin_b), H, W], in the current arithmetic form.  Returns (y as a channels-last [N, cout, Ho, Wo] view, tile_stats, table or
    None) after checking that the margins around y and tile_stats are untouched and that every element between them was written."""
    lib = L.lib()
    exact = enc._exact()
    ho, wo = cc.out_size(c)
    tiles = _variant(L, c)["tiles"]
    assert tiles == lib.gpnerf_conv_out_tiles(c.h, c.w, c.cin + c.cin_b, c.ks, c.stride)
    ybuf, y = _framed(c.n * ho * wo * c.cout)
    tsbuf, ts = _framed(c.n * tiles * c.cout * 3)
    tab = torch.empty((c.n, 3, c.cout), device=DEV, dtype=torch.float32) if norm is not None else None
    run = enc._run_of(x)
    bias = conv.bias.detach().float().contiguous() if conv.bias is not None else None
    packed = enc._packed_weight(conv)
    ptr = lambda t: t.data_ptr() if t is not None else None
    tail = (ptr(bias), c.cout) + ((c.ks, c.stride) if not c.cin_b else ()) + (
        y.data_ptr(), ts.data_ptr(), ptr(norm.weight if norm is not None else None), ptr(norm.bias if norm is not None else None),
        float(norm.eps) if norm is not None else 0.0, ptr(tab), run.tickets.data_ptr() if norm is not None else None,
        None if exact else run.flag_ptr, int(exact), enc._st(x))
    if c.cin_b:
        assert in_tab is None
        xa = x[:, :c.cin].contiguous(memory_format=torch.channels_last)
        xb = x[:, c.cin:].contiguous(memory_format=torch.channels_last)
        # (physical NHWC whatever torch makes of the strides of a size-1 dimension)
        xa, xb = xa.permute(0, 2, 3, 1).contiguous(), xb.permute(0, 2, 3, 1).contiguous()
        L.check(lib.gpnerf_conv2d_norm_cat_nhwc(xa.data_ptr(), c.cin, xb.data_ptr(), c.cin_b, c.n, c.h, c.w, packed.data_ptr(), *tail),
                "gpnerf_conv2d_norm_cat_nhwc")
    else:
        xn = x.permute(0, 2, 3, 1).contiguous()
        L.check(lib.gpnerf_conv2d_norm_nhwc(xn.data_ptr(), c.n, c.h, c.w, c.cin, ptr(in_tab), int(in_act), packed.data_ptr(), *tail),
                "gpnerf_conv2d_norm_nhwc")
    torch.cuda.synchronize()
    assert _margins_untouched(ybuf) and _margins_untouched(tsbuf), c.name
    assert not bool((y == SENTINEL).any()) and not bool((ts == SENTINEL).any()), c.name
    if norm is not None:
        assert int(run.tickets.abs().sum()) == 0
    return y.view(c.n, ho, wo, c.cout).permute(0, 3, 1, 2), ts.view(c.n, tiles, c.cout, 3), tab


def _nchw(x):
    """device copy of a CPU [N, C, H, W] tensor"""
    return x.to(DEV)


IDS = [c.name for c in cc.CASES]


@pytest.mark.parametrize("c", cc.CASES, ids=IDS)
def test_every_variant_matches_float64_torch(c, form, enc, L, errors):
    """The query reports the variant the case is named after; the output is within 2e-5 of float64 nn.Conv2d (scaled by the
    output's range); a second launch gives the same bits; nothing is written outside y and tile_stats, and all of both is written.
    fp32 form: within 3e-6 on operands scaled by 1e4, also of the per-operand restatement gpnerf_conv2d_nhwc_exact."""
    v = _variant(L, c)
    assert (v["family"], v["cot"], v["rw"], v["ksplit"], v["cat"]) == c.variant, v
    conv, x, ref, x_big, ref_big = _data(c)
    with torch.no_grad():
        conv = copy.deepcopy(conv).to(DEV)
        y, ts, _ = _launch(enc, L, c, conv, _nchw(x))
        y_again, ts_again, _ = _launch(enc, L, c, conv, _nchw(x))
        assert y.shape == ref.shape
        assert torch.equal(y, y_again) and torch.equal(ts, ts_again)
        scale = max(1.0, float(ref.abs().max()))
        err = float((y.cpu() - ref).abs().max())
        errors(c, form, "float64", err, 2e-5 * scale)
        assert err < 2e-5 * scale, err
        # the tile sums add up to the output's own sums.  (A tile's float32 sum of 256 values is a tree of depth ~10: at most ~10
        # roundings of 6e-8 relative to the sum of magnitudes; 1e-5 leaves that an order of magnitude.)
        s64, a64 = y.double().sum((2, 3)), y.double().abs().sum((2, 3))
        assert float(((ts[..., 0].double().sum(1) - s64).abs() / (1.0 + a64)).max()) < 1e-5
        if form == "fp32":
            xb = _nchw(x_big)
            y_big, _, _ = _launch(enc, L, c, conv, xb)
            chain = enc._conv_exact(conv, xb)
            scale = max(1.0, float(ref_big.abs().max()))
            err = float((y_big.cpu() - ref_big).abs().max())
            errors(c, form, "float64, operands x 1e4", err, 3e-6 * scale)
            assert err < 3e-6 * scale, err
            assert float((chain.cpu() - ref_big).abs().max()) < 3e-6 * scale and float((chain - y_big).abs().max()) < 3e-6 * scale


NORM_READERS = [c for c in cc.CASES if cc.reads_through_a_norm(c)]


@pytest.mark.parametrize("c", NORM_READERS, ids=[c.name for c in NORM_READERS])
def test_a_pending_input_norm_equals_the_convolution_of_the_materialised_tensor(c, form, enc, L, errors):
    """in_table, both in_act values: bit for bit the convolution of act((x - mean) * scale + beta) written out by
    gpnerf_norm_apply_nhwc, tile_stats and the table behind it included; the ticket words are zero afterwards (_launch); and the
    result is within the convolution's bound of float64 torch on that tensor."""
    gen = torch.Generator().manual_seed(2000 + cc.CASES.index(c))
    conv, x, _, _, _ = _data(c)
    norm = _mk_norm(c.cout, gen).to(DEV)
    t0 = torch.stack([torch.randn((c.n, c.cin), generator=gen) * 0.5, 0.5 + torch.rand((c.n, c.cin), generator=gen),
                      torch.randn((c.n, c.cin), generator=gen) * 0.3], 1).contiguous().to(DEV)
    with torch.no_grad():
        conv = copy.deepcopy(conv).to(DEV)
        xd = _nchw(x).contiguous(memory_format=torch.channels_last)
        for in_act in (0, 1):
            mat = enc._apply(xd, t0, in_act)
            want = (x.double() - t0[:, 0].cpu().double()[:, :, None, None]) * t0[:, 1].cpu().double()[:, :, None, None] + t0[:, 2].cpu().double()[:, :, None, None]
            want = F.relu(want) if in_act else want
            assert float((mat.cpu().double() - want).abs().max()) < 2e-5
            y_mat, ts_mat, tab_mat = _launch(enc, L, c, conv, mat, norm=norm)
            y_fus, ts_fus, tab_fus = _launch(enc, L, c, conv, xd, in_tab=t0, in_act=in_act, norm=norm)
            assert torch.equal(y_mat, y_fus) and torch.equal(ts_mat, ts_fus) and torch.equal(tab_mat, tab_fus), in_act
            ref = _ref64(conv, mat)
            scale = max(1.0, float(ref.abs().max()))
            err = float((y_fus.cpu() - ref).abs().max())
            errors(c, form, "float64, pending input norm", err, 2e-5 * scale)
            assert err < 2e-5 * scale, (in_act, err)


@pytest.mark.parametrize("c", cc.CASES, ids=IDS)
def test_the_fused_table_equals_the_separate_pass(c, form, enc, L, errors):
    """out_table on ordinary activations: normalising with it equals the stand-alone operator's double-precision pass within 2e-6;
    asking for the table changes neither y nor tile_stats.

    (The cases whose output has two to four pixels are the sharp ones: many of their channels have a mean of several sigma, and a
    variance taken as E[y^2] - mean^2 from float32 sums was up to 2.6e-5 off there -- 3x3s2-2x3, 3x3s2-3x2, stem-cot2-cin3-4x4,
    3x3s2-3x3, 1x1-cot1-tiny -- before finalize_if_last took it from the tiles' M2 and the spread of their means.)"""
    gen = torch.Generator().manual_seed(3000 + cc.CASES.index(c))
    conv, x, _, _, _ = _data(c)
    norm = _mk_norm(c.cout, gen).to(DEV)
    with torch.no_grad():
        conv = copy.deepcopy(conv).to(DEV)
        xd = _nchw(x)
        y, ts, tab = _launch(enc, L, c, conv, xd, norm=norm)
        y_plain, ts_plain, _ = _launch(enc, L, c, conv, xd)
        assert torch.equal(y, y_plain) and torch.equal(ts, ts_plain)
        a, b = enc._apply(y, tab, 2), enc._norm_act(norm, y, 2)
        err = float((a - b).abs().max())
        errors(c, form, "table vs separate pass", err, 2e-6)
        assert err < 2e-6, err


# A tile's pixel count enters the table only where it meets another tile's in the merge (tests/test_conv_host.py), so the cases of one
# tile are left out: every tiling is still there at a ragged shape and at a tile count beyond one round of the table's loop.
SEVERAL_TILES = [c for c in cc.CASES if c.name not in cc.ONE_TILE]


@pytest.mark.parametrize("c", SEVERAL_TILES, ids=[c.name for c in SEVERAL_TILES])
def test_the_fused_table_on_a_nearly_constant_channel(c, form, enc, L, errors):
    """A NEARLY CONSTANT channel exactly as tests/test_gpu_conv.py makes it (a default-initialised convolution and norm, the weights
    times 1e-5, the bias 1000, inputs 2 randn + 0.5: outputs that are 1000 give or take one float32 step): the last workgroup merges
    the tiles' M2 with tile_pixels() as their counts.  Within 2e-3 of the stand-alone operator and of float64 -- for every tiling
    (direct, stem, stride 2, 4-row, 8-row, concatenating), at ragged shapes and at tile counts that take the table's tile loop into a
    second round.  tests/test_conv_host.py shows that a wrong count of a ragged tile breaks this bound."""
    assert {k.variant for k in SEVERAL_TILES} == set(cc.VARIANTS)
    gen = torch.Generator().manual_seed(5000 + cc.CASES.index(c))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(5000 + cc.CASES.index(c))
        flat = torch.nn.Conv2d(c.cin + c.cin_b, c.cout, c.ks, stride=c.stride, padding=c.ks // 2, bias=True, padding_mode="reflect").to(DEV)
    norm = torch.nn.InstanceNorm2d(c.cout, track_running_stats=False, affine=True).to(DEV)
    x = (torch.randn((c.n, c.cin + c.cin_b, c.h, c.w), generator=gen) * 2 + 0.5).to(DEV)
    with torch.no_grad():
        flat.weight.mul_(1e-5)
        flat.bias.fill_(1000.0)
        y, _, tab = _launch(enc, L, c, flat, x, norm=norm)
        a, b = enc._apply(y, tab, 0), enc._norm_act(norm, y, 0)
        y64 = y.double()
        mean, var = y64.mean((2, 3), keepdim=True), y64.var((2, 3), unbiased=False, keepdim=True)
        ref = (y64 - mean) / torch.sqrt(var + norm.eps)
        e_sep, e_64 = float((a - b).abs().max()), float((a.double() - ref).abs().max())
        errors(c, form, "nearly constant channel: table vs separate pass", e_sep, 2e-3)
        errors(c, form, "nearly constant channel: table vs float64", e_64, 2e-3)
        assert e_sep < 2e-3 and e_64 < 2e-3, (e_sep, e_64)


CATS = [c for c in cc.CASES if c.cin_b]


@pytest.mark.parametrize("c", CATS, ids=[c.name for c in CATS])
def test_a_concatenation_read_in_place_equals_the_concatenated_tensor(c, form, enc, L):
    """gpnerf_conv2d_norm_cat_nhwc against `_conv_norm` on the tensor itself: bit for bit, table included, when the query reports the
    same KSPLIT for both; where the materialised tensor takes the K-split form (the same terms in another order), within 2e-5."""
    gen = torch.Generator().manual_seed(4000 + cc.CASES.index(c))
    conv, x, _, _, _ = _data(c)
    norm = _mk_norm(c.cout, gen).to(DEV)
    whole = L.conv_variant(c.n, c.h, c.w, c.cin + c.cin_b, 0, c.cout, 3, 1)
    here = _variant(L, c)
    assert (whole["rw"], whole["tiles"]) == (here["rw"], here["tiles"])
    with torch.no_grad():
        conv = copy.deepcopy(conv).to(DEV)
        xd = _nchw(x)
        y_inp, _, t_inp = _launch(enc, L, c, conv, xd, norm=norm)
        y_cat, t_cat = enc._conv_norm(conv, norm, xd)
        if whole["ksplit"] == here["ksplit"]:
            assert torch.equal(y_cat, y_inp) and torch.equal(t_cat, t_inp)
        else:
            assert float((y_cat - y_inp).abs().max()) < 2e-5 and float((t_cat - t_inp).abs().max()) < 2e-5
        assert int(enc._ticket_words(xd.device).abs().sum()) == 0


# ---- the operators beside the convolutions -------------------------------------------------------------------------------------

def _act64(y, act):
    return F.relu(y) if act == 1 else F.elu(y) if act == 2 else y


@pytest.mark.parametrize("ch", [4, 12, 36, 100, 1024])
def test_instance_norm_at_channel_counts_that_do_not_divide_the_block(ch, enc):
    """gpnerf_instance_norm_act_nhwc against a float64 restatement (biased variance, eps inside the root), 2e-5: channel counts whose
    float4 groups do not divide the 256-thread block (threads past the last whole pixel must stay out), one pixel, sizes around one
    256-pixel chunk, and 9 and 17 chunks (the finalize kernel's chunk lanes take a second and a third turn); every activation, with
    and without a residual."""
    gen = torch.Generator().manual_seed(ch)
    norm = _mk_norm(ch, gen)
    g, b = norm.weight.detach().double()[None, :, None, None], norm.bias.detach().double()[None, :, None, None]
    norm = norm.to(DEV)
    for hw in (1, 255, 256, 257, 2049, 4097):            # 2049: 9 chunks, 4097: 17
        n = 3 if hw == 257 else 1
        h, w = (hw, 1) if hw % 2 else (hw // 2, 2)
        x = torch.randn((n, ch, h, w), generator=gen) * 3.0 + 1.5
        r = torch.randn((n, ch, h, w), generator=gen)
        x64 = x.double()
        normed = (x64 - x64.mean((2, 3), keepdim=True)) / torch.sqrt(x64.var((2, 3), unbiased=False, keepdim=True) + norm.eps) * g + b
        for act in (0, 1, 2):
            for res in (False, True):
                ref = _act64(normed + (r.double() if res else 0), act)
                with torch.no_grad():
                    got = enc._norm_act(norm, x.to(DEV), act, residual=r.to(DEV) if res else None)
                assert got.shape == x.shape
                assert float((got.cpu().double() - ref).abs().max()) < 2e-5, (ch, hw, act, res)


def test_instance_norm_refuses_channel_counts_it_is_not_built_for(L):
    lib = L.lib()
    p = 0x1000
    for ch in (1028, 6, 2):
        assert lib.gpnerf_instance_norm_act_nhwc(p, p, p, None, 1, 64, ch, 1e-5, 0, p, p, None) == -1
    assert lib.gpnerf_instance_norm_act_nhwc(p, p, p, None, 1, 64, 1024, 1e-5, 3, p, p, None) == -1
    assert lib.gpnerf_norm_apply_nhwc(p, p, None, p, 1, 64, 32, 0, p, None) == -1        # a residual table without a residual


@pytest.mark.parametrize("ch,n,h,w", [(4, 1, 1, 1), (12, 3, 5, 7), (36, 2, 17, 16), (100, 1, 9, 29)])
def test_norm_apply_with_a_residual_table(ch, n, h, w, enc):
    """gpnerf_norm_apply_nhwc with res_table (the projected shortcut's InstanceNorm applied on the fly), every activation, against
    float64: act((x - mean) * scale + beta + (r - rmean) * rscale + rbeta), 2e-5."""
    gen = torch.Generator().manual_seed(ch + h)
    x, r = torch.randn((n, ch, h, w), generator=gen) * 2 + 0.5, torch.randn((n, ch, h, w), generator=gen) * 3 - 1
    tabs = [torch.stack([torch.randn((n, ch), generator=gen), 0.5 + torch.rand((n, ch), generator=gen), torch.randn((n, ch), generator=gen) * 0.3], 1).contiguous()
            for _ in range(2)]
    col = lambda t, j: t[:, j].double()[:, :, None, None]
    y = (x.double() - col(tabs[0], 0)) * col(tabs[0], 1) + col(tabs[0], 2)
    yr = (r.double() - col(tabs[1], 0)) * col(tabs[1], 1) + col(tabs[1], 2)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    for act in (0, 1, 2):
        with torch.no_grad():
            got = enc._apply(xd, tabs[0].to(DEV), act, residual=r.to(DEV), res_tab=tabs[1].to(DEV))
            plain = enc._apply(xd, tabs[0].to(DEV), act, residual=r.to(DEV))
        assert float((got.cpu().double() - _act64(y + yr, act)).abs().max()) < 2e-5, act
        assert float((plain.cpu().double() - _act64(y + r.double(), act)).abs().max()) < 2e-5, act


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (7, 1), (2, 2), (9, 13), (33, 5)])
def test_upsample2x_at_degenerate_and_odd_sizes(h, w, enc):
    """gpnerf_upsample2x_nhwc against float64 F.interpolate(align_corners=True), 1e-5; the four output corners ARE the input's."""
    for ch in (4, 36, 64):
        for n in (1, 3):
            x = torch.randn((n, ch, h, w), generator=torch.Generator().manual_seed(ch + h + w))
            ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True)
            got = enc._upsample2x(x.to(DEV).contiguous(memory_format=torch.channels_last)).cpu()
            assert got.shape == ref.shape and float((got.double() - ref).abs().max()) < 1e-5, (ch, n)
            for oy, iy in ((0, 0), (2 * h - 1, h - 1)):
                for ox, ix in ((0, 0), (2 * w - 1, w - 1)):
                    assert torch.equal(got[:, :, oy, ox], x[:, :, iy, ix]), (ch, n, oy, ox)
