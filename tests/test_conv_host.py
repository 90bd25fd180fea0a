"""CPU: the launch choice of the encoder's convolutions (gpnerf_conv_variant, host arithmetic only) against a restatement of the
launch rules, the coverage of tests/conv_cases.py, and the tile-moment merge of the fused InstanceNorm table restated in numpy."""
import ctypes as C
import importlib
import random

import numpy as np
import pytest

import conv_cases as cc


@pytest.fixture(scope="module")
def L():
    return importlib.import_module("gp-nerf_amd._lib")


def _ceil(a, b):
    return -(-a // b)


def restated(n, h, w, cin_a, cin_b, cout, ks, stride):
    """The launch rules of csrc/gpnerf_conv.hip, restated: (variant tuple, tiles per image, (tile_h, tile_w)), or None for a shape
    the entry points refuse."""
    if cout < 4 or cout % 4 or n < 0 or cin_b < 0:
        return None
    if cin_b:
        if (ks, stride) != (3, 1) or h < 2 or w < 2 or cin_a < 16 or cin_a % 16 or cin_b < 16 or cin_b % 16:
            return None
    else:
        if ks not in (1, 3, 7) or stride not in (1, 2) or cin_a < 1 or h <= ks // 2 or w <= ks // 2:
            return None
        if cin_a < 8:
            if not ((ks == 7 and stride == 2 and cin_a <= 4) or (ks == 3 and stride == 1)):
                return None
        elif cin_a % 16 or ks == 7:
            return None
    pad = ks // 2
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    cin, ct = cin_a + cin_b, _ceil(cout, 32)
    if ks == 7:                                            # launch_stem
        return (cc.STEM, 2 if ct % 2 == 0 else 1, 2, 1, 0), _ceil(ho, 8) * _ceil(wo, 32), (8, 32)
    if ks == 3 and stride == 2:                            # launch_conv3x3_s2
        return (cc.S2, 1, 1, 1, 0), _ceil(ho, 4) * _ceil(wo, 32), (4, 32)
    if ks == 3 and cin >= 8:                               # conv3x3_rows, launch_conv3x3
        rw = 1 if _ceil(ho, 8) * _ceil(wo, 32) <= 16 and ho > 4 else 2
        tiles, cb = _ceil(ho, 4 * rw) * _ceil(wo, 32), cin // 16
        ksplit = 2 if not cin_b and rw == 1 and cb % 2 == 0 and cb >= 4 and tiles * n * ct <= 256 else 1
        return (cc.S1, 1, rw, ksplit, 1 if cin_b else 0), tiles, (4 * rw, 32)
    tiles, cot = _ceil(ho * wo, 256), 4                    # launch_conv
    while cot > 1 and (ct % cot or tiles * n * (ct // cot) < 256):
        cot //= 2
    return (cc.N3 if ks == 3 else cc.D1, cot, 0, 1, 0), tiles, (0, 256)


def queried(L, *shape):
    v = L.conv_variant(*shape)
    if v["family"] == "REFUSED":
        return None
    return (v["family"], v["cot"], v["rw"], v["ksplit"], v["cat"]), v["tiles"], (v["tile_h"], v["tile_w"])


SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 31, 32, 33, 40, 63, 64, 65, 66, 72, 96, 127, 128, 129, 130, 256, 257, 260, 512)


def sweep():
    """~6 000 shapes: a seeded sample of the product of sizes, channel counts, kernels and strides (valid and not), and every
    convolution the encoder builds at its usual frame sizes"""
    rng = random.Random(20)
    shapes = []
    for _ in range(6000):
        cat = rng.random() < 0.2
        ks, stride = (3, 1) if cat and rng.random() < 0.9 else (rng.choice((1, 3, 3, 3, 5, 7)), rng.choice((1, 1, 2, 2, 3)))
        cin_a = rng.choice((1, 2, 3, 4, 5, 7, 8, 16, 24, 32, 48, 64, 80, 96, 128, 256) if not cat else (8, 16, 32, 48, 64, 128))
        cin_b = rng.choice((16, 24, 48, 64, 128)) if cat else 0
        shapes.append((rng.choice((1, 1, 2, 3, 4)), rng.choice(SIZES), rng.choice(SIZES), cin_a, cin_b,
                       rng.choice((2, 4, 30, 32, 36, 64, 96, 100, 128, 192, 256)), ks, stride))
    for n in (1, 3):
        for side in (64, 128, 256, 512):
            h = side
            shapes.append((n, h, h, 3, 0, 64, 7, 2))
            for cin, cout in ((64, 64), (64, 128), (128, 256)):
                h = (h - 1) // 2 + 1
                shapes += [(n, h, h, cin, 0, cout, 3, 2), (n, h, h, cin, 0, cout, 1, 2), (n, (h - 1) // 2 + 1, (h - 1) // 2 + 1, cout, 0, cout, 3, 1)]
            shapes += [(n, side // 8, side // 8, 256, 0, 128, 3, 1), (n, side // 8, side // 8, 128, 128, 128, 3, 1),
                       (n, side // 4, side // 4, 128, 0, 64, 3, 1), (n, side // 4, side // 4, 64, 64, 32, 3, 1), (n, side // 4, side // 4, 32, 0, 32, 1, 1)]
    return shapes


def test_the_query_agrees_with_the_restated_launch_rules(L):
    lib = L.lib()
    refused = 0
    for s in sweep():
        want, got = restated(*s), queried(L, *s)
        assert got == want, (s, got, want)
        row = (C.c_int32 * len(L.CONV_VARIANT))()
        assert lib.gpnerf_conv_variant(*s, row) == (0 if want else -1), s
        if want is None:
            refused += 1
            assert list(row) == [0] * len(row), s
            continue
        n, h, w, cin_a, cin_b, cout, ks, stride = s
        assert want[1] == lib.gpnerf_conv_out_tiles(h, w, cin_a + cin_b, ks, stride), s
        ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
        th, tw = want[2]
        assert want[1] == (_ceil(ho, th) * _ceil(wo, tw) if th else _ceil(ho * wo, tw)), s
    assert 500 < refused < 5000
    assert lib.gpnerf_conv_variant(1, 8, 8, 16, 0, 32, 3, 1, None) == -1


def _entry_points_refuse(lib, n, h, w, cin_a, cin_b, cout, ks, stride):
    """what the convolution entry points THEMSELVES answer for a shape they must refuse (dummy non-null pointers: an argument error
    comes back before anything touches the device, so this runs without a GPU -- and is only ever called for such shapes)"""
    p = 0x1000
    if cin_b:
        return [lib.gpnerf_conv2d_norm_cat_nhwc(p, cin_a, p, cin_b, n, h, w, p, None, cout, p, p, p, p, 1e-5, p, p, None, e, None) for e in (0, 1)]
    return [lib.gpnerf_conv2d_norm_nhwc(p, n, h, w, cin_a, None, 0, p, None, cout, ks, stride, p, p, p, p, 1e-5, p, p, None, 1, None),
            lib.gpnerf_conv2d_nhwc(p, n, h, w, cin_a, p, None, cout, ks, stride, p, None, None, 0, None)]


def test_every_refused_shape_is_refused_by_the_entry_points_themselves(L):
    """The query, the restatement AND the calls: every shape of the sweep that the rules refuse comes back GPNERF_E_ARG from
    gpnerf_conv2d_nhwc / gpnerf_conv2d_norm_nhwc (cin_b = 0) or gpnerf_conv2d_norm_cat_nhwc (cin_b > 0) before any launch."""
    lib = L.lib()
    seen = 0
    for s in sweep():
        if restated(*s) is None and s[0] > 0:
            # (a 3x3 stride-1 shape is what the concatenating call has: other kernels and strides cannot be put to it)
            if s[4] and (s[6], s[7]) != (3, 1):
                continue
            assert _entry_points_refuse(lib, *s) == [-1, -1], s
            seen += 1
    assert seen > 500


def test_the_concatenating_call_refuses_an_empty_or_partial_second_part(L):
    """gpnerf_conv2d_norm_cat_nhwc with cin_b in {0, 8, 24} (or a first part that is no whole block): GPNERF_E_ARG before any launch.
    cin_b = 0 is NOT the plain convolution there -- its kernel would stage a channel block that neither tensor has."""
    lib = L.lib()
    p = 0x1000
    for cin_a in (3, 16):
        for cin_b in (0, 8, 24):
            for exact in (0, 1):
                assert lib.gpnerf_conv2d_norm_cat_nhwc(p, cin_a, p, cin_b, 1, 8, 8, p, None, 32, p, p, p, p, 1e-5, p, p, None, exact, None) == -1, (cin_a, cin_b)
    for cin_a, cin_b, h, w, cout in ((3, 16, 8, 8, 32), (24, 16, 8, 8, 32), (16, 16, 1, 8, 32), (16, 16, 8, 1, 32), (16, 16, 8, 8, 30), (16, -16, 8, 8, 32)):
        assert lib.gpnerf_conv2d_norm_cat_nhwc(p, cin_a, p, cin_b, 1, h, w, p, None, cout, p, p, p, p, 1e-5, p, p, None, 1, None) == -1
    assert lib.gpnerf_conv2d_norm_cat_nhwc(p, 16, None, 16, 1, 8, 8, p, None, 32, p, p, p, p, 1e-5, p, p, None, 1, None) == -1
    assert lib.gpnerf_conv2d_norm_cat_nhwc(None, 16, None, 0, 0, 8, 8, None, None, 32, None, None, None, None, 1e-5, None, None, None, 1, None) == 0   # nothing to do


def test_the_case_table_names_exactly_the_variants_the_rules_reach(L):
    """A form the launchers can choose but no case runs fails here, and so does a case named after a form they cannot choose."""
    reached = {queried(L, *s)[0] for s in sweep() if restated(*s) is not None}
    assert reached == set(cc.VARIANTS), reached ^ set(cc.VARIANTS)
    assert {c.variant for c in cc.CASES} == set(cc.VARIANTS)
    assert len(set(cc.VARIANTS)) == len(cc.VARIANTS)


def test_every_case_gives_the_variant_it_is_named_after(L):
    for c in cc.CASES:
        s = (c.n, c.h, c.w, c.cin, c.cin_b, c.cout, c.ks, c.stride)
        assert queried(L, *s) == restated(*s) and queried(L, *s)[0] == c.variant, (c.name, queried(L, *s))


def test_the_cases_reach_what_they_are_there_for(L):
    """the properties the table's comments promise: a second round of the table's tile loop for every COT and tiling, ragged tiles, a
    partial channel tile, an odd number of channel blocks, a part-filled last chunk of the flat K, tiles hanging over a tiny image"""
    v = {c.name: L.conv_variant(c.n, c.h, c.w, c.cin, c.cin_b, c.cout, c.ks, c.stride) for c in cc.CASES}
    assert cc.ONE_TILE == {c.name for c in cc.CASES if v[c.name]["tiles"] == 1}
    assert {c.variant for c in cc.CASES if c.name not in cc.ONE_TILE} == set(cc.VARIANTS)
    rounds = {}          # (family, cot, rw) -> most tiles among its cases
    for c in cc.CASES:
        key = (c.variant[0], c.variant[1], c.variant[2])
        rounds[key] = max(rounds.get(key, 0), v[c.name]["tiles"])
    for (family, cot, rw), tiles in rounds.items():
        if (family, rw) == (cc.S1, 1):
            assert tiles == 32           # (4-row tiles are chosen for at most sixteen 8-row tiles: 32 is the most they reach)
        else:
            assert tiles > 64 // cot, (family, cot, rw, tiles)
    for c in cc.CASES:
        if c.variant[0] == cc.N3:
            assert (9 * c.cin) % 16 != 0
    ragged = [c for c in cc.CASES if v[c.name]["tile_h"] and (cc.out_size(c)[0] % v[c.name]["tile_h"] or cc.out_size(c)[1] % 32)]
    assert {c.variant for c in ragged} >= {x for x in cc.VARIANTS if x[0] in (cc.S1, cc.S2, cc.STEM)}
    # a partial last channel tile for every variant that can have one (COT = 4 of the narrow path shares the direct kernel's epilogue
    # with 1x1-cot4-cout100 and would cost another 26 MB output)
    assert {c.variant for c in cc.CASES if c.cout % 32} == set(cc.VARIANTS) - {(cc.N3, 4, 0, 1, 0)}
    assert any(c.variant == (cc.S1, 1, 1, 1, 0) and (c.cin // 16) % 2 == 1 and c.cin > 16 for c in cc.CASES)
    assert any(c.variant == (cc.S1, 1, 1, 1, 0) and c.cin >= 64 and (c.cin // 16) % 2 == 0 for c in cc.CASES)      # kept from the K split by the grid alone
    assert {(c.h, c.w) for c in cc.CASES if c.variant == (cc.S1, 1, 2, 1, 0)} >= {(h, w) for h in (2, 3, 4) for w in (5, 40)}
    # the concatenating form is bit-equal to the plain one on the concatenated tensor only where that takes no K split: one such case per tile height, and one that does split
    whole = {c.name: L.conv_variant(c.n, c.h, c.w, c.cin + c.cin_b, 0, c.cout, 3, 1)["ksplit"] for c in cc.CASES if c.cin_b}
    assert {(cc.BY_NAME[k].variant[2], s) for k, s in whole.items()} == {(1, 1), (1, 2), (2, 1)}
    assert {(c.cin, c.cin_b) for c in cc.CASES if c.cin_b} >= {(16, 48), (48, 16)}
    assert {c.cin for c in cc.CASES if c.variant[0] == cc.N3} == {1, 3, 5, 7} and {c.cin for c in cc.CASES if c.variant[0] == cc.STEM} == {1, 2, 3, 4}


# ---- the table's variance on a nearly constant channel: tile moments merged as Chan et al. (finalize_if_last) ------------------

def tile_pixels(ho, wo, th, tw, k):
    """valid output pixels of workgroup tile k (csrc/gpnerf_conv.hip tile_pixels)"""
    if th == 0:
        return min(tw, ho * wo - k * tw)
    tiles_x = _ceil(wo, tw)
    ty, tx = divmod(k, tiles_x)
    return min(th, ho - ty * th) * min(tw, wo - tx * tw)


def full_tiles_only(ho, wo, th, tw, k):
    """the mistake a ragged tile invites: every tile counted as full"""
    return tw if th == 0 else th * tw


def one_row_short(ho, wo, th, tw, k):
    """... and a subtler one: the last tile row or the flat tiling's last tile miscounted by one image row"""
    right = tile_pixels(ho, wo, th, tw, k)
    last = k == (_ceil(ho * wo, tw) if th == 0 else _ceil(ho, th) * _ceil(wo, tw)) - 1
    return max(1, right - min(wo, tw)) if last else right


def tile_moments(y, th, tw):
    """per tile (float32 sum, float32 M2 about the tile's own mean), as the convolutions' epilogues write them, in tile order"""
    ho, wo = y.shape
    if th == 0:
        flat = y.reshape(-1)
        parts = [flat[i:i + tw] for i in range(0, flat.size, tw)]
    else:
        parts = [y[i:i + th, j:j + tw].reshape(-1) for i in range(0, ho, th) for j in range(0, wo, tw)]
    out = []
    for p in parts:
        s = np.float32(p.sum(dtype=np.float32))
        m = np.float32(s / np.float32(p.size))
        out.append((s, np.float32(((p - m) ** 2).sum(dtype=np.float32))))
    return out


def merged_variance(moments, counts, hw, lanes):
    """finalize_if_last's ill-conditioned branch: `lanes` tile lanes merge every lanes-th tile in tile order, then the lanes are merged"""
    def merge(x, y):
        if y[0] == 0:
            return x
        if x[0] == 0:
            return y
        n, d = x[0] + y[0], y[1] - x[1]
        return (n, x[1] + d * (y[0] / n), x[2] + y[2] + d * d * (x[0] * y[0] / n))
    total = (0.0, 0.0, 0.0)
    for kl in range(lanes):
        mine = (0.0, 0.0, 0.0)
        for k in range(kl, len(moments), lanes):
            cnt = float(counts[k])
            mine = merge(mine, (cnt, float(moments[k][0]) / cnt if cnt > 0 else 0.0, float(moments[k][1])))
        total = merge(total, mine)
    return total[2] / hw


TILINGS = [(c.name, cc.out_size(c), c.variant) for c in cc.CASES
           if c.name in ("1x1-cot4", "1x1-cot2", "1x1-cot1-65tiles", "1x1-cot1-tiny", "3x3-rw2-66x70", "3x3-rw2-81tiles", "3x3-rw2-3x40", "3x3-rw1-cin32",
                         "3x3-rw1-32tiles", "cat-rw2-48+16", "3x3s2-odd", "3x3s2-65tiles", "3x3s2-3x3", "stem-cot2-cin4", "stem-cot2-35tiles", "stem-cot1-cin2")]


@pytest.mark.parametrize("name,size,variant", TILINGS, ids=[t[0] for t in TILINGS])
def test_merged_tile_moments_give_the_float64_variance_of_a_nearly_constant_channel(name, size, variant, L):
    """What the GPU test of the fused table asserts on a nearly constant channel (offset 1000, spread 1e-5: weights x 1e-5, bias 1000)
    -- the normalised values within 2e-3 of float64 -- restated on the CPU for every tiling: it holds with the right pixel counts,
    ragged tiles included, and FAILS with a wrong count for a ragged tile.  (Such a channel's float32 values are 1000 give or take
    one 6e-5 step; with eps = 1e-5 the right variance leaves those steps at ~0.02 of the normalised range, and a wrong count's
    variance, wrong by ~1e5, flattens them to nothing.  A second spread of 1e-2, where the variance itself decides the result, is
    held to the same bound here; on the GPU the float32 tile sums' own rounding of the MEAN would exceed it, so it is not run there.)"""
    ho, wo = size
    c = cc.BY_NAME[name]
    v = L.conv_variant(c.n, c.h, c.w, c.cin, c.cin_b, c.cout, c.ks, c.stride)
    th, tw, lanes = v["tile_h"], v["tile_w"], 256 // (32 * variant[1])
    rng = np.random.default_rng(ho * 1000 + wo)
    eps = 1e-5
    for spread in (1.15e-5, 1e-2):
        y = (1000.0 + spread * rng.standard_normal((ho, wo))).astype(np.float32)
        y64 = y.astype(np.float64)
        mom = tile_moments(y, th, tw)
        assert len(mom) == v["tiles"]
        mean = y64.mean()
        ref = (y64 - mean) / np.sqrt(y64.var() + eps)

        def normalised(count):
            var = merged_variance(mom, [count(ho, wo, th, tw, k) for k in range(len(mom))], float(ho * wo), lanes)
            # (the mean is subtracted in double here: what is under test is the merged variance, not the rounding of a mean near 1000)
            return (y64 - mean) / np.sqrt(np.float32(np.float32(var) + np.float32(eps)))

        assert sum(tile_pixels(ho, wo, th, tw, k) for k in range(len(mom))) == ho * wo
        assert float(np.abs(normalised(tile_pixels) - ref).max()) < 2e-3, (name, spread)
        if len(mom) > 1:                 # (a single tile's count meets no other tile's in the merge)
            for wrong in (full_tiles_only, one_row_short):
                # (spread 1e-5: an image so small that none of its float32 values left 1000 normalises to zero whatever the variance)
                if any(wrong(ho, wo, th, tw, k) != tile_pixels(ho, wo, th, tw, k) for k in range(len(mom))) and (spread > 1e-3 or np.abs(ref).max() > 4e-3):
                    assert float(np.abs(normalised(wrong) - ref).max()) > 2e-3, (name, spread, wrong.__name__)
