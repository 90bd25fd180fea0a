"""The encoder's convolutions, one row per launch variant and shape at which it can still go wrong (csrc/gpnerf_conv.hip).

A variant is the tuple (family, COT, RW, KSPLIT, CAT) that gpnerf_conv_variant reports (include/gpnerf_hip.h GPNERF_CONV_*): the
kernel family, the 32-channel output tiles per workgroup, the rows per wave of the tiled kernels (tile = 4 RW rows x 32 columns; 0
for the direct kernel's 256 consecutive pixels), the halves the channel blocks are split over, and whether a concatenation is read
in place.  VARIANTS names every tuple the launch rules can reach; tests/test_conv_host.py sweeps the rules and fails when they
reach a tuple without a case here (or a case names a tuple they cannot reach), tests/test_gpu_conv_variants.py runs every case.

The shapes are the smallest that still exercise what the variant adds: a ragged last tile in both directions, a partial last
channel tile, tiles that hang over a tiny image, an odd number of channel blocks, and tile counts beyond one round of the
table's tile loop (finalize_if_last adds 8 x 256 / (32 COT) tiles per round: 64, 32, 16 for COT 1, 2, 4).  COT = 4 needs
tiles x N x cout / 32 >= 1024, so those outputs are 32 MB; everything else is a few MB at most.
"""
from collections import namedtuple

D1, N3, S1, S2, STEM = "DIRECT_1X1", "DIRECT_NARROW3", "TILED_S1", "TILED_S2", "STEM"

# every reachable (family, COT, RW, KSPLIT, CAT)
VARIANTS = (
    (D1, 1, 0, 1, 0), (D1, 2, 0, 1, 0), (D1, 4, 0, 1, 0),
    (N3, 1, 0, 1, 0), (N3, 2, 0, 1, 0), (N3, 4, 0, 1, 0),
    (S1, 1, 1, 1, 0), (S1, 1, 1, 2, 0), (S1, 1, 2, 1, 0), (S1, 1, 1, 1, 1), (S1, 1, 2, 1, 1),
    (S2, 1, 1, 1, 0),
    (STEM, 1, 2, 1, 0), (STEM, 2, 2, 1, 0),
)

# cin_b > 0: the concatenating form on [cin channels, cin_b channels].  h, w: the INPUT size.
Case = namedtuple("Case", "name variant n cin cin_b cout ks stride h w bias")


def _c(name, variant, n, cin, cout, ks, stride, h, w, bias=False, cin_b=0):
    return Case(name, variant, n, cin, cin_b, cout, ks, stride, h, w, bias)


CASES = (
    # ---- direct kernel, 1x1: 127 x 129 outputs = 64 tiles with a ragged last one (four rounds of the table's loop at COT = 4, two at COT = 2)
    _c("1x1-cot4", (D1, 4, 0, 1, 0), 4, 16, 128, 1, 1, 127, 129, bias=True),
    _c("1x1-cot4-cout100", (D1, 4, 0, 1, 0), 4, 16, 100, 1, 1, 127, 129),
    _c("1x1-cot2", (D1, 2, 0, 1, 0), 2, 16, 128, 1, 1, 127, 129),
    _c("1x1-cot2-cout36", (D1, 2, 0, 1, 0), 4, 32, 36, 1, 1, 127, 129, bias=True),
    _c("1x1-cot1-65tiles", (D1, 1, 0, 1, 0), 1, 16, 32, 1, 1, 128, 129),
    _c("1x1-cot1-tiny", (D1, 1, 0, 1, 0), 2, 48, 36, 1, 1, 1, 3, bias=True),
    _c("1x1s2-cot4", (D1, 4, 0, 1, 0), 4, 16, 128, 1, 2, 253, 257),
    _c("1x1s2-cot2-cout36", (D1, 2, 0, 1, 0), 4, 16, 36, 1, 2, 254, 258, bias=True),
    _c("1x1s2-cot1-65tiles", (D1, 1, 0, 1, 0), 1, 16, 32, 1, 2, 255, 258),
    _c("1x1s2-cot1-odd", (D1, 1, 0, 1, 0), 3, 32, 64, 1, 2, 37, 45),
    # ---- direct kernel, 3x3 on fewer than 8 channels (flat K: the last 16-deep chunk is part-filled for every one of these widths)
    _c("narrow3-cot4-cin3", (N3, 4, 0, 1, 0), 4, 3, 128, 3, 1, 127, 129, bias=True),
    _c("narrow3-cot2-cin5", (N3, 2, 0, 1, 0), 2, 5, 128, 3, 1, 127, 129),
    _c("narrow3-cot2-cin1-cout36", (N3, 2, 0, 1, 0), 4, 1, 36, 3, 1, 127, 129, bias=True),
    _c("narrow3-cot1-cin7-65tiles", (N3, 1, 0, 1, 0), 1, 7, 32, 3, 1, 128, 129),
    _c("narrow3-cot1-cin1-2x2", (N3, 1, 0, 1, 0), 1, 1, 32, 3, 1, 2, 2),
    _c("narrow3-cot1-cin7-2x3", (N3, 1, 0, 1, 0), 3, 7, 36, 3, 1, 2, 3, bias=True),
    _c("narrow3-cot1-cin5-17x19", (N3, 1, 0, 1, 0), 2, 5, 64, 3, 1, 17, 19),
    _c("narrow3-cot1-cin3-5x2", (N3, 1, 0, 1, 0), 1, 3, 4, 3, 1, 5, 2),
    # ---- tiled 3x3 stride 1, 8-row tiles (RW = 2): the bulk of the encoder at full size
    _c("3x3-rw2-66x70", (S1, 1, 2, 1, 0), 2, 32, 36, 3, 1, 66, 70, bias=True),
    _c("3x3-rw2-81tiles", (S1, 1, 2, 1, 0), 1, 16, 32, 3, 1, 72, 260),
    _c("3x3-rw2-cin48-65x33", (S1, 1, 2, 1, 0), 1, 48, 64, 3, 1, 65, 33),
    _c("3x3-rw2-2x5", (S1, 1, 2, 1, 0), 2, 16, 32, 3, 1, 2, 5),
    _c("3x3-rw2-3x40", (S1, 1, 2, 1, 0), 1, 32, 32, 3, 1, 3, 40, bias=True),
    _c("3x3-rw2-4x5", (S1, 1, 2, 1, 0), 1, 16, 36, 3, 1, 4, 5),
    _c("3x3-rw2-2x40", (S1, 1, 2, 1, 0), 1, 16, 32, 3, 1, 2, 40),
    _c("3x3-rw2-3x5", (S1, 1, 2, 1, 0), 1, 16, 32, 3, 1, 3, 5),
    _c("3x3-rw2-4x40", (S1, 1, 2, 1, 0), 3, 64, 64, 3, 1, 4, 40),
    # ---- 4-row tiles (RW = 1) on several channel blocks without the K split: the patch / weight pipeline swaps its buffers
    _c("3x3-rw1-cin32", (S1, 1, 1, 1, 0), 3, 32, 64, 3, 1, 33, 47),
    _c("3x3-rw1-cin48", (S1, 1, 1, 1, 0), 2, 48, 36, 3, 1, 9, 35, bias=True),
    _c("3x3-rw1-cin64-grid-bound", (S1, 1, 1, 1, 0), 3, 64, 192, 3, 1, 32, 64),
    _c("3x3-rw1-cin80-grid-bound", (S1, 1, 1, 1, 0), 3, 80, 128, 3, 1, 5, 33),
    _c("3x3-rw1-32tiles", (S1, 1, 1, 1, 0), 1, 16, 32, 3, 1, 125, 31),
    # ---- ... and with it (KSPLIT = 2)
    _c("3x3-ksplit-cin64", (S1, 1, 1, 2, 0), 1, 64, 36, 3, 1, 9, 7, bias=True),
    _c("3x3-ksplit-cin96", (S1, 1, 1, 2, 0), 2, 96, 64, 3, 1, 13, 33),
    _c("3x3-ksplit-cin64-5x65", (S1, 1, 1, 2, 0), 1, 64, 32, 3, 1, 5, 65),
    # ---- the concatenating form: unequal parts whose boundary falls on an odd block
    _c("cat-rw1-16+48", (S1, 1, 1, 1, 1), 2, 16, 36, 3, 1, 9, 33, bias=True, cin_b=48),
    _c("cat-rw1-48+16", (S1, 1, 1, 1, 1), 2, 48, 32, 3, 1, 9, 33, cin_b=16),
    _c("cat-rw1-16+48-grid-bound", (S1, 1, 1, 1, 1), 3, 16, 192, 3, 1, 32, 64, cin_b=48),
    _c("cat-rw1-64+64-would-split", (S1, 1, 1, 1, 1), 1, 64, 32, 3, 1, 12, 12, cin_b=64),
    _c("cat-rw2-16+48", (S1, 1, 2, 1, 1), 1, 16, 32, 3, 1, 66, 40, bias=True, cin_b=48),
    _c("cat-rw2-48+16", (S1, 1, 2, 1, 1), 2, 48, 36, 3, 1, 66, 40, cin_b=16),
    _c("cat-rw2-3x40", (S1, 1, 2, 1, 1), 2, 16, 32, 3, 1, 3, 40, cin_b=48),
    # ---- 3x3 stride 2 (4 x 32 output tiles, 9 x 65 patch)
    _c("3x3s2-2x2", (S2, 1, 1, 1, 0), 1, 16, 32, 3, 2, 2, 2),
    _c("3x3s2-2x3", (S2, 1, 1, 1, 0), 2, 16, 32, 3, 2, 2, 3, bias=True),
    _c("3x3s2-3x2", (S2, 1, 1, 1, 0), 1, 32, 36, 3, 2, 3, 2),
    _c("3x3s2-3x3", (S2, 1, 1, 1, 0), 1, 16, 32, 3, 2, 3, 3),
    _c("3x3s2-even", (S2, 1, 1, 1, 0), 2, 48, 64, 3, 2, 10, 66),
    _c("3x3s2-odd", (S2, 1, 1, 1, 0), 2, 32, 64, 3, 2, 11, 67, bias=True),
    _c("3x3s2-65tiles", (S2, 1, 1, 1, 0), 1, 16, 32, 3, 2, 104, 260),
    # ---- the stem
    _c("stem-cot1-cin1-4x4", (STEM, 1, 2, 1, 0), 1, 1, 32, 7, 2, 4, 4),
    _c("stem-cot1-cin2", (STEM, 1, 2, 1, 0), 2, 2, 96, 7, 2, 21, 70, bias=True),
    _c("stem-cot1-cin4-cout68", (STEM, 1, 2, 1, 0), 2, 4, 68, 7, 2, 4, 5),
    _c("stem-cot2-cin3-4x4", (STEM, 2, 2, 1, 0), 3, 3, 64, 7, 2, 4, 4, bias=True),
    _c("stem-cot2-cin4", (STEM, 2, 2, 1, 0), 2, 4, 64, 7, 2, 37, 45),
    _c("stem-cot2-cin2-cout40", (STEM, 2, 2, 1, 0), 1, 2, 40, 7, 2, 18, 66),
    _c("stem-cot2-35tiles", (STEM, 2, 2, 1, 0), 1, 3, 64, 7, 2, 112, 260),
    _c("stem-cot1-72tiles", (STEM, 1, 2, 1, 0), 1, 1, 32, 7, 2, 128, 516),
)

BY_NAME = {c.name: c for c in CASES}
# the cases whose output is one workgroup tile (tests/test_conv_host.py holds this against the query): a single tile's pixel count
# never meets another's in the table's merge, so the nearly-constant-channel check of the GPU tests leaves them out
ONE_TILE = frozenset(("1x1-cot1-tiny", "narrow3-cot1-cin1-2x2", "narrow3-cot1-cin7-2x3", "narrow3-cot1-cin3-5x2", "3x3-rw2-2x5", "3x3-rw2-4x5",
                      "3x3-rw2-3x5", "3x3s2-2x2", "3x3s2-2x3", "3x3s2-3x2", "3x3s2-3x3", "stem-cot1-cin1-4x4", "stem-cot1-cin4-cout68",
                      "stem-cot2-cin3-4x4"))
assert len(BY_NAME) == len(CASES)


def out_size(c):
    pad = c.ks // 2
    return (c.h + 2 * pad - c.ks) // c.stride + 1, (c.w + 2 * pad - c.ks) // c.stride + 1


def reads_through_a_norm(c):
    """the forms that can apply a pending InstanceNorm (+ ReLU) to their input while they read it (include/gpnerf_hip.h in_table)"""
    return c.cin_b == 0 and c.cin % 16 == 0 and c.ks in (1, 3)
