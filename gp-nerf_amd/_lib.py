"""ctypes binding of include/gpnerf_hip.h.

The shared library is built in-tree (gp-nerf_amd/csrc/libgpnerf_hip.so) by
``__graft_entry__.build()`` / ``make -C gp-nerf_amd/csrc``.  There is NO fallback: if the
library is missing or fails to load, every entry point raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree build, always.  GPNERF_LIB_PATH (a differently built library: the A/B measurements of
# tools/ab_libs.sh, the stamps and wavetimes builds of csrc/diag/) is honoured only together with GPNERF_DEBUG=1.
_DEBUG = os.environ.get("GPNERF_DEBUG", "0") == "1"
LIB_PATH = (os.environ.get("GPNERF_LIB_PATH") if _DEBUG else None) or os.path.join(HERE, "csrc", "libgpnerf_hip.so")

VIEWS, CH, LEVELS = 3, 32, 4
FP = C.POINTER(C.c_float)
DP = C.POINTER(C.c_double)
U8P = C.POINTER(C.c_uint8)


class GpnerfFrame(C.Structure):
    _fields_ = [
        ("vol", C.c_void_p * LEVELS),
        ("vol_dhw", (C.c_int32 * 3) * LEVELS),
        ("featmaps", C.c_void_p),
        ("feat_h", C.c_int32), ("feat_w", C.c_int32),
        ("imgs", C.c_void_p),
        ("img_h", C.c_int32), ("img_w", C.c_int32),
        ("proj", (C.c_float * 12) * VIEWS),
        ("Rh", C.c_float * 9), ("Th", C.c_float * 3),
        ("bounds_min", C.c_float * 3), ("voxel", C.c_float * 3),
        ("out_sh", C.c_int32 * 3),
        ("head_blob", C.c_void_p),
        ("head_blob_split", C.c_void_p),
        ("occ", C.c_void_p),
        ("vol_folded", C.c_void_p * LEVELS),
        ("head_blob_ref", C.c_void_p),
    ]


PYRAMID_MAX_LEVELS = 4


class GpnerfSparseConv(C.Structure):
    """include/gpnerf_hip.h: one convolution of the sparse pyramid (gpnerf_sparse_pyramid_run)"""
    _fields_ = [("strided", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32), ("form", C.c_int32),
                ("weight", C.c_void_p), ("bn_scale", C.c_void_p), ("bn_shift", C.c_void_p), ("weight_raw", C.c_void_p)]


class GpnerfPyramid(C.Structure):
    """include/gpnerf_hip.h: the buffers of one frame's pyramid (gpnerf_sparse_pyramid_plan / _run)"""
    _fields_ = [("n_levels", C.c_int32), ("m0", C.c_int32), ("dims0", C.c_int32 * 3),
                ("dims", (C.c_int32 * 3) * PYRAMID_MAX_LEVELS), ("cap", C.c_int32 * PYRAMID_MAX_LEVELS), ("ch", C.c_int32 * PYRAMID_MAX_LEVELS),
                ("coords0", C.c_void_p), ("grid0", C.c_void_p), ("dup_scratch", C.c_void_p),
                ("grid", C.c_void_p * PYRAMID_MAX_LEVELS), ("coords", C.c_void_p * PYRAMID_MAX_LEVELS), ("m", C.c_void_p * PYRAMID_MAX_LEVELS),
                ("vol", C.c_void_p * PYRAMID_MAX_LEVELS), ("feat_a", C.c_void_p), ("feat_b", C.c_void_p), ("feat_c", C.c_void_p)]



HEAD_FIELDS = [
    ("geo", "sigmahead.out_geometry_fc.0"), ("b1", "rgbhead.base_fc.0"), ("b2", "rgbhead.base_fc.2"),
    ("v1", "rgbhead.vis_fc.0"), ("v2", "rgbhead.vis_fc.2"), ("r1", "rgbhead.rgb_fc.0"),
    ("r2", "rgbhead.rgb_fc.2"), ("r3", "rgbhead.rgb_fc.4"), ("d1", "rgbhead.out_geometry_fc.0"),
    ("d2", "rgbhead.out_geometry_fc.2"), ("d3", "rgbhead.out_geometry_fc.4"), ("d4", "rgbhead.out_geometry_fc.6"),
]
HEAD_SHAPES = {
    "geo": (64, 128), "b1": (64, 105), "b2": (32, 64), "v1": (32, 32), "v2": (32, 32), "r1": (32, 96),
    "r2": (16, 32), "r3": (3, 16), "d1": (64, 134), "d2": (32, 64), "d3": (16, 32), "d4": (1, 16),
}


class GpnerfHeadParams(C.Structure):
    _fields_ = [f for s, _ in HEAD_FIELDS for f in ((s + "_w", FP), (s + "_b", FP))]


class GpnerfOutputs(C.Structure):
    _fields_ = [
        ("rgb", C.c_void_p), ("depth", C.c_void_p), ("acc", C.c_void_p), ("disp", C.c_void_p),
        ("weights", C.c_void_p), ("z_vals", C.c_void_p), ("rgb_in", C.c_void_p), ("ray_mask", C.c_void_p),
        ("raw", C.c_void_p), ("samples_done", C.c_void_p), ("step_stats", C.c_void_p),
    ]


PLAN_CLEARS = 5
PLAN_WEIGHTS, PLAN_RAW, PLAN_SAMPLES_DONE, PLAN_FOLDED, PLAN_OCC = 1, 2, 4, 8, 16
SEL_NAMES = ("REF", "FOLD", "SPLIT", "GUARD")
COLOUR_NAMES = ("STEP", "WAVE", "LIST", "UNIFIED")
SHAPE_NAMES = ("STATIC", "QUEUE", "QUEUE_REMAINDER", "REMAINDER_UNITS", "CHAINED")
REGION_NAMES = ("queue", "part", "chain", "list", "mask", "guard")


class GpnerfRegion(C.Structure):
    _fields_ = [("off", C.c_uint64), ("bytes", C.c_uint64)]


class GpnerfRenderPlan(C.Structure):
    """include/gpnerf_hip.h: what gpnerf_render_fused would do with a call (gpnerf_render_plan)"""
    _fields_ = ([("sel", C.c_int32), ("colour", C.c_int32), ("shape", C.c_int32), ("waves", C.c_int32), ("split", C.c_int32),
                 ("grid", C.c_uint32), ("n_cus", C.c_int32), ("reserved_", C.c_int32), ("tiles", C.c_int64), ("main_rays", C.c_int64)]
                + [(n, GpnerfRegion) for n in REGION_NAMES] + [("clear", GpnerfRegion * PLAN_CLEARS)])

    def triple(self):
        return SHAPE_NAMES[self.shape], COLOUR_NAMES[self.colour], SEL_NAMES[self.sel]

    def regions(self):
        """{name: (off, bytes)} of the regions the call uses"""
        return {n: (int(getattr(self, n).off), int(getattr(self, n).bytes)) for n in REGION_NAMES if getattr(self, n).bytes}

    def __str__(self):
        return (f"{'/'.join(self.triple())} waves={self.waves} split={self.split} grid={self.grid} cus={self.n_cus} tiles={self.tiles} "
                f"main_rays={self.main_rays} " + " ".join(f"{n}@{o}+{b}" for n, (o, b) in self.regions().items()))


FLAG_NEG_RAY = 1
FLAG_EARLY_TERM = 2
FLAG_OCC_CULL = 4
FLAG_SPLIT_F16 = 8
FLAG_FLIP_SAMPLES = 16
FLAG_SPLIT_GUARD = 32
FLAG_REF_ORDER = 64
FLAG_NO_EXITS = 128
FLAG_SHARED_DEVICE = 256
FLAG_DENSITY_ONLY = 512
FOLD_FIRST_LEVEL = 2
# gpnerf_cube_clean's flags and the names of its six stats (include/gpnerf_hip.h)
CUBE_KEEP, CUBE_FILL = 1, 2
CUBE_STATS = ("components", "inside_points", "components_kept", "inside_points_kept", "cavities_filled", "points_filled")
# gpnerf_image_metrics' slot (include/gpnerf_hip.h GPNERF_METRICS_*)
METRICS_MSE, METRICS_SSIM, METRICS_X, METRICS_Y, METRICS_W, METRICS_H, METRICS_POPULATION, METRICS_STATUS, METRICS_DOUBLES = range(9)
# the mesh grid's header words, the sampler's status and gpnerf_distance_stats' slot (include/gpnerf_hip.h GPNERF_GRID_* / _SAMPLE_* / _DIST_*)
GRID_OK, GRID_OVERFLOW, GRID_BUILDING = range(3)
GRID_HDR = {"magic": 0, "status": 1, "skipped": 2, "valid": 3, "cells": 4, "n_cells": 7, "cell_cap": 8, "entry_cap": 9, "needed": 10,
            "lo": 12, "size": 15, "inv": 18}
GRID_HDR_INTS = 64
SAMPLE_OK, SAMPLE_NO_AREA = range(2)
DIST_FINITE, DIST_INF, DIST_NAN, DIST_MEAN, DIST_MEAN_SQ, DIST_MAX, DIST_WITHIN = range(7)
DIST_MAX_THRESHOLDS, DIST_DOUBLES = 4, 10
# gpnerf_rigid_fit / gpnerf_align_step: the sums' geometry, the statuses, the slot's indices and the workspace's (doubles) (include/gpnerf_hip.h
# GPNERF_ALIGN_* / GPNERF_XFORM_*)
ALIGN_THREADS, ALIGN_BLOCKS = 256, 64
ALIGN_OK, ALIGN_FEW, ALIGN_SINGULAR = range(3)
ALIGN_STATUS_NAMES = ("ok", "few", "singular")
XFORM_M, XFORM_SCALE, XFORM_STATUS, XFORM_USED, XFORM_SKIPPED, XFORM_TRIMMED, XFORM_WSUM, XFORM_RMS, XFORM_PIVOT = 0, 12, 13, 14, 15, 16, 17, 18, 19
XFORM_DOUBLES = 24
ALIGN_WS = {"sums1": 0, "centroids": 8, "sums2": 16, "step": 32, "counts": 64, "rows": 128, "count_rows": 1984}
ALIGN_WS_DOUBLES = 2240
# gpnerf_mesh_rasterize's stats row and gpnerf_silhouette_stats' row (include/gpnerf_hip.h GPNERF_RASTER_* / GPNERF_SILHOUETTE_*)
RASTER_DRAWN, RASTER_SKIPPED_VERTEX, RASTER_SKIPPED_AREA, RASTER_PIXELS = range(4)
SILHOUETTE_COVERED, SILHOUETTE_GT, SILHOUETTE_BOTH, SILHOUETTE_EITHER, SILHOUETTE_IGNORED, SILHOUETTE_COUNTS = range(6)
RASTER_MAX_VIEWS, RASTER_MAX_ATTRS = 8, 4
# gpnerf_mesh_simplify_count's stats, the workspace's status word and its values (include/gpnerf_hip.h GPNERF_SIMPLIFY_*)
SIMPLIFY_STATS = ("vertices_out", "faces_out", "faces_invalid", "faces_collapsed", "faces_cancelled", "faces_duplicate", "clusters_clamped",
                  "clusters_dropped")
SIMPLIFY_HDR_STATUS = 12
SIMPLIFY_COUNTING, SIMPLIFY_COUNTED, SIMPLIFY_EMITTED, SIMPLIFY_MISMATCH = 1, 2, 3, 4
SIMPLIFY_MAX_CELLS = 1 << 26
# gpnerf_mesh_adjacency's stats, the vertex flags, gpnerf_mesh_adjacency_layout's offsets and gpnerf_mesh_smooth's flag and limits
# (include/gpnerf_hip.h GPNERF_TOPOLOGY_* / GPNERF_VERTEX_* / GPNERF_ADJACENCY_* / GPNERF_SMOOTH_*)
TOPOLOGY_STATS = ("faces_used", "faces_dropped", "vertices_referenced", "edges", "boundary_edges", "nonmanifold_edges", "inconsistent_edges",
                  "euler", "boundary_vertices", "max_valence")
VERTEX_REFERENCED, VERTEX_BOUNDARY = 1, 2
ADJACENCY_START, ADJACENCY_NEIGHBOURS, ADJACENCY_VERTEX_FLAGS = range(3)
SMOOTH_PIN_BOUNDARY = 1
SMOOTH_MAX_ITERATIONS = 10000
ADJACENCY_MAX_FACES = ((1 << 31) - 1) // 3
# gpnerf_mesh_components' stats, its table's columns, the keep modes, gpnerf_mesh_components_layout's offsets, the workspace's status
# word and its values (include/gpnerf_hip.h GPNERF_COMPONENTS_* / GPNERF_COMPONENT_*)
COMPONENT_STATS = ("components", "closed_components", "largest", "largest_faces", "largest_vertices", "largest_euler", "kept_components",
                   "kept_vertices", "kept_faces")
COMPONENT_COLS = ("label", "vertices", "edges", "faces", "euler", "boundary_vertices")
COMPONENTS_KEEP_ALL, COMPONENTS_KEEP_LARGEST, COMPONENTS_KEEP_MIN_FACES = range(3)
COMPONENTS_LABEL, COMPONENTS_VERTEX_COMPONENT, COMPONENTS_FACE_COMPONENT, COMPONENTS_TABLE = range(4)
COMPONENTS_HDR_STATUS = 3
COMPONENTS_COUNTING, COMPONENTS_COUNTED, COMPONENTS_EMITTED, COMPONENTS_MISMATCH, COMPONENTS_NO_ADJACENCY = 1, 2, 3, 4, 5
# gpnerf_mesh_repair's flags, face fates, stats, the workspace's status word and its values (include/gpnerf_hip.h GPNERF_REPAIR_*)
REPAIR_WELD, REPAIR_DROP_DUPLICATES, REPAIR_ORIENT, REPAIR_OUTWARD = 1, 2, 4, 8
REPAIR_FATES = ("kept", "kept_flipped", "invalid", "unkeyable", "collapsed", "duplicate")
REPAIR_STATS = ("vertices_out", "faces_out", "vertices_welded", "vertices_unkeyable", "vertices_unreferenced", "faces_invalid", "faces_unkeyable",
                "faces_collapsed", "faces_duplicate", "faces_flipped", "edges_nonmanifold", "patches", "patches_closed", "patches_unorientable",
                "patches_inverted", "patches_undecided")
REPAIR_HDR_STATUS = 3
REPAIR_COUNTING, REPAIR_COUNTED, REPAIR_EMITTED, REPAIR_MISMATCH, REPAIR_NO_COUNT = 1, 2, 3, 4, 5
REPAIR_MAX_VERTICES = 1 << 30
# gpnerf_mesh_voxelize's rules and stats, gpnerf_voxel_stats' row (include/gpnerf_hip.h GPNERF_VOXEL_*)
VOXEL_PARITY, VOXEL_NONZERO = range(2)
VOXEL_RULES = {"parity": VOXEL_PARITY, "nonzero": VOXEL_NONZERO}
VOXEL_STATS = ("used", "skipped_vertex", "skipped_area", "crossings", "open_columns", "occupied")
VOXEL_A, VOXEL_B, VOXEL_BOTH, VOXEL_EITHER, VOXEL_COUNTS = range(5)
VOXEL_MAX_POINTS = 1 << 28
# gpnerf_mesh_sdf's stats, its tier threshold and its limit on the band in steps (include/gpnerf_hip.h GPNERF_SDF_*)
SDF_STATS = ("used", "skipped_vertex", "skipped_box", "large", "in_band", "inside", "visited", "pairs")
SDF_LARGE_POINTS = 64
SDF_MAX_BAND_STEPS = 1024
# gpnerf_mesh_raycast's modes and gpnerf_pixel_rays' limit on the cameras (include/gpnerf_hip.h GPNERF_RAYCAST_*)
RAYCAST_NEAREST, RAYCAST_ANY = range(2)
RAYCAST_MODES = {"nearest": RAYCAST_NEAREST, "any": RAYCAST_ANY}
RAYCAST_MAX_VIEWS = 8
# gpnerf_texture_points' modes, the fates of a (point, view) pair -- the columns of its stats -- and its limits (include/gpnerf_hip.h
# GPNERF_TEXTURE_*)
TEXTURE_BLEND, TEXTURE_BEST = range(2)
TEXTURE_MODES = {"blend": TEXTURE_BLEND, "best": TEXTURE_BEST}
TEXTURE_STATS = ("used", "behind", "outside", "masked", "backfacing", "occluded")
TEXTURE_USED, TEXTURE_BEHIND, TEXTURE_OUTSIDE, TEXTURE_MASKED, TEXTURE_BACKFACING, TEXTURE_OCCLUDED, TEXTURE_FATES = range(7)
TEXTURE_TOTALS = ("seen", "unseen")
TEXTURE_MAX_VIEWS, TEXTURE_MAX_SHARPNESS, TEXTURE_MAX_CHANNELS = 8, 4, 4
# gpnerf_atlas_layout's row, gpnerf_atlas_pack's coverage values, gpnerf_atlas_shade's filters and the limits on res (include/gpnerf_hip.h
# GPNERF_ATLAS_*)
ATLAS_LAYOUT = ("cells_x", "cells_y", "width", "height", "texels_per_face", "n_texels")
ATLAS_UNOWNED, ATLAS_SEEN, ATLAS_FALLBACK, ATLAS_GUTTER = range(4)
ATLAS_SIMPLEX, ATLAS_NEAREST = range(2)
ATLAS_FILTERS = {"simplex": ATLAS_SIMPLEX, "nearest": ATLAS_NEAREST}
ATLAS_MIN_RES, ATLAS_MAX_RES = 2, 64
# gpnerf_fusion_integrate's fates of a (lattice point, view) pair -- the columns of its stats --, finalise's totals, the bits of a
# point's flag byte and the limit on the views of one call (include/gpnerf_hip.h GPNERF_FUSION_*)
FUSION_FATES = ("behind", "outside", "nodata", "empty", "hidden", "near")
FUSION_BEHIND, FUSION_OUTSIDE, FUSION_NODATA, FUSION_EMPTY, FUSION_HIDDEN, FUSION_NEAR, FUSION_N_FATES = range(7)
FUSION_TOTALS = ("seen", "surface", "interior", "unknown")
FUSION_SEEN, FUSION_SURFACE, FUSION_INTERIOR, FUSION_UNKNOWN, FUSION_N_TOTALS = range(5)
FUSION_FLAG_HIDDEN, FUSION_FLAG_NEAR = 1, 2
FUSION_MAX_VIEWS = 8
# gpnerf_conv_variant's row and its kernel families (include/gpnerf_hip.h GPNERF_CONV_*)
CONV_VARIANT = ("family", "cot", "rw", "ksplit", "cat", "tiles", "tile_h", "tile_w")
CONV_FAMILIES = ("REFUSED", "DIRECT_1X1", "DIRECT_NARROW3", "TILED_S1", "TILED_S2", "STEM")


def conv_variant(n, h, w, cin_a, cin_b, cout, ks, stride):
    """gpnerf_conv_variant as a dict (host arithmetic only): which kernel the convolution calls launch for this shape; the family
    by name, "REFUSED" for a shape they do not take."""
    row = (C.c_int32 * len(CONV_VARIANT))()
    lib().gpnerf_conv_variant(n, h, w, cin_a, cin_b, cout, ks, stride, row)
    v = dict(zip(CONV_VARIANT, row))
    v["family"] = CONV_FAMILIES[v["family"]]
    return v


# every symbol include/gpnerf_hip.h declares: (restype, argtypes)
SYMBOLS = {
    "gpnerf_head_blob_floats": (C.c_int64, []),
    "gpnerf_pack_head": (C.c_int, [C.POINTER(GpnerfHeadParams), FP]),
    "gpnerf_pack_head_ref": (C.c_int, [C.POINTER(GpnerfHeadParams), FP]),
    "gpnerf_head_blob_split_floats": (C.c_int64, []),
    "gpnerf_pack_head_split": (C.c_int, [C.POINTER(GpnerfHeadParams), FP]),
    "gpnerf_render_fused": (C.c_int, [C.POINTER(GpnerfFrame), C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_float,
                                      C.c_void_p, C.POINTER(GpnerfOutputs), C.c_void_p, C.c_size_t, C.c_void_p]),
    "gpnerf_fold_volumes": (C.c_int, [C.POINTER(GpnerfFrame), C.POINTER(C.c_void_p), C.c_void_p]),
    "gpnerf_render_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "gpnerf_render_guard_bytes": (C.c_size_t, [C.c_int64]),
    "gpnerf_render_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32, C.c_size_t, C.POINTER(GpnerfRenderPlan)]),
    "gpnerf_sample_points": (C.c_int, [C.POINTER(GpnerfFrame), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "gpnerf_sample_volume": (C.c_int, [C.POINTER(GpnerfFrame), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gpnerf_project_gather": (C.c_int, [C.POINTER(GpnerfFrame), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "gpnerf_head_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gpnerf_sigma_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_rgb_head_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gpnerf_composite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                   C.POINTER(GpnerfOutputs), C.c_void_p]),
    "gpnerf_make_rays": (C.c_int, [C.c_int32, C.c_int32, DP, DP, DP, FP, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_select_pixels": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, FP, FP, FP, FP, FP, FP, C.c_int32,
                                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_make_rays_demo": (C.c_int, [C.c_int32, C.c_int32, FP, FP, FP, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_conv_packed_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gpnerf_conv_pack_weight": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gpnerf_conv_out_tiles": (C.c_int32, [C.c_int32] * 5),
    "gpnerf_conv_variant": (C.c_int, [C.c_int32] * 8 + [C.POINTER(C.c_int32)]),
    "gpnerf_conv2d_nhwc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gpnerf_conv2d_nhwc_exact": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_void_p]),
    "gpnerf_conv2d_norm_nhwc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gpnerf_conv2d_norm_cat_nhwc": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int32, C.c_void_p]),
    "gpnerf_norm_apply_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p]),
    "gpnerf_instance_norm_nhwc_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int64, C.c_int32]),
    "gpnerf_instance_norm_act_nhwc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
                                                C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_upsample2x_nhwc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gpnerf_vertex_attention": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p]),
    "gpnerf_build_occupancy": (C.c_int, [C.POINTER(GpnerfFrame), C.c_void_p, C.c_void_p]),
    "gpnerf_sparse_index": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "gpnerf_sparse_conv3": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                      C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_sparse_conv3_mfma": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                           C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_sparse_conv3_mfma16": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_sparse_packed_weight16_bytes": (C.c_int64, [C.c_int32]),
    "gpnerf_sparse_pack_weight16": (C.c_int, [FP, C.c_int32, C.c_int32, C.c_void_p]),
    "gpnerf_sparse_packed_weight_floats": (C.c_int64, [C.c_int32]),
    "gpnerf_sparse_pack_weight": (C.c_int, [FP, C.c_int32, C.c_int32, FP]),
    "gpnerf_sparse_pyramid_plan": (C.c_int, [C.POINTER(GpnerfPyramid), C.c_void_p]),
    "gpnerf_sparse_pyramid_run": (C.c_int, [C.POINTER(GpnerfPyramid), C.c_void_p, C.c_int32, C.POINTER(GpnerfSparseConv), C.c_int32, C.c_void_p]),
    "gpnerf_sparse_merge_duplicates": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32),
                                                 C.c_void_p, C.c_void_p]),
    "gpnerf_sparse_down_sites": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.c_void_p]),
    "gpnerf_sparse_to_dense": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "gpnerf_zero_volume": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p]),
    "gpnerf_sparse_scatter_dense": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                              C.POINTER(C.c_int32), C.c_void_p, C.c_int32, C.c_void_p]),
    "gpnerf_relayout_volume": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "gpnerf_relayout_featmaps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "gpnerf_relayout_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "gpnerf_patch_order_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gpnerf_patch_order": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_density_lattice": (C.c_int, [C.POINTER(GpnerfFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_visual_hull": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_density_lattice_masked": (C.c_int, [C.POINTER(GpnerfFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32,
                                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_query_points": (C.c_int, [C.POINTER(GpnerfFrame), C.c_void_p, C.c_int64, C.c_uint32, C.POINTER(C.c_double), C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_workspace_bytes": (C.c_int64, [C.POINTER(C.c_int32)]),
    "gpnerf_mesh_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_emit": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_cube_clean_workspace_bytes": (C.c_int64, [C.POINTER(C.c_int32)]),
    "gpnerf_cube_clean": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_uint32, C.c_int64, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_normals": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_int64, FP, C.c_void_p, C.c_void_p]),
    "gpnerf_metrics_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gpnerf_image_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_grid_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int64]),
    "gpnerf_mesh_grid_build": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gpnerf_mesh_distance": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_sample_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gpnerf_mesh_sample_surface": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_distance_stats": (C.c_int, [C.c_void_p, C.c_int64, FP, C.c_int32, C.c_void_p, C.c_void_p]),
    "gpnerf_align_workspace_bytes": (C.c_size_t, []),
    "gpnerf_rigid_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gpnerf_align_init": (C.c_int, [C.c_void_p, C.c_int64, DP, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gpnerf_transform_points": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gpnerf_align_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gpnerf_mesh_raster_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "gpnerf_mesh_rasterize": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, DP, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_interpolate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, DP, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_double, C.c_void_p, C.c_int32, FP, C.c_void_p, C.c_void_p]),
    "gpnerf_silhouette_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_simplify_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "gpnerf_mesh_simplify_count": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, FP, C.c_float, C.POINTER(C.c_int32), C.c_void_p,
                                             C.c_size_t, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_simplify_emit": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_adjacency_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gpnerf_mesh_adjacency_layout": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "gpnerf_mesh_adjacency": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_smooth": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_int32, C.c_double, C.c_double, C.c_uint32, C.c_void_p,
                                     C.c_void_p]),
    "gpnerf_mesh_components_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gpnerf_mesh_components_layout": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "gpnerf_mesh_components": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_components_emit": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_repair_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "gpnerf_mesh_repair": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p]),
    "gpnerf_mesh_repair_emit": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_voxelize_workspace_bytes": (C.c_size_t, [C.c_int64, C.POINTER(C.c_int32), C.c_int32]),
    "gpnerf_mesh_voxelize": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, DP, C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_voxel_from_cube": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_void_p, C.c_void_p]),
    "gpnerf_voxel_unpack": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "gpnerf_voxel_stats": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "gpnerf_voxel_contains": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), DP, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_sdf_workspace_bytes": (C.c_size_t, [C.c_int64, C.POINTER(C.c_int32)]),
    "gpnerf_mesh_sdf": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, DP, C.POINTER(C.c_int32), C.c_float, C.c_void_p, C.c_void_p,
                                  C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_sdf_sample": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), DP, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gpnerf_mesh_raycast": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_pixel_rays": (C.c_int, [DP, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "gpnerf_texture_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int32]),
    "gpnerf_texture_points": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, DP, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_double, C.c_int32, C.c_float,
                                        C.c_int32, C.c_void_p, FP, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "gpnerf_atlas_layout": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "gpnerf_atlas_texels": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_atlas_pack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, FP, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_atlas_shade": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, DP, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                     C.c_void_p, C.c_int32, C.c_int32, C.c_int32, FP, C.c_void_p, C.c_void_p]),
    "gpnerf_fusion_reset": (C.c_int, [C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_fusion_integrate": (C.c_int, [C.c_void_p, C.c_void_p, DP, C.c_int32, C.c_int32, C.c_int32, DP, C.POINTER(C.c_int32), C.c_float,
                                          C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_fusion_finalise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "gpnerf_fusion_oneshot": (C.c_int, [C.c_void_p, C.c_void_p, DP, C.c_int32, C.c_int32, C.c_int32, DP, C.POINTER(C.c_int32), C.c_float,
                                        C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gpnerf_head_layout": (C.c_int, [C.POINTER(C.c_int32)]),
    "gpnerf_strerror": (C.c_char_p, [C.c_int]),
    "gpnerf_rays_per_tile": (C.c_int32, []),
    "gpnerf_build_info": (C.c_char_p, []),
}

_lib = None


class GpnerfError(RuntimeError):
    pass


def lib():
    """Load the HIP library; fails loudly when it is absent (no CPU / PyTorch fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GpnerfError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C gp-nerf_amd/csrc` (hipcc --offload-arch=gfx950). There is no fallback path.")
        # torch first: it bundles its own HIP runtime, and the one that is loaded first serves the whole process.  Loaded the
        # other way round, this library binds to the system runtime while torch's streams and allocations live in another
        # one, and every launch fails.
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the ABI and the header drift apart
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(code, what):
    if code != 0:
        raise GpnerfError(f"{what} failed: {lib().gpnerf_strerror(code).decode()} ({code})")
