"""CPU: frame keeps its face.  Every name frame.py defined before the mesh tools moved out -- functions, classes, upper-case
constants, and the four private names tests and tools reach for -- is still an attribute of frame; every moved name is the SAME
object in frame and in the module that now holds it; and none of the new modules imports frame (a fresh interpreter says so)."""
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# taken from frame.py at the commit before the split (its top-level defs, classes and upper-case assignments), not from today's code
STAYED = (
    "fetch_host", "pack_head", "Frame", "relayout_images", "patch_order", "patch_order_device", "patch_order_rays", "render_plan",
    "render_fused", "head_forward", "sigma_features", "rgb_head_forward", "composite", "make_rays", "sample_points", "sample_volume",
    "project_gather", "select_rays", "patch_order_of", "MESH_PAD", "lattice_axis", "mesh_box", "lattice_axes", "dataset_lattice_axis",
    "dataset_lattice_axes", "visual_hull", "density_lattice", "lattice_of", "query_points", "parse_keep", "cube_clean", "mesh_normals",
    "extract_mesh",
)
MOVED = {
    "_args": ("_stream_ptr", "_workspace", "_require_gpu"),
    "mesh_edit": ("parse_simplify", "simplify_grid", "simplify_mesh", "parse_smooth", "MeshAdjacency", "mesh_adjacency", "mesh_topology",
                  "read_mesh_topology", "smooth_mesh", "parse_components", "MeshComponents", "mesh_components", "read_mesh_components",
                  "filter_components", "repair_mesh", "read_mesh_repair", "repair_mesh_object", "_repair_flags"),
    "mesh_query": ("mesh_to_device", "mesh_grid_caps", "MeshGrid", "build_mesh_grid", "point_mesh_distance", "sample_surface",
                   "distance_stats", "align_workspace", "rigid_fit", "transform_points", "read_transform", "align_init", "align_step",
                   "align_mesh", "MESH_METRIC_ROWS", "ALIGN_SAMPLES", "mesh_metrics", "read_mesh_metrics", "raycast_mesh", "pixel_rays",
                   "mesh_visibility"),
    "mesh_lattice": ("marching_cubes", "VoxelGrid", "voxelize_mesh", "voxelize_cube", "voxel_stats", "read_volume_metrics", "SdfGrid",
                     "mesh_sdf", "DepthFusion", "fuse_depth", "read_fusion_stats"),
    "mesh_draw": ("rasterize_mesh", "silhouette_stats", "read_silhouette_metrics", "TEXTURE_WANT", "face_vertex_normals", "texture_points",
                  "texture_mesh", "read_texture_stats", "atlas_layout", "atlas_texels", "TextureAtlas", "atlas_face_uvs", "atlas_pack",
                  "texture_atlas"),
}


def test_the_tuple_is_the_parents_whole_surface():
    names = STAYED + tuple(n for group in MOVED.values() for n in group)
    assert len(names) == len(set(names)) == 96 + 4      # 96 public names at the parent, and the four private ones


def test_frame_still_offers_every_name():
    F = importlib.import_module("gp-nerf_amd.frame")
    missing = [n for n in STAYED + tuple(n for group in MOVED.values() for n in group) if not hasattr(F, n)]
    assert not missing, f"frame lost {missing}"


@pytest.mark.parametrize("module", sorted(MOVED))
def test_a_moved_name_is_one_object_in_both_modules(module):
    F = importlib.import_module("gp-nerf_amd.frame")
    M = importlib.import_module(f"gp-nerf_amd.{module}")
    differ = [n for n in MOVED[module] if getattr(M, n, None) is None or getattr(M, n) is not getattr(F, n)]
    assert not differ, f"frame.<name> is not {module}.<name> for {differ}"


def test_the_new_modules_do_not_import_frame():
    code = ("import importlib, sys\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            f"for m in {sorted(MOVED)!r}:\n"
            "    importlib.import_module('gp-nerf_amd.' + m)\n"
            "    assert 'gp-nerf_amd.frame' not in sys.modules, m + ' imports frame'\n"
            "print('clean')\n")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "clean", run.stdout + run.stderr
