// gpnerf_mesh.hip -- marching cubes over the inference renderer's alpha cube on gfx950 (libs/renders/demo_render.py:366-376,
// where the reference copies the cube to the host and runs mcubes.marching_cubes on the CPU).
//
// Two passes, no atomics, so the output is a function of the cube and the iso value alone (not of launch geometry or
// scheduling); include/gpnerf_hip.h states the output's specification:
//   1. count_kernel: per lattice point, its crossed edges along +x, +y, +z (each lattice edge is owned by its lower end) and,
//      where the point is the lowest corner of a cell, the cell's triangle count from the case table; each workgroup scans its
//      1024 points' counts (exclusive, vertices and triangles side by side) and leaves its two totals;
//      scan_blocks_kernel (one workgroup) turns the totals into the workgroups' offsets and the two grand totals;
//   2. emit_kernel: per point, its vertices at (its workgroup's offset + its local offset), and per cell its triangles in table
//      order, each corner the vertex of the crossed edge (looked up the same way at the edge's owner).
// The case tables below are written out from gp-nerf_amd/mesh.py:case_tables() (tests/test_mesh.py holds them equal).
//
// Behind marching cubes, the two calls that finish its input and output (specified in include/gpnerf_hip.h as well): gpnerf_cube_clean
// (floaters and enclosed cavities, by connected components of the cube's points; integer atomics whose outcome does not depend on
// their order) and gpnerf_mesh_normals (the cube's gradient at the vertices).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status

constexpr int MC_THREADS = 256, MC_PER_THREAD = 4, MC_BLOCK = MC_THREADS * MC_PER_THREAD;    // points per scan block
constexpr int MC_MAX_TRIS = 5;
constexpr int64_t MC_MAX_POINTS = (int64_t)1 << 28;      // int32 offsets: <= 3 vertices and <= 5 triangles per point

// corner c of a cell at offset (c in {1,2,5,6}, c in {2,3,6,7}, c >= 4); edge e between corners (a, b)
__constant__ uint8_t c_edge_owner[12][4] = {      // (dx, dy, dz, axis) of each edge's lower end
    {0, 0, 0, 0}, {1, 0, 0, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}, {1, 0, 1, 1},
    {0, 1, 1, 0}, {0, 0, 1, 1}, {0, 0, 0, 2}, {1, 0, 0, 2}, {1, 1, 0, 2}, {0, 1, 0, 2}};
__constant__ uint8_t c_tri_count[256] = {
    0, 1, 1, 2, 1, 2, 2, 3, 1, 2, 2, 3, 2, 3, 3, 2, 1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 2, 3, 4, 4, 3, 3, 4, 4, 3, 4, 5, 5, 2,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 4, 5, 5, 4,
    2, 3, 3, 4, 3, 4, 2, 3, 3, 4, 4, 5, 4, 5, 3, 2, 3, 4, 4, 3, 4, 5, 3, 2, 4, 5, 5, 4, 5, 2, 4, 1,
    1, 2, 2, 3, 2, 3, 3, 4, 2, 3, 3, 4, 3, 4, 4, 3, 2, 3, 3, 4, 3, 4, 4, 5, 3, 2, 4, 3, 4, 3, 5, 2,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 4, 5, 5, 4, 3, 4, 4, 3, 4, 5, 5, 4, 4, 3, 5, 2, 5, 4, 2, 1,
    2, 3, 3, 4, 3, 4, 4, 5, 3, 4, 4, 5, 2, 3, 3, 2, 3, 4, 4, 5, 4, 5, 5, 2, 4, 3, 5, 4, 3, 2, 4, 1,
    3, 4, 4, 5, 4, 5, 3, 4, 4, 5, 5, 2, 3, 4, 2, 1, 2, 3, 3, 2, 3, 4, 2, 1, 3, 2, 4, 1, 2, 1, 1, 0,
};
// triangle c of case k: edges c_tri_table[k][3c .. 3c + 2], -1 past the case's last triangle
__constant__ int8_t c_tri_table[256][3 * MC_MAX_TRIS] = {
    {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 9, 8, 1, 8, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 1, 2, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 2, 10, 0, 10, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {2, 10, 9, 2, 9, 8, 2, 8, 3, -1, -1, -1, -1, -1, -1},
    {2, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 11, 0, 11, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 2, 3, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 9, 8, 1, 8, 11, 1, 11, 2, -1, -1, -1, -1, -1, -1},
    {1, 3, 11, 1, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 11, 0, 11, 10, 0, 10, 1, -1, -1, -1, -1, -1, -1}, {0, 3, 11, 0, 11, 10, 0, 10, 9, -1, -1, -1, -1, -1, -1}, {8, 11, 10, 8, 10, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 4, 7, 0, 7, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 9, 4, 1, 4, 7, 1, 7, 3, -1, -1, -1, -1, -1, -1},
    {1, 2, 10, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 4, 7, 0, 7, 3, 1, 2, 10, -1, -1, -1, -1, -1, -1}, {0, 2, 10, 0, 10, 9, 4, 7, 8, -1, -1, -1, -1, -1, -1}, {2, 10, 9, 2, 9, 4, 2, 4, 7, 2, 7, 3, -1, -1, -1},
    {2, 3, 11, 4, 7, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 4, 7, 0, 7, 11, 0, 11, 2, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 2, 3, 11, 4, 7, 8, -1, -1, -1, -1, -1, -1}, {1, 9, 4, 1, 4, 7, 1, 7, 11, 1, 11, 2, -1, -1, -1},
    {1, 3, 11, 1, 11, 10, 4, 7, 8, -1, -1, -1, -1, -1, -1}, {0, 4, 7, 0, 7, 11, 0, 11, 10, 0, 10, 1, -1, -1, -1}, {0, 3, 11, 0, 11, 10, 0, 10, 9, 4, 7, 8, -1, -1, -1}, {4, 7, 11, 4, 11, 10, 4, 10, 9, -1, -1, -1, -1, -1, -1},
    {4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 5, 0, 5, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 5, 4, 1, 4, 8, 1, 8, 3, -1, -1, -1, -1, -1, -1},
    {1, 2, 10, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 1, 2, 10, 4, 9, 5, -1, -1, -1, -1, -1, -1}, {0, 2, 10, 0, 10, 5, 0, 5, 4, -1, -1, -1, -1, -1, -1}, {2, 10, 5, 2, 5, 4, 2, 4, 8, 2, 8, 3, -1, -1, -1},
    {2, 3, 11, 4, 9, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 11, 0, 11, 2, 4, 9, 5, -1, -1, -1, -1, -1, -1}, {0, 1, 5, 0, 5, 4, 2, 3, 11, -1, -1, -1, -1, -1, -1}, {1, 5, 4, 1, 4, 8, 1, 8, 11, 1, 11, 2, -1, -1, -1},
    {1, 3, 11, 1, 11, 10, 4, 9, 5, -1, -1, -1, -1, -1, -1}, {0, 8, 11, 0, 11, 10, 0, 10, 1, 4, 9, 5, -1, -1, -1}, {0, 3, 11, 0, 11, 10, 0, 10, 5, 0, 5, 4, -1, -1, -1}, {4, 8, 11, 4, 11, 10, 4, 10, 5, -1, -1, -1, -1, -1, -1},
    {5, 7, 8, 5, 8, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 9, 5, 0, 5, 7, 0, 7, 3, -1, -1, -1, -1, -1, -1}, {0, 1, 5, 0, 5, 7, 0, 7, 8, -1, -1, -1, -1, -1, -1}, {1, 5, 7, 1, 7, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 10, 5, 7, 8, 5, 8, 9, -1, -1, -1, -1, -1, -1}, {0, 9, 5, 0, 5, 7, 0, 7, 3, 1, 2, 10, -1, -1, -1}, {0, 2, 10, 0, 10, 5, 0, 5, 7, 0, 7, 8, -1, -1, -1}, {2, 10, 5, 2, 5, 7, 2, 7, 3, -1, -1, -1, -1, -1, -1},
    {2, 3, 11, 5, 7, 8, 5, 8, 9, -1, -1, -1, -1, -1, -1}, {0, 9, 5, 0, 5, 7, 0, 7, 11, 0, 11, 2, -1, -1, -1}, {0, 1, 5, 0, 5, 7, 0, 7, 8, 2, 3, 11, -1, -1, -1}, {1, 5, 7, 1, 7, 11, 1, 11, 2, -1, -1, -1, -1, -1, -1},
    {1, 3, 11, 1, 11, 10, 5, 7, 8, 5, 8, 9, -1, -1, -1}, {0, 9, 5, 0, 5, 7, 0, 7, 11, 0, 11, 10, 0, 10, 1}, {0, 3, 11, 0, 11, 10, 0, 10, 5, 0, 5, 7, 0, 7, 8}, {5, 7, 11, 5, 11, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 9, 8, 1, 8, 3, 5, 10, 6, -1, -1, -1, -1, -1, -1},
    {1, 2, 6, 1, 6, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 1, 2, 6, 1, 6, 5, -1, -1, -1, -1, -1, -1}, {0, 2, 6, 0, 6, 5, 0, 5, 9, -1, -1, -1, -1, -1, -1}, {2, 6, 5, 2, 5, 9, 2, 9, 8, 2, 8, 3, -1, -1, -1},
    {2, 3, 11, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 11, 0, 11, 2, 5, 10, 6, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 2, 3, 11, 5, 10, 6, -1, -1, -1, -1, -1, -1}, {1, 9, 8, 1, 8, 11, 1, 11, 2, 5, 10, 6, -1, -1, -1},
    {1, 3, 11, 1, 11, 6, 1, 6, 5, -1, -1, -1, -1, -1, -1}, {0, 8, 11, 0, 11, 6, 0, 6, 5, 0, 5, 1, -1, -1, -1}, {0, 3, 11, 0, 11, 6, 0, 6, 5, 0, 5, 9, -1, -1, -1}, {5, 9, 8, 5, 8, 11, 5, 11, 6, -1, -1, -1, -1, -1, -1},
    {4, 7, 8, 5, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 4, 7, 0, 7, 3, 5, 10, 6, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 4, 7, 8, 5, 10, 6, -1, -1, -1, -1, -1, -1}, {1, 9, 4, 1, 4, 7, 1, 7, 3, 5, 10, 6, -1, -1, -1},
    {1, 2, 6, 1, 6, 5, 4, 7, 8, -1, -1, -1, -1, -1, -1}, {0, 4, 7, 0, 7, 3, 1, 2, 6, 1, 6, 5, -1, -1, -1}, {0, 2, 6, 0, 6, 5, 0, 5, 9, 4, 7, 8, -1, -1, -1}, {2, 6, 5, 2, 5, 9, 2, 9, 4, 2, 4, 7, 2, 7, 3},
    {2, 3, 11, 4, 7, 8, 5, 10, 6, -1, -1, -1, -1, -1, -1}, {0, 4, 7, 0, 7, 11, 0, 11, 2, 5, 10, 6, -1, -1, -1}, {0, 1, 9, 2, 3, 11, 4, 7, 8, 5, 10, 6, -1, -1, -1}, {1, 9, 4, 1, 4, 7, 1, 7, 11, 1, 11, 2, 5, 10, 6},
    {1, 3, 11, 1, 11, 6, 1, 6, 5, 4, 7, 8, -1, -1, -1}, {0, 4, 7, 0, 7, 11, 0, 11, 6, 0, 6, 5, 0, 5, 1}, {0, 3, 11, 0, 11, 6, 0, 6, 5, 0, 5, 9, 4, 7, 8}, {4, 7, 11, 4, 11, 6, 4, 6, 5, 4, 5, 9, -1, -1, -1},
    {4, 9, 10, 4, 10, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 4, 9, 10, 4, 10, 6, -1, -1, -1, -1, -1, -1}, {0, 1, 10, 0, 10, 6, 0, 6, 4, -1, -1, -1, -1, -1, -1}, {1, 10, 6, 1, 6, 4, 1, 4, 8, 1, 8, 3, -1, -1, -1},
    {1, 2, 6, 1, 6, 4, 1, 4, 9, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 1, 2, 6, 1, 6, 4, 1, 4, 9, -1, -1, -1}, {0, 2, 6, 0, 6, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {2, 6, 4, 2, 4, 8, 2, 8, 3, -1, -1, -1, -1, -1, -1},
    {2, 3, 11, 4, 9, 10, 4, 10, 6, -1, -1, -1, -1, -1, -1}, {0, 8, 11, 0, 11, 2, 4, 9, 10, 4, 10, 6, -1, -1, -1}, {0, 1, 10, 0, 10, 6, 0, 6, 4, 2, 3, 11, -1, -1, -1}, {1, 10, 6, 1, 6, 4, 1, 4, 8, 1, 8, 11, 1, 11, 2},
    {1, 3, 11, 1, 11, 6, 1, 6, 4, 1, 4, 9, -1, -1, -1}, {0, 8, 11, 0, 11, 6, 0, 6, 4, 0, 4, 9, 0, 9, 1}, {0, 3, 11, 0, 11, 6, 0, 6, 4, -1, -1, -1, -1, -1, -1}, {4, 8, 11, 4, 11, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {6, 7, 8, 6, 8, 9, 6, 9, 10, -1, -1, -1, -1, -1, -1}, {0, 9, 10, 0, 10, 6, 0, 6, 7, 0, 7, 3, -1, -1, -1}, {0, 1, 10, 0, 10, 6, 0, 6, 7, 0, 7, 8, -1, -1, -1}, {1, 10, 6, 1, 6, 7, 1, 7, 3, -1, -1, -1, -1, -1, -1},
    {1, 2, 6, 1, 6, 7, 1, 7, 8, 1, 8, 9, -1, -1, -1}, {0, 9, 1, 0, 1, 2, 0, 2, 6, 0, 6, 7, 0, 7, 3}, {0, 2, 6, 0, 6, 7, 0, 7, 8, -1, -1, -1, -1, -1, -1}, {2, 6, 7, 2, 7, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 11, 6, 7, 8, 6, 8, 9, 6, 9, 10, -1, -1, -1}, {0, 9, 10, 0, 10, 6, 0, 6, 7, 0, 7, 11, 0, 11, 2}, {0, 1, 10, 0, 10, 6, 0, 6, 7, 0, 7, 8, 2, 3, 11}, {1, 10, 6, 1, 6, 7, 1, 7, 11, 1, 11, 2, -1, -1, -1},
    {1, 3, 11, 1, 11, 6, 1, 6, 7, 1, 7, 8, 1, 8, 9}, {0, 9, 1, 6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 3, 11, 0, 11, 6, 0, 6, 7, 0, 7, 8, -1, -1, -1}, {6, 7, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {1, 9, 8, 1, 8, 3, 6, 11, 7, -1, -1, -1, -1, -1, -1},
    {1, 2, 10, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 1, 2, 10, 6, 11, 7, -1, -1, -1, -1, -1, -1}, {0, 2, 10, 0, 10, 9, 6, 11, 7, -1, -1, -1, -1, -1, -1}, {2, 10, 9, 2, 9, 8, 2, 8, 3, 6, 11, 7, -1, -1, -1},
    {2, 3, 7, 2, 7, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 7, 0, 7, 6, 0, 6, 2, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 2, 3, 7, 2, 7, 6, -1, -1, -1, -1, -1, -1}, {1, 9, 8, 1, 8, 7, 1, 7, 6, 1, 6, 2, -1, -1, -1},
    {1, 3, 7, 1, 7, 6, 1, 6, 10, -1, -1, -1, -1, -1, -1}, {0, 8, 7, 0, 7, 6, 0, 6, 10, 0, 10, 1, -1, -1, -1}, {0, 3, 7, 0, 7, 6, 0, 6, 10, 0, 10, 9, -1, -1, -1}, {6, 10, 9, 6, 9, 8, 6, 8, 7, -1, -1, -1, -1, -1, -1},
    {4, 6, 11, 4, 11, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 4, 6, 0, 6, 11, 0, 11, 3, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 4, 6, 11, 4, 11, 8, -1, -1, -1, -1, -1, -1}, {1, 9, 4, 1, 4, 6, 1, 6, 11, 1, 11, 3, -1, -1, -1},
    {1, 2, 10, 4, 6, 11, 4, 11, 8, -1, -1, -1, -1, -1, -1}, {0, 4, 6, 0, 6, 11, 0, 11, 3, 1, 2, 10, -1, -1, -1}, {0, 2, 10, 0, 10, 9, 4, 6, 11, 4, 11, 8, -1, -1, -1}, {2, 10, 9, 2, 9, 4, 2, 4, 6, 2, 6, 11, 2, 11, 3},
    {2, 3, 8, 2, 8, 4, 2, 4, 6, -1, -1, -1, -1, -1, -1}, {0, 4, 6, 0, 6, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 2, 3, 8, 2, 8, 4, 2, 4, 6, -1, -1, -1}, {1, 9, 4, 1, 4, 6, 1, 6, 2, -1, -1, -1, -1, -1, -1},
    {1, 3, 8, 1, 8, 4, 1, 4, 6, 1, 6, 10, -1, -1, -1}, {0, 4, 6, 0, 6, 10, 0, 10, 1, -1, -1, -1, -1, -1, -1}, {0, 3, 8, 0, 8, 4, 0, 4, 6, 0, 6, 10, 0, 10, 9}, {4, 6, 10, 4, 10, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 9, 5, 6, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 4, 9, 5, 6, 11, 7, -1, -1, -1, -1, -1, -1}, {0, 1, 5, 0, 5, 4, 6, 11, 7, -1, -1, -1, -1, -1, -1}, {1, 5, 4, 1, 4, 8, 1, 8, 3, 6, 11, 7, -1, -1, -1},
    {1, 2, 10, 4, 9, 5, 6, 11, 7, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 1, 2, 10, 4, 9, 5, 6, 11, 7, -1, -1, -1}, {0, 2, 10, 0, 10, 5, 0, 5, 4, 6, 11, 7, -1, -1, -1}, {2, 10, 5, 2, 5, 4, 2, 4, 8, 2, 8, 3, 6, 11, 7},
    {2, 3, 7, 2, 7, 6, 4, 9, 5, -1, -1, -1, -1, -1, -1}, {0, 8, 7, 0, 7, 6, 0, 6, 2, 4, 9, 5, -1, -1, -1}, {0, 1, 5, 0, 5, 4, 2, 3, 7, 2, 7, 6, -1, -1, -1}, {1, 5, 4, 1, 4, 8, 1, 8, 7, 1, 7, 6, 1, 6, 2},
    {1, 3, 7, 1, 7, 6, 1, 6, 10, 4, 9, 5, -1, -1, -1}, {0, 8, 7, 0, 7, 6, 0, 6, 10, 0, 10, 1, 4, 9, 5}, {0, 3, 7, 0, 7, 6, 0, 6, 10, 0, 10, 5, 0, 5, 4}, {4, 8, 7, 4, 7, 6, 4, 6, 10, 4, 10, 5, -1, -1, -1},
    {5, 6, 11, 5, 11, 8, 5, 8, 9, -1, -1, -1, -1, -1, -1}, {0, 9, 5, 0, 5, 6, 0, 6, 11, 0, 11, 3, -1, -1, -1}, {0, 1, 5, 0, 5, 6, 0, 6, 11, 0, 11, 8, -1, -1, -1}, {1, 5, 6, 1, 6, 11, 1, 11, 3, -1, -1, -1, -1, -1, -1},
    {1, 2, 10, 5, 6, 11, 5, 11, 8, 5, 8, 9, -1, -1, -1}, {0, 9, 5, 0, 5, 6, 0, 6, 11, 0, 11, 3, 1, 2, 10}, {0, 2, 10, 0, 10, 5, 0, 5, 6, 0, 6, 11, 0, 11, 8}, {2, 10, 5, 2, 5, 6, 2, 6, 11, 2, 11, 3, -1, -1, -1},
    {2, 3, 8, 2, 8, 9, 2, 9, 5, 2, 5, 6, -1, -1, -1}, {0, 9, 5, 0, 5, 6, 0, 6, 2, -1, -1, -1, -1, -1, -1}, {0, 1, 5, 0, 5, 6, 0, 6, 2, 0, 2, 3, 0, 3, 8}, {1, 5, 6, 1, 6, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 8, 1, 8, 9, 1, 9, 5, 1, 5, 6, 1, 6, 10}, {0, 9, 5, 0, 5, 6, 0, 6, 10, 0, 10, 1, -1, -1, -1}, {0, 3, 8, 5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {5, 6, 10, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {5, 10, 11, 5, 11, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 5, 10, 11, 5, 11, 7, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 5, 10, 11, 5, 11, 7, -1, -1, -1, -1, -1, -1}, {1, 9, 8, 1, 8, 3, 5, 10, 11, 5, 11, 7, -1, -1, -1},
    {1, 2, 11, 1, 11, 7, 1, 7, 5, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 1, 2, 11, 1, 11, 7, 1, 7, 5, -1, -1, -1}, {0, 2, 11, 0, 11, 7, 0, 7, 5, 0, 5, 9, -1, -1, -1}, {2, 11, 7, 2, 7, 5, 2, 5, 9, 2, 9, 8, 2, 8, 3},
    {2, 3, 7, 2, 7, 5, 2, 5, 10, -1, -1, -1, -1, -1, -1}, {0, 8, 7, 0, 7, 5, 0, 5, 10, 0, 10, 2, -1, -1, -1}, {0, 1, 9, 2, 3, 7, 2, 7, 5, 2, 5, 10, -1, -1, -1}, {1, 9, 8, 1, 8, 7, 1, 7, 5, 1, 5, 10, 1, 10, 2},
    {1, 3, 7, 1, 7, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 8, 7, 0, 7, 5, 0, 5, 1, -1, -1, -1, -1, -1, -1}, {0, 3, 7, 0, 7, 5, 0, 5, 9, -1, -1, -1, -1, -1, -1}, {5, 9, 8, 5, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 5, 10, 4, 10, 11, 4, 11, 8, -1, -1, -1, -1, -1, -1}, {0, 4, 5, 0, 5, 10, 0, 10, 11, 0, 11, 3, -1, -1, -1}, {0, 1, 9, 4, 5, 10, 4, 10, 11, 4, 11, 8, -1, -1, -1}, {1, 9, 4, 1, 4, 5, 1, 5, 10, 1, 10, 11, 1, 11, 3},
    {1, 2, 11, 1, 11, 8, 1, 8, 4, 1, 4, 5, -1, -1, -1}, {0, 4, 5, 0, 5, 1, 0, 1, 2, 0, 2, 11, 0, 11, 3}, {0, 2, 11, 0, 11, 8, 0, 8, 4, 0, 4, 5, 0, 5, 9}, {2, 11, 3, 4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 8, 2, 8, 4, 2, 4, 5, 2, 5, 10, -1, -1, -1}, {0, 4, 5, 0, 5, 10, 0, 10, 2, -1, -1, -1, -1, -1, -1}, {0, 1, 9, 2, 3, 8, 2, 8, 4, 2, 4, 5, 2, 5, 10}, {1, 9, 4, 1, 4, 5, 1, 5, 10, 1, 10, 2, -1, -1, -1},
    {1, 3, 8, 1, 8, 4, 1, 4, 5, -1, -1, -1, -1, -1, -1}, {0, 4, 5, 0, 5, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 3, 8, 0, 8, 4, 0, 4, 5, 0, 5, 9, -1, -1, -1}, {4, 5, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {4, 9, 10, 4, 10, 11, 4, 11, 7, -1, -1, -1, -1, -1, -1}, {0, 8, 3, 4, 9, 10, 4, 10, 11, 4, 11, 7, -1, -1, -1}, {0, 1, 10, 0, 10, 11, 0, 11, 7, 0, 7, 4, -1, -1, -1}, {1, 10, 11, 1, 11, 7, 1, 7, 4, 1, 4, 8, 1, 8, 3},
    {1, 2, 11, 1, 11, 7, 1, 7, 4, 1, 4, 9, -1, -1, -1}, {0, 8, 3, 1, 2, 11, 1, 11, 7, 1, 7, 4, 1, 4, 9}, {0, 2, 11, 0, 11, 7, 0, 7, 4, -1, -1, -1, -1, -1, -1}, {2, 11, 7, 2, 7, 4, 2, 4, 8, 2, 8, 3, -1, -1, -1},
    {2, 3, 7, 2, 7, 4, 2, 4, 9, 2, 9, 10, -1, -1, -1}, {0, 8, 7, 0, 7, 4, 0, 4, 9, 0, 9, 10, 0, 10, 2}, {0, 1, 10, 0, 10, 2, 0, 2, 3, 0, 3, 7, 0, 7, 4}, {1, 10, 2, 4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 7, 1, 7, 4, 1, 4, 9, -1, -1, -1, -1, -1, -1}, {0, 8, 7, 0, 7, 4, 0, 4, 9, 0, 9, 1, -1, -1, -1}, {0, 3, 7, 0, 7, 4, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {4, 8, 7, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {8, 9, 10, 8, 10, 11, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 9, 10, 0, 10, 11, 0, 11, 3, -1, -1, -1, -1, -1, -1}, {0, 1, 10, 0, 10, 11, 0, 11, 8, -1, -1, -1, -1, -1, -1}, {1, 10, 11, 1, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 2, 11, 1, 11, 8, 1, 8, 9, -1, -1, -1, -1, -1, -1}, {0, 9, 1, 0, 1, 2, 0, 2, 11, 0, 11, 3, -1, -1, -1}, {0, 2, 11, 0, 11, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {2, 11, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {2, 3, 8, 2, 8, 9, 2, 9, 10, -1, -1, -1, -1, -1, -1}, {0, 9, 10, 0, 10, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 1, 10, 0, 10, 2, 0, 2, 3, 0, 3, 8, -1, -1, -1}, {1, 10, 2, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
    {1, 3, 8, 1, 8, 9, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 9, 1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {0, 3, 8, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1},
};

struct Grid {
    int nx, ny, nz;
    long p;               // nx * ny * nz
    float iso;
};

__device__ __forceinline__ bool below(const float* __restrict__ cube, long i, float iso) { return cube[i] < iso; }

// crossed edges of point (x, y, z) along +x, +y, +z: bits 0, 1, 2
__device__ __forceinline__ unsigned point_flags(const float* __restrict__ cube, const Grid& g, int x, int y, int z, long i) {
    const bool b = below(cube, i, g.iso);
    unsigned f = 0u;
    if (x + 1 < g.nx && below(cube, i + (long)g.ny * g.nz, g.iso) != b) f |= 1u;
    if (y + 1 < g.ny && below(cube, i + g.nz, g.iso) != b) f |= 2u;
    if (z + 1 < g.nz && below(cube, i + 1, g.iso) != b) f |= 4u;
    return f;
}

// case index of the cell whose lowest corner is (x, y, z) (the caller checks that it is one); bit c: corner c below iso
__device__ __forceinline__ unsigned cell_case(const float* __restrict__ cube, const Grid& g, long i) {
    const long sx = (long)g.ny * g.nz, sy = g.nz;
    const long off[8] = {0, sx, sx + sy, sy, 1, sx + 1, sx + sy + 1, sy + 1};
    unsigned k = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) k |= below(cube, i + off[c], g.iso) ? 1u << c : 0u;
    return k;
}

__device__ __forceinline__ void coords_of(const Grid& g, long i, int& x, int& y, int& z) {
    z = (int)(i % g.nz);
    const long r = i / g.nz;
    y = (int)(r % g.ny);
    x = (int)(r / g.ny);
}

// Pass 1: counts and the workgroup-local exclusive scan.  loc[2 i] / loc[2 i + 1] = vertices / triangles before point i inside its
// block of MC_BLOCK points; bsum[2 b], bsum[2 b + 1] = the block's totals.
__global__ void __launch_bounds__(MC_THREADS) mc_count_kernel(const float* __restrict__ cube, const Grid g, int* __restrict__ loc,
                                                              int* __restrict__ bsum) {
    __shared__ int s_v[MC_THREADS], s_t[MC_THREADS];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * MC_BLOCK + (long)t * MC_PER_THREAD;
    int nv[MC_PER_THREAD], nt[MC_PER_THREAD];
    int sv = 0, st = 0;
#pragma unroll
    for (int j = 0; j < MC_PER_THREAD; ++j) {
        const long i = base + j;
        nv[j] = 0; nt[j] = 0;
        if (i < g.p) {
            int x, y, z;
            coords_of(g, i, x, y, z);
            nv[j] = __popc(point_flags(cube, g, x, y, z, i));
            if (x + 1 < g.nx && y + 1 < g.ny && z + 1 < g.nz) nt[j] = c_tri_count[cell_case(cube, g, i)];
        }
        sv += nv[j]; st += nt[j];
    }
    s_v[t] = sv; s_t[t] = st;
    __syncthreads();
    for (int d = 1; d < MC_THREADS; d <<= 1) {            // inclusive Hillis-Steele scan of the thread totals
        const int av = t >= d ? s_v[t - d] : 0, at = t >= d ? s_t[t - d] : 0;
        __syncthreads();
        s_v[t] += av; s_t[t] += at;
        __syncthreads();
    }
    int ov = s_v[t] - sv, ot = s_t[t] - st;
#pragma unroll
    for (int j = 0; j < MC_PER_THREAD; ++j) {
        const long i = base + j;
        if (i < g.p) { loc[2 * i] = ov; loc[2 * i + 1] = ot; }
        ov += nv[j]; ot += nt[j];
    }
    if (t == MC_THREADS - 1) { bsum[2 * blockIdx.x] = s_v[t]; bsum[2 * blockIdx.x + 1] = s_t[t]; }
}

// One workgroup: boff[2 b], boff[2 b + 1] = exclusive prefix of the block totals; counts[0], counts[1] = the grand totals.
__global__ void __launch_bounds__(1024) mc_scan_blocks_kernel(const int* __restrict__ bsum, const int nb, int* __restrict__ boff,
                                                              int64_t* __restrict__ counts) {
    __shared__ int s_v[1024], s_t[1024];
    const int t = threadIdx.x;
    int cv = 0, ct = 0;                                   // carry of the chunks before
    for (int c0 = 0; c0 < nb; c0 += 1024) {
        const int b = c0 + t;
        const int v = b < nb ? bsum[2 * b] : 0, w = b < nb ? bsum[2 * b + 1] : 0;
        s_v[t] = v; s_t[t] = w;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int av = t >= d ? s_v[t - d] : 0, at = t >= d ? s_t[t - d] : 0;
            __syncthreads();
            s_v[t] += av; s_t[t] += at;
            __syncthreads();
        }
        if (b < nb) { boff[2 * b] = cv + s_v[t] - v; boff[2 * b + 1] = ct + s_t[t] - w; }
        cv += s_v[1023]; ct += s_t[1023];
        __syncthreads();
    }
    if (t == 0) { counts[0] = cv; counts[1] = ct; }
}

__device__ __forceinline__ int vertex_base(const int* __restrict__ loc, const int* __restrict__ boff, long i) {
    return loc[2 * i] + boff[2 * (i / MC_BLOCK)];
}

// Pass 2: one thread per lattice point.
__global__ void __launch_bounds__(256) mc_emit_kernel(const float* __restrict__ cube, const Grid g, const int* __restrict__ loc,
                                                      const int* __restrict__ boff, const long max_v, const long max_t,
                                                      float* __restrict__ verts, int32_t* __restrict__ faces) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.p) return;
    int x, y, z;
    coords_of(g, i, x, y, z);
    const unsigned fl = point_flags(cube, g, x, y, z, i);
    if (fl) {
        const long step[3] = {(long)g.ny * g.nz, (long)g.nz, 1};
        const float f0 = cube[i];
        long v = vertex_base(loc, boff, i);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(fl & (1u << a))) continue;
            const float f1 = cube[i + step[a]];
            const float tt = (g.iso - f0) / (f1 - f0);
            float p[3] = {(float)x, (float)y, (float)z};
            p[a] = p[a] + tt;
            if (v < max_v) { verts[3 * v] = p[0]; verts[3 * v + 1] = p[1]; verts[3 * v + 2] = p[2]; }
            ++v;
        }
    }
    if (x + 1 < g.nx && y + 1 < g.ny && z + 1 < g.nz) {
        const unsigned k = cell_case(cube, g, i);
        const int n = c_tri_count[k];
        if (n == 0) return;
        long tri = (long)loc[2 * i + 1] + boff[2 * (i / MC_BLOCK) + 1];
        for (int c = 0; c < n; ++c, ++tri) {
            int idx[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int e = c_tri_table[k][3 * c + r];
                const int ox = x + c_edge_owner[e][0], oy = y + c_edge_owner[e][1], oz = z + c_edge_owner[e][2], a = c_edge_owner[e][3];
                const long o = ((long)ox * g.ny + oy) * g.nz + oz;
                const unsigned ofl = point_flags(cube, g, ox, oy, oz, o);
                idx[r] = vertex_base(loc, boff, o) + __popc(ofl & ((1u << a) - 1u));
            }
            if (tri < max_t) { faces[3 * tri] = idx[0]; faces[3 * tri + 1] = idx[1]; faces[3 * tri + 2] = idx[2]; }
        }
    }
}

// ---- gpnerf_cube_clean: connected components of the cube's points by a block-based union-find ----------------------------------
// One templated kernel set serves both passes: <9 lower neighbours, inside> labels the solid under 18-connectivity, <3, below> the
// outside under 6-connectivity.  Per pass:
//   1. cc_local_kernel: a workgroup labels one brick of 4 x 8 x 32 points (z fastest: a wavefront reads two whole 128-B lines) in
//      LDS and leaves parent[i] = the lowest point of i's component INSIDE the brick (-1 off the set) and, at those brick roots only,
//      the component's size in the brick (and whether it touches a boundary face of the cube).  A uniform brick -- most of the padding
//      and of the exterior -- skips the unions: one root, one count.
//   2. cc_merge_kernel: unions across brick faces only, on the global parent array.
//   3. cc_flatten_kernel: every point's parent becomes its set's root; every brick root adds its count to that root's.
// The cost per point does not grow with the size or the diameter of its component: a find walks brick roots, not points, and the
// merge compresses the paths it walks.
// Within a brick the local order (x, y, z lexicographic) is the order of the linear indices, so "lowest local index" is "lowest point".
constexpr int BX = 4, BY = 8, BZ = 32, BRICK = BX * BY * BZ, CC_THREADS = BY * BZ;     // a thread owns one (y, z) column of BX points
constexpr unsigned CC_BOUNDARY = 0x80000000u, CC_COUNT = 0x1fffffffu;                   // count word: size (<= 2^28) | boundary bit
__device__ constexpr int8_t c_lower[9][3] = {      // the neighbours of lower linear index; the first 3 are the 6-connected ones
    {-1, 0, 0}, {0, -1, 0}, {0, 0, -1}, {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1}, {-1, 0, 1}, {0, -1, -1}, {0, -1, 1}};

struct Bricks { int nbx, nby, nbz; };
__host__ __device__ inline Bricks bricks_of(const Grid& g) { return {(g.nx + BX - 1) / BX, (g.ny + BY - 1) / BY, (g.nz + BZ - 1) / BZ}; }
__device__ __forceinline__ void brick_origin(const Grid& g, int& x0, int& y0, int& z0) {
    const Bricks b = bricks_of(g);
    const int id = blockIdx.x;
    z0 = (id % b.nbz) * BZ;
    y0 = ((id / b.nbz) % b.nby) * BY;
    x0 = (id / (b.nbz * b.nby)) * BX;
}
template <bool INSIDE> __device__ __forceinline__ bool in_set(float v, float iso) { return INSIDE ? !(v < iso) : (v < iso); }

__device__ __forceinline__ int lds_find(const int* s, int i) {
    int p = s[i];
    while (p != i) { i = p; p = s[i]; }
    return i;
}
// LDS atomicMin union: the larger root is linked below the smaller; a lost race retries from what the word held
__device__ __forceinline__ void lds_union(int* s, int a, int b) {
    while (true) {
        a = lds_find(s, a); b = lds_find(s, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&s[a], b);
        if (old == a) return;
        a = old;
    }
}

template <int NLOWER, bool INSIDE>
__global__ void __launch_bounds__(CC_THREADS) cc_local_kernel(const float* __restrict__ cube, const Grid g, int* __restrict__ parent,
                                                              unsigned* __restrict__ count, unsigned long long* __restrict__ best,
                                                              int64_t* __restrict__ stats) {
    __shared__ int s_par[BRICK];
    __shared__ unsigned s_cnt[BRICK];
    if (stats && blockIdx.x == 0 && threadIdx.x < 6) stats[threadIdx.x] = 0;
    if (best && blockIdx.x == 0 && threadIdx.x == 0) *best = 0ull;
    int x0, y0, z0;
    brick_origin(g, x0, y0, z0);
    const int t = threadIdx.x, lz = t % BZ, ly = t / BZ;
    const int y = y0 + ly, z = z0 + lz;
    const bool col = y < g.ny && z < g.nz;
    bool in[BX], bnd[BX];
    bool all = true, any = false, anyb = false;
#pragma unroll
    for (int lx = 0; lx < BX; ++lx) {
        const int x = x0 + lx;
        const bool ok = col && x < g.nx;
        in[lx] = ok && in_set<INSIDE>(cube[((long)x * g.ny + y) * g.nz + z], g.iso);
        bnd[lx] = in[lx] && (x == 0 || y == 0 || z == 0 || x == g.nx - 1 || y == g.ny - 1 || z == g.nz - 1);
        all = all && (in[lx] || !ok);
        any = any || in[lx];
        anyb = anyb || bnd[lx];
    }
    const int uniform_in = __syncthreads_and(all), some = __syncthreads_or(any);
    if (uniform_in || !some) {
        // one node: the brick's first point (always in the cube) is the root of all its in-cube points, or nothing is in the set
        const int touches = __syncthreads_or(anyb);
        const int ex = min(BX, g.nx - x0), ey = min(BY, g.ny - y0), ez = min(BZ, g.nz - z0);
        const long root = ((long)x0 * g.ny + y0) * g.nz + z0;
#pragma unroll
        for (int lx = 0; lx < BX; ++lx) {
            if (!(col && x0 + lx < g.nx)) continue;
            const long i = ((long)(x0 + lx) * g.ny + y) * g.nz + z;
            parent[i] = some ? (int)root : -1;
            count[i] = (some && i == root) ? (unsigned)(ex * ey * ez) | (touches ? CC_BOUNDARY : 0u) : 0u;
        }
        return;
    }
#pragma unroll
    for (int lx = 0; lx < BX; ++lx) {
        const int l = lx * CC_THREADS + t;               // (lx * BY + ly) * BZ + lz
        s_par[l] = in[lx] ? l : -1;
        s_cnt[l] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int lx = 0; lx < BX; ++lx) {
        if (!in[lx]) continue;
        const int l = lx * CC_THREADS + t;
#pragma unroll
        for (int k = 0; k < NLOWER; ++k) {
            const int qx = lx + c_lower[k][0], qy = ly + c_lower[k][1], qz = lz + c_lower[k][2];
            if (qx < 0 || qy < 0 || qy >= BY || qz < 0 || qz >= BZ) continue;      // another brick's: cc_merge_kernel
            const int q = (qx * BY + qy) * BZ + qz;
            if (s_par[q] >= 0) lds_union(s_par, l, q);       // (-1 never changes; a point off the cube is -1)
        }
    }
    __syncthreads();
    int root[BX];
#pragma unroll
    for (int lx = 0; lx < BX; ++lx) root[lx] = in[lx] ? lds_find(s_par, lx * CC_THREADS + t) : -1;
#pragma unroll
    for (int lx = 0; lx < BX; ++lx) {
        if (!in[lx]) continue;
        atomicAdd(&s_cnt[root[lx]], 1u);
        if (bnd[lx]) atomicOr(&s_cnt[root[lx]], CC_BOUNDARY);
    }
    __syncthreads();
#pragma unroll
    for (int lx = 0; lx < BX; ++lx) {
        if (!(col && x0 + lx < g.nx)) continue;
        const long i = ((long)(x0 + lx) * g.ny + y) * g.nz + z;
        int r = -1;
        if (in[lx]) {
            const int rl = root[lx], rz = rl % BZ, ry = (rl / BZ) % BY, rx = rl / (BY * BZ);
            r = (int)(((long)(x0 + rx) * g.ny + y0 + ry) * g.nz + z0 + rz);
        }
        parent[i] = r;
        count[i] = s_cnt[lx * CC_THREADS + t];            // non-zero at the brick's roots only
    }
}

// The global parent array inside cc_merge_kernel: g_load / g_find / g_find_compress / g_union, every access an agent-scope atomic
// (shared with gpnerf_meshcomp.hip, which unites over a mesh's faces; the header says why no plain load will do and why no lane waits)
#include "gpnerf_unionfind.h"

template <int NLOWER>
__global__ void __launch_bounds__(CC_THREADS) cc_merge_kernel(const Grid g, int* parent) {
    int x0, y0, z0;
    brick_origin(g, x0, y0, z0);
    const int t = threadIdx.x, lz = t % BZ, ly = t / BZ, lane = t % 64;
    const int y = y0 + ly, z = z0 + lz;
    for (int lx = 0; lx < BX; ++lx) {
        const int x = x0 + lx;
        const bool ok = x < g.nx && y < g.ny && z < g.nz;
        const long i = ((long)x * g.ny + y) * g.nz + z;
#pragma unroll
        for (int k = 0; k < NLOWER; ++k) {
            const int dx = c_lower[k][0], dy = c_lower[k][1], dz = c_lower[k][2];
            // wave-uniform skip: lx is uniform, and dx alone decides for the offsets that stay inside the brick in y and z
            const int qx = lx + dx, qy = ly + dy, qz = lz + dz;
            const bool crosses = qx < 0 || qy < 0 || qy >= BY || qz < 0 || qz >= BZ;
            const int nx_ = x + dx, ny_ = y + dy, nz_ = z + dz;
            bool todo = ok && crosses && nx_ >= 0 && ny_ >= 0 && ny_ < g.ny && nz_ >= 0 && nz_ < g.nz;
            if (!__any(todo)) continue;
            int pa = -1, pb = -1;
            if (todo) {
                pa = g_load(parent, i);
                if (pa >= 0) pb = g_load(parent, ((long)nx_ * g.ny + ny_) * g.nz + nz_);
                todo = pa >= 0 && pb >= 0;
            }
            // the same pair of brick roots as the lane one or one row before: that lane's union is this one's too.  (An
            // optimisation only: a pair that differs just because a path was compressed meanwhile is united twice.)
            const int pa1 = __shfl_up(pa, 1), pb1 = __shfl_up(pb, 1), pa32 = __shfl_up(pa, 32), pb32 = __shfl_up(pb, 32);
            if (todo && (lane & 31) != 0 && pa1 == pa && pb1 == pb) todo = false;
            if (todo && lane >= 32 && pa32 == pa && pb32 == pb) todo = false;
            if (todo) g_union(parent, pa, pb);
        }
    }
}

// A kernel of its own, so the unions are complete and visible (kernel boundary).  Plain accesses: nothing is united here, every set's
// root is fixed, and a word is only ever replaced by that root -- a reader on another XCD that still sees the old word walks a
// longer path to the same root.  Each brick root (count != 0) that is not the set's root adds its count to the set's root: integer
// add / or on disjoint bit fields, so the order does not matter; only roots are added to and only non-roots are read.
__global__ void __launch_bounds__(256) cc_flatten_kernel(const long n, int* parent, unsigned* count) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int q = parent[i];
    if (q < 0 || q == (int)i) return;
    int r = q;
    for (int u = parent[r]; u != r; u = parent[r]) r = u;
    if (r != q) parent[i] = r;
    const unsigned c = count[i];
    if (c) {
        atomicAdd(&count[r], c & CC_COUNT);
        if (c & CC_BOUNDARY) atomicOr(&count[r], CC_BOUNDARY);
    }
}

// (not gpnerf_util.h's wave_sum: a shuffle-down reduction, whose sum arrives in the wavefront's first lane only)
__device__ __forceinline__ long wave_sum_lane0(long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    return v;
}

enum KeepMode { KEEP_ALL = 0, KEEP_MIN = 1, KEEP_LARGEST = 2 };
// Over the solid's roots: stats[0..1] (components, inside points) and what is kept -- stats[2..3] for KEEP_ALL / KEEP_MIN, the packed
// (size << 32 | ~label) maximum for KEEP_LARGEST (a total order: ties go to the lower label).  A wavefront sums before its atomics,
// and a wavefront without a root (nearly all) issues none.
__global__ void __launch_bounds__(256) cc_select_kernel(const long n, const int* __restrict__ parent, const unsigned* __restrict__ count,
                                                        const int mode, const long min_points, unsigned long long* __restrict__ best,
                                                        int64_t* __restrict__ stats) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = i < n && parent[i] == (int)i;
    if (!__any(root)) return;
    const long size = root ? (long)(count[i] & CC_COUNT) : 0;
    const bool kept = root && (mode == KEEP_ALL || (mode == KEEP_MIN && size >= min_points));
    const long roots = wave_sum_lane0(root ? 1 : 0), points = wave_sum_lane0(size), kroots = wave_sum_lane0(kept ? 1 : 0), kpoints = wave_sum_lane0(kept ? size : 0);
    unsigned long long key = root ? ((unsigned long long)size << 32) | (unsigned)~(unsigned)i : 0ull;
    if (mode == KEEP_LARGEST) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_down(key, d); key = o > key ? o : key; }
    }
    if (threadIdx.x % 64 == 0) {
        atomicAdd((unsigned long long*)&stats[0], (unsigned long long)roots);
        atomicAdd((unsigned long long*)&stats[1], (unsigned long long)points);
        if (kroots) { atomicAdd((unsigned long long*)&stats[2], (unsigned long long)kroots); atomicAdd((unsigned long long*)&stats[3], (unsigned long long)kpoints); }
        if (mode == KEEP_LARGEST) atomicMax(best, key);
    }
}

// out_cube = cube with the inside points of the components that are not kept written as 0; labels, if wanted
__global__ void __launch_bounds__(256) cc_apply_keep_kernel(const float* __restrict__ cube, const long n, const int* __restrict__ parent,
                                                            const unsigned* __restrict__ count, const int mode, const long min_points,
                                                            const unsigned long long* __restrict__ best, float* __restrict__ out,
                                                            int32_t* __restrict__ labels, int64_t* __restrict__ stats) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long b = mode == KEEP_LARGEST ? *best : 0ull;
    if (mode == KEEP_LARGEST && i == 0) { stats[2] = b ? 1 : 0; stats[3] = (int64_t)(b >> 32); }
    const int r = parent[i];
    float v = cube[i];
    if (r >= 0) {
        bool kept = true;
        if (mode == KEEP_MIN) kept = (long)(count[r] & CC_COUNT) >= min_points;
        if (mode == KEEP_LARGEST) kept = (unsigned)r == ~(unsigned)b;
        if (!kept) v = 0.0f;
    }
    out[i] = v;
    if (labels) labels[i] = r;
}

// every below-iso point of a component that touches no boundary face becomes 1; stats[4..5]
__global__ void __launch_bounds__(256) cc_apply_fill_kernel(const long n, const int* __restrict__ parent, const unsigned* __restrict__ count,
                                                            float* __restrict__ out, int64_t* __restrict__ stats) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int r = i < n ? parent[i] : -1;
    const bool fill = r >= 0 && !(count[r] & CC_BOUNDARY);
    if (!__any(fill)) return;
    if (fill) out[i] = 1.0f;
    const long cav = wave_sum_lane0(fill && r == (int)i ? 1 : 0), pts = wave_sum_lane0(fill ? 1 : 0);
    if (threadIdx.x % 64 == 0) {
        if (cav) atomicAdd((unsigned long long*)&stats[4], (unsigned long long)cav);
        atomicAdd((unsigned long long*)&stats[5], (unsigned long long)pts);
    }
}

// ---- gpnerf_mesh_normals: one lane per vertex ---------------------------------------------------------------------------------
struct Step3 { float v[3]; };
__device__ __forceinline__ float central(const float* __restrict__ cube, const Grid& g, int x, int y, int z, int a, float inv) {
    const int dim[3] = {g.nx, g.ny, g.nz};
    int hi[3] = {x, y, z}, lo[3] = {x, y, z};
    hi[a] = min(hi[a] + 1, dim[a] - 1);
    lo[a] = max(lo[a] - 1, 0);
    const float fh = cube[((long)hi[0] * g.ny + hi[1]) * g.nz + hi[2]], fl = cube[((long)lo[0] * g.ny + lo[1]) * g.nz + lo[2]];
    return ((fh - fl) * 0.5f) * inv;
}
__device__ __forceinline__ float lerp_(float a, float b, float t) { return a + t * (b - a); }

__global__ void __launch_bounds__(256) mesh_normals_kernel(const float* __restrict__ cube, const Grid g, const float* __restrict__ verts,
                                                           const long n, const Step3 inv, float* __restrict__ normals) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int dim[3] = {g.nx, g.ny, g.nz};
    int c[3];
    float t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = verts[3 * i + a];
        float f = floorf(v);
        f = fminf(fmaxf(f, 0.0f), (float)(dim[a] - 2));          // (NaN -> 0: the index stays in the cube whatever the vertex holds)
        c[a] = (int)f;
        t[a] = v - f;
    }
    float gr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float G[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) G[k] = central(cube, g, c[0] + (k >> 2), c[1] + ((k >> 1) & 1), c[2] + (k & 1), a, inv.v[a]);
        const float z00 = lerp_(G[0], G[1], t[2]), z01 = lerp_(G[2], G[3], t[2]), z10 = lerp_(G[4], G[5], t[2]), z11 = lerp_(G[6], G[7], t[2]);
        gr[a] = lerp_(lerp_(z00, z01, t[1]), lerp_(z10, z11, t[1]), t[0]);
    }
    const float len = sqrtf((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
    const bool ok = len > 0.0f && len < __builtin_inff();
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * i + a] = ok ? -gr[a] / len : 0.0f;
}

bool grid_of(const int32_t* dims, float iso, Grid& g) {
    if (!dims || dims[0] < 2 || dims[1] < 2 || dims[2] < 2 || !(iso == iso)) return false;
    const int64_t p = (int64_t)dims[0] * dims[1] * dims[2];
    if (p > MC_MAX_POINTS) return false;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2]; g.p = (long)p; g.iso = iso;
    return true;
}

struct WsLayout { size_t loc, bsum, boff, total; long nb; };
WsLayout layout_of(const Grid& g) {
    WsLayout w;
    w.nb = (g.p + MC_BLOCK - 1) / MC_BLOCK;
    w.loc = 0;
    w.bsum = align256(sizeof(int) * 2 * (size_t)g.p);
    w.boff = w.bsum + align256(sizeof(int) * 2 * (size_t)w.nb);
    w.total = w.boff + align256(sizeof(int) * 2 * (size_t)w.nb);
    return w;
}

struct CleanLayout { size_t parent, count, best, total; };
CleanLayout clean_layout_of(const Grid& g) {
    CleanLayout w;
    w.parent = 0;
    w.count = align256(sizeof(int) * (size_t)g.p);
    w.best = w.count + align256(sizeof(unsigned) * (size_t)g.p);
    w.total = w.best + 256;
    return w;
}

}  // namespace

extern "C" {

int64_t gpnerf_mesh_workspace_bytes(const int32_t* dims) {
    Grid g;
    if (!grid_of(dims, 0.f, g)) return 0;
    return (int64_t)layout_of(g).total;
}

int gpnerf_mesh_count(const float* cube, const int32_t* dims, float iso, void* workspace, size_t workspace_bytes, int64_t* counts,
                      void* stream) {
    Grid g;
    if (!cube || !workspace || !counts || !grid_of(dims, iso, g)) return GPNERF_E_ARG;
    const WsLayout w = layout_of(g);
    if (workspace_bytes < w.total) return GPNERF_E_ARG;
    char* ws = static_cast<char*>(workspace);
    int* loc = reinterpret_cast<int*>(ws + w.loc);
    int* bsum = reinterpret_cast<int*>(ws + w.bsum);
    int* boff = reinterpret_cast<int*>(ws + w.boff);
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)w.nb), dim3(MC_THREADS), 0, S_(stream), cube, g, loc, bsum);
    hipLaunchKernelGGL(mc_scan_blocks_kernel, dim3(1), dim3(1024), 0, S_(stream), bsum, (int)w.nb, boff, counts);
    return launch_status();
}

int gpnerf_mesh_emit(const float* cube, const int32_t* dims, float iso, const void* workspace, size_t workspace_bytes,
                     int64_t max_vertices, int64_t max_triangles, float* vertices, int32_t* faces, void* stream) {
    Grid g;
    if (!cube || !workspace || !grid_of(dims, iso, g) || max_vertices < 0 || max_triangles < 0) return GPNERF_E_ARG;
    if ((max_vertices > 0 && !vertices) || (max_triangles > 0 && !faces)) return GPNERF_E_ARG;
    const WsLayout w = layout_of(g);
    if (workspace_bytes < w.total) return GPNERF_E_ARG;
    const char* ws = static_cast<const char*>(workspace);
    const int* loc = reinterpret_cast<const int*>(ws + w.loc);
    const int* boff = reinterpret_cast<const int*>(ws + w.boff);
    hipLaunchKernelGGL(mc_emit_kernel, dim3((unsigned)((g.p + 255) / 256)), dim3(256), 0, S_(stream), cube, g, loc, boff,
                       (long)max_vertices, (long)max_triangles, vertices, faces);
    return launch_status();
}

int64_t gpnerf_cube_clean_workspace_bytes(const int32_t* dims) {
    Grid g;
    if (!grid_of(dims, 0.f, g)) return 0;
    return (int64_t)clean_layout_of(g).total;
}

int gpnerf_cube_clean(const float* cube, const int32_t* dims, float iso, uint32_t flags, int64_t min_points, void* workspace,
                      size_t workspace_bytes, float* out_cube, int32_t* labels, int64_t* stats, void* stream) {
    Grid g;
    if (!cube || !workspace || !out_cube || !stats || !grid_of(dims, iso, g)) return GPNERF_E_ARG;
    if ((flags & ~(GPNERF_CUBE_KEEP | GPNERF_CUBE_FILL)) || min_points < 0) return GPNERF_E_ARG;
    {   // out_cube must not alias cube (any overlap of the two arrays)
        const uintptr_t a = (uintptr_t)cube, b = (uintptr_t)out_cube, bytes = sizeof(float) * (uintptr_t)g.p;
        if (a < b + bytes && b < a + bytes) return GPNERF_E_ARG;
    }
    const CleanLayout w = clean_layout_of(g);
    if (workspace_bytes < w.total) return GPNERF_E_ARG;
    char* ws = static_cast<char*>(workspace);
    int* parent = reinterpret_cast<int*>(ws + w.parent);
    unsigned* count = reinterpret_cast<unsigned*>(ws + w.count);
    unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + w.best);
    const Bricks b = bricks_of(g);
    const dim3 bricks((unsigned)((long)b.nbx * b.nby * b.nbz)), points((unsigned)((g.p + 255) / 256));
    const int mode = !(flags & GPNERF_CUBE_KEEP) ? KEEP_ALL : min_points > 0 ? KEEP_MIN : KEEP_LARGEST;
    hipStream_t s = S_(stream);
    // the solid: 18-connectivity over the inside points of cube
    hipLaunchKernelGGL((cc_local_kernel<9, true>), bricks, dim3(CC_THREADS), 0, s, cube, g, parent, count, best, stats);
    hipLaunchKernelGGL((cc_merge_kernel<9>), bricks, dim3(CC_THREADS), 0, s, g, parent);
    hipLaunchKernelGGL(cc_flatten_kernel, points, dim3(256), 0, s, g.p, parent, count);
    hipLaunchKernelGGL(cc_select_kernel, points, dim3(256), 0, s, g.p, parent, count, mode, (long)min_points, best, stats);
    hipLaunchKernelGGL(cc_apply_keep_kernel, points, dim3(256), 0, s, cube, g.p, parent, count, mode, (long)min_points, best, out_cube,
                       labels, stats);
    if (flags & GPNERF_CUBE_FILL) {
        // the outside: 6-connectivity over the below-iso points of out_cube (after the step above)
        hipLaunchKernelGGL((cc_local_kernel<3, false>), bricks, dim3(CC_THREADS), 0, s, out_cube, g, parent, count,
                           (unsigned long long*)nullptr, (int64_t*)nullptr);
        hipLaunchKernelGGL((cc_merge_kernel<3>), bricks, dim3(CC_THREADS), 0, s, g, parent);
        hipLaunchKernelGGL(cc_flatten_kernel, points, dim3(256), 0, s, g.p, parent, count);
        hipLaunchKernelGGL(cc_apply_fill_kernel, points, dim3(256), 0, s, g.p, parent, count, out_cube, stats);
    }
    return launch_status();
}

int gpnerf_mesh_normals(const float* cube, const int32_t* dims, const float* vertices, int64_t n_vertices, const float* inv_step,
                        float* normals, void* stream) {
    Grid g;
    if (!cube || !grid_of(dims, 0.f, g) || n_vertices < 0) return GPNERF_E_ARG;
    if (n_vertices == 0) return GPNERF_OK;
    if (!vertices || !normals || n_vertices > ((int64_t)1 << 31) * 255) return GPNERF_E_ARG;
    Step3 inv = {{1.0f, 1.0f, 1.0f}};
    if (inv_step) for (int a = 0; a < 3; ++a) inv.v[a] = inv_step[a];
    hipLaunchKernelGGL(mesh_normals_kernel, dim3((unsigned)((n_vertices + 255) / 256)), dim3(256), 0, S_(stream), cube, g, vertices,
                       (long)n_vertices, inv, normals);
    return launch_status();
}

}  // extern "C"
