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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)

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

bool grid_of(const int32_t* dims, float iso, Grid& g) {
    if (!dims || dims[0] < 2 || dims[1] < 2 || dims[2] < 2 || !(iso == iso)) return false;
    const int64_t p = (int64_t)dims[0] * dims[1] * dims[2];
    if (p > MC_MAX_POINTS) return false;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2]; g.p = (long)p; g.iso = iso;
    return true;
}

constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
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

hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }
int launch_status() { return hipGetLastError() == hipSuccess ? GPNERF_OK : GPNERF_E_LAUNCH; }

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

}  // extern "C"
