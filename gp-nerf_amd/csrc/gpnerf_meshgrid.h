// gpnerf_meshgrid.h -- the layout of the uniform cell grid gpnerf_mesh_grid_build leaves in its workspace, shared by the file that
// builds it and answers point queries through it (gpnerf_meshdist.hip) and the file that walks rays through it (gpnerf_raycast.hip):
// both compile the same layout and the same cell function, so a face the build entered into a cell is found there by either.
// Included INSIDE the including file's unnamed namespace, behind <hip/hip_runtime.h>, <math.h>, <stdint.h>, gpnerf_diag.h (DEV) and
// gpnerf_util.h (align256).  Constants, two small structs and their functions only.  include/gpnerf_hip.h (gpnerf_mesh_grid_build)
// states the grid.
#ifndef GPNERF_MESHGRID_H
#define GPNERF_MESHGRID_H

constexpr int BOX_BLOCKS_MAX = 1024;                     // partial boxes of the reduction
constexpr int MAX_AXIS_CELLS = 1024;                     // per axis: the shell bound's rounding argument relies on it
constexpr int32_t GRID_MAGIC = 0x47524431;               // "GRD1"

struct GridLayout { size_t hdr, part, start, cursor, entries, tmp_face, tmp_cell, total; };

__host__ __device__ inline GridLayout grid_layout(int64_t cell_cap, int64_t entry_cap) {
    GridLayout l;
    size_t o = 0;
    l.hdr = o;      o += 256;
    l.part = o;     o += align256(sizeof(float) * 8 * BOX_BLOCKS_MAX);
    l.start = o;    o += align256(sizeof(int32_t) * (size_t)(cell_cap + 1));
    l.cursor = o;   o += align256(sizeof(int32_t) * (size_t)cell_cap);
    l.entries = o;  o += align256(sizeof(int32_t) * (size_t)entry_cap);
    l.tmp_face = o; o += align256(sizeof(int32_t) * (size_t)entry_cap);
    l.tmp_cell = o; o += align256(sizeof(int32_t) * (size_t)entry_cap);
    l.total = o;
    return l;
}

struct Grid {                                            // the workspace's regions, as the kernels see them
    int32_t* hdr; float* part; int32_t* start; int32_t* cursor; int32_t* entries; int32_t* tmp_face; int32_t* tmp_cell;
};

__host__ __device__ inline Grid grid_of(void* workspace, int64_t cell_cap, int64_t entry_cap) {
    const GridLayout l = grid_layout(cell_cap, entry_cap);
    char* base = static_cast<char*>(workspace);
    Grid g;
    g.hdr = reinterpret_cast<int32_t*>(base + l.hdr);
    g.part = reinterpret_cast<float*>(base + l.part);
    g.start = reinterpret_cast<int32_t*>(base + l.start);
    g.cursor = reinterpret_cast<int32_t*>(base + l.cursor);
    g.entries = reinterpret_cast<int32_t*>(base + l.entries);
    g.tmp_face = reinterpret_cast<int32_t*>(base + l.tmp_face);
    g.tmp_cell = reinterpret_cast<int32_t*>(base + l.tmp_cell);
    return g;
}

// the cell of a coordinate on one axis: monotone in x, clamped, never out of range (the clamp is taken in float: no int overflow)
DEV int cell_of(float x, float lo, float inv, int n) {
    const float t = floorf((x - lo) * inv);
    return (int)fminf(fmaxf(t, 0.f), (float)(n - 1));
}

#endif  // GPNERF_MESHGRID_H
