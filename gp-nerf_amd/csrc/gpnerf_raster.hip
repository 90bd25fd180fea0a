// gpnerf_raster.hip -- drawing a triangle mesh into calibrated cameras on gfx950: depth and face-id maps, vertex attributes
// interpolated over them, and the counts that compare a silhouette with a foreground mask.  include/gpnerf_hip.h states the
// definition operation for operation (gpnerf_mesh_rasterize); DESIGN.md 4.11 the launch shape and what was measured.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone;
// the one data-dependent length (the large-face list's) stays in the workspace header.  No float atomics.  The integer atomics, and
// why their arrival order cannot matter:
//   - a pixel's key is the 64-bit unsigned MINIMUM over the faces that cover it of (bits(depth) << 32) | face: min is commutative and
//     associative, and the positive float32 depths order as their bit patterns do;
//   - the large-face list is filled through a cursor: the SET of (face, view) pairs that lands in it is the same in any order, and
//     what the list's reader does with a pair is again a minimum per pixel;
//   - the statistics are integer sums.
//
// The two-tier walk of gpnerf_tri2d.h over a view's pixels, the vertices snapped to 1/256 pixel.  A body mesh at the project's
// lattice projects to triangles of about a pixel, so the first kernel gives every (face, view) pair ONE lane, which projects the
// three vertices in float64 and walks the face's clipped pixel box, i inside (a row's keys are contiguous in i); the pairs of more
// than LARGE_BOX pixels go through the list to the second kernel.  What is the rasteriser's own: the projection, the inclusive edge
// rule (covers), the perspective-correct depth and the key a covered pixel takes the minimum of.  The cameras travel in the kernel
// argument.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for, sweep_blocks, mesh_ok; wave_count, wave_sum, stat_add
#include "gpnerf_tri2d.h"      // Mesh, Snapped, Setup, Edges, setup_face, count_states, large_append, lane_walk, wave_walk; LARGE_*
#include "gpnerf_rasterface.h" // Cams, Setup8, project_vertex, raster_setup, covers, Persp, persp_of, cams_of; RASTER_VIEWS

constexpr int MAX_VIEWS = RASTER_VIEWS, THREADS = 256, MAX_SIDE = 16384, MAX_ATTRS = 4;
constexpr int COUNT_BLOCKS_MAX = 256;                    // per view, of the silhouette count
constexpr unsigned long long EMPTY = ~0ull;

static_assert(GPNERF_RASTER_DRAWN == FACE_OK && GPNERF_RASTER_SKIPPED_VERTEX == FACE_BAD_VERTEX && GPNERF_RASTER_SKIPPED_AREA == FACE_NO_AREA,
              "count_states adds a face under its state");

struct Layout { size_t hdr, keys, list, total; };

Layout layout_of(int64_t n_faces, int n_views, int H, int W) {
    Layout l;
    size_t o = 0;
    l.hdr = o;  o += 256;                                // the list's length, uint64 at 0
    l.keys = o; o += align256(sizeof(uint64_t) * (size_t)n_views * (size_t)H * (size_t)W);
    l.list = o; o += align256(sizeof(uint64_t) * (size_t)n_faces * (size_t)n_views);
    l.total = o;
    return l;
}

bool sizes_ok(int64_t n_faces, int n_views, int H, int W) {
    return n_faces >= 0 && n_faces <= INT32_MAX && n_views >= 1 && n_views <= MAX_VIEWS && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE;
}

DEV unsigned long long key_of(const Setup8& s, const Edges& e, long f) {
    const float depth = (float)(1.0 / persp_of(s, e).q);
    return ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(uint32_t)f;
}

// what both walks do at a pixel of the face's box: a covered pixel takes the minimum of its key and the face's
struct Draw {
    const Setup8& s;
    unsigned long long* view_keys;
    int W;
    long f;
    DEV void operator()(int i, int j, const Edges e) const {
        if (covers(s, e)) atomicMin(view_keys + (long)j * W + i, key_of(s, e, f));
    }
};

// the keys, the list's length and the statistics start from a kernel of the library's own, not from memset nodes
__global__ __launch_bounds__(THREADS) void raster_clear_kernel(unsigned long long* keys, long n_keys, unsigned long long* list_len,
                                                               long long* stats, int n_stats) {
    const long stride = (long)gridDim.x * THREADS;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n_keys; i += stride) keys[i] = EMPTY;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) *list_len = 0ull;
        if (stats && (int)threadIdx.x < n_stats) stats[threadIdx.x] = 0;
    }
}

// one lane per (face, view); blockIdx.y is the view, so a wavefront's lanes share the camera and the statistics' row
__global__ __launch_bounds__(THREADS) void raster_faces_kernel(const Cams cams, const Mesh m, double z_near, int H, int W,
                                                               unsigned long long* keys, unsigned long long* list,
                                                               unsigned long long* list_len, long long* stats) {
    const int view = blockIdx.y;
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    const bool live = f < m.n_faces;
    Setup8 s;
    FaceState st = FACE_OK;
    long box = 0;
    if (live) {
        st = raster_setup(m, cams.cam[view], z_near, f, H, W, s);
        if (st == FACE_OK) box = s.box();
    }
    if (stats) count_states(live, st, stats + 4 * view);
    const bool large = box > LARGE_BOX;
    const long long at = large_append(large, list_len, (unsigned long long)m.n_faces * gridDim.y);
    if (at >= 0) list[at] = ((unsigned long long)view << 32) | (unsigned long long)(uint32_t)f;
    if (box == 0 || large) return;
    lane_walk<INNER_I>(s, Draw{s, keys + (long)view * H * W, W, f});
}

// fixed grid: a wavefront per listed pair, 64 pixels of its box per step
__global__ __launch_bounds__(THREADS) void raster_large_kernel(const Cams cams, const Mesh m, double z_near, int H, int W, int n_views,
                                                               unsigned long long* keys, const unsigned long long* __restrict__ list,
                                                               const unsigned long long* __restrict__ list_len) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (THREADS / 64) + threadIdx.x / 64, waves = (long)gridDim.x * (THREADS / 64);
    unsigned long long n = *list_len;
    const unsigned long long cap = (unsigned long long)m.n_faces * (unsigned long long)n_views;
    if (n > cap) n = cap;
    for (unsigned long long at = (unsigned long long)wave; at < n; at += (unsigned long long)waves) {
        const unsigned long long pair = list[at];
        const int view = (int)(pair >> 32);
        const long f = (long)(uint32_t)pair;
        if (view < 0 || view >= n_views || f >= m.n_faces) continue;      // (never: the list holds what the first kernel wrote)
        Setup8 s;
        if (raster_setup(m, cams.cam[view], z_near, f, H, W, s) != FACE_OK || s.i1 < s.i0 || s.j1 < s.j0) continue;
        wave_walk<INNER_I>(s, lane, Draw{s, keys + (long)view * H * W, W, f});
    }
}

// keys -> depth / face id, and the covered pixels of each view: one integer add per wavefront
__global__ __launch_bounds__(THREADS) void raster_resolve_kernel(const unsigned long long* __restrict__ keys, long hw, float* depth,
                                                                 int32_t* face_id, long long* stats) {
    const int view = blockIdx.y;
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    bool covered = false;
    if (p < hw) {
        const unsigned long long key = keys[(long)view * hw + p];
        covered = key != EMPTY;
        if (depth) depth[(long)view * hw + p] = covered ? __uint_as_float((uint32_t)(key >> 32)) : __int_as_float(0x7f800000);
        if (face_id) face_id[(long)view * hw + p] = covered ? (int32_t)(uint32_t)key : -1;
    }
    if (stats) {
        const int n = wave_count(covered);
        if ((threadIdx.x & 63) == 0) stat_add(stats + 4 * view, GPNERF_RASTER_PIXELS, n);
    }
}

struct Background { float v[MAX_ATTRS]; };

__global__ __launch_bounds__(THREADS) void raster_interpolate_kernel(const Cams cams, const Mesh m, double z_near, int H, int W,
                                                                     const int32_t* __restrict__ face_id, const float* __restrict__ attrs,
                                                                     int C, Background bg, float* out) {
    const int view = blockIdx.y;
    const long hw = (long)H * W;
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= hw) return;
    float* o = out + ((long)view * hw + p) * C;
    const int32_t f = face_id[(long)view * hw + p];
    Setup8 s;
    bool ok = f >= 0 && f < m.n_faces && raster_setup(m, cams.cam[view], z_near, f, H, W, s) == FACE_OK;
    Edges e;
    if (ok) {
        e = s.edges_at((int)(p % W), (int)(p / W));
        ok = covers(s, e);                               // a face id that is not this pixel's: background
    }
    if (!ok) {
        for (int c = 0; c < C; ++c) o[c] = bg.v[c];
        return;
    }
    const Persp t = persp_of(s, e);
    const double ua = t.ta / t.q, ub = t.tb / t.q, uc = t.tc / t.q;
    const float* aa = attrs + (long)m.faces[3 * (long)f] * C;
    const float* ab = attrs + (long)m.faces[3 * (long)f + 1] * C;
    const float* ac = attrs + (long)m.faces[3 * (long)f + 2] * C;
    for (int c = 0; c < C; ++c) o[c] = (float)((ua * (double)aa[c] + ub * (double)ab[c]) + uc * (double)ac[c]);
}

__global__ void silhouette_zero_kernel(long long* out, int n) {
    if ((int)threadIdx.x < n) out[threadIdx.x] = 0;
}

// blockIdx.y is the view; a thread counts its pixels p, p + stride, ..., a wavefront adds its five sums once
__global__ __launch_bounds__(THREADS) void silhouette_count_kernel(const int32_t* __restrict__ face_id, const uint8_t* __restrict__ masks,
                                                                   long hw, long long* out) {
    const int view = blockIdx.y;
    const long stride = (long)gridDim.x * THREADS;
    int cnt[GPNERF_SILHOUETTE_COUNTS] = {};
    for (long p = (long)blockIdx.x * THREADS + threadIdx.x; p < hw; p += stride) {
        const unsigned mk = masks[(long)view * hw + p];
        const bool cov = face_id[(long)view * hw + p] >= 0;
        if (mk == 100u) { ++cnt[GPNERF_SILHOUETTE_IGNORED]; continue; }
        const bool gt = mk != 0u;
        cnt[GPNERF_SILHOUETTE_COVERED] += cov;
        cnt[GPNERF_SILHOUETTE_GT] += gt;
        cnt[GPNERF_SILHOUETTE_BOTH] += cov && gt;
        cnt[GPNERF_SILHOUETTE_EITHER] += cov || gt;
    }
    for (int k = 0; k < GPNERF_SILHOUETTE_COUNTS; ++k) {
        const int v = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0) stat_add(out + GPNERF_SILHOUETTE_COUNTS * view, k, v);
    }
}

}  // namespace

extern "C" {

size_t gpnerf_mesh_raster_workspace_bytes(int64_t n_faces, int32_t n_views, int32_t H, int32_t W) {
    if (!sizes_ok(n_faces, n_views, H, W)) return 0;
    return layout_of(n_faces, n_views, H, W).total;
}

int gpnerf_mesh_rasterize(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const double* cams,
                          int32_t n_views, int32_t H, int32_t W, double z_near, void* workspace, size_t workspace_bytes, float* depth,
                          int32_t* face_id, int64_t* stats, void* stream) {
    if (!cams || !workspace || !mesh_ok(vertices, n_vertices, faces, n_faces) || !sizes_ok(n_faces, n_views, H, W)) return GPNERF_E_ARG;
    if (!(z_near > 0.0) || !(z_near < (double)INFINITY)) return GPNERF_E_ARG;          // zero, negative, NaN, infinite
    const Layout l = layout_of(n_faces, n_views, H, W);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    char* base = static_cast<char*>(workspace);
    unsigned long long* list_len = reinterpret_cast<unsigned long long*>(base + l.hdr);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + l.keys);
    unsigned long long* list = reinterpret_cast<unsigned long long*>(base + l.list);
    Cams c;
    cams_of(cams, n_views, c);
    const Mesh m = {vertices, faces, (long)n_vertices, (long)n_faces};
    const long hw = (long)H * W, n_keys = hw * n_views;
    long long* st = reinterpret_cast<long long*>(stats);
    hipLaunchKernelGGL(raster_clear_kernel, dim3(sweep_blocks(n_keys, THREADS)), dim3(THREADS), 0, S_(stream), keys, n_keys, list_len, st, 4 * n_views);
    if (n_faces > 0) {
        hipLaunchKernelGGL(raster_faces_kernel, dim3(blocks_for(n_faces, THREADS), (unsigned)n_views), dim3(THREADS), 0, S_(stream), c, m, z_near,
                           H, W, keys, list, list_len, st);
        hipLaunchKernelGGL(raster_large_kernel, dim3(LARGE_BLOCKS), dim3(THREADS), 0, S_(stream), c, m, z_near, H, W, n_views, keys, list,
                           list_len);
    }
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(blocks_for(hw, THREADS), (unsigned)n_views), dim3(THREADS), 0, S_(stream), keys, hw, depth,
                       face_id, st);
    return launch_status();
}

int gpnerf_mesh_interpolate(const int32_t* face_id, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                            const double* cams, int32_t n_views, int32_t H, int32_t W, double z_near, const float* attrs, int32_t C,
                            const float* background, float* out, void* stream) {
    if (!face_id || !cams || !background || !out || !mesh_ok(vertices, n_vertices, faces, n_faces) || !sizes_ok(n_faces, n_views, H, W))
        return GPNERF_E_ARG;
    if (C < 1 || C > MAX_ATTRS || (!attrs && n_vertices > 0)) return GPNERF_E_ARG;
    if (!(z_near > 0.0) || !(z_near < (double)INFINITY)) return GPNERF_E_ARG;
    Cams c;
    cams_of(cams, n_views, c);
    const Mesh m = {vertices, faces, (long)n_vertices, (long)n_faces};
    Background bg = {};
    for (int k = 0; k < C; ++k) bg.v[k] = background[k];
    hipLaunchKernelGGL(raster_interpolate_kernel, dim3(blocks_for((int64_t)H * W, THREADS), (unsigned)n_views), dim3(THREADS), 0, S_(stream), c,
                       m, z_near, H, W, face_id, attrs, C, bg, out);
    return launch_status();
}

int gpnerf_silhouette_stats(const int32_t* face_id, const uint8_t* masks, int32_t n_views, int32_t H, int32_t W, int64_t* out, void* stream) {
    if (!face_id || !masks || !out || !sizes_ok(0, n_views, H, W)) return GPNERF_E_ARG;
    const long hw = (long)H * W;
    long long* o = reinterpret_cast<long long*>(out);
    hipLaunchKernelGGL(silhouette_zero_kernel, dim3(1), dim3(64), 0, S_(stream), o, GPNERF_SILHOUETTE_COUNTS * n_views);
    const unsigned blocks = sweep_blocks(hw, THREADS, COUNT_BLOCKS_MAX);
    hipLaunchKernelGGL(silhouette_count_kernel, dim3(blocks, (unsigned)n_views), dim3(THREADS), 0, S_(stream), face_id, masks, hw, o);
    return launch_status();
}

}  // extern "C"
