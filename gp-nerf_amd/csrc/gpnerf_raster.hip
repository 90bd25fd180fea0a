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
// Two tiers.  A body mesh at the project's lattice projects to triangles of about a pixel, so the first kernel gives every
// (face, view) pair ONE lane, which projects the three vertices in float64, sets up the int64 edge functions and walks the face's
// clipped pixel box with three additions per pixel.  A pair whose box holds more than LARGE_BOX pixels would hold its wavefront's
// other 63 lanes up: it is appended to the list instead (one counter add per wavefront), and a second launch of fixed grid gives each
// listed pair a whole wavefront, 64 pixels of the box per step.  The cameras travel in the kernel argument.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)

constexpr int MAX_VIEWS = 8, THREADS = 256, MAX_SIDE = 16384, MAX_ATTRS = 4;
constexpr int LARGE_BOX = 256;                           // pixels in a clipped box above which a pair goes to the list (chosen, not tuned)
constexpr int LARGE_BLOCKS = 1024;                       // the list reader's fixed grid: 4096 wavefronts
constexpr int COUNT_BLOCKS_MAX = 256;                    // per view, of the silhouette count
constexpr int64_t SNAP = 256;                            // sub-pixel units per pixel
constexpr double GUARD = 1048576.0;                      // 2^20 pixels
constexpr unsigned long long EMPTY = ~0ull;

constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

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

struct Cams { double cam[MAX_VIEWS][21]; };              // K 3x3 row-major, RT 3x4 row-major: gpnerf_visual_hull's layout

struct Mesh {
    const float* vertices; const int32_t* faces;
    long n_vertices, n_faces;
};

struct Snapped { int64_t X, Y; double z; };
DEV int64_t lo_of(int64_t a, int64_t b) { return a < b ? a : b; }
DEV int64_t hi_of(int64_t a, int64_t b) { return a > b ? a : b; }

// one vertex in one view: the hull's projection (float64, multiply then add, unfused), the usable test, the snap to 1/256 pixel
DEV bool project_vertex(const double* __restrict__ cam, const float* __restrict__ p, double z_near, Snapped& s) {
    const double* K = cam;
    const double* RT = cam + 9;
    const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
    const double c0 = ((p0 * RT[0] + p1 * RT[1]) + p2 * RT[2]) + RT[3];
    const double c1 = ((p0 * RT[4] + p1 * RT[5]) + p2 * RT[6]) + RT[7];
    const double c2 = ((p0 * RT[8] + p1 * RT[9]) + p2 * RT[10]) + RT[11];
    const double h0 = (c0 * K[0] + c1 * K[1]) + c2 * K[2];
    const double h1 = (c0 * K[3] + c1 * K[4]) + c2 * K[5];
    const double h2 = (c0 * K[6] + c1 * K[7]) + c2 * K[8];
    const double x = h0 / h2, y = h1 / h2;
    // (every comparison is false for a NaN; an infinite x or y fails the guard band, an infinite z is named)
    if (!(h2 >= z_near) || !(h2 < (double)INFINITY) || !(fabs(x) <= GUARD) || !(fabs(y) <= GUARD)) return false;
    s.X = (int64_t)rint(256.0 * x);
    s.Y = (int64_t)rint(256.0 * y);
    s.z = h2;
    return true;
}

enum FaceState { FACE_OK = 0, FACE_BAD_VERTEX = 1, FACE_NO_AREA = 2 };

struct Setup {
    Snapped a, b, c;
    int64_t A;
    int i0, i1, j0, j1;                                  // the clipped pixel box, inclusive; empty when i1 < i0 or j1 < j0
};

DEV FaceState setup_face(const Mesh& m, const double* __restrict__ cam, double z_near, long f, int H, int W, Setup& s) {
    const int32_t ia = m.faces[3 * f], ib = m.faces[3 * f + 1], ic = m.faces[3 * f + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= m.n_vertices || ib >= m.n_vertices || ic >= m.n_vertices) return FACE_BAD_VERTEX;
    const bool ua = project_vertex(cam, m.vertices + 3 * (long)ia, z_near, s.a);
    const bool ub = project_vertex(cam, m.vertices + 3 * (long)ib, z_near, s.b);
    const bool uc = project_vertex(cam, m.vertices + 3 * (long)ic, z_near, s.c);
    if (!(ua && ub && uc)) return FACE_BAD_VERTEX;
    s.A = (s.b.X - s.a.X) * (s.c.Y - s.a.Y) - (s.b.Y - s.a.Y) * (s.c.X - s.a.X);
    if (s.A == 0) return FACE_NO_AREA;
    const int64_t x0 = lo_of(s.a.X, lo_of(s.b.X, s.c.X)), x1 = hi_of(s.a.X, hi_of(s.b.X, s.c.X));
    const int64_t y0 = lo_of(s.a.Y, lo_of(s.b.Y, s.c.Y)), y1 = hi_of(s.a.Y, hi_of(s.b.Y, s.c.Y));
    // pixel centres are the multiples of 256: ceil(x0 / 256) .. floor(x1 / 256), by arithmetic shifts, clipped to the image
    s.i0 = (int)hi_of(0, (x0 + (SNAP - 1)) >> 8); s.i1 = (int)lo_of(W - 1, x1 >> 8);
    s.j0 = (int)hi_of(0, (y0 + (SNAP - 1)) >> 8); s.j1 = (int)lo_of(H - 1, y1 >> 8);
    return FACE_OK;
}

// the three edge functions at pixel (i, j), each multiplied by sign(A): covered iff none is negative
struct Edges { int64_t ea, eb, ec; };

DEV Edges edges_at(const Setup& s, int i, int j) {
    const int64_t px = SNAP * i, py = SNAP * j;
    Edges e;
    e.ea = (s.c.X - s.b.X) * (py - s.b.Y) - (s.c.Y - s.b.Y) * (px - s.b.X);
    e.eb = (s.a.X - s.c.X) * (py - s.c.Y) - (s.a.Y - s.c.Y) * (px - s.c.X);
    e.ec = (s.b.X - s.a.X) * (py - s.a.Y) - (s.b.Y - s.a.Y) * (px - s.a.X);
    return e;
}

DEV bool covers(const Setup& s, const Edges& e) {
    return s.A > 0 ? (e.ea >= 0 && e.eb >= 0 && e.ec >= 0) : (e.ea <= 0 && e.eb <= 0 && e.ec <= 0);
}

// perspective-correct depth terms of a covered pixel: wk = Ek / A, q = (wa / za + wb / zb) + wc / zc
struct Persp { double ta, tb, tc, q; };                 // tk = wk / zk

DEV Persp persp_of(const Setup& s, const Edges& e) {
    const double A = (double)s.A;
    Persp p;
    p.ta = ((double)e.ea / A) / s.a.z;
    p.tb = ((double)e.eb / A) / s.b.z;
    p.tc = ((double)e.ec / A) / s.c.z;
    p.q = (p.ta + p.tb) + p.tc;
    return p;
}

DEV unsigned long long key_of(const Setup& s, const Edges& e, long f) {
    const float depth = (float)(1.0 / persp_of(s, e).q);
    return ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned long long)(uint32_t)f;
}

DEV int wave_count(bool flag) { return __popcll(__ballot(flag)); }

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
    Setup s;
    FaceState st = FACE_OK;
    long box = 0;
    if (live) {
        st = setup_face(m, cams.cam[view], z_near, f, H, W, s);
        if (st == FACE_OK && s.i1 >= s.i0 && s.j1 >= s.j0) box = (long)(s.i1 - s.i0 + 1) * (s.j1 - s.j0 + 1);
    }
    if (stats) {                                         // one add per wavefront and counter, and none for a zero
        const int drawn = wave_count(live && st == FACE_OK), bad = wave_count(live && st == FACE_BAD_VERTEX);
        const int flat = wave_count(live && st == FACE_NO_AREA);
        if ((threadIdx.x & 63) == 0) {
            if (drawn) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 4 * view + GPNERF_RASTER_DRAWN), (unsigned long long)drawn);
            if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 4 * view + GPNERF_RASTER_SKIPPED_VERTEX), (unsigned long long)bad);
            if (flat) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 4 * view + GPNERF_RASTER_SKIPPED_AREA), (unsigned long long)flat);
        }
    }
    // the large tier: the wavefront's pairs take consecutive places behind one add of their number
    const bool large = box > LARGE_BOX;
    const unsigned long long mask = __ballot(large);
    if (mask) {
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((unsigned long long)mask) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(list_len, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader);
        if (large) {
            const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
            if (at < (unsigned long long)m.n_faces * gridDim.y)        // (always: a pair is appended once)
                list[at] = ((unsigned long long)view << 32) | (unsigned long long)(uint32_t)f;
        }
    }
    if (box == 0 || large) return;
    unsigned long long* row_keys = keys + (long)view * H * W;
    // the box, rows outside: the edge functions are linear, so a pixel to the right adds -256 dY and a row down adds 256 dX (int64: exact)
    const Edges e0 = edges_at(s, s.i0, s.j0);
    const int64_t ax = -SNAP * (s.c.Y - s.b.Y), bx = -SNAP * (s.a.Y - s.c.Y), cx = -SNAP * (s.b.Y - s.a.Y);
    const int64_t ay = SNAP * (s.c.X - s.b.X), by = SNAP * (s.a.X - s.c.X), cy = SNAP * (s.b.X - s.a.X);
    Edges row = e0;
    for (int j = s.j0; j <= s.j1; ++j) {
        Edges e = row;
        for (int i = s.i0; i <= s.i1; ++i) {
            if (covers(s, e)) atomicMin(row_keys + (long)j * W + i, key_of(s, e, f));
            e.ea += ax; e.eb += bx; e.ec += cx;
        }
        row.ea += ay; row.eb += by; row.ec += cy;
    }
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
        Setup s;
        if (setup_face(m, cams.cam[view], z_near, f, H, W, s) != FACE_OK || s.i1 < s.i0 || s.j1 < s.j0) continue;
        const int bw = s.i1 - s.i0 + 1;
        const long box = (long)bw * (s.j1 - s.j0 + 1);
        unsigned long long* view_keys = keys + (long)view * H * W;
        for (long k = lane; k < box; k += 64) {
            const int j = s.j0 + (int)(k / bw), i = s.i0 + (int)(k % bw);
            const Edges e = edges_at(s, i, j);
            if (covers(s, e)) atomicMin(view_keys + (long)j * W + i, key_of(s, e, f));
        }
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
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 4 * view + GPNERF_RASTER_PIXELS), (unsigned long long)n);
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
    Setup s;
    bool ok = f >= 0 && f < m.n_faces && setup_face(m, cams.cam[view], z_near, f, H, W, s) == FACE_OK;
    Edges e;
    if (ok) {
        e = edges_at(s, (int)(p % W), (int)(p / W));
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
        int v = cnt[k];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
        if ((threadIdx.x & 63) == 0 && v)
            atomicAdd(reinterpret_cast<unsigned long long*>(out + GPNERF_SILHOUETTE_COUNTS * view + k), (unsigned long long)v);
    }
}

hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }
int launch_status() { return hipGetLastError() == hipSuccess ? GPNERF_OK : GPNERF_E_LAUNCH; }
unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

void cams_of(const double* cams, int n_views, Cams& c) {
    for (int v = 0; v < MAX_VIEWS; ++v)
        for (int e = 0; e < 21; ++e) c.cam[v][e] = v < n_views ? cams[v * 21 + e] : 0.0;
}

bool mesh_ok(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces) {
    return n_vertices >= 0 && n_vertices <= INT32_MAX && n_faces >= 0 && n_faces <= INT32_MAX && (vertices || n_vertices == 0) &&
           (faces || n_faces == 0);
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
    const unsigned clear_blocks = blocks_for(n_keys, THREADS) < 4096u ? blocks_for(n_keys, THREADS) : 4096u;
    hipLaunchKernelGGL(raster_clear_kernel, dim3(clear_blocks), dim3(THREADS), 0, S_(stream), keys, n_keys, list_len, st, 4 * n_views);
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
    const unsigned blocks = blocks_for(hw, THREADS) < (unsigned)COUNT_BLOCKS_MAX ? blocks_for(hw, THREADS) : (unsigned)COUNT_BLOCKS_MAX;
    hipLaunchKernelGGL(silhouette_count_kernel, dim3(blocks, (unsigned)n_views), dim3(THREADS), 0, S_(stream), face_id, masks, hw, o);
    return launch_status();
}

}  // extern "C"
