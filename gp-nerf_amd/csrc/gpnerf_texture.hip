// gpnerf_texture.hip -- colouring points (a mesh's vertices, surface samples) from calibrated views on gfx950: each point is projected
// into up to eight views as the rasteriser projects a vertex, culled by the near plane, the image's frame, the mask, the facing of its
// normal and the mesh that may lie between it and the camera, sampled bilinearly and blended.  include/gpnerf_hip.h states THE
// DEFINITION operation for operation (gpnerf_texture_points); DESIGN.md 4.19 the argument for each rule and what was measured.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone.
// No float atomics: a point is one lane's, its views are summed by that lane in ascending order.  The only atomics are the integer
// sums of the statistics, one add per wavefront and counter.
//
// Lane mapping: one point per lane in both kernels, the views in a loop inside the lane.  A lane per (point, view) pair would give
// eight times the lanes, but the blend is a sum over a point's views IN ORDER: it would come back as a cross-lane reduction of
// float64 values with an order to keep, for a loop of at most eight steps.  Neighbouring vertices of an extracted mesh are
// neighbours in space, so the 64 points of a wavefront project to neighbouring pixels of a view and their taps share cache lines; the
// cameras travel in the kernel argument and are read through scalar loads (the view index is uniform).  The cast in between is
// gpnerf_mesh_raycast itself, one ray per lane over the [n][n_views] rows.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for; wave_count, stat_add

constexpr int MAX_VIEWS = GPNERF_TEXTURE_MAX_VIEWS, THREADS = 256, MAX_SIDE = 16384, MAX_CH = 4;
constexpr int FATES = GPNERF_TEXTURE_FATES;

struct Layout { size_t rays, t, face, w, fate, total; };

Layout layout_of(int64_t n, int n_views) {
    const size_t pairs = (size_t)n * (size_t)n_views;
    Layout l;
    size_t o = 0;
    l.rays = o; o += align256(32 * pairs);               // gpnerf_mesh_raycast's rows
    l.t = o;    o += align256(4 * pairs);                // its t
    l.face = o; o += align256(4 * pairs);                // its face
    l.w = o;    o += align256(8 * pairs);                // the pair's weight, float64
    l.fate = o; o += align256(pairs);                    // the pair's fate after rules 1-4
    l.total = o;
    return l;
}

bool sizes_ok(int64_t n, int n_views) { return n >= 0 && n <= INT32_MAX && n_views >= 1 && n_views <= MAX_VIEWS; }

struct Views {
    double cam[MAX_VIEWS][21];                           // K 3x3 row-major, RT 3x4 row-major: gpnerf_mesh_rasterize's layout
    float eye[MAX_VIEWS][3];                             // -R^T T, float64 rounded once
};
struct Fill { float v[MAX_CH]; };

// rule 1 and the position rule 2 reads: gpnerf_mesh_rasterize's projection of a vertex (float64, multiply then add, unfused)
DEV bool project_point(const double* __restrict__ cam, double p0, double p1, double p2, double z_near, double& x, double& y) {
    const double* K = cam;
    const double* RT = cam + 9;
    const double c0 = ((p0 * RT[0] + p1 * RT[1]) + p2 * RT[2]) + RT[3];
    const double c1 = ((p0 * RT[4] + p1 * RT[5]) + p2 * RT[6]) + RT[7];
    const double c2 = ((p0 * RT[8] + p1 * RT[9]) + p2 * RT[10]) + RT[11];
    const double h0 = (c0 * K[0] + c1 * K[1]) + c2 * K[2];
    const double h1 = (c0 * K[3] + c1 * K[4]) + c2 * K[5];
    const double h2 = (c0 * K[6] + c1 * K[7]) + c2 * K[8];
    x = h0 / h2;
    y = h1 / h2;
    // (every comparison is false for a NaN)
    return h2 >= z_near && h2 < (double)INFINITY && fabs(x) < (double)INFINITY && fabs(y) < (double)INFINITY;
}

DEV bool inside_image(double x, double y, int H, int W) { return x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1); }

// (a) rules 1-4 for every view of a point: the pair's fate so far (USED = not culled yet), its weight and its row for the cast.  A
// culled pair's row has tmin > tmax: "not a ray", which the cast answers without a walk.  Block 0 also zeroes the statistics.
__global__ __launch_bounds__(THREADS) void texture_prepare_kernel(const Views views, int n_views, const float* __restrict__ points,
                                                                  const float* __restrict__ normals, long n, int H, int W,
                                                                  const uint8_t* __restrict__ masks, double z_near, double cos2, int sharpness,
                                                                  float eps, float* rays, double* weights, uint8_t* fates, long long* stats,
                                                                  long long* totals) {
    if (blockIdx.x == 0) {
        if (stats && (int)threadIdx.x < FATES * n_views) stats[threadIdx.x] = 0;
        if (totals && threadIdx.x < 2) totals[threadIdx.x] = 0;
    }
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float pf[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
    const double p0 = (double)pf[0], p1 = (double)pf[1], p2 = (double)pf[2];
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, nn = 0.0;
    bool normal_ok = true;
    if (normals) {
        n0 = (double)normals[3 * i]; n1 = (double)normals[3 * i + 1]; n2 = (double)normals[3 * i + 2];
        nn = (n0 * n0 + n1 * n1) + n2 * n2;
        normal_ok = nn < (double)INFINITY;               // (a NaN fails; float32 squares do not overflow float64)
    }
    for (int v = 0; v < n_views; ++v) {
        double x, y, w = 0.0;
        int fate = GPNERF_TEXTURE_USED;
        // v = e - p in float32, the row mesh_visibility composes
        const float d[3] = {views.eye[v][0] - pf[0], views.eye[v][1] - pf[1], views.eye[v][2] - pf[2]};
        if (!project_point(views.cam[v], p0, p1, p2, z_near, x, y)) fate = GPNERF_TEXTURE_BEHIND;
        else if (!inside_image(x, y, H, W)) fate = GPNERF_TEXTURE_OUTSIDE;
        else if (masks && masks[((long)v * H + (long)rint(y)) * W + (long)rint(x)] != 1) fate = GPNERF_TEXTURE_MASKED;
        else if (normals) {
            const double d0 = (double)d[0], d1 = (double)d[1], d2 = (double)d[2];
            const double a = (n0 * d0 + n1 * d1) + n2 * d2, vv = (d0 * d0 + d1 * d1) + d2 * d2;
            if (!normal_ok || !(a > 0.0) || !(a * a >= (cos2 * nn) * vv)) fate = GPNERF_TEXTURE_BACKFACING;
            else {
                const double r = (a * a) / (nn * vv);
                w = sharpness == 0 ? 1.0 : r;
                for (int k = 1; k < sharpness; ++k) w *= r;
            }
        } else {
            w = 1.0;
        }
        const long pair = i * n_views + v;
        fates[pair] = (uint8_t)fate;
        weights[pair] = w;
        if (rays) {
            const bool cast = fate == GPNERF_TEXTURE_USED;
            float4* row = reinterpret_cast<float4*>(rays + 8 * pair);
            row[0] = cast ? make_float4(pf[0], pf[1], pf[2], d[0]) : make_float4(0.f, 0.f, 0.f, 0.f);
            row[1] = cast ? make_float4(d[1], d[2], eps, 1.f) : make_float4(0.f, 1.f, 1.f, 0.f);
        }
    }
}

template <int C> struct Tap { float v[C]; };

template <int C>
DEV Tap<C> load_tap(const float* __restrict__ img, long pixel) {
    Tap<C> t;
#pragma unroll
    for (int c = 0; c < C; ++c) t.v[c] = img[pixel * C + c];
    return t;
}
template <>
DEV Tap<4> load_tap<4>(const float* __restrict__ img, long pixel) {                       // one 16-byte load
    const float4 q = reinterpret_cast<const float4*>(img)[pixel];
    return Tap<4>{{q.x, q.y, q.z, q.w}};
}

// rule 6: the bilinear sample of one view's image at (x, y), pixel centres at integer coordinates, float64
template <int C>
DEV void sample_view(const float* __restrict__ img, int H, int W, double x, double y, double* colour) {
    const double fi = floor(x), fj = floor(y);
    const int i0 = (int)fi, j0 = (int)fj, i1 = min(i0 + 1, W - 1), j1 = min(j0 + 1, H - 1);
    const double fx = x - fi, fy = y - fj;
    const Tap<C> c00 = load_tap<C>(img, (long)j0 * W + i0), c10 = load_tap<C>(img, (long)j0 * W + i1);
    const Tap<C> c01 = load_tap<C>(img, (long)j1 * W + i0), c11 = load_tap<C>(img, (long)j1 * W + i1);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double top = (double)c00.v[c] * (1.0 - fx) + (double)c10.v[c] * fx;
        const double bottom = (double)c01.v[c] * (1.0 - fx) + (double)c11.v[c] * fx;
        colour[c] = top * (1.0 - fy) + bottom * fy;
    }
}

// (c) rule 5's answer read from the cast, rule 6, the blend, the outputs and the counts
template <int C>
__global__ __launch_bounds__(THREADS) void texture_blend_kernel(const Views views, int n_views, const float* __restrict__ points, long n,
                                                                const float* __restrict__ images, int H, int W, double z_near,
                                                                const double* __restrict__ weights, const uint8_t* __restrict__ fates,
                                                                const float* __restrict__ cast_t, int mode,
                                                                const float* __restrict__ fallback, const Fill background, float* color,
                                                                float* weight, uint8_t* used_views, long long* stats, long long* totals) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    const bool live = i < n;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (live) { p0 = (double)points[3 * i]; p1 = (double)points[3 * i + 1]; p2 = (double)points[3 * i + 2]; }
    double num[C], den = 0.0, best_w = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) num[c] = 0.0;
    int best = -1;
    unsigned bits = 0u;
    const long hw = (long)H * W;
    for (int v = 0; v < n_views; ++v) {                  // (uniform: every lane of the wavefront reaches the counts)
        int fate = -1;
        double w = 0.0;
        if (live) {
            const long pair = i * n_views + v;
            fate = fates[pair];
            w = weights[pair];
            // mesh_visibility's answer: seen iff the ANY ray's t > 0 (0: a face lies between; NaN: a row or a grid the cast refuses)
            if (fate == GPNERF_TEXTURE_USED && cast_t && !(cast_t[pair] > 0.f)) fate = GPNERF_TEXTURE_OCCLUDED;
        }
        if (fate == GPNERF_TEXTURE_USED) {
            if (mode == GPNERF_TEXTURE_BEST) {
                if (best < 0 || w > best_w) { best = v; best_w = w; }
            } else {
                double x, y, colour[C];
                project_point(views.cam[v], p0, p1, p2, z_near, x, y);
                sample_view<C>(images + (long)v * hw * C, H, W, x, y, colour);
#pragma unroll
                for (int c = 0; c < C; ++c) num[c] = num[c] + w * colour[c];
                den = den + w;
                bits |= 1u << v;
            }
        }
        if (stats) {
#pragma unroll
            for (int k = 0; k < FATES; ++k) {
                const int cnt = wave_count(fate == k);
                if ((threadIdx.x & 63) == 0) stat_add(stats + FATES * v, k, cnt);
            }
        }
    }
    float out[C], out_w = 0.f;
    if (live) {
        if (mode == GPNERF_TEXTURE_BEST && best >= 0) {
            double x, y, colour[C];
            project_point(views.cam[best], p0, p1, p2, z_near, x, y);
            sample_view<C>(images + (long)best * hw * C, H, W, x, y, colour);
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = (float)colour[c];
            out_w = (float)best_w;
            bits = 1u << best;
        } else if (bits) {
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = (float)(num[c] / den);
            out_w = (float)den;
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] = fallback ? fallback[i * C + c] : background.v[c];
        }
        if (color) {
#pragma unroll
            for (int c = 0; c < C; ++c) color[i * C + c] = out[c];
        }
        if (weight) weight[i] = out_w;
        if (used_views) used_views[i] = (uint8_t)bits;
    }
    if (totals) {
        const int seen = wave_count(live && bits != 0u), unseen = wave_count(live && bits == 0u);
        if ((threadIdx.x & 63) == 0) { stat_add(totals, 0, seen); stat_add(totals, 1, unseen); }
    }
}

}  // namespace

extern "C" {

size_t gpnerf_texture_workspace_bytes(int64_t n_points, int32_t n_views) {
    if (!sizes_ok(n_points, n_views)) return 0;
    return layout_of(n_points, n_views).total;
}

int gpnerf_texture_points(const float* points, int64_t n_points, const float* normals, const double* cams, int32_t n_views,
                          const float* images, int32_t H, int32_t W, int32_t C, const uint8_t* masks, const float* vertices,
                          int64_t n_vertices, const int32_t* faces, int64_t n_faces, void* grid_workspace, double z_near, double cos_min,
                          int32_t sharpness, float eps, int32_t mode, const float* fallback, const float* background, void* workspace,
                          size_t workspace_bytes, float* color, float* weight, uint8_t* views, int64_t* stats, int64_t* totals,
                          void* stream) {
    if (!sizes_ok(n_points, n_views) || !cams || !images || !background || !workspace || (!points && n_points > 0)) return GPNERF_E_ARG;
    if (H < 1 || H > MAX_SIDE || W < 1 || W > MAX_SIDE || C < 1 || C > MAX_CH) return GPNERF_E_ARG;
    if (C == 4 && (reinterpret_cast<uintptr_t>(images) & 15u)) return GPNERF_E_ARG;       // a tap is one 16-byte load
    if (!(z_near > 0.0) || !(z_near < (double)INFINITY)) return GPNERF_E_ARG;             // zero, negative, NaN, infinite
    if (!(cos_min >= 0.0) || !(cos_min < 1.0) || sharpness < 0 || sharpness > GPNERF_TEXTURE_MAX_SHARPNESS) return GPNERF_E_ARG;
    if (!(eps >= 0.f) || !(eps <= 1.f)) return GPNERF_E_ARG;                              // the row's tmin, tmax = 1
    if (mode != GPNERF_TEXTURE_BLEND && mode != GPNERF_TEXTURE_BEST) return GPNERF_E_ARG;
    if (n_faces < 0 || n_faces > INT32_MAX || (n_faces == 0 && grid_workspace)) return GPNERF_E_ARG;
    if (n_faces > 0 && (!vertices || !faces || n_vertices < 0)) return GPNERF_E_ARG;
    const Layout l = layout_of(n_points, n_views);
    if (workspace_bytes < l.total || (reinterpret_cast<uintptr_t>(workspace) & 15u)) return GPNERF_E_ARG;   // the rows are 16-byte stores
    Views vw = {};
    for (int v = 0; v < n_views; ++v) {
        const double* RT = cams + 21 * v + 9;
        for (int e = 0; e < 21; ++e) vw.cam[v][e] = cams[21 * v + e];
        for (int a = 0; a < 3; ++a) vw.eye[v][a] = (float)(-((RT[a] * RT[3] + RT[4 + a] * RT[7]) + RT[8 + a] * RT[11]));
    }
    Fill bg = {};
    for (int c = 0; c < C; ++c) bg.v[c] = background[c];
    char* base = static_cast<char*>(workspace);
    const bool occlude = n_faces > 0;
    float* rays = occlude ? reinterpret_cast<float*>(base + l.rays) : nullptr;
    float* cast_t = occlude ? reinterpret_cast<float*>(base + l.t) : nullptr;
    int32_t* cast_face = reinterpret_cast<int32_t*>(base + l.face);
    double* w = reinterpret_cast<double*>(base + l.w);
    uint8_t* fates = reinterpret_cast<uint8_t*>(base + l.fate);
    long long* st = reinterpret_cast<long long*>(stats);
    long long* tot = reinterpret_cast<long long*>(totals);
    const unsigned blocks = n_points > 0 ? blocks_for(n_points, THREADS) : 1u;           // (an empty list still zeroes the counts)
    hipLaunchKernelGGL(texture_prepare_kernel, dim3(blocks), dim3(THREADS), 0, S_(stream), vw, (int)n_views, points, normals, (long)n_points,
                       (int)H, (int)W, masks, z_near, cos_min * cos_min, (int)sharpness, eps, rays, w, fates, st, tot);
    if (n_points == 0) return launch_status();
    if (occlude) {
        const int rc = gpnerf_mesh_raycast(rays, n_points * n_views, vertices, n_vertices, faces, n_faces, grid_workspace, GPNERF_RAYCAST_ANY,
                                           cast_t, cast_face, nullptr, stream);
        if (rc != GPNERF_OK) return rc;
    }
#define GPNERF_TEXTURE_BLEND_LAUNCH(CH)                                                                                                  \
    hipLaunchKernelGGL(texture_blend_kernel<CH>, dim3(blocks), dim3(THREADS), 0, S_(stream), vw, (int)n_views, points, (long)n_points, images, \
                       (int)H, (int)W, z_near, w, fates, cast_t, (int)mode, fallback, bg, color, weight, views, st, tot)
    switch (C) {
        case 1: GPNERF_TEXTURE_BLEND_LAUNCH(1); break;
        case 2: GPNERF_TEXTURE_BLEND_LAUNCH(2); break;
        case 3: GPNERF_TEXTURE_BLEND_LAUNCH(3); break;
        default: GPNERF_TEXTURE_BLEND_LAUNCH(4); break;
    }
#undef GPNERF_TEXTURE_BLEND_LAUNCH
    return launch_status();
}

}  // extern "C"
