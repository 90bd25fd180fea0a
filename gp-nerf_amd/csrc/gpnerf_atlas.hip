// gpnerf_atlas.hip -- a per-face texture atlas on gfx950: every face of a mesh owns a triangular lattice of res (res + 1) / 2 texels, two
// faces share a rectangular cell of the atlas image.  The texels' surface points (which gpnerf_texture_points colours from the views,
// unchanged), the colour list packed into the image, and the mesh drawn from the image through gpnerf_mesh_rasterize's face ids.
// include/gpnerf_hip.h states THE DEFINITION operation for operation (gpnerf_atlas_*); DESIGN.md 4.21 the argument and what was measured.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone.  No
// atomic of any kind: every output element is one lane's, and the pack is a GATHER (a lane per image texel inverts the packing and
// reads its owner's row), so there is no clear pass and no scatter.
//
// Lane mapping.  texels: a lane per texel, texels of a face consecutive, so a wavefront reads the corners of one to three faces and
// writes 64 consecutive rows.  pack: a lane per image texel, rows of the image consecutive: the stores are contiguous, the reads of
// the list run along a face's rows of i (ascending for the even face of a cell, descending for the odd one).  shade: a lane per pixel
// and view, gpnerf_mesh_interpolate's mapping; neighbouring pixels share a face or neighbouring faces, whose texels are neighbours in
// the image.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // S_, launch_status, blocks_for, mesh_ok
#include "gpnerf_tri2d.h"      // Mesh, Setup, Edges, setup_face
#include "gpnerf_rasterface.h" // Cams, Setup8, raster_setup, covers, Persp, persp_of, cams_of; RASTER_VIEWS

constexpr int THREADS = 256, MAX_SIDE = 16384, MAX_CH = 4, RES_MIN = 2, RES_MAX = 64;

// section 1 of THE DEFINITION, host arithmetic
struct Atlas { long cells, cx, cy, width, height, tpf, texels; };

bool atlas_of(int64_t n_faces, int res, Atlas& a) {
    if (res < RES_MIN || res > RES_MAX || n_faces < 0 || n_faces > INT32_MAX) return false;
    a.cells = (long)((n_faces + 1) / 2);
    long cx = (long)sqrt((double)a.cells);
    while (cx * cx < a.cells) ++cx;
    while (cx > 0 && (cx - 1) * (cx - 1) >= a.cells) --cx;
    a.cx = cx;
    a.cy = cx ? (a.cells + cx - 1) / cx : 0;
    a.width = a.cx * (res + 2);
    a.height = a.cy * res;
    a.tpf = (long)res * (res + 1) / 2;
    a.texels = (long)n_faces * a.tpf;
    return a.width <= MAX_SIDE && a.height <= MAX_SIDE && a.texels <= (long)INT32_MAX;
}

// what the kernels need of it
struct Packing { int R, cx; long cells, n_faces, width, height; };

Packing packing_of(const Atlas& a, int res, int64_t n_faces) { return {res, (int)a.cx, a.cells, (long)n_faces, a.width, a.height}; }

// t = j R - j (j - 1) / 2 + i: the row j of texel t by its quadratic, corrected in integers
DEV int row_start(int j, int R) { return j * R - j * (j - 1) / 2; }

DEV void texel_ij(int t, int R, int& i, int& j) {
    const float b = (float)(2 * R + 1);
    j = (int)((b - sqrtf(b * b - 8.f * (float)t)) * 0.5f);
    j = j < 0 ? 0 : j > R - 1 ? R - 1 : j;
    while (j > 0 && row_start(j, R) > t) --j;
    while (j < R - 1 && row_start(j + 1, R) <= t) ++j;
    i = t - row_start(j, R);
}

// the image texel of face f's texel (i, j)
DEV long image_texel(const Packing& p, long f, int i, int j) {
    const long q = f >> 1;
    const int x = (f & 1) ? p.R + 1 - i : i, y = (f & 1) ? p.R - 1 - j : j;
    return ((q / p.cx) * p.R + y) * p.width + (q % p.cx) * (p.R + 2) + x;
}

enum Owner { UNOWNED = 0, OWNED = 1, GUTTER = 3 };

// the packing inverted at image texel (X, Y) inside the image: OWNED with the row of the colour list, GUTTER or UNOWNED
DEV Owner owner_of(const Packing& p, long X, long Y, long& row) {
    const long q = (Y / p.R) * p.cx + X / (p.R + 2);
    if (q >= p.cells) return UNOWNED;
    const int x = (int)(X % (p.R + 2)), y = (int)(Y % p.R);
    if (x + y == p.R) return GUTTER;
    const bool odd = x + y > p.R;
    const long f = 2 * q + (odd ? 1 : 0);
    if (f >= p.n_faces) return UNOWNED;
    const int i = odd ? p.R + 1 - x : x, j = odd ? p.R - 1 - y : y;
    row = f * (long)(p.R * (p.R + 1) / 2) + row_start(j, p.R) + i;
    return OWNED;
}

DEV float nan_f() { return __int_as_float(0x7fc00000); }

// (wa a + wb b) + wc c, float64, rounded once
DEV float combine(double wa, double wb, double wc, float a, float b, float c) {
    return (float)((wa * (double)a + wb * (double)b) + wc * (double)c);
}

__global__ __launch_bounds__(THREADS) void atlas_texels_kernel(const Mesh m, const float* __restrict__ normals, const float* __restrict__ attrs,
                                                               int C, int R, long first_face, long n, float* points, float* out_normals,
                                                               float* out_attrs) {
    const long k = (long)blockIdx.x * THREADS + threadIdx.x;
    if (k >= n) return;
    const int tpf = R * (R + 1) / 2;
    const long f = first_face + k / tpf;
    int i, j;
    texel_ij((int)(k % tpf), R, i, j);
    const int32_t ia = m.faces[3 * f], ib = m.faces[3 * f + 1], ic = m.faces[3 * f + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= m.n_vertices || ib >= m.n_vertices || ic >= m.n_vertices) {
        for (int a = 0; a < 3; ++a) {
            if (points) points[3 * k + a] = nan_f();
            if (out_normals) out_normals[3 * k + a] = nan_f();
        }
        if (out_attrs)
            for (int c = 0; c < C; ++c) out_attrs[k * C + c] = nan_f();
        return;
    }
    const double d = (double)(R - 1);
    const double wb = (double)i / d, wc = (double)j / d, wa = (double)(R - 1 - i - j) / d;
    const float* pa = m.vertices + 3 * (long)ia;
    const float* pb = m.vertices + 3 * (long)ib;
    const float* pc = m.vertices + 3 * (long)ic;
    if (points)
        for (int a = 0; a < 3; ++a) points[3 * k + a] = combine(wa, wb, wc, pa[a], pb[a], pc[a]);
    if (out_normals) {
        if (normals) {
            const float* na = normals + 3 * (long)ia;
            const float* nb = normals + 3 * (long)ib;
            const float* nc = normals + 3 * (long)ic;
            for (int a = 0; a < 3; ++a) out_normals[3 * k + a] = combine(wa, wb, wc, na[a], nb[a], nc[a]);
        } else {
            const double u0 = (double)pb[0] - (double)pa[0], u1 = (double)pb[1] - (double)pa[1], u2 = (double)pb[2] - (double)pa[2];
            const double v0 = (double)pc[0] - (double)pa[0], v1 = (double)pc[1] - (double)pa[1], v2 = (double)pc[2] - (double)pa[2];
            out_normals[3 * k] = (float)(u1 * v2 - u2 * v1);
            out_normals[3 * k + 1] = (float)(u2 * v0 - u0 * v2);
            out_normals[3 * k + 2] = (float)(u0 * v1 - u1 * v0);
        }
    }
    if (out_attrs) {
        const float* aa = attrs + (long)ia * C;
        const float* ab = attrs + (long)ib * C;
        const float* ac = attrs + (long)ic * C;
        for (int c = 0; c < C; ++c) out_attrs[k * C + c] = combine(wa, wb, wc, aa[c], ab[c], ac[c]);
    }
}

struct Fill { float v[MAX_CH]; };

template <int C>
__global__ __launch_bounds__(THREADS) void atlas_pack_kernel(const Packing p, const float* __restrict__ colors, const uint8_t* __restrict__ views,
                                                             const Fill background, float* atlas, uint8_t* coverage) {
    const long at = (long)blockIdx.x * THREADS + threadIdx.x;
    if (at >= p.width * p.height) return;
    const long X = at % p.width, Y = at / p.width;
    long row = 0;
    const Owner own = owner_of(p, X, Y, row);
    float out[C];
    int cov = own;
    if (own == OWNED) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = colors[row * C + c];
        cov = (!views || views[row] != 0) ? 1 : 2;
    } else if (own == GUTTER) {
        // the left, upper, right and lower neighbours, in that order, whose owning face exists (none of them is a gutter texel)
        const long nx[4] = {X - 1, X, X + 1, X}, ny[4] = {Y, Y - 1, Y, Y + 1};
        double sum[C];
#pragma unroll
        for (int c = 0; c < C; ++c) sum[c] = 0.0;
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            long r = 0;
            if (nx[k] < 0 || nx[k] >= p.width || ny[k] < 0 || ny[k] >= p.height || owner_of(p, nx[k], ny[k], r) != OWNED) continue;
#pragma unroll
            for (int c = 0; c < C; ++c) sum[c] = sum[c] + (double)colors[r * C + c];
            ++n;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = n ? (float)(sum[c] / (double)n) : background.v[c];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = background.v[c];
    }
    if (atlas) {
#pragma unroll
        for (int c = 0; c < C; ++c) atlas[at * C + c] = out[c];
    }
    if (coverage) coverage[at] = (uint8_t)cov;
}

template <int C>
__global__ __launch_bounds__(THREADS) void atlas_shade_kernel(const Cams cams, const Mesh m, double z_near, int H, int W,
                                                              const int32_t* __restrict__ face_id, const Packing p,
                                                              const float* __restrict__ atlas, int filter, const Fill background, float* out) {
    const int view = blockIdx.y;
    const long hw = (long)H * W;
    const long px = (long)blockIdx.x * THREADS + threadIdx.x;
    if (px >= hw) return;
    float* o = out + ((long)view * hw + px) * C;
    const int32_t f = face_id[(long)view * hw + px];
    Setup8 s;
    bool ok = f >= 0 && f < m.n_faces && raster_setup(m, cams.cam[view], z_near, f, H, W, s) == FACE_OK;
    Edges e;
    if (ok) {
        e = s.edges_at((int)(px % W), (int)(px / W));
        ok = covers(s, e);                               // a face id that is not this pixel's: background
    }
    if (!ok) {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = background.v[c];
        return;
    }
    const Persp t = persp_of(s, e);
    const double ub = t.tb / t.q, uc = t.tc / t.q;
    const int R = p.R;
    const double top = (double)(R - 1);
    double ss = ub * top;
    ss = ss > 0.0 ? ss : 0.0;                            // (a NaN becomes 0)
    ss = ss < top ? ss : top;
    const double room = top - ss;
    double tt = uc * top;
    tt = tt > 0.0 ? tt : 0.0;
    tt = tt < room ? tt : room;
    int i0 = (int)floor(ss), j0 = (int)floor(tt);
    i0 = i0 < R - 1 ? i0 : R - 1;
    j0 = j0 < R - 1 - i0 ? j0 : R - 1 - i0;
    const double fs = ss - (double)i0, ft = tt - (double)j0;
    // the taps (i0 + di, j0 + dj) in the order (0,0), (1,0), (0,1), (1,1) and their weights; one of the four is not a tap (weight unused)
    const bool lower = fs + ft <= 1.0 || i0 + j0 >= R - 2;
    const double w[4] = {(1.0 - fs) - ft, lower ? fs : 1.0 - ft, lower ? ft : 1.0 - fs, (fs + ft) - 1.0};
    const bool tap[4] = {lower, true, true, !lower};
    double sum[C], den = 0.0, best_w = 0.0;
    long best = -1;
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = i0 + (k & 1), j = j0 + (k >> 1);
        if (!tap[k] || i + j > R - 1) continue;          // beyond the face's lattice: not read, its weight dropped
        const long at = image_texel(p, f, i, j);
        if (filter == GPNERF_ATLAS_NEAREST) {
            if (best < 0 || w[k] > best_w) { best = at; best_w = w[k]; }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) sum[c] = sum[c] + w[k] * (double)atlas[at * C + c];
            den = den + w[k];
        }
    }
    if (filter == GPNERF_ATLAS_NEAREST) {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = best >= 0 ? atlas[best * C + c] : background.v[c];   // (some tap is always read)
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = (float)(sum[c] / den);
    }
}

}  // namespace

extern "C" {

int gpnerf_atlas_layout(int64_t n_faces, int32_t res, int64_t* layout) {
    Atlas a;
    if (!layout || !atlas_of(n_faces, res, a)) return GPNERF_E_ARG;
    layout[GPNERF_ATLAS_CELLS_X] = a.cx;
    layout[GPNERF_ATLAS_CELLS_Y] = a.cy;
    layout[GPNERF_ATLAS_WIDTH] = a.width;
    layout[GPNERF_ATLAS_HEIGHT] = a.height;
    layout[GPNERF_ATLAS_TEXELS_PER_FACE] = a.tpf;
    layout[GPNERF_ATLAS_N_TEXELS] = a.texels;
    return GPNERF_OK;
}

int gpnerf_atlas_texels(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* normals,
                        const float* attrs, int32_t C, int32_t res, int64_t first_face, int64_t n_faces_here, float* points,
                        float* out_normals, float* out_attrs, void* stream) {
    Atlas a;
    if (!mesh_ok(vertices, n_vertices, faces, n_faces) || !atlas_of(n_faces, res, a)) return GPNERF_E_ARG;
    if (first_face < 0 || n_faces_here < 0 || first_face > n_faces || n_faces_here > n_faces - first_face) return GPNERF_E_ARG;
    if ((attrs || out_attrs) && (C < 1 || C > MAX_CH)) return GPNERF_E_ARG;
    if (out_attrs && !attrs && n_vertices > 0) return GPNERF_E_ARG;
    const long n = (long)n_faces_here * a.tpf;
    if (n == 0 || (!points && !out_normals && !out_attrs)) return GPNERF_OK;
    const Mesh m = {vertices, faces, (long)n_vertices, (long)n_faces};
    hipLaunchKernelGGL(atlas_texels_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, S_(stream), m, normals, attrs, (int)C, (int)res,
                       (long)first_face, n, points, out_normals, out_attrs);
    return launch_status();
}

int gpnerf_atlas_pack(const float* colors, const uint8_t* views, int64_t n_faces, int32_t res, int32_t C, const float* background,
                      float* atlas, uint8_t* coverage, void* stream) {
    Atlas a;
    if (!background || !atlas_of(n_faces, res, a) || C < 1 || C > MAX_CH || (!colors && a.texels > 0)) return GPNERF_E_ARG;
    const long n = a.width * a.height;
    if (n == 0 || (!atlas && !coverage)) return GPNERF_OK;
    const Packing p = packing_of(a, res, n_faces);
    Fill bg = {};
    for (int c = 0; c < C; ++c) bg.v[c] = background[c];
#define GPNERF_ATLAS_PACK_LAUNCH(CH)                                                                                                     \
    hipLaunchKernelGGL(atlas_pack_kernel<CH>, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, S_(stream), p, colors, views, bg, atlas, coverage)
    switch (C) {
        case 1: GPNERF_ATLAS_PACK_LAUNCH(1); break;
        case 2: GPNERF_ATLAS_PACK_LAUNCH(2); break;
        case 3: GPNERF_ATLAS_PACK_LAUNCH(3); break;
        default: GPNERF_ATLAS_PACK_LAUNCH(4); break;
    }
#undef GPNERF_ATLAS_PACK_LAUNCH
    return launch_status();
}

int gpnerf_atlas_shade(const int32_t* face_id, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                       const double* cams, int32_t n_views, int32_t H, int32_t W, double z_near, const float* atlas, int32_t res, int32_t C,
                       int32_t filter, const float* background, float* out, void* stream) {
    Atlas a;
    if (!face_id || !cams || !background || !out || !mesh_ok(vertices, n_vertices, faces, n_faces) || !atlas_of(n_faces, res, a))
        return GPNERF_E_ARG;
    if (n_views < 1 || n_views > RASTER_VIEWS || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || C < 1 || C > MAX_CH) return GPNERF_E_ARG;
    if ((!atlas && n_faces > 0) || (filter != GPNERF_ATLAS_SIMPLEX && filter != GPNERF_ATLAS_NEAREST)) return GPNERF_E_ARG;
    if (!(z_near > 0.0) || !(z_near < (double)INFINITY)) return GPNERF_E_ARG;             // zero, negative, NaN, infinite
    Cams c;
    cams_of(cams, n_views, c);
    const Mesh m = {vertices, faces, (long)n_vertices, (long)n_faces};
    const Packing p = packing_of(a, res, n_faces);
    Fill bg = {};
    for (int k = 0; k < C; ++k) bg.v[k] = background[k];
    const dim3 grid(blocks_for((int64_t)H * W, THREADS), (unsigned)n_views);
#define GPNERF_ATLAS_SHADE_LAUNCH(CH)                                                                                                    \
    hipLaunchKernelGGL(atlas_shade_kernel<CH>, grid, dim3(THREADS), 0, S_(stream), c, m, z_near, (int)H, (int)W, face_id, p, atlas, (int)filter, \
                       bg, out)
    switch (C) {
        case 1: GPNERF_ATLAS_SHADE_LAUNCH(1); break;
        case 2: GPNERF_ATLAS_SHADE_LAUNCH(2); break;
        case 3: GPNERF_ATLAS_SHADE_LAUNCH(3); break;
        default: GPNERF_ATLAS_SHADE_LAUNCH(4); break;
    }
#undef GPNERF_ATLAS_SHADE_LAUNCH
    return launch_status();
}

}  // extern "C"
