// gpnerf_raycast.hip -- casting rays against a triangle mesh on gfx950: the nearest hit (or any hit) of each ray of a list, through
// the uniform cell grid gpnerf_mesh_grid_build left behind or against every face, and the rays through the pixel centres of
// calibrated cameras.  include/gpnerf_hip.h states THE INTERSECTION, the walk, its margins and their proof.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone.
// No atomics at all: a ray is one lane's, and the one reduction (the faces' largest cell span) is a tree in LDS whose partial
// results every workgroup of the walk folds again for itself.
//
// Lane mapping: one ray per lane in both forms.  The renderer's rays arrive patch-ordered (4 x 8 or 32 x 8 pixel patches), so the 64
// rays of a wavefront enter the grid side by side and walk neighbouring cells: their slab counts differ by a few, the entries they
// read share cache lines.  A wavefront per ray with the lanes over a cell's entries would idle: a cell of a body-sized mesh holds
// 3 - 6 entries.  The brute-force form stages the faces through LDS in tiles of 256 (nine floats and a flag per face, read by every
// lane at the same address: a broadcast, no bank conflict) as distance_brute_kernel does.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for
#include "gpnerf_tridist.h"    // V3, sub, load3, finite3, face_valid: the mesh's validity rule
#include "gpnerf_meshgrid.h"   // Grid, grid_of, cell_of: the grid's layout
#include "gpnerf_raytri.h"     // Ray, RayAxes, RayBest, ray_triangle, test_ray_face: THE intersection and its tie rule

constexpr int THREADS = 256;
constexpr int TILE = 256;                                // faces per LDS tile of the brute-force form
constexpr int64_t MAX_FACES = INT32_MAX;
constexpr double PAD_CELLS = 1.0 / 2048.0;               // 2^-11 of a cell: the cell function's rounding (under 2^-12), doubled
constexpr double PAD_REL = 1.0 / 1048576.0;              // 2^-20 = 16 * 2^-24: the intersection's own error (under 10 * 2^-24), relative to R

DEV void write_ray(long i, float t, int32_t f, float wb, float wc, float* t_out, int32_t* face_out, float* bary) {
    t_out[i] = t;
    face_out[i] = f;
    if (bary) { bary[2 * i] = wb; bary[2 * i + 1] = wc; }
}

// what a ray's result is once the search is over.  NEAREST: the best face's t and weights, +inf / -1 / NaN without one.  ANY: 0 for
// a ray some face stops, +inf for a free one, the face that was found first, no weights.
template <bool ANY>
DEV void write_result(long i, const RayBest& best, float* t_out, int32_t* face_out, float* bary) {
    const bool hit = best.f >= 0;
    if (ANY) write_ray(i, hit ? 0.f : inff_(), best.f, nanf_(), nanf_(), t_out, face_out, bary);
    else write_ray(i, hit ? best.t : inff_(), best.f, hit ? best.wb : nanf_(), hit ? best.wc : nanf_(), t_out, face_out, bary);
}

// ---------------------------------------------------------------- every face

template <bool ANY>
__global__ __launch_bounds__(THREADS) void raycast_brute_kernel(const float* __restrict__ rays, long n_rays, const float* __restrict__ vertices,
                                                                int64_t n_vertices, const int32_t* __restrict__ faces, long n_faces,
                                                                float* t_out, int32_t* face_out, float* bary) {
    __shared__ float s_v[9][TILE];
    __shared__ int s_ok[TILE];
    const int t = threadIdx.x;
    const long i = (long)blockIdx.x * THREADS + t;
    const bool live = i < n_rays;
    const Ray r = live ? load_ray(rays, i) : Ray{{0.f, 0.f, 0.f}, {0.f, 0.f, 1.f}, 0.f, 0.f};
    const bool valid = live && ray_valid(r);
    const RayAxes k = ray_axes(valid ? r.d : V3{0.f, 0.f, 1.f});
    RayBest best = {inff_(), -1, nanf_(), nanf_()};
    bool done = !valid;                                  // such a lane only helps to stage
    for (long f0 = 0; f0 < n_faces; f0 += TILE) {
        __syncthreads();                                 // the previous tile has been read
        V3 a = {0.f, 0.f, 0.f}, b = a, c = a;
        const bool ok = f0 + t < n_faces && face_valid(vertices, n_vertices, faces, f0 + t, a, b, c);
        s_v[0][t] = a.x; s_v[1][t] = a.y; s_v[2][t] = a.z; s_v[3][t] = b.x; s_v[4][t] = b.y; s_v[5][t] = b.z;
        s_v[6][t] = c.x; s_v[7][t] = c.y; s_v[8][t] = c.z;
        s_ok[t] = ok;
        __syncthreads();
        if (done) continue;
        const int m = (int)min((long)TILE, n_faces - f0);
        for (int j = 0; j < m; ++j) {
            if (!s_ok[j]) continue;                      // (uniform: every lane reads the same word)
            const bool hit = test_ray_face(best, r, k, V3{s_v[0][j], s_v[1][j], s_v[2][j]}, V3{s_v[3][j], s_v[4][j], s_v[5][j]},
                                           V3{s_v[6][j], s_v[7][j], s_v[8][j]}, (int32_t)(f0 + j));
            if (ANY && hit) { done = true; break; }
        }
    }
    if (!live) return;
    if (!valid) write_ray(i, nanf_(), -1, nanf_(), nanf_(), t_out, face_out, bary);
    else write_result<ANY>(i, best, t_out, face_out, bary);
}

// ---------------------------------------------------------------- through the grid

// the largest number of cell steps any valid face spans on each axis (cell(max corner) - cell(min corner), the build's own range):
// one partial maximum per workgroup, left in the first three words of the workgroup's row of the grid's partial boxes -- a region
// the build has finished with -- for the walk to fold.  A grid that is not OK is not touched.
__global__ __launch_bounds__(THREADS) void raycast_span_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                               const int32_t* __restrict__ faces, long n_faces, void* workspace) {
    __shared__ int s_span[3][THREADS];
    const int32_t* hdr = static_cast<const int32_t*>(workspace);
    if (hdr[GPNERF_GRID_HDR_MAGIC] != GRID_MAGIC || hdr[GPNERF_GRID_HDR_STATUS] != GPNERF_GRID_OK) return;        // (uniform)
    const Grid g = grid_of(workspace, hdr[GPNERF_GRID_HDR_CELL_CAP], hdr[GPNERF_GRID_HDR_ENTRY_CAP]);
    const int t = threadIdx.x;
    const long stride = (long)gridDim.x * THREADS;
    int span[3] = {0, 0, 0};
    for (long f = (long)blockIdx.x * THREADS + t; f < n_faces; f += stride) {
        V3 a, b, c;
        if (!face_valid(vertices, n_vertices, faces, f, a, b, c)) continue;
        const float mn[3] = {fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z))};
        const float mx[3] = {fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z))};
        for (int k = 0; k < 3; ++k) {
            const float lo = __int_as_float(hdr[GPNERF_GRID_HDR_LO + k]), inv = __int_as_float(hdr[GPNERF_GRID_HDR_INV + k]);
            const int n = hdr[GPNERF_GRID_HDR_CELLS + k];
            span[k] = max(span[k], cell_of(mx[k], lo, inv, n) - cell_of(mn[k], lo, inv, n));
        }
    }
    for (int k = 0; k < 3; ++k) s_span[k][t] = span[k];
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < 3; ++k) s_span[k][t] = max(s_span[k][t], s_span[k][t + s]);
        __syncthreads();
    }
    if (t < 3) reinterpret_cast<int32_t*>(g.part)[8 * blockIdx.x + t] = s_span[t][0];
}

DEV double sel3(double a0, double a1, double a2, int k) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }
DEV int sel3(int a0, int a1, int a2, int k) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }
// floor, clamped to [0, n - 1] in double (no int overflow; a NaN gives 0)
DEV int cell_clamp(double x, int n) { return (int)fmin(fmax(floor(x), 0.0), (double)(n - 1)); }

// The walk (include/gpnerf_hip.h, THE WALK): slab by slab along z = the axis of the largest |d|, front to back; in a slab the
// rectangle of cells the ray's padded extent covers on the other two axes; it stops once the slab ahead lies more than `span`
// slabs behind the slab of min(tmax, best).  The walk's own arithmetic is float64.
template <bool ANY>
__global__ __launch_bounds__(THREADS) void raycast_grid_kernel(const float* __restrict__ rays, long n_rays, const float* __restrict__ vertices,
                                                               int64_t n_vertices, const int32_t* __restrict__ faces, long n_faces,
                                                               void* workspace, int n_parts, float* t_out, int32_t* face_out, float* bary) {
    __shared__ int s_span[3][THREADS];
    const int32_t* hdr = static_cast<const int32_t*>(workspace);
    const bool grid_ok = hdr[GPNERF_GRID_HDR_MAGIC] == GRID_MAGIC && hdr[GPNERF_GRID_HDR_STATUS] == GPNERF_GRID_OK;  // (uniform)
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * THREADS + tid;
    if (!grid_ok) {                                      // a half-built grid is never read
        if (i < n_rays) write_ray(i, nanf_(), -1, nanf_(), nanf_(), t_out, face_out, bary);
        return;
    }
    const Grid g = grid_of(workspace, hdr[GPNERF_GRID_HDR_CELL_CAP], hdr[GPNERF_GRID_HDR_ENTRY_CAP]);
    {   // the faces' largest spans, from raycast_span_kernel's partial maxima
        const int32_t* part = reinterpret_cast<const int32_t*>(g.part);
        int span[3] = {0, 0, 0};
        for (int p = tid; p < n_parts; p += THREADS)
            for (int k = 0; k < 3; ++k) span[k] = max(span[k], part[8 * p + k]);
        for (int k = 0; k < 3; ++k) s_span[k][tid] = span[k];
        __syncthreads();
        for (int s = THREADS / 2; s > 0; s >>= 1) {
            if (tid < s)
                for (int k = 0; k < 3; ++k) s_span[k][tid] = max(s_span[k][tid], s_span[k][tid + s]);
            __syncthreads();
        }
    }
    if (i >= n_rays) return;
    const Ray r = load_ray(rays, i);
    if (!ray_valid(r)) {
        write_ray(i, nanf_(), -1, nanf_(), nanf_(), t_out, face_out, bary);
        return;
    }
    const RayAxes k = ray_axes(r.d);
    const int n0 = hdr[GPNERF_GRID_HDR_CELLS], n1 = hdr[GPNERF_GRID_HDR_CELLS + 1], n2 = hdr[GPNERF_GRID_HDR_CELLS + 2];
    // per axis, in cells: the origin, the direction, the cell count; R bounds |vertex - origin| on every axis for every valid vertex
    double rho[3], drho[3], cs[3], R = 0.0;
    const float oc[3] = {r.o.x, r.o.y, r.o.z}, dc[3] = {r.d.x, r.d.y, r.d.z};
    const int nc[3] = {n0, n1, n2};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cs[a] = (double)__int_as_float(hdr[GPNERF_GRID_HDR_SIZE + a]);
        const double rel = (double)oc[a] - (double)__int_as_float(hdr[GPNERF_GRID_HDR_LO + a]);
        rho[a] = rel / cs[a];
        drho[a] = (double)dc[a] / cs[a];
        R = fmax(R, fabs(rel) + 1.001 * (double)nc[a] * cs[a]);
    }
    double pad[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) pad[a] = PAD_REL * R / cs[a] + PAD_CELLS;
    // the ray's parameter interval inside the padded box
    double b0 = -INFINITY, b1 = INFINITY;
    bool outside = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = -pad[a], hi = (double)nc[a] + pad[a];
        if (drho[a] == 0.0) {
            outside = outside || rho[a] < lo || rho[a] > hi;
        } else {
            const double sa = (lo - rho[a]) / drho[a], sb = (hi - rho[a]) / drho[a];
            b0 = fmax(b0, fmin(sa, sb));
            b1 = fmin(b1, fmax(sa, sb));
        }
    }
    RayBest best = {inff_(), -1, nanf_(), nanf_()};
    if (!outside && b0 <= b1) {
        const int az = k.kz, ax = az == 2 ? 0 : az + 1, ay = ax == 2 ? 0 : ax + 1;
        const int nz = sel3(n0, n1, n2, az), nx = sel3(n0, n1, n2, ax), ny = sel3(n0, n1, n2, ay);
        const int stz = sel3(n1 * n2, n2, 1, az), stx = sel3(n1 * n2, n2, 1, ax), sty = sel3(n1 * n2, n2, 1, ay);
        const double rz = sel3(rho[0], rho[1], rho[2], az), rx = sel3(rho[0], rho[1], rho[2], ax), ry = sel3(rho[0], rho[1], rho[2], ay);
        const double dz = sel3(drho[0], drho[1], drho[2], az), dx = sel3(drho[0], drho[1], drho[2], ax), dy = sel3(drho[0], drho[1], drho[2], ay);
        const double pz = sel3(pad[0], pad[1], pad[2], az), px = sel3(pad[0], pad[1], pad[2], ax), py = sel3(pad[0], pad[1], pad[2], ay);
        const double span = (double)s_span[az][0];
        // zeta: the z coordinate in cells, counted in the ray's direction of travel, so that it grows with the parameter
        const bool up = dz > 0.0;
        const double z0 = up ? rz : (double)nz - rz, dzeta = fabs(dz);
        const double first = fmax(fmax(floor(z0 + b0 * dzeta - pz), floor(z0 + (double)r.tmin * dzeta - pz) - span), 0.0);
        const double last = fmin(floor(z0 + b1 * dzeta + pz), (double)(nz - 1));
        if (first <= last) {                             // (both in [0, nz - 1] now)
            for (int j = (int)first; j <= (int)last; ++j) {
                if ((double)j > floor(z0 + (double)fminf(r.tmax, best.t) * dzeta + pz) + span) break;
                const int c = up ? j : nz - 1 - j;
                // the parameters at which the ray crosses the slab's padded planes, and its extent on the other axes between them
                const double sa = ((double)c - PAD_CELLS - rz) / dz, sb = ((double)(c + 1) + PAD_CELLS - rz) / dz;
                const double xa = rx + sa * dx, xb = rx + sb * dx, ya = ry + sa * dy, yb = ry + sb * dy;
                const int cx0 = cell_clamp(fmin(xa, xb) - px, nx), cx1 = cell_clamp(fmax(xa, xb) + px, nx);
                const int cy0 = cell_clamp(fmin(ya, yb) - py, ny), cy1 = cell_clamp(fmax(ya, yb) + py, ny);
                bool stop = false;
                for (int cx = cx0; cx <= cx1 && !stop; ++cx)
                    for (int cy = cy0; cy <= cy1 && !stop; ++cy) {
                        const int cell = c * stz + cx * stx + cy * sty;
                        const int32_t s = g.start[cell], e = g.start[cell + 1];
                        for (int32_t q = s; q < e; ++q) {
                            const int32_t f = g.entries[q];
                            V3 a, b, cc;
                            if ((uint32_t)f < (uint32_t)n_faces && face_valid(vertices, n_vertices, faces, f, a, b, cc) &&
                                test_ray_face(best, r, k, a, b, cc, f) && ANY) {
                                stop = true;
                                break;
                            }
                        }
                    }
                if (stop) break;
            }
        }
    }
    write_result<ANY>(i, best, t_out, face_out, bary);
}

// ---------------------------------------------------------------- camera rays

struct PixelCam { double Kinv[9], Rinv[9], o[3]; };
struct PixelCams { PixelCam v[GPNERF_RAYCAST_MAX_VIEWS]; };

// inverse = adjugate / determinant, the determinant along the first row: include/gpnerf_hip.h (gpnerf_pixel_rays) states the order
bool invert3(const double* m, double* inv) {
    const double c[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                         m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                         m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
    const double det = (m[0] * c[0] + m[1] * c[3]) + m[2] * c[6];
    if (!(det != 0.0) || !isfinite(det)) return false;
    for (int i = 0; i < 9; ++i) inv[i] = c[i] / det;
    return true;
}

__global__ __launch_bounds__(THREADS) void pixel_rays_kernel(PixelCams cams, int n_views, int H, int W, float z_near, float* rays) {
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    const long per = (long)H * W;
    if (p >= per * n_views) return;
    const int view = (int)(p / per);
    const long q = p - view * per;
    const double col = (double)(q % W), row = (double)(q / W);
    const PixelCam& cam = cams.v[view];
    const double c0 = (cam.Kinv[0] * col + cam.Kinv[1] * row) + cam.Kinv[2], c1 = (cam.Kinv[3] * col + cam.Kinv[4] * row) + cam.Kinv[5],
                 c2 = (cam.Kinv[6] * col + cam.Kinv[7] * row) + cam.Kinv[8];
    const double u = c0 / c2, v = c1 / c2;
    float* out = rays + 8 * p;
    for (int a = 0; a < 3; ++a) {
        out[a] = (float)cam.o[a];
        out[3 + a] = (float)((cam.Rinv[3 * a] * u + cam.Rinv[3 * a + 1] * v) + cam.Rinv[3 * a + 2]);
    }
    out[6] = z_near;
    out[7] = inff_();
}

}  // namespace

extern "C" {

int gpnerf_mesh_raycast(const float* rays, int64_t n_rays, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                        void* grid_workspace, int32_t mode, float* t, int32_t* face, float* bary, void* stream) {
    if (n_rays < 0 || n_rays > (int64_t)INT32_MAX * THREADS || n_vertices < 0 || n_faces < 1 || n_faces > MAX_FACES || !vertices || !faces)
        return GPNERF_E_ARG;
    if (mode != GPNERF_RAYCAST_NEAREST && mode != GPNERF_RAYCAST_ANY) return GPNERF_E_ARG;
    if (n_rays == 0) return GPNERF_OK;
    if (!rays || !t || !face) return GPNERF_E_ARG;
    const unsigned blocks = blocks_for(n_rays, THREADS);
    const bool any = mode == GPNERF_RAYCAST_ANY;
    if (grid_workspace) {
        const int parts = (int)((n_faces + THREADS - 1) / THREADS < BOX_BLOCKS_MAX ? (n_faces + THREADS - 1) / THREADS : BOX_BLOCKS_MAX);
        hipLaunchKernelGGL(raycast_span_kernel, dim3((unsigned)parts), dim3(THREADS), 0, S_(stream), vertices, n_vertices, faces, (long)n_faces,
                           grid_workspace);
        if (any)
            hipLaunchKernelGGL(raycast_grid_kernel<true>, dim3(blocks), dim3(THREADS), 0, S_(stream), rays, (long)n_rays, vertices, n_vertices,
                               faces, (long)n_faces, grid_workspace, parts, t, face, bary);
        else
            hipLaunchKernelGGL(raycast_grid_kernel<false>, dim3(blocks), dim3(THREADS), 0, S_(stream), rays, (long)n_rays, vertices, n_vertices,
                               faces, (long)n_faces, grid_workspace, parts, t, face, bary);
    } else if (any) {
        hipLaunchKernelGGL(raycast_brute_kernel<true>, dim3(blocks), dim3(THREADS), 0, S_(stream), rays, (long)n_rays, vertices, n_vertices, faces,
                           (long)n_faces, t, face, bary);
    } else {
        hipLaunchKernelGGL(raycast_brute_kernel<false>, dim3(blocks), dim3(THREADS), 0, S_(stream), rays, (long)n_rays, vertices, n_vertices, faces,
                           (long)n_faces, t, face, bary);
    }
    return launch_status();
}

int gpnerf_pixel_rays(const double* cams, int32_t n_views, int32_t H, int32_t W, double z_near, float* rays, void* stream) {
    if (!cams || !rays || n_views < 1 || n_views > GPNERF_RAYCAST_MAX_VIEWS || H < 1 || H > 16384 || W < 1 || W > 16384) return GPNERF_E_ARG;
    if (!(z_near > 0.0) || !isfinite(z_near)) return GPNERF_E_ARG;
    PixelCams pc = {};
    for (int v = 0; v < n_views; ++v) {
        const double* K = cams + 21 * v;
        const double* RT = K + 9;
        const double Rm[9] = {RT[0], RT[1], RT[2], RT[4], RT[5], RT[6], RT[8], RT[9], RT[10]};
        const double T[3] = {RT[3], RT[7], RT[11]};
        PixelCam& c = pc.v[v];
        if (!invert3(K, c.Kinv) || !invert3(Rm, c.Rinv)) return GPNERF_E_ARG;
        for (int a = 0; a < 3; ++a) c.o[a] = -((c.Rinv[3 * a] * T[0] + c.Rinv[3 * a + 1] * T[1]) + c.Rinv[3 * a + 2] * T[2]);
    }
    const int64_t total = (int64_t)n_views * H * W;
    hipLaunchKernelGGL(pixel_rays_kernel, dim3(blocks_for(total, THREADS)), dim3(THREADS), 0, S_(stream), pc, (int)n_views, (int)H, (int)W,
                       (float)z_near, rays);
    return launch_status();
}

}  // extern "C"
