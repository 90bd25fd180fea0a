// gpnerf_fusion.hip -- fusing calibrated depth maps into a truncated signed distance field on a lattice (Curless and Levoy, 1996) on
// gfx950: every lattice point is projected into up to eight views as the rasteriser projects a vertex, reads the NEAREST depth pixel,
// and adds the truncated difference between that depth and its own camera z to a weighted running sum.  include/gpnerf_hip.h states THE
// DEFINITION operation for operation (gpnerf_fusion_integrate); DESIGN.md 4.20 the argument for each rule and what was measured.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone.
// No float atomics: a lattice point is one lane's, its views are summed by that lane in ascending order.  The only atomics are the
// integer sums of the counts -- one add per wavefront and counter in LDS, one per block and counter in memory --, into counters a
// kernel of this file zeroes first.
//
// Lane mapping: one lattice point per lane and step of a sweep over the lattice by at most 768 blocks of 512 lanes, consecutive lanes
// consecutive k (z fastest), so a wavefront's loads and stores of the state are three contiguous runs (512 + 512 + 64 bytes) and its
// 64 points project to a short run of pixels in every view.  The counts gather in LDS and reach memory once per block.  The
// views run in a loop inside the lane; the cameras travel in the kernel argument and are read through scalar loads (the view index
// is uniform).  The state form moves 17 bytes per point in and 17 out per call, and finalise 17 in and 4 out; the ONE-SHOT form is the
// same body with the sums kept in registers and writes 4 bytes per point (5 with the flag byte).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // S_, launch_status, blocks_for, sweep_blocks; wave_count, stat_add

constexpr int MAX_VIEWS = GPNERF_FUSION_MAX_VIEWS, THREADS = 256, MAX_SIDE = 16384;
constexpr int SWEEP = 512, SWEEP_GRID = 768;           // the sweeping kernels: lanes per block, and at most that many blocks (three per compute unit:
                                                        // the state form's 102 SGPRs allow 7 wavefronts per SIMD, a block is 2)
constexpr int FATES = GPNERF_FUSION_FATES, TOTALS = GPNERF_FUSION_TOTALS;
constexpr double MAX_BAND_STEPS = (double)GPNERF_SDF_MAX_BAND_STEPS;
constexpr int64_t MAX_POINTS = (int64_t)1 << 28;         // gpnerf_mesh_sdf's limit, marching cubes'

struct Views { double cam[MAX_VIEWS][21]; };             // K 3x3 row-major, RT 3x4 row-major: gpnerf_mesh_rasterize's layout
struct Lattice {
    double lo[3], step[3];
    int n[3];
};

bool dims_ok(const int32_t* dims) {
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
    const int64_t xy = (int64_t)dims[0] * dims[1];       // (< 2^62)
    return xy <= MAX_POINTS && xy * dims[2] <= MAX_POINTS;
}

bool lattice_ok(const double* lattice) {
    if (!lattice) return false;
    for (int a = 0; a < 3; ++a) {
        if (!(fabs(lattice[a]) < (double)INFINITY)) return false;                              // NaN, infinite
        if (!(lattice[3 + a] > 0.0) || !(lattice[3 + a] < (double)INFINITY)) return false;     // zero, negative, NaN, infinite
    }
    return true;
}

bool band_ok(float band, const double* lattice) {        // gpnerf_mesh_sdf's rule
    const double least = fmin(lattice[3], fmin(lattice[4], lattice[5]));
    return band > 0.f && (double)band <= MAX_BAND_STEPS * least;                               // (false for a NaN; an infinite band fails the second)
}

bool views_ok(const double* cams, int n_views, int H, int W, double z_near, int carve) {
    return cams && n_views >= 1 && n_views <= MAX_VIEWS && H >= 1 && H <= MAX_SIDE && W >= 1 && W <= MAX_SIDE && z_near > 0.0 &&
           z_near < (double)INFINITY && (carve == 0 || carve == 1);
}

int64_t points_of(const int32_t* dims) { return (int64_t)dims[0] * dims[1] * dims[2]; }

// the counters are zeroed by a kernel of the library's own: no memset node in a captured graph
__global__ __launch_bounds__(64) void fusion_zero_kernel(long long* a, int na, long long* b, int nb) {
    const int t = threadIdx.x;
    if (a && t < na) a[t] = 0;
    if (b && t < nb) b[t] = 0;
}

__global__ __launch_bounds__(THREADS) void fusion_reset_kernel(double* sum, double* weight, uint8_t* flags, long n) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    sum[i] = 0.0;
    weight[i] = 0.0;
    flags[i] = 0;
}

// Finalise, per point: the value and which of the totals it counts under (bit 0: weight > 0, bit 1: the NEAR bit, bit 2: interior
// filled, bit 3: unknown)
DEV float finalise_point(double sum, double weight, unsigned flags, float band, unsigned& kind) {
    kind = (flags & GPNERF_FUSION_FLAG_NEAR) ? 2u : 0u;
    if (weight > 0.0) {
        kind |= 1u;
        const float v = (float)(sum / weight);
        return fminf(fmaxf(v, -band), band);
    }
    if (flags & GPNERF_FUSION_FLAG_HIDDEN) {
        kind |= 4u;
        return -band;
    }
    kind |= 8u;
    return band;
}

// The counts go through the block: a wavefront adds its wave_count to a counter in LDS (one integer add per wavefront and counter),
// and the block adds what it gathered to the counters in memory once, when it has swept its share of the lattice.  A global add per
// wavefront and counter was measured at 15 x the rest of the kernel on the body lattice: every add of a counter
// meets every other at one address.
constexpr int COUNTERS = FATES * MAX_VIEWS + TOTALS;    // [view][fate], then the totals

DEV void counters_clear(unsigned* counts) {
    for (int t = threadIdx.x; t < COUNTERS; t += SWEEP) counts[t] = 0u;
    __syncthreads();
}

// every lane of the wavefront reaches this
DEV void count_in_block(unsigned* counts, int which, bool flag) {
    const int cnt = wave_count(flag);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(counts + which, (unsigned)cnt);
}

// every lane of the block reaches this
DEV void counters_flush(const unsigned* counts, int first, int n, long long* out) {
    __syncthreads();
    const int t = threadIdx.x;
    if (out && t < n) stat_add(out, t, (long long)counts[first + t]);
}

// the lattice is swept in steps of the whole grid: step `base` gives lane t point base + t, so consecutive lanes are consecutive k
DEV long sweep_first() { return (long)blockIdx.x * SWEEP; }
DEV long sweep_stride() { return (long)gridDim.x * SWEEP; }

// THE DEFINITION's integration of n_views views into a point's sums.  ONESHOT: the sums start at zero in registers and go straight
// through finalise; otherwise they are loaded from and stored to the state.
template <bool ONESHOT>
__global__ __launch_bounds__(SWEEP) void fusion_integrate_kernel(const Views views, int n_views, const float* __restrict__ depth,
                                                                 const float* __restrict__ weights, int H, int W, const Lattice g,
                                                                 float band, double z_near, int carve, double* sum, double* weight,
                                                                 uint8_t* flags, float* sdf, long long* stats, long long* totals) {
    __shared__ unsigned counts[COUNTERS];
    counters_clear(counts);
    const long n = (long)g.n[0] * g.n[1] * g.n[2];
    const double b = (double)band;
    const long hw = (long)H * W;
    for (long base = sweep_first(); base < n; base += sweep_stride()) {       // (uniform in the block)
        const long i = base + threadIdx.x;
        const bool live = i < n;
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, acc = 0.0, den = 0.0;
        unsigned bits = 0u;
        if (live) {
            const int iz = (int)(i % g.n[2]);
            const long ij = i / g.n[2];
            const int iy = (int)(ij % g.n[1]), ix = (int)(ij / g.n[1]);
            // lattice point (ix, iy, iz): the product and the sum in float64, one rounding to float32, widened again
            p0 = (double)(float)(g.lo[0] + (double)ix * g.step[0]);
            p1 = (double)(float)(g.lo[1] + (double)iy * g.step[1]);
            p2 = (double)(float)(g.lo[2] + (double)iz * g.step[2]);
            if (!ONESHOT) { acc = sum[i]; den = weight[i]; bits = flags[i]; }
        }
        for (int v = 0; v < n_views; ++v) {              // (uniform: every lane of the wavefront reaches the counts)
            int fate = -1;
            if (live) {
                // gpnerf_mesh_rasterize's projection of a vertex (float64, multiply then add, unfused)
                const double* K = views.cam[v];
                const double* RT = views.cam[v] + 9;
                const double c0 = ((p0 * RT[0] + p1 * RT[1]) + p2 * RT[2]) + RT[3];
                const double c1 = ((p0 * RT[4] + p1 * RT[5]) + p2 * RT[6]) + RT[7];
                const double c2 = ((p0 * RT[8] + p1 * RT[9]) + p2 * RT[10]) + RT[11];
                const double h0 = (c0 * K[0] + c1 * K[1]) + c2 * K[2];
                const double h1 = (c0 * K[3] + c1 * K[4]) + c2 * K[5];
                const double z = (c0 * K[6] + c1 * K[7]) + c2 * K[8];
                const double x = h0 / z, y = h1 / z;
                // (every comparison is false for a NaN)
                if (!(z >= z_near && z < (double)INFINITY && fabs(x) < (double)INFINITY && fabs(y) < (double)INFINITY)) fate = GPNERF_FUSION_BEHIND;
                else if (!(x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1))) fate = GPNERF_FUSION_OUTSIDE;
                else {
                    const long pixel = (long)v * hw + (long)rint(y) * W + (long)rint(x);      // rint: half to even
                    const float d = depth[pixel];
                    const float wf = weights ? weights[pixel] : 1.f;
                    const double w = (double)wf;
                    const bool background = d == INFINITY;
                    if (!(d > 0.f) || !(wf > 0.f) || !(wf < INFINITY) || (background && !carve)) fate = GPNERF_FUSION_NODATA;
                    else {
                        double t = b;
                        if (background) fate = GPNERF_FUSION_EMPTY;
                        else {
                            const double s = (double)d - z;
                            if (s < -b) { fate = GPNERF_FUSION_HIDDEN; bits |= GPNERF_FUSION_FLAG_HIDDEN; }
                            else if (s >= b) fate = GPNERF_FUSION_EMPTY;
                            else { fate = GPNERF_FUSION_NEAR; bits |= GPNERF_FUSION_FLAG_NEAR; t = s; }
                        }
                        if (fate != GPNERF_FUSION_HIDDEN) {
                            acc = acc + w * t;
                            den = den + w;
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < FATES; ++k) count_in_block(counts, FATES * v + k, fate == k);
        }
        unsigned kind = 0u;
        if (live) {
            if (ONESHOT) {
                sdf[i] = finalise_point(acc, den, bits, band, kind);
                if (flags) flags[i] = (uint8_t)bits;
            } else {
                sum[i] = acc;
                weight[i] = den;
                flags[i] = (uint8_t)bits;
            }
        }
        if (ONESHOT) {
#pragma unroll
            for (int k = 0; k < TOTALS; ++k) count_in_block(counts, FATES * MAX_VIEWS + k, live && (kind >> k & 1u));
        }
    }
    counters_flush(counts, 0, FATES * n_views, stats);
    if (ONESHOT) counters_flush(counts, FATES * MAX_VIEWS, TOTALS, totals);
}

__global__ __launch_bounds__(SWEEP) void fusion_finalise_kernel(const double* __restrict__ sum, const double* __restrict__ weight,
                                                                const uint8_t* __restrict__ flags, long n, float band, float* sdf,
                                                                long long* totals) {
    __shared__ unsigned counts[COUNTERS];
    counters_clear(counts);
    for (long base = sweep_first(); base < n; base += sweep_stride()) {
        const long i = base + threadIdx.x;
        const bool live = i < n;
        unsigned kind = 0u;
        if (live) sdf[i] = finalise_point(sum[i], weight[i], flags[i], band, kind);
#pragma unroll
        for (int k = 0; k < TOTALS; ++k) count_in_block(counts, FATES * MAX_VIEWS + k, live && (kind >> k & 1u));
    }
    counters_flush(counts, FATES * MAX_VIEWS, TOTALS, totals);
}

Views views_of(const double* cams, int n_views) {
    Views vw = {};
    for (int v = 0; v < n_views; ++v)
        for (int e = 0; e < 21; ++e) vw.cam[v][e] = cams[21 * v + e];
    return vw;
}

Lattice lattice_of(const double* lattice, const int32_t* dims) {
    Lattice g;
    for (int a = 0; a < 3; ++a) { g.lo[a] = lattice[a]; g.step[a] = lattice[3 + a]; g.n[a] = dims[a]; }
    return g;
}

}  // namespace

extern "C" {

int gpnerf_fusion_reset(const int32_t* dims, double* sum, double* weight, uint8_t* flags, void* stream) {
    if (!dims_ok(dims) || !sum || !weight || !flags) return GPNERF_E_ARG;
    const int64_t n = points_of(dims);
    hipLaunchKernelGGL(fusion_reset_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, S_(stream), sum, weight, flags, (long)n);
    return launch_status();
}

int gpnerf_fusion_integrate(const float* depth, const float* weights, const double* cams, int32_t n_views, int32_t H, int32_t W,
                            const double* lattice, const int32_t* dims, float band, double z_near, int32_t carve, double* sum,
                            double* weight, uint8_t* flags, int64_t* stats, void* stream) {
    if (!depth || !sum || !weight || !flags || !stats || !views_ok(cams, n_views, H, W, z_near, carve) || !dims_ok(dims) ||
        !lattice_ok(lattice) || !band_ok(band, lattice))
        return GPNERF_E_ARG;
    long long* st = reinterpret_cast<long long*>(stats);
    hipLaunchKernelGGL(fusion_zero_kernel, dim3(1), dim3(64), 0, S_(stream), st, FATES * (int)n_views, (long long*)nullptr, 0);
    hipLaunchKernelGGL(fusion_integrate_kernel<false>, dim3(sweep_blocks(points_of(dims), SWEEP, SWEEP_GRID)), dim3(SWEEP), 0, S_(stream),
                       views_of(cams, n_views), (int)n_views, depth, weights, (int)H, (int)W, lattice_of(lattice, dims), band, z_near,
                       (int)carve, sum, weight, flags, (float*)nullptr, st, (long long*)nullptr);
    return launch_status();
}

int gpnerf_fusion_finalise(const double* sum, const double* weight, const uint8_t* flags, const int32_t* dims, float band, float* sdf,
                           int64_t* totals, void* stream) {
    if (!sum || !weight || !flags || !sdf || !totals || !dims_ok(dims) || !(band > 0.f) || !(band < INFINITY)) return GPNERF_E_ARG;
    long long* tot = reinterpret_cast<long long*>(totals);
    const int64_t n = points_of(dims);
    hipLaunchKernelGGL(fusion_zero_kernel, dim3(1), dim3(64), 0, S_(stream), tot, TOTALS, (long long*)nullptr, 0);
    hipLaunchKernelGGL(fusion_finalise_kernel, dim3(sweep_blocks(n, SWEEP, SWEEP_GRID)), dim3(SWEEP), 0, S_(stream), sum, weight, flags, (long)n, band,
                       sdf, tot);
    return launch_status();
}

int gpnerf_fusion_oneshot(const float* depth, const float* weights, const double* cams, int32_t n_views, int32_t H, int32_t W,
                          const double* lattice, const int32_t* dims, float band, double z_near, int32_t carve, float* sdf, uint8_t* flags,
                          int64_t* stats, int64_t* totals, void* stream) {
    if (!depth || !sdf || !stats || !totals || !views_ok(cams, n_views, H, W, z_near, carve) || !dims_ok(dims) || !lattice_ok(lattice) ||
        !band_ok(band, lattice))
        return GPNERF_E_ARG;
    long long* st = reinterpret_cast<long long*>(stats);
    long long* tot = reinterpret_cast<long long*>(totals);
    hipLaunchKernelGGL(fusion_zero_kernel, dim3(1), dim3(64), 0, S_(stream), st, FATES * (int)n_views, tot, TOTALS);
    hipLaunchKernelGGL(fusion_integrate_kernel<true>, dim3(sweep_blocks(points_of(dims), SWEEP, SWEEP_GRID)), dim3(SWEEP), 0, S_(stream),
                       views_of(cams, n_views), (int)n_views, depth, weights, (int)H, (int)W, lattice_of(lattice, dims), band, z_near,
                       (int)carve, (double*)nullptr, (double*)nullptr, flags, sdf, st, tot);
    return launch_status();
}

}  // extern "C"
