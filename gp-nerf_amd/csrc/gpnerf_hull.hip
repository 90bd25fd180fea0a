// gpnerf_hull.hip -- the visual hull of the dense renderer's geometry mode on gfx950: ZjumocapDataset.prepare_inside_pts
// (libs/datasets/ZjumocapDataset.py:259-283) with data_utils.project (:239-250), which the reference runs in numpy on a loader
// worker for every batch.  include/gpnerf_hip.h states the semantics (gpnerf_visual_hull); DESIGN.md 4.9 the launch shape.
//
// One kernel: a lane owns four consecutive bytes of the flat [X][Y][Z] output -- a run of z-neighbours that
// wraps into the next (y, x) row where a row ends -- carves its four points against the views in float64 and stores one packed
// 32-bit word, so a wavefront writes 256 contiguous bytes.  Taking the runs from the flat array and not from each row keeps every
// word aligned whatever Z is; the array's last, partial run and an output pointer that is not 4-aligned go out as byte stores.  The
// cameras travel in the kernel argument, the masks (<= 8 MB) are read through the cache, no LDS.  The count of non-zero values is
// one wavefront reduction and one integer atomic per wavefront (order-independent).  Measured, the kernel is bound by its float64
// arithmetic (two divisions per point and view), not by its stores: DESIGN.md 4.9.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // S_, launch_status; wave_sum

constexpr int HULL_MAX_VIEWS = 8, HULL_THREADS = 256;
constexpr int64_t HULL_MAX_POINTS = (int64_t)1 << 28;

struct HullArgs {
    double cam[HULL_MAX_VIEWS][21];     // K 3x3 row-major, RT 3x4 row-major
    const float* axis[3];
    const uint8_t* masks;               // [n_views][mh][mw]
    uint8_t* inside;                    // [n0][n1][n2]
    unsigned long long* n_inside;
    long total;
    int n[3];
    int n_views, mh, mw;
    int words;                          // inside is 4-aligned: full runs are stored as one word
};

// np.round(v).astype(np.int32) followed by np.clip(., 0, hi) (:274-276).  np.round rounds half to even (rint).  The conversion of a
// value that is not finite or does not fit gives INT32_MIN on x86-64, which the clip turns into 0; the device's conversion instruction
// saturates and maps NaN to 0 instead, so the range is tested here.
__device__ __forceinline__ int pixel_of(const double v, const int hi) {
    const double r = rint(v);
    if (!(fabs(r) < 2147483648.0)) return 0;
    const int q = (int)r;
    return q < 0 ? 0 : (q > hi ? hi : q);
}

// one point against the views in order, only while its value is exactly 1 (the reference's `ind = inside == 1`): a point that picks
// up 0 or a border value (100) is tested by no later view.  Float64, multiply then add, unfused (the build's -ffp-contract=off).
__device__ __forceinline__ unsigned carve_point(const HullArgs& a, const float x, const float y, const float z) {
    const double p0 = (double)x, p1 = (double)y, p2 = (double)z;
    unsigned v = 1u;
    for (int w = 0; w < a.n_views && v == 1u; ++w) {
        const double* K = a.cam[w];
        const double* RT = a.cam[w] + 9;
        // np.dot(xyz, RT[:, :3].T) + RT[:, 3:].T, then np.dot(., K.T) (data_utils.py:246-248)
        const double c0 = ((p0 * RT[0] + p1 * RT[1]) + p2 * RT[2]) + RT[3];
        const double c1 = ((p0 * RT[4] + p1 * RT[5]) + p2 * RT[6]) + RT[7];
        const double c2 = ((p0 * RT[8] + p1 * RT[9]) + p2 * RT[10]) + RT[11];
        const double h0 = (c0 * K[0] + c1 * K[1]) + c2 * K[2];
        const double h1 = (c0 * K[3] + c1 * K[4]) + c2 * K[5];
        const double h2 = (c0 * K[6] + c1 * K[7]) + c2 * K[8];
        const int col = pixel_of(h0 / h2, a.mw - 1), row = pixel_of(h1 / h2, a.mh - 1);
        v = a.masks[((long)w * a.mh + row) * a.mw + col];
    }
    return v;
}

__global__ void hull_zero_count_kernel(unsigned long long* n) { *n = 0ull; }

__global__ void __launch_bounds__(HULL_THREADS) visual_hull_kernel(const HullArgs a) {
    const long flat0 = ((long)blockIdx.x * HULL_THREADS + threadIdx.x) * 4;
    int nonzero = 0;
    if (flat0 < a.total) {
        const int n1 = a.n[1], n2 = a.n[2];
        int k = (int)(flat0 % n2);
        const long r = flat0 / n2;
        int j = (int)(r % n1), i = (int)(r / n1);
        const int run = a.total - flat0 < 4 ? (int)(a.total - flat0) : 4;
        unsigned word = 0u;
        for (int b = 0; b < run; ++b) {
            const unsigned v = carve_point(a, a.axis[0][i], a.axis[1][j], a.axis[2][k]);
            word |= v << (8 * b);
            nonzero += v != 0u;
            if (++k == n2) {
                k = 0;
                if (++j == n1) { j = 0; ++i; }
            }
        }
        if (run == 4 && a.words) *reinterpret_cast<unsigned*>(a.inside + flat0) = word;
        else for (int b = 0; b < run; ++b) a.inside[flat0 + b] = (uint8_t)(word >> (8 * b));
    }
    if (a.n_inside) {
        nonzero = wave_sum(nonzero);
        if ((threadIdx.x & 63) == 0 && nonzero) atomicAdd(a.n_inside, (unsigned long long)nonzero);
    }
}

}  // namespace

extern "C" {

int gpnerf_visual_hull(const float* axis_x, const float* axis_y, const float* axis_z, const int32_t* dims, int32_t n_views,
                       const uint8_t* masks, int32_t mask_h, int32_t mask_w, const double* cams, uint8_t* inside, int64_t* n_inside,
                       void* stream) {
    if (!axis_x || !axis_y || !axis_z || !dims || !masks || !cams || !inside) return GPNERF_E_ARG;
    if (n_views < 1 || n_views > HULL_MAX_VIEWS || mask_h < 1 || mask_w < 1) return GPNERF_E_ARG;
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return GPNERF_E_ARG;
    if ((int64_t)dims[0] * dims[1] > HULL_MAX_POINTS || (int64_t)dims[0] * dims[1] * dims[2] > HULL_MAX_POINTS) return GPNERF_E_ARG;
    if ((int64_t)n_views * mask_h * mask_w >= ((int64_t)1 << 40)) return GPNERF_E_ARG;
    HullArgs a;
    for (int v = 0; v < HULL_MAX_VIEWS; ++v)
        for (int e = 0; e < 21; ++e) a.cam[v][e] = v < n_views ? cams[v * 21 + e] : 0.0;
    a.axis[0] = axis_x; a.axis[1] = axis_y; a.axis[2] = axis_z;
    a.masks = masks;
    a.inside = inside;
    a.n_inside = reinterpret_cast<unsigned long long*>(n_inside);
    for (int i = 0; i < 3; ++i) a.n[i] = dims[i];
    a.total = (long)dims[0] * dims[1] * dims[2];
    a.n_views = n_views; a.mh = mask_h; a.mw = mask_w;
    a.words = ((uintptr_t)inside & 3u) == 0;
    // the count starts from a kernel of the library's own, not from a memset node
    if (n_inside) hipLaunchKernelGGL(hull_zero_count_kernel, dim3(1), dim3(1), 0, S_(stream), a.n_inside);
    const long lanes = (a.total + 3) / 4;
    hipLaunchKernelGGL(visual_hull_kernel, dim3((unsigned)((lanes + HULL_THREADS - 1) / HULL_THREADS)), dim3(HULL_THREADS), 0,
                       S_(stream), a);
    return launch_status();
}

}  // extern "C"
