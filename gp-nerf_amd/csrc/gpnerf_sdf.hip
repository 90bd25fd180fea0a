// gpnerf_sdf.hip -- the truncated signed distance field of a triangle mesh on a lattice, on gfx950, and its trilinear sampling at
// points.  include/gpnerf_hip.h states the definition operation for operation (gpnerf_mesh_sdf, gpnerf_sdf_sample) and the argument
// why a face's widened box holds every lattice point it can reach; DESIGN.md 4.17 the launch shape and the measurements.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone;
// the one data-dependent length (the large-face list's) stays in the workspace header.  No float atomics.  The integer atomics, and
// why their arrival order cannot matter:
//   - a lattice point keeps the unsigned 64-bit MINIMUM of (bits(distance) << 32) | face over the faces that reach it within the
//     band (atomicMin, no return value): a distance is >= +0, so its bits order as the floats do, and the low word breaks a tie for
//     the lower face.  A minimum is idempotent, commutative and associative: the key is a function of the SET of (face, point) pairs;
//   - a relaxed read of the key skips an atomic that cannot lower it: keys only ever fall, so a stale read is too high, and all it
//     can do is let through an atomic that changes nothing;
//   - the large-face list is filled through a cursor: the SET of faces that lands in it is the same in any order, and what the
//     list's reader does with a face is again minima;
//   - the statistics are integer sums.
//
// The scatter goes face -> lattice, as the rasteriser's and the voxeliser's do: the first kernel gives every face ONE lane, which
// tests the face, finds the index range of its box widened by the band and one step, and walks the box's points; a face whose box
// holds more than LARGE_POINTS points goes through the list to the second kernel, a launch of fixed grid that gives each listed face
// a wavefront, 64 points of the box per step, z fastest (a wavefront's reads of the keys are runs of a column).  With a band of a few
// steps every face of a body-sized mesh is in the second tier; the first is for bands under a step and for faces cut by the border.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for, sweep_blocks, mesh_ok; wave_count, wave_sum, stat_add
#include "gpnerf_tri2d.h"      // large_append, LARGE_BLOCKS
#include "gpnerf_tridist.h"    // V3, closest_on_triangle: THE distance, the one gpnerf_mesh_distance computes

constexpr int THREADS = 256;
constexpr int LARGE_POINTS = GPNERF_SDF_LARGE_POINTS;    // box points above which a face takes a wavefront: one step of it (chosen, not tuned)
constexpr double GUARD = 65536.0;                        // 2^16 lattice steps, the voxeliser's guard band, on all three axes here
constexpr double MAX_BAND_STEPS = (double)GPNERF_SDF_MAX_BAND_STEPS;
constexpr int64_t MAX_POINTS = (int64_t)1 << 28;         // marching cubes' limit
constexpr unsigned long long KEY_NONE = ~0ull;           // above every key: the high word of a key is a finite float's bits

struct Lattice {
    double lo[3], step[3];
    int n[3];
};

struct Layout { size_t hdr, keys, list, total; };

Layout layout_of(int64_t n_faces, const int32_t* dims) {
    Layout l;
    size_t o = 0;
    l.hdr = o;  o += 256;                                // the list's length, uint64 at 0
    l.keys = o; o += align256(sizeof(unsigned long long) * (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2]);
    l.list = o; o += align256(sizeof(uint32_t) * (size_t)n_faces);
    l.total = o;
    return l;
}

bool dims_ok(const int32_t* dims, int least) {
    if (!dims || dims[0] < least || dims[1] < least || dims[2] < least) return false;
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

bool band_ok(float band, const double* lattice) {
    const double least = fmin(lattice[3], fmin(lattice[4], lattice[5]));
    return band > 0.f && (double)band <= MAX_BAND_STEPS * least;                               // (false for a NaN; an infinite band fails the second)
}

Lattice lattice_of(const double* lattice, const int32_t* dims) {
    Lattice g;
    for (int a = 0; a < 3; ++a) { g.lo[a] = lattice[a]; g.step[a] = lattice[3 + a]; g.n[a] = dims[a]; }
    return g;
}

// lattice point i of axis a: the product and the sum in double, one rounding to float32
DEV float point_of(const Lattice& g, int a, int i) { return (float)(g.lo[a] + (double)i * g.step[a]); }

enum SdfFace { SDF_USED = GPNERF_SDF_USED, SDF_BAD_VERTEX = GPNERF_SDF_SKIPPED_VERTEX, SDF_NO_BOX = GPNERF_SDF_SKIPPED_BOX };

// the inclusive index range of a face's widened box, clipped to the lattice; empty on an axis where hi < lo
struct Box {
    int lo[3], hi[3];
    DEV int w(int a) const { return hi[a] - lo[a] + 1; }
    DEV unsigned points() const { return (unsigned)w(0) * (unsigned)w(1) * (unsigned)w(2); }   // (a non-empty box: <= 2^28)
};

// face f: its vertices, whether all three are usable, and the box of lattice points within band + one step of its extent
DEV SdfFace sdf_setup(const float* __restrict__ vertices, long n_vertices, const int32_t* __restrict__ faces, const Lattice& g, float band, long f,
                      V3& a, V3& b, V3& c, Box& box) {
    const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= n_vertices || ib >= n_vertices || ic >= n_vertices) return SDF_BAD_VERTEX;
    a = load3(vertices, ia); b = load3(vertices, ib); c = load3(vertices, ic);
    const float va[3] = {a.x, a.y, a.z}, vb[3] = {b.x, b.y, b.z}, vc[3] = {c.x, c.y, c.z};
    bool usable = true;
    for (int k = 0; k < 3; ++k) {
        // (every comparison is false for a NaN; an infinite coordinate fails the guard band)
        const double ua = ((double)va[k] - g.lo[k]) / g.step[k], ub = ((double)vb[k] - g.lo[k]) / g.step[k];
        const double uc = ((double)vc[k] - g.lo[k]) / g.step[k];
        usable = usable && fabs(ua) <= GUARD && fabs(ub) <= GUARD && fabs(uc) <= GUARD;
    }
    if (!usable) return SDF_BAD_VERTEX;
    bool hit = true;
    for (int k = 0; k < 3; ++k) {
        const double mn = (double)fminf(va[k], fminf(vb[k], vc[k])), mx = (double)fmaxf(va[k], fmaxf(vb[k], vc[k]));
        // |index| <= 2^16 + 1024 + 2 here: the clip is taken in double, and the conversion of what is left is exact
        const double i0 = ceil(((mn - (double)band) - g.lo[k]) / g.step[k]) - 1.0;
        const double i1 = floor(((mx + (double)band) - g.lo[k]) / g.step[k]) + 1.0;
        const double c0 = fmax(i0, 0.0), c1 = fmin(i1, (double)(g.n[k] - 1));
        hit = hit && c0 <= c1;
        box.lo[k] = (int)c0;
        box.hi[k] = (int)c1;
    }
    return hit ? SDF_USED : SDF_NO_BOX;
}

// one (face, lattice point) pair: THE distance, and the point's key lowered when the distance is within the band.  Returns whether
// it was (the PAIRS statistic: a function of the inputs, unlike the number of atomics the read below lets through).
DEV bool sdf_visit(const Lattice& g, float band, unsigned long long* keys, V3 a, V3 b, V3 c, int32_t f, int i, int j, int k) {
    const V3 p = {point_of(g, 0, i), point_of(g, 1, j), point_of(g, 2, k)};
    const V3 cp = closest_on_triangle(sub(a, p), sub(b, p), sub(c, p));
    const float d = sqrtf(dot(cp, cp));
    if (!(d <= band)) return false;
    const unsigned long long key = ((unsigned long long)(uint32_t)__float_as_int(d) << 32) | (unsigned long long)(uint32_t)f;
    unsigned long long* at = keys + ((long)i * g.n[1] + j) * g.n[2] + k;
    // (keys only fall: a stale value is too high and lets a harmless atomic through)
    if (key < __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(at, key);
    return true;
}

// the keys, the list's length and the statistics start from a kernel of the library's own, not from memset nodes
__global__ __launch_bounds__(THREADS) void sdf_clear_kernel(unsigned long long* keys, long n_points, unsigned long long* list_len, long long* stats) {
    const long stride = (long)gridDim.x * THREADS;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n_points; i += stride) keys[i] = KEY_NONE;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) *list_len = 0ull;
        if ((int)threadIdx.x < GPNERF_SDF_STATS) stats[threadIdx.x] = 0;
    }
}

// one lane per face; every lane stays to the end (the counts are summed over the wavefront)
__global__ __launch_bounds__(THREADS) void sdf_faces_kernel(const float* __restrict__ vertices, long n_vertices, const int32_t* __restrict__ faces,
                                                            long n_faces, const Lattice g, float band, unsigned long long* keys, uint32_t* list,
                                                            unsigned long long* list_len, long long* stats) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    const bool live = f < n_faces;
    const int lane = threadIdx.x & 63;
    V3 a = {0.f, 0.f, 0.f}, b = a, c = a;
    Box box = {{0, 0, 0}, {-1, -1, -1}};
    SdfFace st = SDF_NO_BOX;
    if (live) st = sdf_setup(vertices, n_vertices, faces, g, band, f, a, b, c, box);
    const bool used = live && st == SDF_USED;
    const bool large = used && box.points() > (unsigned)LARGE_POINTS;
    const int n_used = wave_count(used), n_bad = wave_count(live && st == SDF_BAD_VERTEX), n_miss = wave_count(live && st == SDF_NO_BOX);
    const int n_large = wave_count(large);
    const long long at = large_append(large, list_len, (unsigned long long)n_faces);
    if (at >= 0) list[at] = (uint32_t)f;
    long long visited = 0, pairs = 0;
    if (used && !large) {
        for (int i = box.lo[0]; i <= box.hi[0]; ++i)
            for (int j = box.lo[1]; j <= box.hi[1]; ++j)
                for (int k = box.lo[2]; k <= box.hi[2]; ++k) pairs += sdf_visit(g, band, keys, a, b, c, (int32_t)f, i, j, k);
        visited = box.points();
    }
    visited = wave_sum(visited);
    pairs = wave_sum(pairs);
    if (lane == 0) {
        stat_add(stats, GPNERF_SDF_USED, n_used);
        stat_add(stats, GPNERF_SDF_SKIPPED_VERTEX, n_bad);
        stat_add(stats, GPNERF_SDF_SKIPPED_BOX, n_miss);
        stat_add(stats, GPNERF_SDF_LARGE, n_large);
        stat_add(stats, GPNERF_SDF_VISITED, visited);
        stat_add(stats, GPNERF_SDF_PAIRS, pairs);
    }
}

// fixed grid: a wavefront per listed face, 64 points of its box per step, z fastest
__global__ __launch_bounds__(THREADS) void sdf_large_kernel(const float* __restrict__ vertices, long n_vertices, const int32_t* __restrict__ faces,
                                                            long n_faces, const Lattice g, float band, unsigned long long* keys,
                                                            const uint32_t* __restrict__ list, const unsigned long long* __restrict__ list_len,
                                                            long long* stats) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (THREADS / 64) + threadIdx.x / 64, waves = (long)gridDim.x * (THREADS / 64);
    unsigned long long n = *list_len;
    if (n > (unsigned long long)n_faces) n = (unsigned long long)n_faces;
    long long visited = 0, pairs = 0;
    for (unsigned long long at = (unsigned long long)wave; at < n; at += (unsigned long long)waves) {
        const long f = (long)list[at];
        if (f >= n_faces) continue;                      // (never: the list holds what the first kernel wrote)
        V3 a, b, c;
        Box box;
        if (sdf_setup(vertices, n_vertices, faces, g, band, f, a, b, c, box) != SDF_USED) continue;
        // (unsigned: the extents are at least 1 here and the box holds at most 2^28 points)
        const unsigned wz = (unsigned)box.w(2), wyz = wz * (unsigned)box.w(1), points = box.points();
        for (unsigned p = (unsigned)lane; p < points; p += 64) {
            const unsigned di = p / wyz, r = p - di * wyz, dj = r / wz, dk = r - dj * wz;
            pairs += sdf_visit(g, band, keys, a, b, c, (int32_t)f, box.lo[0] + (int)di, box.lo[1] + (int)dj, box.lo[2] + (int)dk);
        }
        if (lane == 0) visited += points;
    }
    visited = wave_sum(visited);
    pairs = wave_sum(pairs);
    if (lane == 0) {
        stat_add(stats, GPNERF_SDF_VISITED, visited);
        stat_add(stats, GPNERF_SDF_PAIRS, pairs);
    }
}

// one lane per lattice point: the key and the point's bit become the value and the face
__global__ __launch_bounds__(THREADS) void sdf_resolve_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ bits, int nz,
                                                              long n_points, float band, float* sdf, int32_t* face_id, long long* stats) {
    const long stride = (long)gridDim.x * THREADS;
    const int nzw = (nz + 31) / 32;
    long long in_band = 0, inside = 0;
    // (every lane of a wavefront runs the same number of rounds: the sums below are over the whole wavefront)
    for (long p0 = (long)blockIdx.x * THREADS; p0 < n_points; p0 += stride) {
        const long p = p0 + threadIdx.x;
        if (p >= n_points) continue;
        const unsigned long long key = keys[p];
        const bool hit = key != KEY_NONE;
        const long col = p / nz;
        const int k = (int)(p - col * nz);
        const bool in = bits && ((bits[col * nzw + (k >> 5)] >> (k & 31)) & 1u);
        const float m = hit ? __int_as_float((int)(uint32_t)(key >> 32)) : band;
        sdf[p] = in ? -m : m;
        if (face_id) face_id[p] = hit ? (int32_t)(uint32_t)(key & 0xffffffffull) : -1;
        in_band += hit;
        inside += in;
    }
    in_band = wave_sum(in_band);
    inside = wave_sum(inside);
    if ((threadIdx.x & 63) == 0) {
        stat_add(stats, GPNERF_SDF_IN_BAND, in_band);
        stat_add(stats, GPNERF_SDF_INSIDE, inside);
    }
}

// one axis of a sample: the cell and the weight, false for a coordinate that is not finite or lies outside [0, n - 1]
DEV bool sample_axis(const Lattice& g, int a, float x, int& cell, double& t) {
    const double u = ((double)x - g.lo[a]) / g.step[a];
    if (!(u >= 0.0 && u <= (double)(g.n[a] - 1))) return false;          // (false for a NaN)
    double c = floor(u);
    if (c > (double)(g.n[a] - 2)) c = (double)(g.n[a] - 2);              // u == n - 1: the last cell, t = 1
    cell = (int)c;
    t = u - c;
    return true;
}

DEV double lerp_(double a, double b, double t) { return a + t * (b - a); }

// one lane per point: z, then y, then x, in double, one rounding to float32
__global__ __launch_bounds__(THREADS) void sdf_sample_kernel(const float* __restrict__ sdf, const Lattice g, const float* __restrict__ points, long n,
                                                             float* out) {
    const long q = (long)blockIdx.x * THREADS + threadIdx.x;
    if (q >= n) return;
    int ci, cj, ck;
    double tx, ty, tz;
    const bool okx = sample_axis(g, 0, points[3 * q], ci, tx), oky = sample_axis(g, 1, points[3 * q + 1], cj, ty);
    const bool okz = sample_axis(g, 2, points[3 * q + 2], ck, tz);
    if (!(okx && oky && okz)) {
        out[q] = nanf_();
        return;
    }
    const long sy = g.n[2], sx = (long)g.n[1] * g.n[2];
    const float* v = sdf + (long)ci * sx + (long)cj * sy + ck;
    const double z00 = lerp_((double)v[0], (double)v[1], tz), z01 = lerp_((double)v[sy], (double)v[sy + 1], tz);
    const double z10 = lerp_((double)v[sx], (double)v[sx + 1], tz), z11 = lerp_((double)v[sx + sy], (double)v[sx + sy + 1], tz);
    out[q] = (float)lerp_(lerp_(z00, z01, ty), lerp_(z10, z11, ty), tx);
}

}  // namespace

extern "C" {

size_t gpnerf_mesh_sdf_workspace_bytes(int64_t n_faces, const int32_t* dims) {
    if (n_faces < 0 || n_faces > INT32_MAX || !dims_ok(dims, 1)) return 0;
    return layout_of(n_faces, dims).total;
}

int gpnerf_mesh_sdf(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const double* lattice, const int32_t* dims,
                    float band, const uint32_t* bits, void* workspace, size_t workspace_bytes, float* sdf, int32_t* face_id, int64_t* stats,
                    void* stream) {
    if (!workspace || !sdf || !stats || !mesh_ok(vertices, n_vertices, faces, n_faces) || !dims_ok(dims, 1) || !lattice_ok(lattice) ||
        !band_ok(band, lattice))
        return GPNERF_E_ARG;
    const Layout l = layout_of(n_faces, dims);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    char* base = static_cast<char*>(workspace);
    unsigned long long* list_len = reinterpret_cast<unsigned long long*>(base + l.hdr);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + l.keys);
    uint32_t* list = reinterpret_cast<uint32_t*>(base + l.list);
    const Lattice g = lattice_of(lattice, dims);
    const long n_points = (long)dims[0] * dims[1] * dims[2];
    long long* st = reinterpret_cast<long long*>(stats);
    hipLaunchKernelGGL(sdf_clear_kernel, dim3(sweep_blocks(n_points, THREADS)), dim3(THREADS), 0, S_(stream), keys, n_points, list_len, st);
    if (n_faces > 0) {
        hipLaunchKernelGGL(sdf_faces_kernel, dim3(blocks_for(n_faces, THREADS)), dim3(THREADS), 0, S_(stream), vertices, (long)n_vertices, faces,
                           (long)n_faces, g, band, keys, list, list_len, st);
        hipLaunchKernelGGL(sdf_large_kernel, dim3(LARGE_BLOCKS), dim3(THREADS), 0, S_(stream), vertices, (long)n_vertices, faces, (long)n_faces, g,
                           band, keys, list, list_len, st);
    }
    hipLaunchKernelGGL(sdf_resolve_kernel, dim3(sweep_blocks(n_points, THREADS)), dim3(THREADS), 0, S_(stream), keys, bits, (int)dims[2], n_points,
                       band, sdf, face_id, st);
    return launch_status();
}

int gpnerf_sdf_sample(const float* sdf, const int32_t* dims, const double* lattice, const float* points, int64_t n, float* out, void* stream) {
    if (!sdf || !dims_ok(dims, 2) || !lattice_ok(lattice) || n < 0 || n > INT32_MAX || ((!points || !out) && n > 0)) return GPNERF_E_ARG;
    if (n == 0) return GPNERF_OK;
    const Lattice g = lattice_of(lattice, dims);
    hipLaunchKernelGGL(sdf_sample_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, S_(stream), sdf, g, points, (long)n, out);
    return launch_status();
}

}  // extern "C"
