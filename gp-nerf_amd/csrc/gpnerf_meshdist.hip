// gpnerf_meshdist.hip -- evaluating an extracted mesh on gfx950: the exact nearest point of a triangle mesh for a list of query points
// (point-to-surface, Chamfer, normal consistency, F-score all reduce to it), area-weighted surface samples, and the reduction of a
// list of distances into one slot of doubles.  include/gpnerf_hip.h states the definitions, the shell bound and its proof.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone;
// every data-dependent length (the box, the cell counts, the entries in use) stays in the workspace header.  No float atomics.  The
// integer atomics, and why their arrival order cannot matter:
//   - grid_count_kernel adds 1 to a cell's count per (face, cell) pair: integer addition commutes;
//   - grid_fill_kernel draws a slot of the cell's run from a cursor: the SET of faces that lands in a run is the same in any order,
//     and grid_rank_kernel then writes every face at (run start + number of smaller faces in the run), which is the ascending order.
//
// Lane mapping of the distance kernels: one query per lane.  The queries the metrics hand in are stratified surface samples, i.e.
// ordered by face index, and marching cubes emits faces in cell order, so the 64 queries of a wavefront start in neighbouring cells
// and walk nearly the same entries (L1/L2 hits, little divergence in the shell count).  A wavefront per query with the lanes over a
// cell's entries would leave most lanes idle: a cell of a body-sized mesh holds 3 - 6 entries.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for
#include "gpnerf_tridist.h"    // V3, Best, closest_on_triangle, test_face, face_valid: THE distance and its tie rule

#include "gpnerf_meshgrid.h"   // GridLayout, grid_layout, Grid, grid_of, cell_of: the grid's layout, shared with gpnerf_raycast.hip

constexpr int THREADS = 256;
constexpr int SCAN_THREADS = 1024;
constexpr int STAT_THREADS = 256;
constexpr int64_t MAX_CELL_CAP = (int64_t)1 << 24, MAX_ENTRY_CAP = (int64_t)1 << 30, MAX_FACES = INT32_MAX;
constexpr int SAMPLE_CHUNK = 1024;                       // faces per block of the area scan (4 per thread)
constexpr int TILE = 256;                                // faces per LDS tile of the brute-force form

bool grid_sizes_ok(int64_t n_faces, int64_t cell_cap, int64_t entry_cap) {
    return n_faces >= 1 && n_faces <= MAX_FACES && cell_cap >= 1 && cell_cap <= MAX_CELL_CAP && entry_cap >= 1 && entry_cap <= MAX_ENTRY_CAP;
}

// what a query's result is once the search is over: max_dist's rule, closest, cosine
DEV void write_result(long i, V3 p, Best best, float max_dist, const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                      const float* __restrict__ query_normals, float* dist, int32_t* face, float* closest, float* cosine) {
    const bool hit = best.f >= 0 && !(best.d > max_dist);
    dist[i] = hit ? best.d : inff_();
    face[i] = hit ? best.f : -1;
    if (closest) {
        closest[3 * i] = hit ? p.x + best.cp.x : nanf_();
        closest[3 * i + 1] = hit ? p.y + best.cp.y : nanf_();
        closest[3 * i + 2] = hit ? p.z + best.cp.z : nanf_();
    }
    if (cosine) {
        float cs = nanf_();
        if (hit) {
            const V3 a = load3(vertices, faces[3 * (long)best.f]), b = load3(vertices, faces[3 * (long)best.f + 1]),
                     c = load3(vertices, faces[3 * (long)best.f + 2]);
            const V3 n = cross(sub(b, a), sub(c, a)), q = load3(query_normals, i);
            const float len = sqrtf(dot(n, n));
            cs = (len > 0.f && isfinite(len)) ? fabsf(dot(q, n) / len) : 0.f;
            if (!(cs == cs)) cs = 0.f;
        }
        cosine[i] = cs;
    }
}

DEV void write_nan(long i, float* dist, int32_t* face, float* closest, float* cosine) {
    dist[i] = nanf_();
    face[i] = -1;
    if (closest) closest[3 * i] = closest[3 * i + 1] = closest[3 * i + 2] = nanf_();
    if (cosine) cosine[i] = nanf_();
}

// ---------------------------------------------------------------- the grid

__global__ __launch_bounds__(THREADS) void grid_box_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                           const int32_t* __restrict__ faces, long n_faces, int64_t cell_cap, Grid g) {
    __shared__ float s_box[6][THREADS];
    __shared__ int s_cnt[THREADS];
    const int t = threadIdx.x;
    const long stride = (long)gridDim.x * THREADS;
    for (long c = (long)blockIdx.x * THREADS + t; c <= cell_cap; c += stride) g.start[c] = 0;      // the counts, for grid_count_kernel
    float lo[3] = {inff_(), inff_(), inff_()}, hi[3] = {-inff_(), -inff_(), -inff_()};
    int valid = 0;
    for (long f = (long)blockIdx.x * THREADS + t; f < n_faces; f += stride) {
        V3 a, b, c;
        if (!face_valid(vertices, n_vertices, faces, f, a, b, c)) continue;
        ++valid;
        lo[0] = fminf(lo[0], fminf(a.x, fminf(b.x, c.x))); hi[0] = fmaxf(hi[0], fmaxf(a.x, fmaxf(b.x, c.x)));
        lo[1] = fminf(lo[1], fminf(a.y, fminf(b.y, c.y))); hi[1] = fmaxf(hi[1], fmaxf(a.y, fmaxf(b.y, c.y)));
        lo[2] = fminf(lo[2], fminf(a.z, fminf(b.z, c.z))); hi[2] = fmaxf(hi[2], fmaxf(a.z, fmaxf(b.z, c.z)));
    }
    for (int k = 0; k < 3; ++k) { s_box[k][t] = lo[k]; s_box[3 + k][t] = hi[k]; }
    s_cnt[t] = valid;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            for (int k = 0; k < 3; ++k) {
                s_box[k][t] = fminf(s_box[k][t], s_box[k][t + s]);
                s_box[3 + k][t] = fmaxf(s_box[3 + k][t], s_box[3 + k][t + s]);
            }
            s_cnt[t] += s_cnt[t + s];
        }
        __syncthreads();
    }
    if (t < 6) g.part[8 * blockIdx.x + t] = s_box[t][0];
    if (t == 6) g.part[8 * blockIdx.x + 6] = __int_as_float(s_cnt[0]);
}

// one workgroup: the box from the partial boxes, then thread 0 plans the cells
__global__ __launch_bounds__(THREADS) void grid_plan_kernel(int n_parts, long n_faces, int64_t cell_cap, int64_t entry_cap, Grid g) {
    __shared__ float s_box[6][THREADS];
    __shared__ int s_cnt[THREADS];
    const int t = threadIdx.x;
    float box[6] = {inff_(), inff_(), inff_(), -inff_(), -inff_(), -inff_()};
    int valid = 0;
    for (int p = t; p < n_parts; p += THREADS) {
        for (int k = 0; k < 3; ++k) { box[k] = fminf(box[k], g.part[8 * p + k]); box[3 + k] = fmaxf(box[3 + k], g.part[8 * p + 3 + k]); }
        valid += __float_as_int(g.part[8 * p + 6]);
    }
    for (int k = 0; k < 6; ++k) s_box[k][t] = box[k];
    s_cnt[t] = valid;
    __syncthreads();
    if (t != 0) return;
    for (int j = 1; j < THREADS; ++j) {
        for (int k = 0; k < 3; ++k) { box[k] = fminf(box[k], s_box[k][j]); box[3 + k] = fmaxf(box[3 + k], s_box[3 + k][j]); }
        valid += s_cnt[j];
    }
    int n[3] = {1, 1, 1};
    float lo[3] = {0.f, 0.f, 0.f}, cs[3] = {1.f, 1.f, 1.f};
    if (valid > 0) {
        double e[3];
        bool open[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = box[a];
            e[a] = (double)box[3 + a] - (double)box[a];
            open[a] = e[a] > 0.0;                        // a zero-extent axis keeps one cell
        }
        // cubic cells of edge s with prod(e / s) = cell_cap over the axes still open; an axis thinner than s drops to one cell and
        // the others share the cap again (at most three rounds)
        for (int round = 0; round < 3; ++round) {
            int k = 0;
            double vol = 1.0;
            for (int a = 0; a < 3; ++a) if (open[a]) { ++k; vol *= e[a]; }
            if (!k) break;
            const double s = pow(vol / (double)cell_cap, 1.0 / k);
            bool dropped = false;
            for (int a = 0; a < 3; ++a) {
                if (!open[a]) continue;
                const double c = floor(e[a] / s);
                if (c < 1.0) { open[a] = false; n[a] = 1; dropped = true; }
                else n[a] = (int)fmin(c, (double)MAX_AXIS_CELLS);
            }
            if (!dropped) break;
        }
        while ((int64_t)n[0] * n[1] * n[2] > cell_cap) {  // (rounding of pow / floor: give the longest axis one cell less)
            int a = n[0] >= n[1] ? (n[0] >= n[2] ? 0 : 2) : (n[1] >= n[2] ? 1 : 2);
            --n[a];
        }
        for (int a = 0; a < 3; ++a) {
            const float w = (float)(e[a] / n[a]);
            cs[a] = (w > 0.f && isfinite(w)) ? w : 1.f;
        }
    }
    g.hdr[GPNERF_GRID_HDR_MAGIC] = GRID_MAGIC;
    g.hdr[GPNERF_GRID_HDR_STATUS] = GPNERF_GRID_BUILDING;
    g.hdr[GPNERF_GRID_HDR_SKIPPED] = (int32_t)(n_faces - valid);
    g.hdr[GPNERF_GRID_HDR_VALID] = valid;
    for (int a = 0; a < 3; ++a) {
        g.hdr[GPNERF_GRID_HDR_CELLS + a] = n[a];
        g.hdr[GPNERF_GRID_HDR_LO + a] = __float_as_int(lo[a]);
        g.hdr[GPNERF_GRID_HDR_SIZE + a] = __float_as_int(cs[a]);
        g.hdr[GPNERF_GRID_HDR_INV + a] = __float_as_int(1.f / cs[a]);
    }
    g.hdr[GPNERF_GRID_HDR_N_CELLS] = n[0] * n[1] * n[2];
    g.hdr[GPNERF_GRID_HDR_CELL_CAP] = (int32_t)cell_cap;
    g.hdr[GPNERF_GRID_HDR_ENTRY_CAP] = (int32_t)entry_cap;
    g.hdr[GPNERF_GRID_HDR_NEEDED] = 0;
    g.hdr[GPNERF_GRID_HDR_NEEDED + 1] = 0;
}

struct CellRange { int lo[3], hi[3], ny, nz; };

DEV CellRange range_of(const int32_t* __restrict__ hdr, V3 a, V3 b, V3 c) {
    CellRange r;
    const float mn[3] = {fminf(a.x, fminf(b.x, c.x)), fminf(a.y, fminf(b.y, c.y)), fminf(a.z, fminf(b.z, c.z))};
    const float mx[3] = {fmaxf(a.x, fmaxf(b.x, c.x)), fmaxf(a.y, fmaxf(b.y, c.y)), fmaxf(a.z, fmaxf(b.z, c.z))};
    for (int k = 0; k < 3; ++k) {
        const float lo = __int_as_float(hdr[GPNERF_GRID_HDR_LO + k]), inv = __int_as_float(hdr[GPNERF_GRID_HDR_INV + k]);
        const int n = hdr[GPNERF_GRID_HDR_CELLS + k];
        r.lo[k] = cell_of(mn[k], lo, inv, n);
        r.hi[k] = cell_of(mx[k], lo, inv, n);
    }
    r.ny = hdr[GPNERF_GRID_HDR_CELLS + 1];
    r.nz = hdr[GPNERF_GRID_HDR_CELLS + 2];
    return r;
}

// one wavefront per face, the lanes over the cells its bounding box overlaps (a face that spans the box lands in every cell).
// FILL false: count; FILL true: draw a slot of the cell's run and leave (face, cell) there for grid_rank_kernel.
template <bool FILL>
__global__ __launch_bounds__(THREADS) void grid_enter_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                             const int32_t* __restrict__ faces, long n_faces, Grid g) {
    if (FILL && g.hdr[GPNERF_GRID_HDR_STATUS] != GPNERF_GRID_OK) return;       // overflow: nothing is written
    const long f = (long)blockIdx.x * (THREADS / 64) + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (f >= n_faces) return;
    V3 a, b, c;
    if (!face_valid(vertices, n_vertices, faces, f, a, b, c)) return;
    const CellRange r = range_of(g.hdr, a, b, c);
    const int wy = r.hi[1] - r.lo[1] + 1, wz = r.hi[2] - r.lo[2] + 1;
    const long cells = (long)(r.hi[0] - r.lo[0] + 1) * wy * wz;
    const int32_t entry_cap = g.hdr[GPNERF_GRID_HDR_ENTRY_CAP];
    for (long k = lane; k < cells; k += 64) {
        const int cz = r.lo[2] + (int)(k % wz), cy = r.lo[1] + (int)((k / wz) % wy), cx = r.lo[0] + (int)(k / ((long)wz * wy));
        const int cell = (cx * r.ny + cy) * r.nz + cz;
        if (!FILL) {
            atomicAdd(&g.start[cell], 1);
        } else {
            const int pos = atomicAdd(&g.cursor[cell], 1);
            if (pos >= 0 && pos < entry_cap) {                                 // (always, with status OK; the capacity is never passed)
                g.tmp_face[pos] = (int32_t)f;
                g.tmp_cell[pos] = cell;
            }
        }
    }
}

// one workgroup: the exclusive scan of the cells' counts (integers: any association gives the same sums), the cursors, the status
__global__ __launch_bounds__(SCAN_THREADS) void grid_scan_kernel(Grid g) {
    __shared__ long long s_sum[SCAN_THREADS];
    const int t = threadIdx.x;
    const int n_cells = g.hdr[GPNERF_GRID_HDR_N_CELLS];
    const long long entry_cap = g.hdr[GPNERF_GRID_HDR_ENTRY_CAP];
    const int per = (n_cells + SCAN_THREADS - 1) / SCAN_THREADS, c0 = min(t * per, n_cells), c1 = min(c0 + per, n_cells);
    long long sum = 0;
    for (int c = c0; c < c1; ++c) sum += g.start[c];
    s_sum[t] = sum;
    __syncthreads();
    long long before = 0, total = 0;
    for (int k = 0; k < SCAN_THREADS; ++k) {
        if (k < t) before += s_sum[k];
        total += s_sum[k];
    }
    const bool fits = total <= entry_cap;
    for (int c = c0; c < c1; ++c) {
        const int cnt = g.start[c];
        const int32_t at = fits ? (int32_t)before : 0;   // overflow: no run is laid out
        g.start[c] = at;
        g.cursor[c] = at;
        before += cnt;
    }
    if (t == 0) {
        g.start[n_cells] = fits ? (int32_t)total : 0;
        g.hdr[GPNERF_GRID_HDR_NEEDED] = (int32_t)(total & 0xffffffffll);
        g.hdr[GPNERF_GRID_HDR_NEEDED + 1] = (int32_t)(total >> 32);
        g.hdr[GPNERF_GRID_HDR_STATUS] = fits ? GPNERF_GRID_OK : GPNERF_GRID_OVERFLOW;
    }
}

// one thread per entry: its place in its cell's run is the number of smaller faces there (a face enters a cell once)
__global__ __launch_bounds__(THREADS) void grid_rank_kernel(Grid g) {
    if (g.hdr[GPNERF_GRID_HDR_STATUS] != GPNERF_GRID_OK) return;
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (long)g.hdr[GPNERF_GRID_HDR_NEEDED]) return;                      // (status OK: needed <= entry_cap < 2^31)
    const int32_t f = g.tmp_face[e], cell = g.tmp_cell[e];
    const int32_t s = g.start[cell], end = g.start[cell + 1];
    int rank = 0;
    for (int32_t j = s; j < end; ++j) rank += g.tmp_face[j] < f;
    g.entries[s + rank] = f;
}

// ---------------------------------------------------------------- distance

__global__ __launch_bounds__(THREADS) void distance_grid_kernel(const float* __restrict__ points, long n_points,
                                                                const float* __restrict__ vertices, int64_t n_vertices,
                                                                const int32_t* __restrict__ faces, long n_faces, void* workspace,
                                                                float max_dist, const float* __restrict__ query_normals, float* dist,
                                                                int32_t* face, float* closest, float* cosine) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_points) return;
    const int32_t* hdr = static_cast<const int32_t*>(workspace);
    const V3 p = load3(points, i);
    if (hdr[GPNERF_GRID_HDR_MAGIC] != GRID_MAGIC || hdr[GPNERF_GRID_HDR_STATUS] != GPNERF_GRID_OK || !finite3(p)) {
        write_nan(i, dist, face, closest, cosine);
        return;
    }
    const Grid g = grid_of(workspace, hdr[GPNERF_GRID_HDR_CELL_CAP], hdr[GPNERF_GRID_HDR_ENTRY_CAP]);
    int n[3], q[3];
    float cs[3];
    const float pc[3] = {p.x, p.y, p.z};
    for (int k = 0; k < 3; ++k) {
        n[k] = hdr[GPNERF_GRID_HDR_CELLS + k];
        cs[k] = __int_as_float(hdr[GPNERF_GRID_HDR_SIZE + k]);
        q[k] = cell_of(pc[k], __int_as_float(hdr[GPNERF_GRID_HDR_LO + k]), __int_as_float(hdr[GPNERF_GRID_HDR_INV + k]), n[k]);
    }
    Best best = {inff_(), -1, {0.f, 0.f, 0.f}};
    auto visit = [&](int cx, int cy, int cz) {
        const int cell = (cx * n[1] + cy) * n[2] + cz;
        const int32_t s = g.start[cell], e = g.start[cell + 1];
        for (int32_t j = s; j < e; ++j) {
            const int32_t f = g.entries[j];
            V3 a, b, c;
            if ((uint32_t)f < (uint32_t)n_faces && face_valid(vertices, n_vertices, faces, f, a, b, c)) test_face(best, p, a, b, c, f);
        }
    };
    for (int r = 0;; ++r) {
        // shell r: the cells at Chebyshev distance exactly r from the query's cell, clipped to the grid
        const int x0 = max(q[0] - r, 0), x1 = min(q[0] + r, n[0] - 1), y0 = max(q[1] - r, 0), y1 = min(q[1] + r, n[1] - 1);
        const int z0 = max(q[2] - r, 0), z1 = min(q[2] + r, n[2] - 1);
        for (int cx = x0; cx <= x1; ++cx)
            for (int cy = y0; cy <= y1; ++cy) {
                if (abs(cx - q[0]) == r || abs(cy - q[1]) == r) {
                    for (int cz = z0; cz <= z1; ++cz) visit(cx, cy, cz);
                } else {
                    if (q[2] - r >= 0) visit(cx, cy, q[2] - r);
                    if (r > 0 && q[2] + r <= n[2] - 1) visit(cx, cy, q[2] + r);
                }
            }
        // everything not yet visited lies beyond (r - 1/16) cells along an axis the shells have not covered from end to end
        float w = inff_();
        for (int k = 0; k < 3; ++k)
            if (q[k] - r > 0 || q[k] + r < n[k] - 1) w = fminf(w, cs[k]);
        if (w == inff_()) break;                          // every cell has been visited
        const float bound = ((float)r - 0.0625f) * w * 0.999f;
        if (best.d <= bound || bound >= max_dist) break;
    }
    write_result(i, p, best, max_dist, vertices, faces, query_normals, dist, face, closest, cosine);
}

__global__ __launch_bounds__(THREADS) void distance_brute_kernel(const float* __restrict__ points, long n_points,
                                                                 const float* __restrict__ vertices, int64_t n_vertices,
                                                                 const int32_t* __restrict__ faces, long n_faces, float max_dist,
                                                                 const float* __restrict__ query_normals, float* dist, int32_t* face,
                                                                 float* closest, float* cosine) {
    __shared__ float s_v[9][TILE];
    __shared__ int s_ok[TILE];
    const int t = threadIdx.x;
    const long i = (long)blockIdx.x * THREADS + t;
    const bool live = i < n_points;
    const V3 p = live ? load3(points, i) : V3{0.f, 0.f, 0.f};
    Best best = {inff_(), -1, {0.f, 0.f, 0.f}};
    for (long f0 = 0; f0 < n_faces; f0 += TILE) {
        __syncthreads();                                 // the previous tile has been read
        V3 a = {0.f, 0.f, 0.f}, b = a, c = a;
        const bool ok = f0 + t < n_faces && face_valid(vertices, n_vertices, faces, f0 + t, a, b, c);
        s_v[0][t] = a.x; s_v[1][t] = a.y; s_v[2][t] = a.z; s_v[3][t] = b.x; s_v[4][t] = b.y; s_v[5][t] = b.z;
        s_v[6][t] = c.x; s_v[7][t] = c.y; s_v[8][t] = c.z;
        s_ok[t] = ok;
        __syncthreads();
        const int m = (int)min((long)TILE, n_faces - f0);
        for (int j = 0; j < m; ++j) {
            if (!s_ok[j]) continue;                      // (uniform: every lane reads the same word)
            test_face(best, p, V3{s_v[0][j], s_v[1][j], s_v[2][j]}, V3{s_v[3][j], s_v[4][j], s_v[5][j]}, V3{s_v[6][j], s_v[7][j], s_v[8][j]},
                      (int32_t)(f0 + j));
        }
    }
    if (!live) return;
    if (!finite3(p)) write_nan(i, dist, face, closest, cosine);
    else write_result(i, p, best, max_dist, vertices, faces, query_normals, dist, face, closest, cosine);
}

// ---------------------------------------------------------------- surface samples

struct SampleLayout { size_t hdr, local, blocksum, blockoff, total; long nb; };

SampleLayout sample_layout(int64_t n_faces) {
    SampleLayout l;
    l.nb = (long)((n_faces + SAMPLE_CHUNK - 1) / SAMPLE_CHUNK);
    size_t o = 0;
    l.hdr = o;      o += 256;                            // int32 status at 0, double total at 8
    l.local = o;    o += align256(sizeof(double) * (size_t)n_faces);
    l.blocksum = o; o += align256(sizeof(double) * (size_t)l.nb);
    l.blockoff = o; o += align256(sizeof(double) * (size_t)l.nb);
    l.total = o;
    return l;
}

struct SampleWs { int32_t* status; double* total; double* local; double* blocksum; double* blockoff; };

// areas in double and their inclusive prefix sums inside a chunk of SAMPLE_CHUNK faces, in a fixed association: four faces in a
// thread, the threads' offsets added up in thread order, so that the prefix never decreases
__global__ __launch_bounds__(THREADS) void sample_area_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                              const int32_t* __restrict__ faces, long n_faces, SampleWs ws) {
    __shared__ double s_tot[THREADS], s_off[THREADS];
    const int t = threadIdx.x;
    const long f0 = (long)blockIdx.x * SAMPLE_CHUNK + 4 * t;
    double run[4], acc = 0.0;
    for (int k = 0; k < 4; ++k) {
        double area = 0.0;
        const long f = f0 + k;
        if (f < n_faces) {
            V3 a, b, c;
            if (face_valid(vertices, n_vertices, faces, f, a, b, c)) {       // an invalid face has no area: it receives no sample
                const double ux = (double)b.x - a.x, uy = (double)b.y - a.y, uz = (double)b.z - a.z;
                const double vx = (double)c.x - a.x, vy = (double)c.y - a.y, vz = (double)c.z - a.z;
                const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
                area = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
            }
        }
        acc += area;
        run[k] = acc;
    }
    s_tot[t] = acc;
    __syncthreads();
    if (t == 0) {
        double off = 0.0;
        for (int k = 0; k < THREADS; ++k) { s_off[k] = off; off += s_tot[k]; }
        ws.blocksum[blockIdx.x] = off;
    }
    __syncthreads();
    for (int k = 0; k < 4; ++k)
        if (f0 + k < n_faces) ws.local[f0 + k] = s_off[t] + run[k];
}

__global__ void sample_scan_kernel(long nb, SampleWs ws) {
    double off = 0.0;
    for (long b = 0; b < nb; ++b) { ws.blockoff[b] = off; off += ws.blocksum[b]; }
    *ws.total = off;
    *ws.status = (off > 0.0 && isfinite(off)) ? GPNERF_SAMPLE_OK : GPNERF_SAMPLE_NO_AREA;
}

// murmur3's 32-bit finalizer (Appleby, MurmurHash3 fmix32)
DEV uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

DEV double prefix_at(const SampleWs& ws, long f) { return ws.blockoff[f / SAMPLE_CHUNK] + ws.local[f]; }

__global__ __launch_bounds__(THREADS) void sample_points_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                                long n_faces, long n_samples, uint32_t seed, SampleWs ws, float* points,
                                                                int32_t* sample_face, float* sample_normal) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_samples) return;
    if (*ws.status != GPNERF_SAMPLE_OK) {
        points[3 * i] = points[3 * i + 1] = points[3 * i + 2] = nanf_();
        if (sample_face) sample_face[i] = -1;
        if (sample_normal) sample_normal[3 * i] = sample_normal[3 * i + 1] = sample_normal[3 * i + 2] = nanf_();
        return;
    }
    const double target = ((double)i + 0.5) / (double)n_samples * *ws.total;
    long lo = 0, hi = n_faces - 1;                       // the first face whose prefix exceeds the target (the last one's does)
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (prefix_at(ws, mid) > target) hi = mid; else lo = mid + 1;
    }
    const long f = lo;                                   // its area is positive, so it is a valid face
    const V3 a = load3(vertices, faces[3 * f]), b = load3(vertices, faces[3 * f + 1]), c = load3(vertices, faces[3 * f + 2]);
    const uint32_t k = (uint32_t)i;
    const float r1 = (float)(fmix32(seed ^ fmix32(2u * k)) >> 8) * 5.9604644775390625e-8f;          // 2^-24: [0, 1)
    const float r2 = (float)(fmix32(seed ^ fmix32(2u * k + 1u)) >> 8) * 5.9604644775390625e-8f;
    const float s = sqrtf(r1), wa = 1.f - s, wb = s * (1.f - r2), wc = s * r2;
    points[3 * i] = (wa * a.x + wb * b.x) + wc * c.x;
    points[3 * i + 1] = (wa * a.y + wb * b.y) + wc * c.y;
    points[3 * i + 2] = (wa * a.z + wb * b.z) + wc * c.z;
    if (sample_face) sample_face[i] = (int32_t)f;
    if (sample_normal) {
        const V3 n = cross(sub(b, a), sub(c, a));
        const float len = sqrtf(dot(n, n));
        const bool ok = len > 0.f && isfinite(len);
        sample_normal[3 * i] = ok ? n.x / len : 0.f;
        sample_normal[3 * i + 1] = ok ? n.y / len : 0.f;
        sample_normal[3 * i + 2] = ok ? n.z / len : 0.f;
    }
}

// ---------------------------------------------------------------- stats

struct Thresholds { float v[GPNERF_DIST_MAX_THRESHOLDS]; int n; };

// one workgroup: every thread takes the values t, t + 256, ... in order, then a fixed tree over the threads
__global__ __launch_bounds__(STAT_THREADS) void distance_stats_kernel(const float* __restrict__ values, long n, Thresholds th, double* out) {
    __shared__ double s_sum[STAT_THREADS], s_sq[STAT_THREADS], s_max[STAT_THREADS];
    __shared__ long long s_cnt[3 + GPNERF_DIST_MAX_THRESHOLDS][STAT_THREADS];
    const int t = threadIdx.x;
    double sum = 0.0, sq = 0.0, mx = -INFINITY;
    long long cnt[3 + GPNERF_DIST_MAX_THRESHOLDS] = {};
    for (long i = t; i < n; i += STAT_THREADS) {
        const float v = values[i];
        if (v != v) { ++cnt[2]; continue; }
        if (isinf(v)) { ++cnt[1]; continue; }             // either sign: counted, within no threshold
        for (int k = 0; k < th.n; ++k) cnt[3 + k] += v <= th.v[k];
        ++cnt[0];
        sum += (double)v;
        sq += (double)v * (double)v;
        mx = fmax(mx, (double)v);
    }
    s_sum[t] = sum; s_sq[t] = sq; s_max[t] = mx;
    for (int k = 0; k < 3 + GPNERF_DIST_MAX_THRESHOLDS; ++k) s_cnt[k][t] = cnt[k];
    __syncthreads();
    for (int s = STAT_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            s_sum[t] += s_sum[t + s]; s_sq[t] += s_sq[t + s]; s_max[t] = fmax(s_max[t], s_max[t + s]);
            for (int k = 0; k < 3 + GPNERF_DIST_MAX_THRESHOLDS; ++k) s_cnt[k][t] += s_cnt[k][t + s];
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double finite = (double)s_cnt[0][0], inf = (double)s_cnt[1][0];
    out[GPNERF_DIST_FINITE] = finite;
    out[GPNERF_DIST_INF] = inf;
    out[GPNERF_DIST_NAN] = (double)s_cnt[2][0];
    out[GPNERF_DIST_MEAN] = finite > 0.0 ? s_sum[0] / finite : nan;
    out[GPNERF_DIST_MEAN_SQ] = finite > 0.0 ? s_sq[0] / finite : nan;
    out[GPNERF_DIST_MAX] = finite > 0.0 ? s_max[0] : nan;
    for (int k = 0; k < GPNERF_DIST_MAX_THRESHOLDS; ++k)
        out[GPNERF_DIST_WITHIN + k] = (k < th.n && finite + inf > 0.0) ? (double)s_cnt[3 + k][0] / (finite + inf) : nan;
}

}  // namespace

extern "C" {

size_t gpnerf_mesh_grid_workspace_bytes(int64_t n_faces, int64_t cell_cap, int64_t entry_cap) {
    if (!grid_sizes_ok(n_faces, cell_cap, entry_cap)) return 0;
    return grid_layout(cell_cap, entry_cap).total;
}

int gpnerf_mesh_grid_build(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int64_t cell_cap,
                           int64_t entry_cap, void* workspace, size_t workspace_bytes, void* stream) {
    if (!vertices || !faces || !workspace || n_vertices < 0 || !grid_sizes_ok(n_faces, cell_cap, entry_cap)) return GPNERF_E_ARG;
    if (workspace_bytes < grid_layout(cell_cap, entry_cap).total) return GPNERF_E_ARG;
    const Grid g = grid_of(workspace, cell_cap, entry_cap);
    const int parts = (int)((n_faces + THREADS - 1) / THREADS < BOX_BLOCKS_MAX ? (n_faces + THREADS - 1) / THREADS : BOX_BLOCKS_MAX);
    const unsigned face_blocks = blocks_for(n_faces, THREADS / 64);
    hipLaunchKernelGGL(grid_box_kernel, dim3((unsigned)parts), dim3(THREADS), 0, S_(stream), vertices, n_vertices, faces, (long)n_faces, cell_cap, g);
    hipLaunchKernelGGL(grid_plan_kernel, dim3(1), dim3(THREADS), 0, S_(stream), parts, (long)n_faces, cell_cap, entry_cap, g);
    hipLaunchKernelGGL(grid_enter_kernel<false>, dim3(face_blocks), dim3(THREADS), 0, S_(stream), vertices, n_vertices, faces, (long)n_faces, g);
    hipLaunchKernelGGL(grid_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, S_(stream), g);
    hipLaunchKernelGGL(grid_enter_kernel<true>, dim3(face_blocks), dim3(THREADS), 0, S_(stream), vertices, n_vertices, faces, (long)n_faces, g);
    hipLaunchKernelGGL(grid_rank_kernel, dim3(blocks_for(entry_cap, THREADS)), dim3(THREADS), 0, S_(stream), g);
    return launch_status();
}

int gpnerf_mesh_distance(const float* points, int64_t n_points, const float* vertices, int64_t n_vertices, const int32_t* faces,
                         int64_t n_faces, void* grid_workspace, float max_dist, const float* query_normals, float* dist, int32_t* face,
                         float* closest, float* cosine, void* stream) {
    if (n_points < 0 || n_points > (int64_t)INT32_MAX * THREADS || n_vertices < 0 || n_faces < 1 || n_faces > MAX_FACES || !vertices || !faces)
        return GPNERF_E_ARG;
    if (!(max_dist > 0.f)) return GPNERF_E_ARG;           // zero, negative, NaN
    if ((cosine != nullptr) != (query_normals != nullptr)) return GPNERF_E_ARG;
    if (n_points == 0) return GPNERF_OK;
    if (!points || !dist || !face) return GPNERF_E_ARG;
    const unsigned blocks = blocks_for(n_points, THREADS);
    if (grid_workspace)
        hipLaunchKernelGGL(distance_grid_kernel, dim3(blocks), dim3(THREADS), 0, S_(stream), points, (long)n_points, vertices, n_vertices, faces,
                           (long)n_faces, grid_workspace, max_dist, query_normals, dist, face, closest, cosine);
    else
        hipLaunchKernelGGL(distance_brute_kernel, dim3(blocks), dim3(THREADS), 0, S_(stream), points, (long)n_points, vertices, n_vertices, faces,
                           (long)n_faces, max_dist, query_normals, dist, face, closest, cosine);
    return launch_status();
}

size_t gpnerf_mesh_sample_workspace_bytes(int64_t n_faces) {
    if (n_faces < 1 || n_faces > MAX_FACES) return 0;
    return sample_layout(n_faces).total;
}

int gpnerf_mesh_sample_surface(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, int64_t n_samples,
                               uint32_t seed, void* workspace, size_t workspace_bytes, float* points, int32_t* sample_face,
                               float* sample_normal, void* stream) {
    if (!vertices || !faces || !workspace || n_vertices < 0 || n_faces < 1 || n_faces > MAX_FACES || n_samples < 0 || n_samples > INT32_MAX)
        return GPNERF_E_ARG;
    const SampleLayout l = sample_layout(n_faces);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    if (n_samples == 0) return GPNERF_OK;
    if (!points) return GPNERF_E_ARG;
    char* base = static_cast<char*>(workspace);
    SampleWs ws;
    ws.status = reinterpret_cast<int32_t*>(base + l.hdr);
    ws.total = reinterpret_cast<double*>(base + l.hdr + 8);
    ws.local = reinterpret_cast<double*>(base + l.local);
    ws.blocksum = reinterpret_cast<double*>(base + l.blocksum);
    ws.blockoff = reinterpret_cast<double*>(base + l.blockoff);
    hipLaunchKernelGGL(sample_area_kernel, dim3((unsigned)l.nb), dim3(THREADS), 0, S_(stream), vertices, n_vertices, faces, (long)n_faces, ws);
    hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(1), 0, S_(stream), l.nb, ws);
    hipLaunchKernelGGL(sample_points_kernel, dim3(blocks_for(n_samples, THREADS)), dim3(THREADS), 0, S_(stream), vertices, faces, (long)n_faces,
                       (long)n_samples, seed, ws, points, sample_face, sample_normal);
    return launch_status();
}

int gpnerf_distance_stats(const float* values, int64_t n, const float* thresholds, int32_t n_thresholds, double* out, void* stream) {
    if (!out || n < 0 || (n > 0 && !values) || n_thresholds < 0 || n_thresholds > GPNERF_DIST_MAX_THRESHOLDS || (n_thresholds > 0 && !thresholds))
        return GPNERF_E_ARG;
    Thresholds th = {};
    th.n = n_thresholds;
    for (int k = 0; k < n_thresholds; ++k) th.v[k] = thresholds[k];
    hipLaunchKernelGGL(distance_stats_kernel, dim3(1), dim3(STAT_THREADS), 0, S_(stream), values, (long)n, th, out);
    return launch_status();
}

}  // extern "C"
