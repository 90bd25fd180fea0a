// gpnerf_simplify.hip -- simplifying a triangle mesh on gfx950 by quadric vertex clustering: the vertices of a cubic cell collapse to
// one point, the minimiser of the cell's plane quadric regularised toward the cell's centre and kept inside the cell; faces that lose
// a corner go, faces that fold onto each other cancel or merge by orientation.  include/gpnerf_hip.h states the definition, the
// summation order and the workspace formula; tests/simplify_cases.py restates it in numpy.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone;
// every data-dependent length (clusters, list entries, the two output sizes) stays in the workspace header.  No float atomics.  The
// integer atomics and the plain racing stores, and why their arrival order cannot matter:
//   - face_mark_kernel stores 1 into the cell of every corner of a valid face: every writer stores the same value;
//   - face_cluster_kernel adds 1 to a cluster's count per (face, distinct cluster) pair: integer addition commutes;
//   - list_fill_kernel draws a slot of the cluster's run from a cursor: the SET of faces in a run is the same in any order, and
//     list_rank_kernel then writes every face at (run start + number of smaller faces in the run), which is the ascending order;
//   - face_verdict_kernel stores 1 into the clusters of a kept face (same value), and the counters of the stats are integer sums.
// The quadrics are float64 sums in an order fixed by the sorted lists (position_kernel), one wavefront per cluster.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for; wave_count

#include "gpnerf_scan.h"       // the three-launch integer scan (shared with gpnerf_meshtopo.hip): SCAN_CHUNK, scan_launch

struct SimplifyScan;           // names this file's instances of the scan kernels

constexpr int THREADS = 256;
constexpr int64_t MAX_CELLS = (int64_t)1 << 26;
constexpr int64_t MAX_COUNT = ((int64_t)1 << 31) - 1;
constexpr long long SIMPLIFY_MAGIC = 0x53494d5031ll;     // "SIMP1"

typedef unsigned long long u64;

// the header's 64-bit words
enum { H_MAGIC, H_NV, H_NF, H_CLUSTERS, H_ENTRIES, H_OUT_V, H_OUT_F, H_INVALID, H_COLLAPSED, H_CANCELLED, H_DUPLICATE, H_CLAMPED,
       H_STATUS = GPNERF_SIMPLIFY_HDR_STATUS, H_CELLS, H_WORDS = H_CELLS + 3 };
static_assert(H_CLAMPED + 1 == H_STATUS && H_WORDS <= 32, "the header's words");

struct Layout { size_t hdr, vcell, fclu, fkeep, cl_cell, cl_cnt, cl_fill, cl_start, cl_used, cl_pos, tmp, entries, cellmap, bsum, total;
                int64_t scan_blocks; };

__host__ inline int64_t blocks_of(int64_t n, int64_t per) { return (n + per - 1) / per; }

// the formula of include/gpnerf_hip.h.  A mesh has at most one cluster per vertex, so the clusters' arrays are sized by n_vertices;
// the two regions whose size depends on the grid come last, so that gpnerf_mesh_simplify_emit, which is not told the grid, finds
// every region from the two counts alone.
__host__ inline Layout layout_of(int64_t nv, int64_t nf, int64_t n_cells) {
    Layout l;
    int64_t longest = n_cells > nf ? n_cells : nf;
    if (nv + 1 > longest) longest = nv + 1;
    l.scan_blocks = blocks_of(longest, SCAN_CHUNK);
    size_t o = 0;
    l.hdr = o;      o += 256;
    l.vcell = o;    o += align256(4 * (size_t)nv);
    l.fclu = o;     o += align256(12 * (size_t)nf);
    l.fkeep = o;    o += align256(4 * (size_t)nf);
    l.cl_cell = o;  o += align256(4 * (size_t)nv);
    l.cl_cnt = o;   o += align256(4 * (size_t)nv);
    l.cl_fill = o;  o += align256(4 * (size_t)nv);
    l.cl_used = o;  o += align256(4 * (size_t)nv);
    l.cl_start = o; o += align256(8 * (size_t)(nv + 1));
    l.cl_pos = o;   o += align256(12 * (size_t)nv);
    l.tmp = o;      o += align256(12 * (size_t)nf);
    l.entries = o;  o += align256(12 * (size_t)nf);
    l.cellmap = o;  o += align256(4 * (size_t)n_cells);
    l.bsum = o;     o += align256(8 * (size_t)l.scan_blocks);
    l.total = o;
    return l;
}

struct Ws {                                              // the workspace's regions, as the kernels see them
    long long* hdr; int32_t* vcell; int32_t* cellmap; int32_t* fclu; int32_t* fkeep; int32_t* cl_cell; int32_t* cl_cnt; int32_t* cl_fill;
    long long* cl_start; int32_t* cl_used; float* cl_pos; int32_t* tmp; int32_t* entries; long long* bsum;
};

__host__ inline Ws ws_of(void* workspace, const Layout& l) {
    char* b = static_cast<char*>(workspace);
    Ws w;
    w.hdr = reinterpret_cast<long long*>(b + l.hdr);
    w.vcell = reinterpret_cast<int32_t*>(b + l.vcell);
    w.fclu = reinterpret_cast<int32_t*>(b + l.fclu);
    w.fkeep = reinterpret_cast<int32_t*>(b + l.fkeep);
    w.cl_cell = reinterpret_cast<int32_t*>(b + l.cl_cell);
    w.cl_cnt = reinterpret_cast<int32_t*>(b + l.cl_cnt);
    w.cl_fill = reinterpret_cast<int32_t*>(b + l.cl_fill);
    w.cl_start = reinterpret_cast<long long*>(b + l.cl_start);
    w.cl_used = reinterpret_cast<int32_t*>(b + l.cl_used);
    w.cl_pos = reinterpret_cast<float*>(b + l.cl_pos);
    w.tmp = reinterpret_cast<int32_t*>(b + l.tmp);
    w.entries = reinterpret_cast<int32_t*>(b + l.entries);
    w.cellmap = reinterpret_cast<int32_t*>(b + l.cellmap);
    w.bsum = reinterpret_cast<long long*>(b + l.bsum);
    return w;
}

// the grid's number of cells, 0 for sizes the calls refuse
int64_t cells_of(int64_t nv, int64_t nf, const int32_t* cells) {
    if (!cells || nv < 0 || nf < 0 || nv > MAX_COUNT || nf > MAX_COUNT) return 0;
    int64_t prod = 1;
    for (int k = 0; k < 3; ++k) {
        if (cells[k] < 1) return 0;
        prod *= cells[k];                                // (each factor < 2^31 and the running product <= 2^26: no overflow)
        if (prod > MAX_CELLS) return 0;
    }
    return prod;
}

struct GridArgs { float lo[3]; float cell; int32_t cells[3]; };

// ---------------------------------------------------------------- clearing, cells, validity

__global__ __launch_bounds__(THREADS) void clear_kernel(Ws w, long n_cells, long nv, long nf, GridArgs g) {
    const long stride = (long)gridDim.x * THREADS, i0 = (long)blockIdx.x * THREADS + threadIdx.x;
    for (long i = i0; i < n_cells; i += stride) w.cellmap[i] = 0;
    for (long i = i0; i < nv; i += stride) { w.cl_cnt[i] = 0; w.cl_fill[i] = 0; w.cl_used[i] = 0; }
    if (i0 == 0) {
        for (int k = 0; k < 32; ++k) w.hdr[k] = 0;
        w.hdr[H_MAGIC] = SIMPLIFY_MAGIC;
        w.hdr[H_NV] = nv;
        w.hdr[H_NF] = nf;
        w.hdr[H_STATUS] = GPNERF_SIMPLIFY_COUNTING;
        for (int k = 0; k < 3; ++k) w.hdr[H_CELLS + k] = g.cells[k];
    }
}

// step 1: float32 subtraction, IEEE division, floor (the library builds with -ffp-contract=off)
__global__ __launch_bounds__(THREADS) void vertex_cell_kernel(const float* __restrict__ vertices, long nv, GridArgs g, Ws w) {
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= nv) return;
    int q[3];
    bool in = true;
    for (int k = 0; k < 3; ++k) {
        const float x = vertices[3 * v + k];
        const float t = floorf((x - g.lo[k]) / g.cell);
        in = in && isfinite(x) && t >= 0.f && t < (float)g.cells[k];       // (NaN t fails both comparisons)
        q[k] = in ? (int)t : 0;
    }
    w.vcell[v] = in ? (q[0] * g.cells[1] + q[1]) * g.cells[2] + q[2] : -1;
}

__global__ __launch_bounds__(THREADS) void face_mark_kernel(const int32_t* __restrict__ faces, long nf, long nv, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    bool invalid = false;
    if (f < nf) {
        int32_t c[3];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            const int32_t i = faces[3 * f + k];
            ok = ok && i >= 0 && i < nv;
            c[k] = ok ? w.vcell[i] : -1;
            ok = ok && c[k] >= 0;
        }
        if (ok) for (int k = 0; k < 3; ++k) w.cellmap[c[k]] = 1;
        w.fkeep[f] = ok ? 1 : 0;                         // valid, until face_verdict_kernel decides
        invalid = !ok;
    }
    wave_count(invalid, &w.hdr[H_INVALID]);
}

// ---------------------------------------------------------------- clusters and their face lists

// the distinct clusters among a face's three, in corner order
DEV int distinct_of(const int32_t* id, int32_t* out) {
    int n = 0;
    out[n++] = id[0];
    if (id[1] != id[0]) out[n++] = id[1];
    if (id[2] != id[0] && id[2] != id[1]) out[n++] = id[2];
    return n;
}

__global__ __launch_bounds__(THREADS) void face_cluster_kernel(const int32_t* __restrict__ faces, long nf, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= nf) return;
    int32_t id[3] = {-1, -1, -1};
    if (w.fkeep[f]) {
        for (int k = 0; k < 3; ++k) id[k] = w.cellmap[w.vcell[faces[3 * f + k]]];
        int32_t d[3];
        const int n = distinct_of(id, d);
        for (int k = 0; k < n; ++k) atomicAdd(&w.cl_cnt[d[k]], 1);
    }
    for (int k = 0; k < 3; ++k) w.fclu[3 * f + k] = id[k];
}

__global__ __launch_bounds__(THREADS) void list_fill_kernel(long nf, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= nf) return;
    const int32_t id[3] = {w.fclu[3 * f], w.fclu[3 * f + 1], w.fclu[3 * f + 2]};
    if (id[0] < 0) return;
    int32_t d[3];
    const int n = distinct_of(id, d);
    for (int k = 0; k < n; ++k) w.tmp[w.cl_start[d[k]] + atomicAdd(&w.cl_fill[d[k]], 1)] = (int32_t)f;
}

// one thread per (face, corner): the face's place in that cluster's run is the number of smaller faces there.  A long list is thus
// ranked by as many wavefronts as it has entries / 64, across the whole device, every lane walking the same words.
__global__ __launch_bounds__(THREADS) void list_rank_kernel(long nf, Ws w) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    const long f = e / 3;
    const int k = (int)(e - 3 * f);
    if (f >= nf) return;
    const int32_t id[3] = {w.fclu[3 * f], w.fclu[3 * f + 1], w.fclu[3 * f + 2]};
    if (id[0] < 0) return;
    if ((k == 1 && id[1] == id[0]) || (k == 2 && (id[2] == id[0] || id[2] == id[1]))) return;    // entered once per distinct cluster
    const long long s = w.cl_start[id[k]], end = w.cl_start[id[k] + 1];
    long long rank = 0;
#pragma unroll 8                                         // (eight independent loads in flight: the walk waits on memory, not on the adds)
    for (long long j = s; j < end; ++j) rank += w.tmp[j] < (int32_t)f;
    w.entries[s + rank] = (int32_t)f;
}

// ---------------------------------------------------------------- positions

// steps 4 and 5 of the definition, float64, written out operation by operation (tests/simplify_cases.py spells the same ones)
__global__ __launch_bounds__(THREADS) void position_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, GridArgs g, Ws w) {
    __shared__ double s_part[THREADS / 64][9][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long id = (long)blockIdx.x * (THREADS / 64) + wave;
    const bool live = id < (long)w.hdr[H_CLUSTERS];      // (uniform in the wavefront)
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // Axx Axy Axz Ayy Ayz Azz bx by bz
    if (live) {
        const long long s = w.cl_start[id], end = w.cl_start[id + 1];
        for (long long j = s + lane; j < end; j += 64) {                // partial `lane`: entries lane, lane + 64, ... in order
            const long f = w.entries[j];
            const long i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            const double p0x = vertices[3 * i0], p0y = vertices[3 * i0 + 1], p0z = vertices[3 * i0 + 2];
            const double ax = (double)vertices[3 * i1] - p0x, ay = (double)vertices[3 * i1 + 1] - p0y, az = (double)vertices[3 * i1 + 2] - p0z;
            const double bx = (double)vertices[3 * i2] - p0x, by = (double)vertices[3 * i2 + 1] - p0y, bz = (double)vertices[3 * i2 + 2] - p0z;
            const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            const double l = sqrt((nx * nx + ny * ny) + nz * nz);
            if (l == 0.0) continue;
            const double ux = nx / l, uy = ny / l, uz = nz / l, wt = 0.5 * l;
            const double d = -((ux * p0x + uy * p0y) + uz * p0z);
            const double wx = wt * ux, wy = wt * uy, wz = wt * uz, wd = wt * d;
            acc[0] += wx * ux; acc[1] += wx * uy; acc[2] += wx * uz; acc[3] += wy * uy; acc[4] += wy * uz; acc[5] += wz * uz;
            acc[6] += wd * ux; acc[7] += wd * uy; acc[8] += wd * uz;
        }
    }
    for (int k = 0; k < 9; ++k) s_part[wave][k][lane] = acc[k];
    __syncthreads();
    if (live && lane < 9) {                              // the partials, added in order 0 .. 63 (row `lane` is this lane's alone)
        double sum = s_part[wave][lane][0];
        for (int j = 1; j < 64; ++j) sum += s_part[wave][lane][j];
        s_part[wave][lane][0] = sum;
    }
    __syncthreads();
    if (!live || lane != 0) return;
    const double Axx = s_part[wave][0][0], Axy = s_part[wave][1][0], Axz = s_part[wave][2][0], Ayy = s_part[wave][3][0],
                 Ayz = s_part[wave][4][0], Azz = s_part[wave][5][0], bx = s_part[wave][6][0], by = s_part[wave][7][0], bz = s_part[wave][8][0];
    const int32_t cell = w.cl_cell[id];
    const int q[3] = {cell / (g.cells[1] * g.cells[2]), (cell / g.cells[2]) % g.cells[1], cell % g.cells[2]};
    double c[3], blo[3], bhi[3];
    for (int k = 0; k < 3; ++k) {
        c[k] = (double)g.lo[k] + ((double)q[k] + 0.5) * (double)g.cell;
        blo[k] = (double)g.lo[k] + (double)q[k] * (double)g.cell;
        bhi[k] = (double)g.lo[k] + ((double)q[k] + 1.0) * (double)g.cell;
    }
    double x[3] = {c[0], c[1], c[2]};
    const double lam = (1e-3 * ((Axx + Ayy) + Azz)) / 3.0;
    if (lam != 0.0) {
        const double m00 = Axx + lam, m11 = Ayy + lam, m22 = Azz + lam;
        const double r0 = ((Axx * c[0] + Axy * c[1]) + Axz * c[2]) + bx;
        const double r1 = ((Axy * c[0] + Ayy * c[1]) + Ayz * c[2]) + by;
        const double r2 = ((Axz * c[0] + Ayz * c[1]) + Azz * c[2]) + bz;
        const double l00 = sqrt(m00), l10 = Axy / l00, l20 = Axz / l00;
        const double l11 = sqrt(m11 - l10 * l10), l21 = (Ayz - l20 * l10) / l11;
        const double l22 = sqrt((m22 - l20 * l20) - l21 * l21);
        const double y0 = r0 / l00, y1 = (r1 - l10 * y0) / l11, y2 = ((r2 - l20 * y0) - l21 * y1) / l22;
        const double s2 = y2 / l22, s1 = (y1 - l21 * s2) / l11, s0 = ((y0 - l10 * s1) - l20 * s2) / l00;
        const double t[3] = {c[0] - s0, c[1] - s1, c[2] - s2};
        if (isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2])) { x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; }
    }
    bool moved = false;
    for (int k = 0; k < 3; ++k) {
        const double y = x[k] < blo[k] ? blo[k] : (x[k] > bhi[k] ? bhi[k] : x[k]);
        moved = moved || y != x[k];
        w.cl_pos[3 * id + k] = (float)y;
    }
    if (moved) atomicAdd(reinterpret_cast<u64*>(&w.hdr[H_CLAMPED]), (u64)1);
}

// ---------------------------------------------------------------- faces

DEV void sort3(const int32_t* id, int32_t* s, int& parity) {
    int32_t a = id[0], b = id[1], c = id[2], t;
    parity = 1;
    if (a > b) { t = a; a = b; b = t; parity = -parity; }
    if (b > c) { t = b; b = c; c = t; parity = -parity; }
    if (a > b) { t = a; a = b; b = t; parity = -parity; }
    s[0] = a; s[1] = b; s[2] = c;
}

// step 6: one thread per face.  The group of a face (the faces with its sorted triple) lies wholly in the list of each of its three
// clusters; the shortest of the three is walked (a tie: the earlier corner).
__global__ __launch_bounds__(THREADS) void face_verdict_kernel(long nf, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    bool collapsed = false;
    if (f < nf && w.fkeep[f]) {
        const int32_t id[3] = {w.fclu[3 * f], w.fclu[3 * f + 1], w.fclu[3 * f + 2]};
        collapsed = id[0] == id[1] || id[1] == id[2] || id[0] == id[2];
        bool keep = false;
        if (!collapsed) {
            int32_t mine[3];
            int parity;
            sort3(id, mine, parity);
            int32_t walk = id[0];
            long long len = w.cl_start[id[0] + 1] - w.cl_start[id[0]];
            for (int k = 1; k < 3; ++k) {
                const long long lk = w.cl_start[id[k] + 1] - w.cl_start[id[k]];
                if (lk < len) { len = lk; walk = id[k]; }
            }
            const long long s = w.cl_start[walk];
            long long pos = 0, neg = 0;
            int32_t first_pos = INT32_MAX, first_neg = INT32_MAX;       // the lowest face of either parity
            for (long long j = s; j < s + len; ++j) {
                const int32_t h = w.entries[j];
                const int32_t o[3] = {w.fclu[3 * (long)h], w.fclu[3 * (long)h + 1], w.fclu[3 * (long)h + 2]};
                int32_t theirs[3];
                int p;
                sort3(o, theirs, p);
                if (theirs[0] != mine[0] || theirs[1] != mine[1] || theirs[2] != mine[2]) continue;
                if (p > 0) { ++pos; first_pos = min(first_pos, h); } else { ++neg; first_neg = min(first_neg, h); }
            }
            const long long net = pos - neg;
            keep = net != 0 && (int32_t)f == (net > 0 ? first_pos : first_neg);
            if ((int32_t)f == min(first_pos, first_neg)) {               // the group is counted once, by its lowest face
                const long long pairs = pos < neg ? pos : neg, surplus = (net < 0 ? -net : net) - 1;
                if (pairs) atomicAdd(reinterpret_cast<u64*>(&w.hdr[H_CANCELLED]), (u64)(2 * pairs));
                if (surplus > 0) atomicAdd(reinterpret_cast<u64*>(&w.hdr[H_DUPLICATE]), (u64)surplus);
            }
            if (keep) for (int k = 0; k < 3; ++k) w.cl_used[id[k]] = 1;
        }
        w.fkeep[f] = keep ? 1 : 0;
    }
    wave_count(collapsed, &w.hdr[H_COLLAPSED]);
}

__global__ void finish_kernel(Ws w, int64_t* stats) {
    stats[GPNERF_SIMPLIFY_VERTICES_OUT] = w.hdr[H_OUT_V];
    stats[GPNERF_SIMPLIFY_FACES_OUT] = w.hdr[H_OUT_F];
    stats[GPNERF_SIMPLIFY_FACES_INVALID] = w.hdr[H_INVALID];
    stats[GPNERF_SIMPLIFY_FACES_COLLAPSED] = w.hdr[H_COLLAPSED];
    stats[GPNERF_SIMPLIFY_FACES_CANCELLED] = w.hdr[H_CANCELLED];
    stats[GPNERF_SIMPLIFY_FACES_DUPLICATE] = w.hdr[H_DUPLICATE];
    stats[GPNERF_SIMPLIFY_CLUSTERS_CLAMPED] = w.hdr[H_CLAMPED];
    stats[GPNERF_SIMPLIFY_CLUSTERS_DROPPED] = w.hdr[H_CLUSTERS] - w.hdr[H_OUT_V];
    w.hdr[H_STATUS] = GPNERF_SIMPLIFY_COUNTED;
}

// ---------------------------------------------------------------- emit

// one thread: the sizes the caller brought against those counted
__global__ void emit_check_kernel(Ws w, long nv, long nf, long n_out_v, long n_out_f) {
    const long long st = w.hdr[H_STATUS];
    const bool counted = w.hdr[H_MAGIC] == SIMPLIFY_MAGIC && (st == GPNERF_SIMPLIFY_COUNTED || st == GPNERF_SIMPLIFY_EMITTED || st == GPNERF_SIMPLIFY_MISMATCH);
    if (!counted) return;                                // (nothing to compare with: the emit kernels write nothing either)
    const bool same = w.hdr[H_NV] == nv && w.hdr[H_NF] == nf && w.hdr[H_OUT_V] == n_out_v && w.hdr[H_OUT_F] == n_out_f;
    w.hdr[H_STATUS] = same ? GPNERF_SIMPLIFY_EMITTED : GPNERF_SIMPLIFY_MISMATCH;
}

DEV bool emit_ok(const Ws& w) { return w.hdr[H_MAGIC] == SIMPLIFY_MAGIC && w.hdr[H_STATUS] == GPNERF_SIMPLIFY_EMITTED; }

__global__ __launch_bounds__(THREADS) void emit_vertices_kernel(Ws w, float* out_vertices) {
    const long id = (long)blockIdx.x * THREADS + threadIdx.x;
    if (!emit_ok(w) || id >= (long)w.hdr[H_CLUSTERS]) return;
    const int32_t v = w.cl_used[id];
    if (v < 0) return;
    for (int k = 0; k < 3; ++k) out_vertices[3 * (long)v + k] = w.cl_pos[3 * id + k];
}

__global__ __launch_bounds__(THREADS) void emit_faces_kernel(Ws w, long nf, int32_t* out_faces) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    if (!emit_ok(w) || f >= nf) return;
    const int32_t o = w.fkeep[f];
    if (o < 0) return;
    for (int k = 0; k < 3; ++k) out_faces[3 * (long)o + k] = w.cl_used[w.fclu[3 * f + k]];
}

__global__ __launch_bounds__(THREADS) void emit_map_kernel(Ws w, long nv, int32_t* vertex_map) {
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    if (!emit_ok(w) || v >= nv) return;
    const int32_t cell = w.vcell[v];
    const int32_t id = cell >= 0 ? w.cellmap[cell] : -1;
    vertex_map[v] = (id >= 0 && w.hdr[H_OUT_V] > 0) ? w.cl_used[id] : -1;          // (no output vertex: the cell map was never numbered)
}

// a scan over n items (n >= 1, host-known) with the workspace's block sums
template <int MODE>
void scan(const int32_t* in, int64_t n, const long long* n_dev, const Ws& w, long long* total_out, long long* out64, int32_t* out32,
          int32_t* inverse, hipStream_t st) {
    scan_launch<SimplifyScan, MODE>(in, n, n_dev, w.bsum, total_out, out64, out32, inverse, st);
}

}  // namespace

extern "C" {

size_t gpnerf_mesh_simplify_workspace_bytes(int64_t n_vertices, int64_t n_faces, const int32_t* cells) {
    const int64_t n_cells = cells_of(n_vertices, n_faces, cells);
    return n_cells ? layout_of(n_vertices, n_faces, n_cells).total : 0;
}

int gpnerf_mesh_simplify_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float* lo, float cell,
                               const int32_t* cells, void* workspace, size_t workspace_bytes, int64_t* stats, void* stream) {
    const int64_t n_cells = cells_of(n_vertices, n_faces, cells);
    if (!lo || !workspace || !stats || !n_cells) return GPNERF_E_ARG;
    if ((!vertices && n_vertices > 0) || (!faces && n_faces > 0)) return GPNERF_E_ARG;
    if (!(cell > 0.f) || !isfinite(cell)) return GPNERF_E_ARG;
    for (int k = 0; k < 3; ++k) if (!isfinite(lo[k])) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces, n_cells);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    const Ws w = ws_of(workspace, l);
    GridArgs g;
    for (int k = 0; k < 3; ++k) { g.lo[k] = lo[k]; g.cells[k] = cells[k]; }
    g.cell = cell;
    hipStream_t st = S_(stream);
    const long nv = (long)n_vertices, nf = (long)n_faces;
    const int64_t clear_items = n_cells > nv ? n_cells : nv;
    hipLaunchKernelGGL(clear_kernel, dim3(blocks_for(clear_items < (1 << 22) ? clear_items : (1 << 22), THREADS)), dim3(THREADS), 0, st, w,
                       (long)n_cells, nv, nf, g);
    if (nv > 0) hipLaunchKernelGGL(vertex_cell_kernel, dim3(blocks_for(nv, THREADS)), dim3(THREADS), 0, st, vertices, nv, g, w);
    if (nf > 0 && nv > 0) {
        const unsigned fb = blocks_for(nf, THREADS);
        hipLaunchKernelGGL(face_mark_kernel, dim3(fb), dim3(THREADS), 0, st, faces, nf, nv, w);
        scan<1>(w.cellmap, n_cells, nullptr, w, &w.hdr[H_CLUSTERS], nullptr, w.cellmap, w.cl_cell, st);
        hipLaunchKernelGGL(face_cluster_kernel, dim3(fb), dim3(THREADS), 0, st, faces, nf, w);
        scan<0>(w.cl_cnt, nv + 1, &w.hdr[H_CLUSTERS], w, &w.hdr[H_ENTRIES], w.cl_start, nullptr, nullptr, st);
        hipLaunchKernelGGL(list_fill_kernel, dim3(fb), dim3(THREADS), 0, st, nf, w);
        hipLaunchKernelGGL(list_rank_kernel, dim3(blocks_for(3 * n_faces, THREADS)), dim3(THREADS), 0, st, nf, w);
        hipLaunchKernelGGL(position_kernel, dim3(blocks_for(nv, THREADS / 64)), dim3(THREADS), 0, st, vertices, faces, g, w);
        hipLaunchKernelGGL(face_verdict_kernel, dim3(fb), dim3(THREADS), 0, st, nf, w);
        scan<1>(w.fkeep, nf, nullptr, w, &w.hdr[H_OUT_F], nullptr, w.fkeep, nullptr, st);
        scan<1>(w.cl_used, nv, &w.hdr[H_CLUSTERS], w, &w.hdr[H_OUT_V], nullptr, w.cl_used, nullptr, st);
    } else if (nf > 0) {                                 // no vertex: every face is invalid
        hipLaunchKernelGGL(face_mark_kernel, dim3(blocks_for(nf, THREADS)), dim3(THREADS), 0, st, faces, nf, nv, w);
    }
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1), 0, st, w, stats);
    return launch_status();
}

int gpnerf_mesh_simplify_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, void* workspace,
                              size_t workspace_bytes, int64_t n_out_vertices, int64_t n_out_faces, float* out_vertices, int32_t* out_faces,
                              int32_t* vertex_map, void* stream) {
    if (!workspace || n_vertices < 0 || n_faces < 0 || n_vertices > MAX_COUNT || n_faces > MAX_COUNT) return GPNERF_E_ARG;
    if ((!vertices && n_vertices > 0) || (!faces && n_faces > 0)) return GPNERF_E_ARG;
    if (n_out_vertices < 0 || n_out_faces < 0 || n_out_vertices > n_vertices || n_out_faces > n_faces) return GPNERF_E_ARG;
    if ((!out_vertices && n_out_vertices > 0) || (!out_faces && n_out_faces > 0)) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces, 1);   // (the regions up to the cell map do not depend on the grid)
    if (workspace_bytes < l.total) return GPNERF_E_ARG;   // the smallest workspace any grid needs
    const Ws w = ws_of(workspace, l);
    hipStream_t st = S_(stream);
    hipLaunchKernelGGL(emit_check_kernel, dim3(1), dim3(1), 0, st, w, (long)n_vertices, (long)n_faces, (long)n_out_vertices, (long)n_out_faces);
    if (n_out_vertices > 0)
        hipLaunchKernelGGL(emit_vertices_kernel, dim3(blocks_for(n_vertices, THREADS)), dim3(THREADS), 0, st, w, out_vertices);
    if (n_out_faces > 0)
        hipLaunchKernelGGL(emit_faces_kernel, dim3(blocks_for(n_faces, THREADS)), dim3(THREADS), 0, st, w, (long)n_faces, out_faces);
    if (vertex_map && n_vertices > 0)
        hipLaunchKernelGGL(emit_map_kernel, dim3(blocks_for(n_vertices, THREADS)), dim3(THREADS), 0, st, w, (long)n_vertices, vertex_map);
    return launch_status();
}

}  // extern "C"
