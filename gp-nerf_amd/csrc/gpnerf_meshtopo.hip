// gpnerf_meshtopo.hip -- the adjacency of a triangle mesh on gfx950: its unique undirected edges with their classes (boundary,
// manifold, inconsistent, non-manifold), the topology counts that follow from them, every vertex's unique neighbours as a CSR in
// ascending index, and Taubin's lambda | mu smoothing over that CSR.  include/gpnerf_hip.h states the definition, the order of the
// sums and the workspace formula; tests/smooth_cases.py restates it in numpy.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone;
// every data-dependent length (half-edges, neighbour entries) stays in the workspace.  No float atomics; the smoothing has no atomic
// at all.  The integer atomics and the plain racing stores of the build, and why their arrival order cannot matter:
//   - face_count_kernel adds 1 to the list length of a half-edge's lower vertex (integer addition commutes) and stores FLAG_REFERENCED
//     into the flags of a usable face's corners: every writer of the launch stores the same value;
//   - halfedge_fill_kernel draws a slot of the vertex's run from a cursor: the SET of keys in a run is the same in any order, and
//     nothing reads a run's order -- edge_kernel only counts over it;
//   - edge_kernel: the head of an edge (the lowest key among its half-edges) adds 1 to both ends' degrees and to its class's counter, and
//     stores FLAG_REFERENCED | FLAG_BOUNDARY into both ends' flags where the edge is open or non-manifold (same value again: a vertex
//     on an edge is referenced);
//   - neighbour_fill_kernel draws slots by cursor, and neighbour_rank_kernel writes every neighbour at (run start + number of smaller
//     neighbours in the run), which is the ascending order: a vertex's neighbours are distinct because the edges are.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for; wave_count
#include "gpnerf_scan.h"       // the three-launch integer scan (shared with gpnerf_simplify.hip)

struct TopoScan;               // names this file's instances of the scan kernels

constexpr int THREADS = 256;
constexpr int64_t MAX_VERTICES = ((int64_t)1 << 31) - 1;
constexpr int64_t MAX_FACES = (((int64_t)1 << 31) - 1) / 3;  // a half-edge's number 3 f + k fits 31 bits
constexpr int64_t MAX_ITERATIONS = 10000;
constexpr long long TOPO_MAGIC = 0x544f504f31ll;         // "TOPO1"
constexpr uint8_t FLAG_REFERENCED = GPNERF_VERTEX_REFERENCED, FLAG_BOUNDARY = GPNERF_VERTEX_BOUNDARY;

typedef unsigned long long u64;

// the header's 64-bit words
enum { H_MAGIC, H_NV, H_NF, H_DONE, H_HALFEDGES, H_ENTRIES, H_BOUNDARY, H_NONMANIFOLD, H_INCONSISTENT,
       H_VREF, H_VBOUNDARY, H_MAX_VALENCE, H_WORDS };
static_assert(H_WORDS <= 32, "the header's words");

// the formula of include/gpnerf_hip.h.  Everything gpnerf_mesh_smooth touches except the neighbours sits in front of the regions
// sized by n_faces, and the neighbours come first among those: smooth, which is not told n_faces, finds its regions from n_vertices.
struct Layout { size_t hdr, start, vflags, pos0, pos1, he_start, he_cnt, he_fill, deg, nb_fill, bsum, neighbours, keys, head, total; };

__host__ inline Layout layout_of(int64_t nv, int64_t nf) {
    Layout l;
    size_t o = 0;
    l.hdr = o;        o += 256;
    l.start = o;      o += align256(8 * (size_t)(nv + 1));
    l.vflags = o;     o += align256((size_t)nv);
    l.pos0 = o;       o += align256(16 * (size_t)nv);
    l.pos1 = o;       o += align256(16 * (size_t)nv);
    l.he_start = o;   o += align256(8 * (size_t)(nv + 1));
    l.he_cnt = o;     o += align256(4 * (size_t)(nv + 1));
    l.he_fill = o;    o += align256(4 * (size_t)nv);
    l.deg = o;        o += align256(4 * (size_t)(nv + 1));
    l.nb_fill = o;    o += align256(4 * (size_t)nv);
    l.bsum = o;       o += align256(8 * (size_t)((nv + SCAN_CHUNK) / SCAN_CHUNK));       // ceil((nv + 1) / 2048) block sums
    l.neighbours = o; o += align256(24 * (size_t)nf);
    l.keys = o;       o += align256(24 * (size_t)nf);     // 3 nf half-edge keys of 8 bytes, then 6 nf unsorted neighbour entries of 4
    l.head = o;       o += align256(3 * (size_t)nf);
    l.total = o;
    return l;
}

struct Ws {                                              // the workspace's regions, as the kernels see them
    long long* hdr; long long* start; uint8_t* vflags; float4* pos[2]; long long* he_start; int32_t* he_cnt; int32_t* he_fill; int32_t* deg;
    int32_t* nb_fill; long long* bsum; int32_t* neighbours; u64* keys; int32_t* nb_tmp; uint8_t* head;
};

__host__ inline Ws ws_of(void* workspace, const Layout& l) {
    char* b = static_cast<char*>(workspace);
    Ws w;
    w.hdr = reinterpret_cast<long long*>(b + l.hdr);
    w.start = reinterpret_cast<long long*>(b + l.start);
    w.vflags = reinterpret_cast<uint8_t*>(b + l.vflags);
    w.pos[0] = reinterpret_cast<float4*>(b + l.pos0);
    w.pos[1] = reinterpret_cast<float4*>(b + l.pos1);
    w.he_start = reinterpret_cast<long long*>(b + l.he_start);
    w.he_cnt = reinterpret_cast<int32_t*>(b + l.he_cnt);
    w.he_fill = reinterpret_cast<int32_t*>(b + l.he_fill);
    w.deg = reinterpret_cast<int32_t*>(b + l.deg);
    w.nb_fill = reinterpret_cast<int32_t*>(b + l.nb_fill);
    w.bsum = reinterpret_cast<long long*>(b + l.bsum);
    w.neighbours = reinterpret_cast<int32_t*>(b + l.neighbours);
    w.keys = reinterpret_cast<u64*>(b + l.keys);
    w.nb_tmp = reinterpret_cast<int32_t*>(b + l.keys);   // (the keys are dead once the edges are classified)
    w.head = reinterpret_cast<uint8_t*>(b + l.head);
    return w;
}

bool sizes_ok(int64_t nv, int64_t nf) { return nv >= 0 && nf >= 0 && nv <= MAX_VERTICES && nf <= MAX_FACES; }

// a face's corners when it is usable: indices in [0, nv), pairwise distinct
DEV bool usable_face(const int32_t* __restrict__ faces, long f, long nv, int32_t* c) {
    for (int k = 0; k < 3; ++k) c[k] = faces[3 * f + k];
    return c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] < nv && c[1] < nv && c[2] < nv && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

// the key of half-edge k of face f, a -> b: (the higher end, 3 f + k, 1 when it runs from the higher end to the lower)
DEV u64 key_of(int32_t a, int32_t b, long f, int k) {
    return ((u64)(uint32_t)(a > b ? a : b) << 32) | ((u64)(3 * f + k) << 1) | (u64)(a > b);
}

// ---------------------------------------------------------------- the build

__global__ __launch_bounds__(THREADS) void topology_clear_kernel(Ws w, long nv, long nf) {
    const long stride = (long)gridDim.x * THREADS, i0 = (long)blockIdx.x * THREADS + threadIdx.x;
    for (long i = i0; i <= nv; i += stride) {
        w.he_cnt[i] = 0;
        w.deg[i] = 0;
        if (i < nv) { w.he_fill[i] = 0; w.nb_fill[i] = 0; w.vflags[i] = 0; }
    }
    if (i0 == 0) {
        for (int k = 0; k < 32; ++k) w.hdr[k] = 0;
        w.hdr[H_MAGIC] = TOPO_MAGIC;
        w.hdr[H_NV] = nv;
        w.hdr[H_NF] = nf;
    }
}

__global__ __launch_bounds__(THREADS) void face_count_kernel(const int32_t* __restrict__ faces, long nf, long nv, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    int32_t c[3];
    const bool ok = f < nf && usable_face(faces, f, nv, c);
    if (ok) {
        for (int k = 0; k < 3; ++k) {
            const int32_t a = c[k], b = c[k == 2 ? 0 : k + 1];
            atomicAdd(&w.he_cnt[a < b ? a : b], 1);
            w.vflags[a] = FLAG_REFERENCED;
        }
    }
}                                                        // (the used faces are counted by the scan: a third of the half-edges)

__global__ __launch_bounds__(THREADS) void halfedge_fill_kernel(const int32_t* __restrict__ faces, long nf, long nv, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    int32_t c[3];
    if (f >= nf || !usable_face(faces, f, nv, c)) return;
    for (int k = 0; k < 3; ++k) {
        const int32_t a = c[k], b = c[k == 2 ? 0 : k + 1], lo = a < b ? a : b;
        w.keys[w.he_start[lo] + atomicAdd(&w.he_fill[lo], 1)] = key_of(a, b, f, k);
    }
}

// one thread per (face, corner), i.e. per half-edge: a walk over the run of its lower vertex counts the half-edges of the same edge
// (same higher end) by direction and those among them with a smaller key.  The half-edge with none smaller is the edge's HEAD: it
// classifies the edge, counts it, and adds 1 to both ends' degrees.  Quadratic in a run's length, but spread over as many lanes as the
// run has entries, the lanes of a wavefront mostly walking the same words.
__global__ __launch_bounds__(THREADS) void edge_kernel(const int32_t* __restrict__ faces, long nf, long nv, Ws w) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    const long f = e / 3;
    const int k = (int)(e - 3 * f);
    int32_t c[3];
    bool head = false;
    long long fwd = 0, bwd = 0;
    if (f < nf) {
        int32_t lo = 0, hi = 0;
        if (usable_face(faces, f, nv, c)) {
            const int32_t a = c[k], b = c[k == 2 ? 0 : k + 1];
            lo = a < b ? a : b;
            hi = a < b ? b : a;
            const u64 mine = key_of(a, b, f, k);
            const long long s = w.he_start[lo], end = w.he_start[lo + 1];
            long long smaller = 0;
#pragma unroll 4
            for (long long j = s; j < end; ++j) {
                const u64 other = w.keys[j];
                const bool same = (uint32_t)(other >> 32) == (uint32_t)hi;
                smaller += same && other < mine;
                bwd += same && (other & 1);
                fwd += same && !(other & 1);
            }
            head = smaller == 0;
        }
        w.head[e] = head ? 1 : 0;
        if (head) {
            atomicAdd(&w.deg[lo], 1);
            atomicAdd(&w.deg[hi], 1);
            if (fwd + bwd != 2) { w.vflags[lo] = FLAG_REFERENCED | FLAG_BOUNDARY; w.vflags[hi] = FLAG_REFERENCED | FLAG_BOUNDARY; }
        }
    }
    const long long m = fwd + bwd;
    // (the edges are counted by the scan over the degrees: half its total; the three classes below are rare on a closed mesh)
    wave_count(head && m == 1, &w.hdr[H_BOUNDARY]);
    wave_count(head && m >= 3, &w.hdr[H_NONMANIFOLD]);
    wave_count(head && m == 2 && fwd != bwd, &w.hdr[H_INCONSISTENT]);
}

__global__ __launch_bounds__(THREADS) void neighbour_fill_kernel(const int32_t* __restrict__ faces, long nf, Ws w) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    const long f = e / 3;
    const int k = (int)(e - 3 * f);
    if (f >= nf || !w.head[e]) return;                   // (a head's face is usable)
    const int32_t a = faces[3 * f + k], b = faces[3 * f + (k == 2 ? 0 : k + 1)];
    w.nb_tmp[w.start[a] + atomicAdd(&w.nb_fill[a], 1)] = b;
    w.nb_tmp[w.start[b] + atomicAdd(&w.nb_fill[b], 1)] = a;
}

// the number of entries of v's unsorted run below x: x's place in the ascending run
DEV long long rank_in(const Ws& w, int32_t v, int32_t x) {
    const long long s = w.start[v], end = w.start[v + 1];
    long long rank = 0;
#pragma unroll 8                                         // (eight independent loads in flight: the walk waits on memory, not on the adds)
    for (long long j = s; j < end; ++j) rank += w.nb_tmp[j] < x;
    return s + rank;
}

// one thread per head: both ends' entries go to their places.  Quadratic in a valence, spread over as many lanes as the vertex has edges.
__global__ __launch_bounds__(THREADS) void neighbour_rank_kernel(const int32_t* __restrict__ faces, long nf, Ws w) {
    const long e = (long)blockIdx.x * THREADS + threadIdx.x;
    const long f = e / 3;
    const int k = (int)(e - 3 * f);
    if (f >= nf || !w.head[e]) return;
    const int32_t a = faces[3 * f + k], b = faces[3 * f + (k == 2 ? 0 : k + 1)];
    w.neighbours[rank_in(w, a, b)] = b;
    w.neighbours[rank_in(w, b, a)] = a;
}

// a lane per vertex: the counts over the vertices (the caller-visible flags are already in place), reduced per workgroup so that the
// three counters see one atomic each per 256 vertices
__global__ __launch_bounds__(THREADS) void vertex_count_kernel(long nv, Ws w) {
    __shared__ long long s_part[THREADS / 64][3];
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    uint8_t fl = 0;
    long long valence = 0;
    if (v < nv) {
        fl = w.vflags[v];
        valence = w.start[v + 1] - w.start[v];
    }
    const u64 referenced = __ballot(fl & FLAG_REFERENCED), boundary = __ballot(fl & FLAG_BOUNDARY);
    for (int off = 32; off > 0; off >>= 1) {             // the wavefront's largest valence
        const long long o = __shfl_xor(valence, off);
        valence = o > valence ? o : valence;
    }
    if ((threadIdx.x & 63) == 0) {
        s_part[wave][0] = __popcll(referenced);
        s_part[wave][1] = __popcll(boundary);
        s_part[wave][2] = valence;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long n_ref = 0, n_bnd = 0, top = 0;
    for (int k = 0; k < THREADS / 64; ++k) {
        n_ref += s_part[k][0];
        n_bnd += s_part[k][1];
        top = s_part[k][2] > top ? s_part[k][2] : top;
    }
    if (n_ref) atomicAdd(reinterpret_cast<u64*>(&w.hdr[H_VREF]), (u64)n_ref);
    if (n_bnd) atomicAdd(reinterpret_cast<u64*>(&w.hdr[H_VBOUNDARY]), (u64)n_bnd);
    if (top) atomicMax(reinterpret_cast<u64*>(&w.hdr[H_MAX_VALENCE]), (u64)top);
}

__global__ void topology_finish_kernel(Ws w, int64_t* stats) {
    const long long used = w.hdr[H_HALFEDGES] / 3, edges = w.hdr[H_ENTRIES] / 2;      // three half-edges a face, two entries an edge
    stats[GPNERF_TOPOLOGY_FACES_USED] = used;
    stats[GPNERF_TOPOLOGY_FACES_DROPPED] = w.hdr[H_NF] - used;
    stats[GPNERF_TOPOLOGY_VERTICES_REFERENCED] = w.hdr[H_VREF];
    stats[GPNERF_TOPOLOGY_EDGES] = edges;
    stats[GPNERF_TOPOLOGY_BOUNDARY_EDGES] = w.hdr[H_BOUNDARY];
    stats[GPNERF_TOPOLOGY_NONMANIFOLD_EDGES] = w.hdr[H_NONMANIFOLD];
    stats[GPNERF_TOPOLOGY_INCONSISTENT_EDGES] = w.hdr[H_INCONSISTENT];
    stats[GPNERF_TOPOLOGY_EULER] = w.hdr[H_VREF] - edges + used;
    stats[GPNERF_TOPOLOGY_BOUNDARY_VERTICES] = w.hdr[H_VBOUNDARY];
    stats[GPNERF_TOPOLOGY_MAX_VALENCE] = w.hdr[H_MAX_VALENCE];
    w.hdr[H_DONE] = 1;
}

// ---------------------------------------------------------------- smoothing

// the workspace holds a finished adjacency of a mesh of nv vertices (otherwise the smoothing kernels write nothing)
DEV bool adjacency_ok(const Ws& w, long nv) { return w.hdr[H_MAGIC] == TOPO_MAGIC && w.hdr[H_DONE] == 1 && w.hdr[H_NV] == nv; }

template <bool PACKED> DEV void load3(const void* __restrict__ src, long i, float* x) {
    if (PACKED) {                                        // one 16-byte load
        const float4 p = static_cast<const float4*>(src)[i];
        x[0] = p.x; x[1] = p.y; x[2] = p.z;
    } else {
        const float* p = static_cast<const float*>(src) + 3 * i;
        x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
    }
}

// one Jacobi pass with factor t, a lane per vertex: float64 on the float32 positions, the neighbours added in ascending index, nothing
// fused (the library builds with -ffp-contract=off).  SRC4 / DST4: the side is one of the workspace's float4 arrays, otherwise the
// caller's [n][3].
template <bool SRC4, bool DST4>
__global__ __launch_bounds__(THREADS) void smooth_pass_kernel(const void* __restrict__ src, void* __restrict__ dst, long nv, double t, int pin, Ws w) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= nv || !adjacency_ok(w, nv)) return;
    float y[3];                                          // a vertex that does not move is copied as it is
    load3<SRC4>(src, i, y);
    const long long s = w.start[i], end = w.start[i + 1];
    if (end > s && !(pin && (w.vflags[i] & FLAG_BOUNDARY))) {
        double sum[3] = {0.0, 0.0, 0.0};
        for (long long j = s; j < end; ++j) {
            float p[3];
            load3<SRC4>(src, w.neighbours[j], p);
            sum[0] = sum[0] + (double)p[0]; sum[1] = sum[1] + (double)p[1]; sum[2] = sum[2] + (double)p[2];
        }
        const double k = (double)(end - s);
        for (int a = 0; a < 3; ++a) { const double x = (double)y[a]; y[a] = (float)(x + t * (sum[a] / k - x)); }
    }
    if (DST4) static_cast<float4*>(dst)[i] = make_float4(y[0], y[1], y[2], 0.f);
    else { float* o = static_cast<float*>(dst) + 3 * i; o[0] = y[0]; o[1] = y[1]; o[2] = y[2]; }
}

// iterations == 0
__global__ __launch_bounds__(THREADS) void copy_kernel(const float* src, float* dst, long n, long nv, Ws w) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (i < n && adjacency_ok(w, nv)) dst[i] = src[i];
}

}  // namespace

extern "C" {

size_t gpnerf_mesh_adjacency_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    return sizes_ok(n_vertices, n_faces) ? layout_of(n_vertices, n_faces).total : 0;
}

int gpnerf_mesh_adjacency_layout(int64_t n_vertices, int64_t n_faces, int64_t* offsets) {
    if (!offsets || !sizes_ok(n_vertices, n_faces)) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces);
    offsets[GPNERF_ADJACENCY_START] = (int64_t)l.start;
    offsets[GPNERF_ADJACENCY_NEIGHBOURS] = (int64_t)l.neighbours;
    offsets[GPNERF_ADJACENCY_VERTEX_FLAGS] = (int64_t)l.vflags;
    return GPNERF_OK;
}

int gpnerf_mesh_adjacency(const int32_t* faces, int64_t n_faces, int64_t n_vertices, void* workspace, size_t workspace_bytes, int64_t* stats,
                          void* stream) {
    if (!workspace || !stats || !sizes_ok(n_vertices, n_faces) || (!faces && n_faces > 0)) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    const Ws w = ws_of(workspace, l);
    hipStream_t st = S_(stream);
    const long nv = (long)n_vertices, nf = (long)n_faces;
    hipLaunchKernelGGL(topology_clear_kernel, dim3(blocks_for(nv + 1 < (1 << 22) ? nv + 1 : (1 << 22), THREADS)), dim3(THREADS), 0, st, w, nv, nf);
    const unsigned fb = blocks_for(nf, THREADS), eb = blocks_for(3 * n_faces, THREADS);
    if (nf > 0) hipLaunchKernelGGL(face_count_kernel, dim3(fb), dim3(THREADS), 0, st, faces, nf, nv, w);
    scan_launch<TopoScan, 0>(w.he_cnt, nv + 1, nullptr, w.bsum, &w.hdr[H_HALFEDGES], w.he_start, nullptr, nullptr, st);
    if (nf > 0) {
        hipLaunchKernelGGL(halfedge_fill_kernel, dim3(fb), dim3(THREADS), 0, st, faces, nf, nv, w);
        hipLaunchKernelGGL(edge_kernel, dim3(eb), dim3(THREADS), 0, st, faces, nf, nv, w);
    }
    scan_launch<TopoScan, 0>(w.deg, nv + 1, nullptr, w.bsum, &w.hdr[H_ENTRIES], w.start, nullptr, nullptr, st);
    if (nf > 0) {
        hipLaunchKernelGGL(neighbour_fill_kernel, dim3(eb), dim3(THREADS), 0, st, faces, nf, w);
        hipLaunchKernelGGL(neighbour_rank_kernel, dim3(eb), dim3(THREADS), 0, st, faces, nf, w);
    }
    if (nv > 0) hipLaunchKernelGGL(vertex_count_kernel, dim3(blocks_for(nv, THREADS)), dim3(THREADS), 0, st, nv, w);
    hipLaunchKernelGGL(topology_finish_kernel, dim3(1), dim3(1), 0, st, w, stats);
    return launch_status();
}

int gpnerf_mesh_smooth(const float* vertices, int64_t n_vertices, void* workspace, size_t workspace_bytes, int32_t iterations, double lam,
                       double mu, uint32_t flags, float* out_vertices, void* stream) {
    if (!workspace || !sizes_ok(n_vertices, 0) || ((!vertices || !out_vertices) && n_vertices > 0)) return GPNERF_E_ARG;
    if (iterations < 0 || iterations > MAX_ITERATIONS || (flags & ~(uint32_t)GPNERF_SMOOTH_PIN_BOUNDARY)) return GPNERF_E_ARG;
    if (!(lam > 0.0 && lam <= 1.0) || !(mu >= -1.0 && mu <= 0.0)) return GPNERF_E_ARG;      // (a NaN fails both comparisons)
    const Layout l = layout_of(n_vertices, 0);           // (the regions up to the neighbours do not depend on n_faces)
    if (workspace_bytes < l.total) return GPNERF_E_ARG;   // the smallest workspace a mesh of n_vertices needs
    if (n_vertices == 0) return GPNERF_OK;
    const Ws w = ws_of(workspace, l);
    hipStream_t st = S_(stream);
    const long nv = (long)n_vertices;
    const int pin = (flags & GPNERF_SMOOTH_PIN_BOUNDARY) ? 1 : 0;
    const dim3 grid(blocks_for(nv, THREADS)), block(THREADS);
    if (iterations == 0) {
        hipLaunchKernelGGL(copy_kernel, dim3(blocks_for(3 * n_vertices, THREADS)), block, 0, st, vertices, out_vertices, 3 * nv, nv, w);
        return launch_status();
    }
    const int passes = 2 * iterations;
    for (int p = 0; p < passes; ++p) {
        const double t = (p & 1) ? mu : lam;
        const void* src = p == 0 ? static_cast<const void*>(vertices) : static_cast<const void*>(w.pos[(p - 1) & 1]);
        void* dst = p == passes - 1 ? static_cast<void*>(out_vertices) : static_cast<void*>(w.pos[p & 1]);
        if (p == 0) hipLaunchKernelGGL((smooth_pass_kernel<false, true>), grid, block, 0, st, src, dst, nv, t, pin, w);
        else if (p == passes - 1) hipLaunchKernelGGL((smooth_pass_kernel<true, false>), grid, block, 0, st, src, dst, nv, t, pin, w);
        else hipLaunchKernelGGL((smooth_pass_kernel<true, true>), grid, block, 0, st, src, dst, nv, t, pin, w);
    }
    return launch_status();
}

}  // extern "C"
