// gpnerf_meshcomp.hip -- the connected components of a triangle mesh on gfx950: a label per vertex (the smallest vertex index of its
// component), the components numbered in ascending label, a table of every component's counts and Euler characteristic, and the mesh
// of the components the caller keeps.  include/gpnerf_hip.h states the definition and the workspace formula; tests/component_cases.py
// restates it in numpy.  It reads a finished adjacency (gpnerf_meshtopo.hip) for the vertex flags and the degrees.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone;
// the number of components stays in the workspace.  A FIXED number of launches: the labels come from the lock-free min-label
// union-find of gpnerf_unionfind.h over the faces -- no device-wide barrier, no cooperative launch, and no lane waits for a value
// another lane has yet to write.  The atomics, all on integers, and why their arrival order cannot matter:
//   - union_kernel: atomicMin links of the larger root below the smaller.  Whatever the order of the links, the sets at the kernel's
//     end are the components and every set's root is its smallest member;
//   - vertex_table_kernel / face_table_kernel: integer adds into the component's row (addition commutes); the root's lane stores LABEL;
//   - row_kernel: an add per wavefront into two counters and the maximum of the packed word (FACES << 32 | ~number), a total order.
// The scans (gpnerf_scan.h) have no atomic.  No float is computed anywhere; emit copies coordinates as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for, sweep_blocks; wave_count, wave_sum
#include "gpnerf_scan.h"       // the three-launch integer scan (shared with gpnerf_simplify.hip and gpnerf_meshtopo.hip)
#include "gpnerf_unionfind.h"  // g_load, g_find, g_find_compress, g_union (shared with gpnerf_mesh.hip)

struct CompScan;               // names this file's instances of the scan kernels

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int64_t MAX_VERTICES = ((int64_t)1 << 31) - 1;
constexpr int64_t MAX_FACES = (((int64_t)1 << 31) - 1) / 3;  // the adjacency's limits
constexpr long long COMP_MAGIC = 0x434f4d5031ll;         // "COMP1"
constexpr int COLS = GPNERF_COMPONENT_COLS;

typedef unsigned long long u64;

// the header's 64-bit words
enum { H_MAGIC, H_NV, H_NF, H_STATUS = GPNERF_COMPONENTS_HDR_STATUS, H_COMPONENTS, H_KEPT_V, H_KEPT_F, H_BEST, H_CLOSED, H_MIN_ROWS, H_KEEP,
       H_MIN_FACES, H_WORDS };
static_assert(H_NF + 1 == H_STATUS && H_WORDS <= 32, "the header's words");

// what this file reads of the workspace gpnerf_mesh_adjacency filled (gpnerf_meshtopo.hip): its header's first four 64-bit words --
// magic, n_vertices, n_faces, done -- and, at gpnerf_mesh_adjacency_layout's offsets, the CSR's starts and neighbours and the vertex flags
constexpr long long ADJ_MAGIC = 0x544f504f31ll;          // "TOPO1"
enum { ADJ_H_MAGIC, ADJ_H_NV, ADJ_H_NF, ADJ_H_DONE };
struct Adj { const long long* hdr; const long long* start; const int32_t* neighbours; const uint8_t* vflags; };

// the formula of include/gpnerf_hip.h
struct Layout { size_t hdr, label, vcomp, rootid, vnew, fcomp, fnew, table, bsum, total; };

__host__ inline int64_t table_rows(int64_t nv) { return nv / 3; }

__host__ inline Layout layout_of(int64_t nv, int64_t nf) {
    Layout l;
    size_t o = 0;
    const int64_t most = nv > nf ? nv : nf;
    l.hdr = o;    o += 256;
    l.label = o;  o += align256(4 * (size_t)nv);
    l.vcomp = o;  o += align256(4 * (size_t)nv);
    l.rootid = o; o += align256(4 * (size_t)nv);
    l.vnew = o;   o += align256(4 * (size_t)nv);
    l.fcomp = o;  o += align256(4 * (size_t)nf);
    l.fnew = o;   o += align256(4 * (size_t)nf);
    l.table = o;  o += align256(8 * (size_t)COLS * (size_t)table_rows(nv));
    l.bsum = o;   o += align256(8 * (size_t)(((most > 1 ? most : 1) + SCAN_CHUNK - 1) / SCAN_CHUNK));
    l.total = o;
    return l;
}

struct Ws {                                              // the workspace's regions, as the kernels see them
    long long* hdr; int32_t* label; int32_t* vcomp; int32_t* rootid; int32_t* vnew; int32_t* fcomp; int32_t* fnew; long long* table;
    long long* bsum;
};

__host__ inline Ws ws_of(void* workspace, const Layout& l) {
    char* b = static_cast<char*>(workspace);
    Ws w;
    w.hdr = reinterpret_cast<long long*>(b + l.hdr);
    w.label = reinterpret_cast<int32_t*>(b + l.label);
    w.vcomp = reinterpret_cast<int32_t*>(b + l.vcomp);
    w.rootid = reinterpret_cast<int32_t*>(b + l.rootid);
    w.vnew = reinterpret_cast<int32_t*>(b + l.vnew);
    w.fcomp = reinterpret_cast<int32_t*>(b + l.fcomp);
    w.fnew = reinterpret_cast<int32_t*>(b + l.fnew);
    w.table = reinterpret_cast<long long*>(b + l.table);
    w.bsum = reinterpret_cast<long long*>(b + l.bsum);
    return w;
}

bool sizes_ok(int64_t nv, int64_t nf) { return nv >= 0 && nf >= 0 && nv <= MAX_VERTICES && nf <= MAX_FACES; }

// a face's corners when it is usable: indices in [0, nv), pairwise distinct (the adjacency's rule)
DEV bool usable_face(const int32_t* __restrict__ faces, long f, long nv, int32_t* c) {
    for (int k = 0; k < 3; ++k) c[k] = faces[3 * f + k];
    return c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] < nv && c[1] < nv && c[2] < nv && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

// the adjacency workspace holds a finished adjacency of a mesh of these sizes
DEV bool adjacency_ok(const Adj& a, long nv, long nf) {
    return a.hdr[ADJ_H_MAGIC] == ADJ_MAGIC && a.hdr[ADJ_H_DONE] == 1 && a.hdr[ADJ_H_NV] == nv && a.hdr[ADJ_H_NF] == nf;
}

// what every launch behind the first checks before it writes: the adjacency's header words, and that this call's first launch saw them too
DEV bool counting(const Ws& w, const Adj& a, long nv, long nf) {
    return adjacency_ok(a, nv, nf) && w.hdr[H_MAGIC] == COMP_MAGIC && w.hdr[H_STATUS] == GPNERF_COMPONENTS_COUNTING;
}

// ---------------------------------------------------------------- labels

// parent[v] = the smaller of v and its smallest neighbour -- the first entry of its ascending CSR run -- (in `label`), the table's rows
// zeroed, the header.  Starting from that forest and not from parent[v] = v keeps the union-find's invariant (a word points at a lower
// member of its own set, or at itself) and leaves union_kernel little to link: only the vertices without a lower neighbour are roots
// (measured: DESIGN.md 4.15).
__global__ __launch_bounds__(THREADS) void init_kernel(Ws w, Adj a, long nv, long nf, long words, int keep, long long min_faces) {
    const bool ok = adjacency_ok(a, nv, nf);
    const long stride = (long)gridDim.x * THREADS, i0 = (long)blockIdx.x * THREADS + threadIdx.x;
    if (ok) {
        for (long i = i0; i < nv; i += stride) {
            const long long s = a.start[i];
            const int32_t low = s < a.start[i + 1] ? a.neighbours[s] : (int32_t)i;
            w.label[i] = low < (int32_t)i ? low : (int32_t)i;
        }
        for (long i = i0; i < words; i += stride) w.table[i] = 0;
    }
    if (i0 == 0) {
        for (int k = 0; k < 32; ++k) w.hdr[k] = 0;
        w.hdr[H_MAGIC] = COMP_MAGIC;
        w.hdr[H_NV] = nv;
        w.hdr[H_NF] = nf;
        w.hdr[H_KEEP] = keep;
        w.hdr[H_MIN_FACES] = min_faces;
        w.hdr[H_STATUS] = ok ? GPNERF_COMPONENTS_COUNTING : GPNERF_COMPONENTS_NO_ADJACENCY;
    }
}

// Most of a mesh's unions are redundant -- every edge comes with two faces, every vertex with about six --, so two read-only walks come
// first: when both end at the same root (a root at the time it was read, and sets only ever merge) the two are united already, and no
// word is written.  Only a union that may have to link goes through g_union and its path compression, whose atomicMin on the words
// just below a large set's root would otherwise be issued by every lane of the launch (measured: DESIGN.md 4.15).
DEV void unite(int32_t* p, int32_t a, int32_t b) {
    if (g_find(p, a) != g_find(p, b)) g_union(p, a, b);
}

// a lane per face: a usable face (a, b, c) unites a with b and b with c.  Atomic accesses only (gpnerf_unionfind.h); no lane waits.
__global__ __launch_bounds__(THREADS) void union_kernel(const int32_t* __restrict__ faces, long nf, long nv, Ws w, Adj a) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    int32_t c[3];
    if (f >= nf || !counting(w, a, nv, nf) || !usable_face(faces, f, nv, c)) return;
    unite(w.label, c[0], c[1]);
    unite(w.label, c[1], c[2]);
}

// A kernel of its own, so the unions are complete and visible (kernel boundary).  Plain accesses: nothing is united here, every set's
// root is fixed, and a word is only ever replaced by that root (a reader that still sees the old word walks a longer path to the same
// root) or, for a vertex no usable face references -- a set of its own that no other walk passes through --, by -1.
__global__ __launch_bounds__(THREADS) void flatten_kernel(long nv, long nf, Ws w, Adj a) {
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= nv || !counting(w, a, nv, nf)) return;
    if (!(a.vflags[v] & GPNERF_VERTEX_REFERENCED)) {
        w.label[v] = -1;
        w.rootid[v] = 0;
        return;
    }
    const int32_t q = w.label[v];
    int32_t r = q;
    for (int32_t u = w.label[r]; u != r; u = w.label[r]) r = u;
    if (r != q) w.label[v] = r;
    w.rootid[v] = r == (int32_t)v ? 1 : 0;               // the scan turns the marks into the components' numbers
}

// ---------------------------------------------------------------- the table

// Adds val[0 .. N) to columns col[0 .. N) of row `comp` of the table for every lane with comp >= 0, with as few atomics as the
// wavefronts' agreement allows: 15 360 wavefronts adding to one address serialise at 8 - 10 ns each, and a body mesh is
// ONE component, so that every lane of the launch targets one row.  A wavefront whose active lanes share a component sums first;
// the workgroup's first thread then merges the runs of wavefronts that agree: one add per counter and workgroup for a mesh of one
// component.  A mixed wavefront adds once per distinct component among its lanes (on a surface of one large piece and many crumbs nearly
// every lane of a mixed wavefront still belongs to the large piece).  EVERY thread of the workgroup must reach this call.
template <int N>
DEV void component_add(long long* __restrict__ table, int32_t comp, const long long (&val)[N], const int (&col)[N], int32_t (&s_comp)[WAVES],
                       long long (&s_val)[WAVES][N]) {
    const int wave = threadIdx.x >> 6;
    const bool active = comp >= 0;
    const u64 m = __ballot(active);
    const int32_t c0 = m ? __shfl(comp, __ffsll((long long)m) - 1) : -1;
    const bool uniform = __all(!active || comp == c0);
    if (uniform) {
        long long sum[N];
        for (int k = 0; k < N; ++k) sum[k] = wave_sum(active ? val[k] : 0ll);
        if ((threadIdx.x & 63) == 0) {
            s_comp[wave] = c0;                               // (-1: a wavefront with nothing to add)
            for (int k = 0; k < N; ++k) s_val[wave][k] = sum[k];
        }
    } else {                                                 // one round per distinct component of the wavefront, its first lane adding the round's sums
        if ((threadIdx.x & 63) == 0) s_comp[wave] = -1;
        u64 todo = m;
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int32_t c = __shfl(comp, lead);
            const bool mine = active && comp == c;
            for (int k = 0; k < N; ++k) {
                const long long sum = wave_sum(mine ? val[k] : 0ll);
                if ((int)(threadIdx.x & 63) == lead && sum) atomicAdd(reinterpret_cast<u64*>(&table[(long)c * COLS + col[k]]), (u64)sum);
            }
            todo &= ~__ballot(mine);
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int32_t cur = -1;
    long long acc[N] = {};
    for (int wv = 0; wv <= WAVES; ++wv) {
        const int32_t c = wv < WAVES ? s_comp[wv] : -1;
        if (wv < WAVES && c < 0) continue;
        if (c != cur) {                                      // a run of agreeing wavefronts ends (wv == WAVES: the last one)
            if (cur >= 0)
                for (int k = 0; k < N; ++k)
                    if (acc[k]) atomicAdd(reinterpret_cast<u64*>(&table[(long)cur * COLS + col[k]]), (u64)acc[k]);
            cur = c;
            for (int k = 0; k < N; ++k) acc[k] = 0;
        }
        if (wv < WAVES)
            for (int k = 0; k < N; ++k) acc[k] += s_val[wv][k];
    }
}

// a lane per vertex: its component's number; 1, its degree and its boundary flag into the component's row; the root stores LABEL
__global__ __launch_bounds__(THREADS) void vertex_table_kernel(long nv, long nf, Ws w, Adj a) {
    __shared__ int32_t s_comp[WAVES];
    __shared__ long long s_val[WAVES][3];
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    const bool ok = counting(w, a, nv, nf);                  // (uniform over the launch)
    int32_t comp = -1;
    long long val[3] = {0, 0, 0};
    if (ok && v < nv) {
        const int32_t l = w.label[v];
        if (l >= 0) {
            comp = w.rootid[l];                              // the scan's: the number at a root
            val[0] = 1;
            val[1] = a.start[v + 1] - a.start[v];
            val[2] = (a.vflags[v] & GPNERF_VERTEX_BOUNDARY) ? 1 : 0;
            if (l == (int32_t)v) w.table[(long)comp * COLS + GPNERF_COMPONENT_LABEL] = l;
        }
        w.vcomp[v] = comp;
    }
    const int col[3] = {GPNERF_COMPONENT_VERTICES, GPNERF_COMPONENT_EDGES, GPNERF_COMPONENT_BOUNDARY_VERTICES};   // (EDGES: twice, until row_kernel)
    component_add<3>(w.table, comp, val, col, s_comp, s_val);
}

// a lane per face: its component's number, -1 when it is not usable; 1 into the component's row
__global__ __launch_bounds__(THREADS) void face_table_kernel(const int32_t* __restrict__ faces, long nf, long nv, Ws w, Adj a) {
    __shared__ int32_t s_comp[WAVES];
    __shared__ long long s_val[WAVES][1];
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    const bool ok = counting(w, a, nv, nf);
    int32_t comp = -1, c[3];
    if (ok && f < nf) {
        if (usable_face(faces, f, nv, c)) comp = w.vcomp[c[0]];
        w.fcomp[f] = comp;
    }
    const long long val[1] = {comp >= 0 ? 1 : 0};
    const int col[1] = {GPNERF_COMPONENT_FACES};
    component_add<1>(w.table, comp, val, col, s_comp, s_val);
}

// a lane per row of the table: EDGES halved, EULER; the closed rows and those of at least min_faces faces counted, one add per
// wavefront; the packed (FACES << 32 | ~number) maximum -- a total order: a tie goes to the lower number
__global__ __launch_bounds__(THREADS) void row_kernel(long rows, long nv, long nf, Ws w, Adj a) {
    const long r = (long)blockIdx.x * THREADS + threadIdx.x;
    const bool ok = counting(w, a, nv, nf);
    const bool live = ok && r < rows && r < w.hdr[H_COMPONENTS];
    if (!__any(live)) return;
    bool closed = false, enough = false;
    u64 key = 0;
    if (live) {
        long long* row = w.table + r * COLS;
        const long long edges = row[GPNERF_COMPONENT_EDGES] / 2, f = row[GPNERF_COMPONENT_FACES];
        row[GPNERF_COMPONENT_EDGES] = edges;
        row[GPNERF_COMPONENT_EULER] = row[GPNERF_COMPONENT_VERTICES] - edges + f;
        closed = row[GPNERF_COMPONENT_BOUNDARY_VERTICES] == 0;
        enough = f >= w.hdr[H_MIN_FACES];
        key = ((u64)f << 32) | (u64)(uint32_t)~(uint32_t)r;
    }
    wave_count(closed, &w.hdr[H_CLOSED]);
    wave_count(enough, &w.hdr[H_MIN_ROWS]);
    for (int d = 32; d > 0; d >>= 1) { const u64 o = __shfl_xor(key, d); key = o > key ? o : key; }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(reinterpret_cast<u64*>(&w.hdr[H_BEST]), key);
}

// ---------------------------------------------------------------- the selection

DEV bool kept(const Ws& w, int32_t comp) {
    if (comp < 0) return false;
    const long long keep = w.hdr[H_KEEP];
    if (keep == GPNERF_COMPONENTS_KEEP_LARGEST) return (uint32_t)comp == ~(uint32_t)(u64)w.hdr[H_BEST];      // (a component exists: BEST != 0)
    if (keep == GPNERF_COMPONENTS_KEEP_MIN_FACES) return w.table[(long)comp * COLS + GPNERF_COMPONENT_FACES] >= w.hdr[H_MIN_FACES];
    return true;
}

// a lane per vertex and per face: 1 where it is kept; the scans turn the marks into the new numbers
__global__ __launch_bounds__(THREADS) void mark_kernel(long nv, long nf, Ws w, Adj a) {
    const long i = (long)blockIdx.x * THREADS + threadIdx.x;
    if (!counting(w, a, nv, nf)) return;
    if (i < nv) w.vnew[i] = kept(w, w.vcomp[i]) ? 1 : 0;
    if (i < nf) w.fnew[i] = kept(w, w.fcomp[i]) ? 1 : 0;
}

__global__ void finish_kernel(long nv, long nf, Ws w, Adj a, int64_t* stats) {
    if (!counting(w, a, nv, nf)) return;
    const long long n = w.hdr[H_COMPONENTS], keep = w.hdr[H_KEEP];
    const u64 best = (u64)w.hdr[H_BEST];
    const long long largest = n > 0 ? (long long)(uint32_t)~(uint32_t)best : -1;
    const long long* row = w.table + (n > 0 ? largest : 0) * COLS;
    stats[GPNERF_COMPONENTS_COMPONENTS] = n;
    stats[GPNERF_COMPONENTS_CLOSED_COMPONENTS] = w.hdr[H_CLOSED];
    stats[GPNERF_COMPONENTS_LARGEST] = largest;
    stats[GPNERF_COMPONENTS_LARGEST_FACES] = n > 0 ? row[GPNERF_COMPONENT_FACES] : 0;
    stats[GPNERF_COMPONENTS_LARGEST_VERTICES] = n > 0 ? row[GPNERF_COMPONENT_VERTICES] : 0;
    stats[GPNERF_COMPONENTS_LARGEST_EULER] = n > 0 ? row[GPNERF_COMPONENT_EULER] : 0;
    stats[GPNERF_COMPONENTS_KEPT_COMPONENTS] = keep == GPNERF_COMPONENTS_KEEP_LARGEST ? (n > 0 ? 1 : 0)
                                               : keep == GPNERF_COMPONENTS_KEEP_MIN_FACES ? w.hdr[H_MIN_ROWS] : n;
    stats[GPNERF_COMPONENTS_KEPT_VERTICES] = w.hdr[H_KEPT_V];
    stats[GPNERF_COMPONENTS_KEPT_FACES] = w.hdr[H_KEPT_F];
    w.hdr[H_STATUS] = GPNERF_COMPONENTS_COUNTED;
}

// ---------------------------------------------------------------- emit

// one thread: the sizes the caller brought against those counted
__global__ void component_emit_check_kernel(Ws w, long nv, long nf, long n_out_v, long n_out_f) {
    const long long st = w.hdr[H_STATUS];
    const bool counted = w.hdr[H_MAGIC] == COMP_MAGIC && (st == GPNERF_COMPONENTS_COUNTED || st == GPNERF_COMPONENTS_EMITTED || st == GPNERF_COMPONENTS_MISMATCH);
    if (!counted) return;                                // (nothing to compare with: the emit kernels write nothing either)
    const bool same = w.hdr[H_NV] == nv && w.hdr[H_NF] == nf && w.hdr[H_KEPT_V] == n_out_v && w.hdr[H_KEPT_F] == n_out_f;
    w.hdr[H_STATUS] = same ? GPNERF_COMPONENTS_EMITTED : GPNERF_COMPONENTS_MISMATCH;
}

DEV bool emit_ok(const Ws& w) { return w.hdr[H_MAGIC] == COMP_MAGIC && w.hdr[H_STATUS] == GPNERF_COMPONENTS_EMITTED; }

// a lane per input vertex: a kept one goes to its new number (< KEPT_VERTICES, which component_emit_check_kernel found equal to the outputs' size),
// the three words copied as they are
__global__ __launch_bounds__(THREADS) void component_emit_vertices_kernel(Ws w, const uint32_t* __restrict__ vertices, long nv, uint32_t* __restrict__ out_vertices,
                                                                int32_t* __restrict__ vertex_map, int32_t* __restrict__ kept_vertices) {
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= nv || !emit_ok(w)) return;
    const int32_t n = w.vnew[v];
    if (vertex_map) vertex_map[v] = n;
    if (n < 0) return;
    for (int k = 0; k < 3; ++k) out_vertices[3 * (long)n + k] = vertices[3 * v + k];
    if (kept_vertices) kept_vertices[n] = (int32_t)v;
}

// a lane per input face: a kept one (usable, so its corners are in range, and of a kept component, so they are kept) goes to its new number
__global__ __launch_bounds__(THREADS) void component_emit_faces_kernel(Ws w, const int32_t* __restrict__ faces, long nf, long nv, int32_t* __restrict__ out_faces) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= nf || !emit_ok(w)) return;
    const int32_t n = w.fnew[f];
    if (n < 0) return;
    for (int k = 0; k < 3; ++k) {
        const int32_t i = faces[3 * f + k];                 // (in range for the faces that were counted; -1 rather than a stray read for others)
        out_faces[3 * (long)n + k] = i >= 0 && i < nv ? w.vnew[i] : -1;
    }
}

}  // namespace

extern "C" {

size_t gpnerf_mesh_components_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    return sizes_ok(n_vertices, n_faces) ? layout_of(n_vertices, n_faces).total : 0;
}

int gpnerf_mesh_components_layout(int64_t n_vertices, int64_t n_faces, int64_t* offsets) {
    if (!offsets || !sizes_ok(n_vertices, n_faces)) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces);
    offsets[GPNERF_COMPONENTS_LABEL] = (int64_t)l.label;
    offsets[GPNERF_COMPONENTS_VERTEX_COMPONENT] = (int64_t)l.vcomp;
    offsets[GPNERF_COMPONENTS_FACE_COMPONENT] = (int64_t)l.fcomp;
    offsets[GPNERF_COMPONENTS_TABLE] = (int64_t)l.table;
    return GPNERF_OK;
}

int gpnerf_mesh_components(const int32_t* faces, int64_t n_faces, int64_t n_vertices, const void* adjacency_workspace, size_t adjacency_bytes,
                           int32_t keep, int64_t min_faces, void* workspace, size_t workspace_bytes, int64_t* stats, void* stream) {
    if (!workspace || !adjacency_workspace || !stats || !sizes_ok(n_vertices, n_faces) || (!faces && n_faces > 0)) return GPNERF_E_ARG;
    if (keep != GPNERF_COMPONENTS_KEEP_ALL && keep != GPNERF_COMPONENTS_KEEP_LARGEST && keep != GPNERF_COMPONENTS_KEEP_MIN_FACES) return GPNERF_E_ARG;
    if (keep == GPNERF_COMPONENTS_KEEP_MIN_FACES && min_faces < 1) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces);
    int64_t adj_off[3];
    if (workspace_bytes < l.total || adjacency_bytes < gpnerf_mesh_adjacency_workspace_bytes(n_vertices, n_faces) ||
        gpnerf_mesh_adjacency_layout(n_vertices, n_faces, adj_off) != GPNERF_OK)
        return GPNERF_E_ARG;
    const Ws w = ws_of(workspace, l);
    const char* ab = static_cast<const char*>(adjacency_workspace);
    const Adj a = {reinterpret_cast<const long long*>(ab), reinterpret_cast<const long long*>(ab + adj_off[GPNERF_ADJACENCY_START]),
                   reinterpret_cast<const int32_t*>(ab + adj_off[GPNERF_ADJACENCY_NEIGHBOURS]),
                   reinterpret_cast<const uint8_t*>(ab + adj_off[GPNERF_ADJACENCY_VERTEX_FLAGS])};
    hipStream_t st = S_(stream);
    const long nv = (long)n_vertices, nf = (long)n_faces, rows = (long)table_rows(n_vertices), words = rows * COLS;
    const long long mf = keep == GPNERF_COMPONENTS_KEEP_MIN_FACES ? (long long)min_faces : 1;
    const dim3 block(THREADS), vgrid(blocks_for(nv, THREADS)), fgrid(blocks_for(nf, THREADS));
    hipLaunchKernelGGL(init_kernel, dim3(sweep_blocks(nv > words ? nv : words, THREADS)), block, 0, st, w, a, nv, nf, words, (int)keep, mf);
    if (nv > 0) {
        if (nf > 0) hipLaunchKernelGGL(union_kernel, fgrid, block, 0, st, faces, nf, nv, w, a);
        hipLaunchKernelGGL(flatten_kernel, vgrid, block, 0, st, nv, nf, w, a);
        scan_launch<CompScan, 1>(w.rootid, nv, nullptr, w.bsum, &w.hdr[H_COMPONENTS], nullptr, w.rootid, nullptr, st);
        hipLaunchKernelGGL(vertex_table_kernel, vgrid, block, 0, st, nv, nf, w, a);
        if (nf > 0) hipLaunchKernelGGL(face_table_kernel, fgrid, block, 0, st, faces, nf, nv, w, a);
        if (rows > 0) hipLaunchKernelGGL(row_kernel, dim3(blocks_for(rows, THREADS)), block, 0, st, rows, nv, nf, w, a);
        hipLaunchKernelGGL(mark_kernel, dim3(blocks_for(nv > nf ? nv : nf, THREADS)), block, 0, st, nv, nf, w, a);
        scan_launch<CompScan, 1>(w.vnew, nv, nullptr, w.bsum, &w.hdr[H_KEPT_V], nullptr, w.vnew, nullptr, st);
        if (nf > 0) scan_launch<CompScan, 1>(w.fnew, nf, nullptr, w.bsum, &w.hdr[H_KEPT_F], nullptr, w.fnew, nullptr, st);
    }
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1), 0, st, nv, nf, w, a, stats);
    return launch_status();
}

int gpnerf_mesh_components_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, void* workspace,
                                size_t workspace_bytes, int64_t n_out_vertices, int64_t n_out_faces, float* out_vertices, int32_t* out_faces,
                                int32_t* vertex_map, int32_t* kept_vertices, void* stream) {
    if (!workspace || !sizes_ok(n_vertices, n_faces) || (!vertices && n_vertices > 0) || (!faces && n_faces > 0)) return GPNERF_E_ARG;
    if (n_out_vertices < 0 || n_out_vertices > n_vertices || n_out_faces < 0 || n_out_faces > n_faces) return GPNERF_E_ARG;
    if ((!out_vertices && n_out_vertices > 0) || (!out_faces && n_out_faces > 0)) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    const Ws w = ws_of(workspace, l);
    hipStream_t st = S_(stream);
    const long nv = (long)n_vertices, nf = (long)n_faces;
    hipLaunchKernelGGL(component_emit_check_kernel, dim3(1), dim3(1), 0, st, w, nv, nf, (long)n_out_vertices, (long)n_out_faces);
    if (nv > 0 && (n_out_vertices > 0 || vertex_map))
        hipLaunchKernelGGL(component_emit_vertices_kernel, dim3(blocks_for(nv, THREADS)), dim3(THREADS), 0, st, w, reinterpret_cast<const uint32_t*>(vertices), nv,
                           reinterpret_cast<uint32_t*>(out_vertices), vertex_map, kept_vertices);
    if (n_out_faces > 0) hipLaunchKernelGGL(component_emit_faces_kernel, dim3(blocks_for(nf, THREADS)), dim3(THREADS), 0, st, w, faces, nf, nv, out_faces);
    return launch_status();
}

}  // extern "C"
