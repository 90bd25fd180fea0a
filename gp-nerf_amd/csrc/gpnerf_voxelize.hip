// gpnerf_voxelize.hip -- a triangle mesh turned into solid occupancy on a lattice, on gfx950: packed bits per lattice point, the
// counts that give a volume, and the small operations on packed cubes that go with them (from a density cube, back to a float cube,
// popcounts of two cubes for a volume IoU, containment of points).  include/gpnerf_hip.h states the definition operation for
// operation (gpnerf_mesh_voxelize); DESIGN.md 4.14 the launch shape and the reasons for it.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone;
// the one data-dependent length (the large-face list's) stays in the workspace header.  No float atomics.  The integer atomics, and
// why their arrival order cannot matter:
//   - a crossing toggles ONE bit (rule PARITY: atomicXor) or adds +-1 to ONE int32 count (rule NONZERO: atomicAdd) at index kc of its
//     column's toggle row; XOR and integer addition are commutative and associative;
//   - the large-face list is filled through a cursor: the SET of faces that lands in it is the same in any order, and what the list's
//     reader does with a face is again toggles;
//   - the statistics are integer sums.
// A crossing never flips the column's prefix of points below it (nz / 32 atomics per crossing): the resolve pass takes the suffix
// XOR / suffix sum of the toggle row once per column.
//
// The two-tier walk of gpnerf_tri2d.h over the lattice's columns, the vertices snapped to 1/4096 step: the ray axis is z, so a
// face's work is the columns (i, j) its projection owns.  The first kernel gives every face ONE lane, which maps the three vertices
// to lattice units in float64 and walks the face's clipped column box, j inside (a column's toggles follow those of the column
// before it in j); the faces of more than LARGE_BOX columns go through the list to the second kernel.  What is the voxeliser's own:
// the lattice mapping, the (eps, eps^2) rule that gives a column exactly on an edge to ONE face (vox_owns), the crossing's height
// and the toggle it makes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for, sweep_blocks, mesh_ok; wave_sum, stat_add
#include "gpnerf_tri2d.h"      // Mesh, Snapped, Setup, Edges, setup_face, count_states, large_append, lane_walk, wave_walk; LARGE_*

constexpr int THREADS = 256;
constexpr int COUNT_BLOCKS_MAX = 256;                    // of the popcount of two cubes
constexpr int SNAP_SHIFT = 12;                           // 4096 sub-column units per lattice step
constexpr double GUARD = 65536.0;                        // 2^16 lattice steps
constexpr int64_t MAX_POINTS = (int64_t)1 << 28;         // marching cubes' limit

static_assert(GPNERF_VOXEL_USED == FACE_OK && GPNERF_VOXEL_SKIPPED_VERTEX == FACE_BAD_VERTEX && GPNERF_VOXEL_SKIPPED_AREA == FACE_NO_AREA,
              "count_states adds a face under its state");

struct Lattice {
    double lo[3], step[3];
    int nx, ny, nz;
};

// a column's toggle row: nz + 1 places (kc = 0 .. nz); PARITY packs them into words, NONZERO keeps an int32 each
DEV long toggle_row(int nz, int rule) { return rule == GPNERF_VOXEL_PARITY ? (long)(nz / 32 + 1) : (long)nz + 1; }
size_t toggle_row_host(int nz, int rule) { return rule == GPNERF_VOXEL_PARITY ? (size_t)(nz / 32 + 1) : (size_t)nz + 1; }

struct Layout { size_t hdr, toggles, list, total; };

Layout layout_of(int64_t n_faces, const int32_t* dims, int rule) {
    Layout l;
    size_t o = 0;
    l.hdr = o;     o += 256;                             // the list's length, uint64 at 0
    l.toggles = o; o += align256(sizeof(uint32_t) * (size_t)dims[0] * (size_t)dims[1] * toggle_row_host(dims[2], rule));
    l.list = o;    o += align256(sizeof(uint32_t) * (size_t)n_faces);
    l.total = o;
    return l;
}

bool dims_ok(const int32_t* dims) {
    if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
    const int64_t xy = (int64_t)dims[0] * dims[1];       // (< 2^62)
    return xy <= MAX_POINTS && xy * dims[2] <= MAX_POINTS;
}

bool rule_ok(int rule) { return rule == GPNERF_VOXEL_PARITY || rule == GPNERF_VOXEL_NONZERO; }

bool lattice_ok(const double* lattice) {
    if (!lattice) return false;
    for (int a = 0; a < 3; ++a) {
        if (!(fabs(lattice[a]) < (double)INFINITY)) return false;                              // NaN, infinite
        if (!(lattice[3 + a] > 0.0) || !(lattice[3 + a] < (double)INFINITY)) return false;     // zero, negative, NaN, infinite
    }
    return true;
}

Lattice lattice_of(const double* lattice, const int32_t* dims) {
    Lattice g;
    for (int a = 0; a < 3; ++a) { g.lo[a] = lattice[a]; g.step[a] = lattice[3 + a]; }
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    return g;
}

// one vertex in lattice units: float64, subtract then divide; the usable test; the snap of x and y to 1/4096 step
DEV bool vox_vertex(const Lattice& g, const float* __restrict__ p, Snapped& s) {
    const double ux = ((double)p[0] - g.lo[0]) / g.step[0];
    const double uy = ((double)p[1] - g.lo[1]) / g.step[1];
    const double uz = ((double)p[2] - g.lo[2]) / g.step[2];
    // (every comparison is false for a NaN; an infinite x or y fails the guard band, an infinite z is named)
    if (!(fabs(ux) <= GUARD) || !(fabs(uy) <= GUARD) || !(fabs(uz) < (double)INFINITY)) return false;
    s.X = (int64_t)rint(4096.0 * ux);
    s.Y = (int64_t)rint(4096.0 * uy);
    s.z = uz;
    return true;
}

// a column on an edge with vector (dx, dy) belongs to the face it enters when nudged by (eps, eps^2): E changes by dx eps^2 - dy eps
DEV bool vox_tie(int sgn, int64_t dx, int64_t dy) {
    const int64_t sy = sgn * dy, sx = sgn * dx;
    return sy < 0 || (sy == 0 && sx > 0);
}

using VoxSetup = Setup<SNAP_SHIFT>;

// face f: its corners in lattice units, A and the column box clipped to the lattice
DEV FaceState vox_setup(const Mesh& m, const Lattice& g, long f, VoxSetup& s) {
    return setup_face(m, f, g.nx, g.ny, [&](const float* p, Snapped& v) { return vox_vertex(g, p, v); }, s);
}

// what a walk of face s needs beside its edge functions: the sign of A, and whether a column exactly ON an edge belongs to the face
struct VoxTies {
    int sgn;
    bool tie_a, tie_b, tie_c;
    DEV explicit VoxTies(const VoxSetup& s) {
        sgn = s.A > 0 ? 1 : -1;
        tie_a = vox_tie(sgn, s.c.X - s.b.X, s.c.Y - s.b.Y);
        tie_b = vox_tie(sgn, s.a.X - s.c.X, s.a.Y - s.c.Y);
        tie_c = vox_tie(sgn, s.b.X - s.a.X, s.b.Y - s.a.Y);
    }
};

DEV bool vox_edge_in(int sgn, int64_t e, bool tie) { return e == 0 ? tie : ((e > 0) == (sgn > 0)); }

// (& on ints, not &&: three tests and one branch per column, where && left the third test behind a branch of its own)
DEV bool vox_owns(const VoxTies& t, const Edges& e) {
    return (int)vox_edge_in(t.sgn, e.ea, t.tie_a) & (int)vox_edge_in(t.sgn, e.eb, t.tie_b) & (int)vox_edge_in(t.sgn, e.ec, t.tie_c);
}

// the crossing of an owned column: float64, unfused; the number of the column's lattice points strictly below it, 0 .. nz
DEV int vox_crossing(const VoxSetup& s, const Edges& e, int nz) {
    const double A = (double)s.A;
    const double wa = (double)e.ea / A, wb = (double)e.eb / A, wc = (double)e.ec / A;
    const double z = (wa * s.a.z + wb * s.b.z) + wc * s.c.z;
    const double c = ceil(z);
    if (!(c > 0.0)) return 0;
    return c >= (double)nz ? nz : (int)c;
}

// one no-return atomic per crossing, at index kc of the column's toggle row
DEV void vox_toggle(uint32_t* toggles, const Lattice& g, int rule, int i, int j, int kc, int sgn) {
    const long col = (long)i * g.ny + j;
    if (rule == GPNERF_VOXEL_PARITY) atomicXor(toggles + col * toggle_row(g.nz, rule) + (kc >> 5), 1u << (kc & 31));
    else atomicAdd(reinterpret_cast<int*>(toggles) + col * toggle_row(g.nz, rule) + kc, sgn);
}

// what both walks do at a column of the face's box: an owned column gets the toggle of its crossing, and is counted
struct Cross {
    const VoxSetup& s;
    const VoxTies t;
    const Lattice& g;
    int rule;
    uint32_t* toggles;
    long long& crossings;
    DEV void operator()(int i, int j, const Edges e) const {
        if (vox_owns(t, e)) {
            vox_toggle(toggles, g, rule, i, j, vox_crossing(s, e, g.nz), t.sgn);
            ++crossings;
        }
    }
};

// the toggles, the list's length and the statistics start from a kernel of the library's own, not from memset nodes
__global__ __launch_bounds__(THREADS) void voxelize_clear_kernel(uint32_t* toggles, long n_words, unsigned long long* list_len, long long* stats) {
    const long stride = (long)gridDim.x * THREADS;
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n_words; i += stride) toggles[i] = 0u;
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) *list_len = 0ull;
        if ((int)threadIdx.x < GPNERF_VOXEL_STATS) stats[threadIdx.x] = 0;
    }
}

// one lane per face; every lane stays to the end (the counts are summed over the wavefront)
__global__ __launch_bounds__(THREADS) void voxelize_faces_kernel(const Mesh m, const Lattice g, int rule, uint32_t* toggles, uint32_t* list,
                                                                 unsigned long long* list_len, long long* stats) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    const bool live = f < m.n_faces;
    const int lane = threadIdx.x & 63;
    VoxSetup s;
    FaceState st = FACE_OK;
    long box = 0;
    if (live) {
        st = vox_setup(m, g, f, s);
        if (st == FACE_OK) box = s.box();
    }
    count_states(live, st, stats);
    const bool large = box > LARGE_BOX;
    const long long at = large_append(large, list_len, (unsigned long long)m.n_faces);
    if (at >= 0) list[at] = (uint32_t)f;
    long long crossings = 0;
    if (box > 0 && !large) lane_walk<INNER_J>(s, Cross{s, VoxTies(s), g, rule, toggles, crossings});
    crossings = wave_sum(crossings);
    if (lane == 0) stat_add(stats, GPNERF_VOXEL_CROSSINGS, crossings);
}

// fixed grid: a wavefront per listed face, 64 columns of its box per step
__global__ __launch_bounds__(THREADS) void voxelize_large_kernel(const Mesh m, const Lattice g, int rule, uint32_t* toggles,
                                                                 const uint32_t* __restrict__ list, const unsigned long long* __restrict__ list_len,
                                                                 long long* stats) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (THREADS / 64) + threadIdx.x / 64, waves = (long)gridDim.x * (THREADS / 64);
    unsigned long long n = *list_len;
    if (n > (unsigned long long)m.n_faces) n = (unsigned long long)m.n_faces;
    long long crossings = 0;
    for (unsigned long long at = (unsigned long long)wave; at < n; at += (unsigned long long)waves) {
        const long f = (long)list[at];
        if (f >= m.n_faces) continue;                    // (never: the list holds what the first kernel wrote)
        VoxSetup s;
        if (vox_setup(m, g, f, s) != FACE_OK || s.i1 < s.i0 || s.j1 < s.j0) continue;
        wave_walk<INNER_J>(s, lane, Cross{s, VoxTies(s), g, rule, toggles, crossings});
    }
    crossings = wave_sum(crossings);
    if (lane == 0) stat_add(stats, GPNERF_VOXEL_CROSSINGS, crossings);
}

// within a word: bit b becomes the XOR of bits b .. 31
DEV uint32_t vox_suffix_xor(uint32_t x) {
    x ^= x >> 1; x ^= x >> 2; x ^= x >> 4; x ^= x >> 8; x ^= x >> 16;
    return x;
}

// rule PARITY.  A column's toggle row is tw = nz / 32 + 1 words; S[m] = the XOR of the toggles m .. nz; point k is occupied iff
// S[k + 1], the column is open iff S[0].  Lanes take CONSECUTIVE words of the toggle array: for tw <= 64 a wavefront takes
// 64 / tw whole columns per step (one contiguous load), and the carry into a word -- the parity of the words above it in its column --
// comes from a ballot of word parities masked to the same column.  For tw > 64 a wavefront takes one column per step, 64 words at a
// time from the top down, the carry going from chunk to chunk.
__global__ __launch_bounds__(THREADS) void voxelize_resolve_parity_kernel(const uint32_t* __restrict__ toggles, int nz, long n_cols, uint32_t* bits,
                                                                          long long* stats) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (THREADS / 64) + threadIdx.x / 64, waves = (long)gridDim.x * (THREADS / 64);
    const int tw = nz / 32 + 1, nzw = (nz + 31) / 32;
    const uint32_t top_mask = (nz & 31) ? ((1u << (nz & 31)) - 1u) : 0xffffffffu;      // of the output's last word
    long long occupied = 0, open = 0;
    if (tw <= 64) {
        const int per = 64 / tw;                         // columns per wavefront and step
        const int c = lane / tw, w = lane % tw;          // this lane's column of the step and its word
        const bool mine = c < per;
        // the lanes of the same column that hold HIGHER words: lane + 1 .. c tw + tw - 1
        const int last = c * tw + tw - 1;                // (< 64 when mine)
        const unsigned long long above = mine && last > lane ? ((~0ull >> (63 - last)) & ~(~0ull >> (63 - lane))) : 0ull;
        for (long c0 = wave * per; c0 < n_cols; c0 += waves * per) {
            const long col = c0 + c;
            const bool live = mine && col < n_cols;
            const uint32_t x = live ? toggles[col * tw + w] : 0u;
            const unsigned long long odd = __ballot(live && (__popc(x) & 1));
            const uint32_t carry = (uint32_t)(__popcll(odd & above) & 1);
            const uint32_t S = vox_suffix_xor(x) ^ (0u - carry);
            if (live) {
                if (w < nzw) {
                    uint32_t o = (S >> 1) | (carry << 31);
                    if (w == nzw - 1) o &= top_mask;
                    bits[col * nzw + w] = o;
                    occupied += __popc(o);
                }
                if (w == 0) open += S & 1u;
            }
        }
    } else {
        for (long col = wave; col < n_cols; col += waves) {
            uint32_t carry = 0;                          // the parity of the words above the chunk
            for (int w0 = (tw - 1) / 64 * 64; w0 >= 0; w0 -= 64) {
                const int w = w0 + lane;
                const bool live = w < tw;
                const uint32_t x = live ? toggles[col * tw + w] : 0u;
                const unsigned long long odd = __ballot(live && (__popc(x) & 1));
                const unsigned long long above = lane < 63 ? ~0ull << (lane + 1) : 0ull;
                const uint32_t cin = (carry ^ (uint32_t)(__popcll(odd & above) & 1));
                const uint32_t S = vox_suffix_xor(x) ^ (0u - cin);
                if (live) {
                    if (w < nzw) {
                        uint32_t o = (S >> 1) | (cin << 31);
                        if (w == nzw - 1) o &= top_mask;
                        bits[col * nzw + w] = o;
                        occupied += __popc(o);
                    }
                    if (w == 0) open += S & 1u;
                }
                carry ^= (uint32_t)(__popcll(odd) & 1);
            }
        }
    }
    occupied = wave_sum(occupied);
    open = wave_sum(open);
    if (lane == 0) {
        stat_add(stats, GPNERF_VOXEL_OCCUPIED, occupied);
        stat_add(stats, GPNERF_VOXEL_OPEN_COLUMNS, open);
    }
}

// rule NONZERO.  A column's toggle row is nz + 1 int32 counts; S[m] = the sum of the counts m .. nz; point k is occupied iff
// S[k + 1] != 0, the column is open iff S[0] != 0.  A wavefront takes one column per step, 64 consecutive counts m = 64 q + 1 + lane at
// a time from the top down (one contiguous load; a ballot of the 64 flags is the output's words 2 q and 2 q + 1), a shuffle suffix
// sum inside the chunk and a carry from chunk to chunk.  |S| <= the column's crossings < 2^31.
__global__ __launch_bounds__(THREADS) void voxelize_resolve_nonzero_kernel(const int* __restrict__ counts, int nz, long n_cols, uint32_t* bits,
                                                                           long long* stats) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (THREADS / 64) + threadIdx.x / 64, waves = (long)gridDim.x * (THREADS / 64);
    const int nzw = (nz + 31) / 32;
    const long row = (long)nz + 1;
    long long occupied = 0, open = 0;
    for (long col = wave; col < n_cols; col += waves) {
        int carry = 0;                                   // the sum of the counts above the chunk
        for (int q = (nz - 1) / 64; q >= 0; --q) {
            const int mth = 64 * q + 1 + lane;
            const bool live = mth <= nz;
            int v = live ? counts[col * row + mth] : 0;
            for (int d = 1; d < 64; d <<= 1) {           // inclusive suffix sum over the lanes
                const int up = __shfl_down(v, d);
                if (lane + d < 64) v += up;
            }
            const int total = __shfl(v, 0);
            const unsigned long long set = __ballot(live && (v + carry) != 0);
            if (lane < 2 && 2 * q + lane < nzw) {
                const uint32_t o = (uint32_t)(set >> (32 * lane));
                bits[col * nzw + 2 * q + lane] = o;
                occupied += __popc(o);
            }
            carry += total;
        }
        if (lane == 0) open += (carry + counts[col * row]) != 0;
    }
    occupied = wave_sum(occupied);
    open = wave_sum(open);
    if (lane == 0) {
        stat_add(stats, GPNERF_VOXEL_OCCUPIED, occupied);
        stat_add(stats, GPNERF_VOXEL_OPEN_COLUMNS, open);
    }
}

// cube > iso, packed: a wavefront takes 64 consecutive points of a column (one contiguous load), the ballot is two words
__global__ __launch_bounds__(THREADS) void voxel_pack_kernel(const float* __restrict__ cube, int nz, long n_cols, float iso, uint32_t* bits) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (THREADS / 64) + threadIdx.x / 64, waves = (long)gridDim.x * (THREADS / 64);
    const int nzw = (nz + 31) / 32, chunks = (nz + 63) / 64;
    for (long t = wave; t < n_cols * chunks; t += waves) {
        const long col = t / chunks;
        const int q = (int)(t % chunks), k = 64 * q + lane;
        const unsigned long long set = __ballot(k < nz && cube[col * nz + k] > iso);
        if (lane < 2 && 2 * q + lane < nzw) bits[col * nzw + 2 * q + lane] = (uint32_t)(set >> (32 * lane));
    }
}

__global__ __launch_bounds__(THREADS) void voxel_unpack_kernel(const uint32_t* __restrict__ bits, int nz, long n_cols, float* cube) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (THREADS / 64) + threadIdx.x / 64, waves = (long)gridDim.x * (THREADS / 64);
    const int nzw = (nz + 31) / 32, chunks = (nz + 63) / 64;
    for (long t = wave; t < n_cols * chunks; t += waves) {
        const long col = t / chunks;
        const int q = (int)(t % chunks), k = 64 * q + lane;
        if (k < nz) cube[col * nz + k] = (bits[col * nzw + (k >> 5)] >> (k & 31)) & 1u ? 1.0f : 0.0f;
    }
}

__global__ void voxel_counts_zero_kernel(long long* out) {
    if ((int)threadIdx.x < GPNERF_VOXEL_COUNTS) out[threadIdx.x] = 0;
}

// a thread counts its words p, p + stride, ...; a wavefront adds its four sums once
__global__ __launch_bounds__(THREADS) void voxel_counts_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, long n_words,
                                                               long long* out) {
    const long stride = (long)gridDim.x * THREADS;
    long long cnt[GPNERF_VOXEL_COUNTS] = {};
    for (long p = (long)blockIdx.x * THREADS + threadIdx.x; p < n_words; p += stride) {
        const uint32_t wa = a[p], wb = b ? b[p] : 0u;
        cnt[GPNERF_VOXEL_A] += __popc(wa);
        cnt[GPNERF_VOXEL_B] += __popc(wb);
        cnt[GPNERF_VOXEL_BOTH] += __popc(wa & wb);
        cnt[GPNERF_VOXEL_EITHER] += __popc(wa | wb);
    }
    for (int k = 0; k < GPNERF_VOXEL_COUNTS; ++k) {
        const long long v = wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0) stat_add(out, k, v);
    }
}

// one lane per point: the nearest lattice point's bit
__global__ __launch_bounds__(THREADS) void voxel_contains_kernel(const uint32_t* __restrict__ bits, const Lattice g, const float* __restrict__ points,
                                                                 long n, uint8_t* out) {
    const long p = (long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= n) return;
    const double r0 = rint(((double)points[3 * p] - g.lo[0]) / g.step[0]);
    const double r1 = rint(((double)points[3 * p + 1] - g.lo[1]) / g.step[1]);
    const double r2 = rint(((double)points[3 * p + 2] - g.lo[2]) / g.step[2]);
    // (every comparison is false for a NaN)
    const bool inside = r0 >= 0.0 && r0 < (double)g.nx && r1 >= 0.0 && r1 < (double)g.ny && r2 >= 0.0 && r2 < (double)g.nz;
    uint8_t v = 0;
    if (inside) {
        const int k = (int)r2;
        const long col = (long)(int)r0 * g.ny + (int)r1;
        v = (uint8_t)((bits[col * ((g.nz + 31) / 32) + (k >> 5)] >> (k & 31)) & 1u);
    }
    out[p] = v;
}

}  // namespace

extern "C" {

size_t gpnerf_mesh_voxelize_workspace_bytes(int64_t n_faces, const int32_t* dims, int32_t rule) {
    if (n_faces < 0 || n_faces > INT32_MAX || !dims_ok(dims) || !rule_ok(rule)) return 0;
    return layout_of(n_faces, dims, rule).total;
}

int gpnerf_mesh_voxelize(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const double* lattice,
                         const int32_t* dims, int32_t rule, void* workspace, size_t workspace_bytes, uint32_t* bits, int64_t* stats,
                         void* stream) {
    if (!workspace || !bits || !stats || !mesh_ok(vertices, n_vertices, faces, n_faces) || !dims_ok(dims) || !lattice_ok(lattice) || !rule_ok(rule))
        return GPNERF_E_ARG;
    const Layout l = layout_of(n_faces, dims, rule);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    char* base = static_cast<char*>(workspace);
    unsigned long long* list_len = reinterpret_cast<unsigned long long*>(base + l.hdr);
    uint32_t* toggles = reinterpret_cast<uint32_t*>(base + l.toggles);
    uint32_t* list = reinterpret_cast<uint32_t*>(base + l.list);
    const Lattice g = lattice_of(lattice, dims);
    const Mesh m = {vertices, faces, (long)n_vertices, (long)n_faces};
    const long n_cols = (long)g.nx * g.ny, n_words = n_cols * (long)toggle_row_host(g.nz, rule);
    long long* st = reinterpret_cast<long long*>(stats);
    hipLaunchKernelGGL(voxelize_clear_kernel, dim3(sweep_blocks(n_words, THREADS)), dim3(THREADS), 0, S_(stream), toggles, n_words, list_len, st);
    if (n_faces > 0) {
        hipLaunchKernelGGL(voxelize_faces_kernel, dim3(blocks_for(n_faces, THREADS)), dim3(THREADS), 0, S_(stream), m, g, (int)rule, toggles, list,
                           list_len, st);
        hipLaunchKernelGGL(voxelize_large_kernel, dim3(LARGE_BLOCKS), dim3(THREADS), 0, S_(stream), m, g, (int)rule, toggles, list, list_len, st);
    }
    if (rule == GPNERF_VOXEL_PARITY) {
        const int tw = g.nz / 32 + 1;
        const int64_t steps = tw <= 64 ? (n_cols + 64 / tw - 1) / (64 / tw) : n_cols;            // wavefront steps
        hipLaunchKernelGGL(voxelize_resolve_parity_kernel, dim3(sweep_blocks(steps, THREADS / 64)), dim3(THREADS), 0, S_(stream), toggles, g.nz,
                           n_cols, bits, st);
    } else {
        hipLaunchKernelGGL(voxelize_resolve_nonzero_kernel, dim3(sweep_blocks(n_cols, THREADS / 64)), dim3(THREADS), 0, S_(stream),
                           reinterpret_cast<const int*>(toggles), g.nz, n_cols, bits, st);
    }
    return launch_status();
}

int gpnerf_voxel_from_cube(const float* cube, const int32_t* dims, float iso, uint32_t* bits, void* stream) {
    if (!cube || !bits || !dims_ok(dims)) return GPNERF_E_ARG;
    const long n_cols = (long)dims[0] * dims[1];
    const int64_t steps = n_cols * ((dims[2] + 63) / 64);
    hipLaunchKernelGGL(voxel_pack_kernel, dim3(sweep_blocks(steps, THREADS / 64)), dim3(THREADS), 0, S_(stream), cube, (int)dims[2], n_cols, iso, bits);
    return launch_status();
}

int gpnerf_voxel_unpack(const uint32_t* bits, const int32_t* dims, float* cube, void* stream) {
    if (!cube || !bits || !dims_ok(dims)) return GPNERF_E_ARG;
    const long n_cols = (long)dims[0] * dims[1];
    const int64_t steps = n_cols * ((dims[2] + 63) / 64);
    hipLaunchKernelGGL(voxel_unpack_kernel, dim3(sweep_blocks(steps, THREADS / 64)), dim3(THREADS), 0, S_(stream), bits, (int)dims[2], n_cols, cube);
    return launch_status();
}

int gpnerf_voxel_stats(const uint32_t* a, const uint32_t* b, const int32_t* dims, int64_t* out, void* stream) {
    if (!a || !out || !dims_ok(dims)) return GPNERF_E_ARG;
    const long n_words = (long)dims[0] * dims[1] * ((dims[2] + 31) / 32);
    long long* o = reinterpret_cast<long long*>(out);
    hipLaunchKernelGGL(voxel_counts_zero_kernel, dim3(1), dim3(64), 0, S_(stream), o);
    const unsigned blocks = sweep_blocks(n_words, THREADS, COUNT_BLOCKS_MAX);
    hipLaunchKernelGGL(voxel_counts_kernel, dim3(blocks), dim3(THREADS), 0, S_(stream), a, b, n_words, o);
    return launch_status();
}

int gpnerf_voxel_contains(const uint32_t* bits, const int32_t* dims, const double* lattice, const float* points, int64_t n, uint8_t* out,
                          void* stream) {
    if (!bits || !dims_ok(dims) || !lattice_ok(lattice) || n < 0 || n > INT32_MAX || ((!points || !out) && n > 0)) return GPNERF_E_ARG;
    if (n == 0) return GPNERF_OK;
    const Lattice g = lattice_of(lattice, dims);
    hipLaunchKernelGGL(voxel_contains_kernel, dim3(blocks_for(n, THREADS)), dim3(THREADS), 0, S_(stream), bits, g, points, (long)n, out);
    return launch_status();
}

}  // extern "C"
