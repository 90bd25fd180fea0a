// gpnerf_meshrepair.hip -- the repair of a loaded triangle mesh on gfx950: vertices of one key welded to the lowest index among them,
// invalid / unkeyable / collapsed / repeated faces dropped, every edge-connected patch given one winding and, where it is closed, turned
// to enclose positive volume.  include/gpnerf_hip.h states the definition and the workspace formula; tests/repair_cases.py restates it
// in numpy.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from the arguments alone;
// the output sizes stay in the workspace.  A FIXED number of launches for a given set of flags, no device-wide barrier, no cooperative
// launch, and no lane waits for a value another lane has yet to write.  The atomics, all on integers, and why their arrival order
// cannot matter:
//   - the three open-addressing hash tables.  A slot never empties and never changes its key, so whatever the races a key ends in ONE
//     slot: the first empty slot of its probe sequence at the time of its first insert, which every later insert of that key walks up
//     to.  The index-valued tables (vertices, faces) CAS the own index into an empty slot and atomicMin it into a slot whose occupant
//     has an equal key: at the kernel's end the slot holds the key's smallest index.  WHICH slot a key ends in depends on the order;
//     what a lookup behind the kernel boundary returns does not.  The edge table's slot holds the packed edge itself; beside it an
//     incidence count (an add) and the first two incidences in arrival order -- only edges of exactly two incidences are read, as an
//     unordered pair.  A fourth table counts, for the non-manifold edges only, the half-edges per (edge, patch): its slot keeps its
//     first occupant, and only the count beside it is read;
//   - the union-find over faces whose word packs (parent << 1) | parity-to-parent: see unite();
//   - integer adds into the patch's row and the header's counters (addition commutes); the bounding box by atomicMin / atomicMax on
//     the order-preserving integer image of the float32 coordinates.
// The scans (gpnerf_scan.h) have no atomic.  The only floating-point arithmetic is per vertex (the key of a tolerance, the
// quantisation): no float is summed; emit copies coordinates as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status, blocks_for, sweep_blocks; wave_count, wave_sum
#include "gpnerf_scan.h"       // the three-launch integer scan

struct RepairScan;             // names this file's instances of the scan kernels

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int64_t MAX_VERTICES = (int64_t)1 << 30;
constexpr int64_t MAX_FACES = (((int64_t)1 << 31) - 1) / 3;  // the adjacency's limit
constexpr long long REPAIR_MAGIC = 0x5245504131ll;       // "REPA1"
constexpr uint32_t ALL_FLAGS = GPNERF_REPAIR_WELD | GPNERF_REPAIR_DROP_DUPLICATES | GPNERF_REPAIR_ORIENT | GPNERF_REPAIR_OUTWARD;

typedef unsigned long long u64;
constexpr u64 EDGE_EMPTY = ~(u64)0;                      // (no packed edge: a vertex index is below 2^30)

// the header's 64-bit words
enum { H_MAGIC, H_NV, H_NF, H_STATUS = GPNERF_REPAIR_HDR_STATUS, H_FLAGS, H_V_OUT, H_F_OUT, H_WELDED, H_V_UNKEYABLE, H_F_INVALID, H_F_UNKEYABLE,
       H_F_COLLAPSED, H_F_DUPLICATE, H_F_FLIPPED, H_E_NONMANIFOLD, H_PATCHES, H_P_CLOSED, H_P_UNORIENTABLE, H_P_INVERTED, H_P_UNDECIDED,
       H_BOX_LO, H_BOX_HI = H_BOX_LO + 3, H_WORDS = H_BOX_HI + 3 };
static_assert(H_NF + 1 == H_STATUS && H_WORDS <= 32, "the header's words");

// a patch's row, indexed by its root face
enum { P_OPEN, P_FACES, P_FLIPPED, P_BAD, P_HI, P_LO, P_DECIDE, PCOLS };       // (OPEN first: repair_shared_lookup_kernel adds to it alone)
enum { DECIDE_INVERT = 1, DECIDE_UNORIENTABLE = 2 };
enum { BIT_OPEN = 1, BIT_BAD = 2, BIT_SHARED = 4 };      // fbits (SHARED: the face has a non-manifold edge)

// the formula of include/gpnerf_hip.h
__host__ inline int64_t table_capacity(int64_t n) {
    int64_t c = 64;
    while (c < 2 * n) c <<= 1;
    return c;
}

struct Layout { size_t hdr, rep, vnew, vtab, fate, fbits, fnew, parent, froot, ftab, ekey, ecnt, einc, htab, hcnt, ptab, bsum, total; int64_t cap_v, cap_f, cap_e; };

__host__ inline Layout layout_of(int64_t nv, int64_t nf) {
    Layout l;
    size_t o = 0;
    const int64_t most = nv > nf ? nv : nf;
    l.cap_v = table_capacity(nv);
    l.cap_f = table_capacity(nf);
    l.cap_e = table_capacity(3 * nf);
    l.hdr = o;    o += 256;
    l.rep = o;    o += align256(4 * (size_t)nv);
    l.vnew = o;   o += align256(4 * (size_t)nv);
    l.vtab = o;   o += align256(4 * (size_t)l.cap_v);
    l.fate = o;   o += align256((size_t)nf);
    l.fbits = o;  o += align256((size_t)nf);
    l.fnew = o;   o += align256(4 * (size_t)nf);
    l.parent = o; o += align256(4 * (size_t)nf);
    l.froot = o;  o += align256(4 * (size_t)nf);
    l.ftab = o;   o += align256(4 * (size_t)l.cap_f);
    l.ekey = o;   o += align256(8 * (size_t)l.cap_e);
    l.ecnt = o;   o += align256(4 * (size_t)l.cap_e);
    l.einc = o;   o += align256(8 * (size_t)l.cap_e);
    l.htab = o;   o += align256(4 * (size_t)l.cap_e);
    l.hcnt = o;   o += align256(4 * (size_t)l.cap_e);
    l.ptab = o;   o += align256(8 * (size_t)PCOLS * (size_t)nf);
    l.bsum = o;   o += align256(8 * (size_t)(((most > 1 ? most : 1) + SCAN_CHUNK - 1) / SCAN_CHUNK));
    l.total = o;
    return l;
}

struct Ws {                                              // the workspace's regions, as the kernels see them
    long long* hdr; int32_t* rep; int32_t* vnew; int32_t* vtab; uint8_t* fate; uint8_t* fbits; int32_t* fnew; uint32_t* parent; uint32_t* froot;
    int32_t* ftab; u64* ekey; int32_t* ecnt; int32_t* einc; int32_t* htab; int32_t* hcnt; long long* ptab; long long* bsum;
    u64 mask_v, mask_f, mask_e;
};

__host__ inline Ws ws_of(void* workspace, const Layout& l) {
    char* b = static_cast<char*>(workspace);
    Ws w;
    w.hdr = reinterpret_cast<long long*>(b + l.hdr);
    w.rep = reinterpret_cast<int32_t*>(b + l.rep);
    w.vnew = reinterpret_cast<int32_t*>(b + l.vnew);
    w.vtab = reinterpret_cast<int32_t*>(b + l.vtab);
    w.fate = reinterpret_cast<uint8_t*>(b + l.fate);
    w.fbits = reinterpret_cast<uint8_t*>(b + l.fbits);
    w.fnew = reinterpret_cast<int32_t*>(b + l.fnew);
    w.parent = reinterpret_cast<uint32_t*>(b + l.parent);
    w.froot = reinterpret_cast<uint32_t*>(b + l.froot);
    w.ftab = reinterpret_cast<int32_t*>(b + l.ftab);
    w.ekey = reinterpret_cast<u64*>(b + l.ekey);
    w.ecnt = reinterpret_cast<int32_t*>(b + l.ecnt);
    w.einc = reinterpret_cast<int32_t*>(b + l.einc);
    w.htab = reinterpret_cast<int32_t*>(b + l.htab);
    w.hcnt = reinterpret_cast<int32_t*>(b + l.hcnt);
    w.ptab = reinterpret_cast<long long*>(b + l.ptab);
    w.bsum = reinterpret_cast<long long*>(b + l.bsum);
    w.mask_v = (u64)l.cap_v - 1;
    w.mask_f = (u64)l.cap_f - 1;
    w.mask_e = (u64)l.cap_e - 1;
    return w;
}

bool sizes_ok(int64_t nv, int64_t nf) { return nv >= 0 && nf >= 0 && nv <= MAX_VERTICES && nf <= MAX_FACES; }

// ---------------------------------------------------------------- keys and tables

DEV u64 mix64(u64 x) {                                   // (splitmix64's finaliser; any function would do: step 8)
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

DEV int32_t a_load(int32_t* p, u64 i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DEV uint32_t a_load(uint32_t* p, u64 i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
DEV u64 a_load(u64* p, u64 i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct VKey { long long k[3]; };

// step 1: false for an UNKEYABLE vertex
DEV bool vertex_key(const float* __restrict__ vertices, long v, double tol, VKey* key) {
    for (int a = 0; a < 3; ++a) {
        const float x = vertices[3 * v + a];
        if (!(fabsf(x) <= 3.402823466e+38f)) return false;   // not finite
        if (tol > 0.0) {
            const double d = (double)x / tol;
            if (!(fabs(d) < 4611686018427387904.0)) return false;     // 2^62
            key->k[a] = (long long)floor(d);
        } else {
            const uint32_t bits = __float_as_uint(x);
            key->k[a] = bits == 0x80000000u ? 0 : (long long)bits;      // -0.0 is +0.0
        }
    }
    return true;
}
DEV bool same(const VKey& a, const VKey& b) { return a.k[0] == b.k[0] && a.k[1] == b.k[1] && a.k[2] == b.k[2]; }
DEV u64 hash_of(const VKey& a) { return mix64((u64)a.k[0] + mix64((u64)a.k[1] + mix64((u64)a.k[2]))); }

struct FKey { int32_t r[3]; };                           // the representatives of a face's corners, ascending

// steps 3's first three fates; GPNERF_REPAIR_KEPT and the sorted triple when none applies
DEV int face_class(const int32_t* __restrict__ faces, long f, long nv, const int32_t* __restrict__ rep, FKey* key, int32_t* corner_rep) {
    int32_t r[3];
    for (int k = 0; k < 3; ++k) {
        const int32_t i = faces[3 * f + k];
        if (i < 0 || i >= nv) return GPNERF_REPAIR_INVALID;
        r[k] = i;
    }
    for (int k = 0; k < 3; ++k) {
        r[k] = rep[r[k]];
        if (r[k] < 0) return GPNERF_REPAIR_UNKEYABLE;
    }
    if (r[0] == r[1] || r[1] == r[2] || r[0] == r[2]) return GPNERF_REPAIR_COLLAPSED;
    if (corner_rep)
        for (int k = 0; k < 3; ++k) corner_rep[k] = r[k];
    if (r[0] > r[1]) { const int32_t t = r[0]; r[0] = r[1]; r[1] = t; }
    if (r[1] > r[2]) { const int32_t t = r[1]; r[1] = r[2]; r[2] = t; }
    if (r[0] > r[1]) { const int32_t t = r[0]; r[0] = r[1]; r[1] = t; }
    for (int k = 0; k < 3; ++k) key->r[k] = r[k];
    return GPNERF_REPAIR_KEPT;
}
DEV bool same(const FKey& a, const FKey& b) { return a.r[0] == b.r[0] && a.r[1] == b.r[1] && a.r[2] == b.r[2]; }
DEV u64 hash_of(const FKey& a) { return mix64(((u64)(uint32_t)a.r[0] << 32 | (uint32_t)a.r[1]) + mix64((u64)(uint32_t)a.r[2])); }

DEV u64 edge_key(int32_t a, int32_t b) { return a < b ? ((u64)(uint32_t)a << 32 | (uint32_t)b) : ((u64)(uint32_t)b << 32 | (uint32_t)a); }

// the slot of a packed edge: found, or claimed by CAS.  (The table has at least as many empty slots as keys: the probe ends.)
DEV u64 edge_insert(u64* ekey, u64 mask, u64 key) {
    u64 s = mix64(key) & mask;
    while (true) {
        u64 cur = a_load(ekey, s);
        if (cur == EDGE_EMPTY) {
            cur = atomicCAS(&ekey[s], EDGE_EMPTY, key);
            if (cur == EDGE_EMPTY) return s;
        }
        if (cur == key) return s;
        s = (s + 1) & mask;
    }
}

// behind the kernel boundary: the slot of a packed edge, or an empty slot when it was never inserted
DEV u64 edge_find(const u64* __restrict__ ekey, u64 mask, u64 key) {
    u64 s = mix64(key) & mask;
    while (ekey[s] != key && ekey[s] != EDGE_EMPTY) s = (s + 1) & mask;
    return s;
}

// ---------------------------------------------------------------- the count

// the tables the flags use cleared, the patches' rows zeroed, the header
__global__ __launch_bounds__(THREADS) void repair_clear_kernel(Ws w, long nv, long nf, uint32_t flags) {
    const long stride = (long)gridDim.x * THREADS, i0 = (long)blockIdx.x * THREADS + threadIdx.x;
    if (flags & GPNERF_REPAIR_WELD)
        for (u64 i = i0; i <= w.mask_v; i += stride) w.vtab[i] = -1;
    if (flags & GPNERF_REPAIR_DROP_DUPLICATES)
        for (u64 i = i0; i <= w.mask_f; i += stride) w.ftab[i] = -1;
    if (flags & GPNERF_REPAIR_ORIENT) {
        for (u64 i = i0; i <= w.mask_e; i += stride) { w.ekey[i] = EDGE_EMPTY; w.ecnt[i] = 0; w.htab[i] = -1; w.hcnt[i] = 0; }
        for (long i = i0; i < nf * PCOLS; i += stride) w.ptab[i] = 0;
    }
    if (i0 == 0) {
        for (int k = 0; k < 32; ++k) w.hdr[k] = 0;
        w.hdr[H_MAGIC] = REPAIR_MAGIC;
        w.hdr[H_NV] = nv;
        w.hdr[H_NF] = nf;
        w.hdr[H_FLAGS] = flags;
        for (int a = 0; a < 3; ++a) { w.hdr[H_BOX_LO + a] = 0xffffffffll; w.hdr[H_BOX_HI + a] = 0; }
        w.hdr[H_STATUS] = GPNERF_REPAIR_COUNTING;
    }
}

// WELD, a lane per keyable vertex: its index into its key's slot -- CAS into an empty one, atomicMin into one whose occupant has an
// equal key (the occupant may change under the lane's eyes, its key cannot)
__global__ __launch_bounds__(THREADS) void repair_vertex_insert_kernel(const float* __restrict__ vertices, long nv, double tol, Ws w) {
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    VKey key, other;
    if (v >= nv || !vertex_key(vertices, v, tol, &key)) return;
    u64 s = hash_of(key) & w.mask_v;
    while (true) {
        int32_t cur = a_load(w.vtab, s);
        if (cur < 0) {
            cur = atomicCAS(&w.vtab[s], -1, (int32_t)v);
            if (cur < 0) return;
        }
        if (cur == (int32_t)v) return;
        vertex_key(vertices, cur, tol, &other);                 // (an occupant is keyable)
        if (same(key, other)) { atomicMin(&w.vtab[s], (int32_t)v); return; }
        s = (s + 1) & w.mask_v;
    }
}

// a lane per vertex, behind the kernel boundary: rep (step 2), -1 for an unkeyable vertex; the marks of the output vertices cleared
__global__ __launch_bounds__(THREADS) void repair_vertex_lookup_kernel(const float* __restrict__ vertices, long nv, double tol, uint32_t flags, Ws w) {
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    bool welded = false, unkeyable = false;
    if (v < nv) {
        VKey key, other;
        int32_t r = -1;
        if (!vertex_key(vertices, v, tol, &key)) unkeyable = true;
        else if (!(flags & GPNERF_REPAIR_WELD)) r = (int32_t)v;
        else {
            u64 s = hash_of(key) & w.mask_v;
            while (true) {
                r = w.vtab[s];
                if (r < 0 || r == (int32_t)v) break;
                vertex_key(vertices, r, tol, &other);
                if (same(key, other)) break;
                s = (s + 1) & w.mask_v;
            }
            if (r < 0) r = (int32_t)v;                          // (not reached: every keyable vertex was inserted)
            welded = r != (int32_t)v;
        }
        w.rep[v] = r;
        w.vnew[v] = 0;
    }
    wave_count(welded, &w.hdr[H_WELDED]);
    wave_count(unkeyable, &w.hdr[H_V_UNKEYABLE]);
}

// a lane per face: the fates INVALID, UNKEYABLE and COLLAPSED; with DROP_DUPLICATES the others' indices into the slot of their sorted triple
__global__ __launch_bounds__(THREADS) void repair_face_insert_kernel(const int32_t* __restrict__ faces, long nf, long nv, uint32_t flags, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= nf) return;
    FKey key, other;
    const int fate = face_class(faces, f, nv, w.rep, &key, nullptr);
    w.fate[f] = (uint8_t)fate;
    if (fate != GPNERF_REPAIR_KEPT || !(flags & GPNERF_REPAIR_DROP_DUPLICATES)) return;
    u64 s = hash_of(key) & w.mask_f;
    while (true) {
        int32_t cur = a_load(w.ftab, s);
        if (cur < 0) {
            cur = atomicCAS(&w.ftab[s], -1, (int32_t)f);
            if (cur < 0) return;
        }
        if (cur == (int32_t)f) return;
        face_class(faces, cur, nv, w.rep, &other, nullptr);     // (an occupant reached this step)
        if (same(key, other)) { atomicMin(&w.ftab[s], (int32_t)f); return; }
        s = (s + 1) & w.mask_f;
    }
}

// a lane per face, behind the kernel boundary: DUPLICATE when the key's slot holds a lower index; the LIVE faces marked, their
// representatives marked as output vertices, their word of the union-find set to a root; with ORIENT their three half-edges entered:
// the incidence count, the first two incidences as (face << 1 | direction), direction 1 for a half-edge that runs from the lower
// representative to the higher.  The third incidence of an edge counts it as non-manifold, once.
__global__ __launch_bounds__(THREADS) void repair_face_lookup_kernel(const int32_t* __restrict__ faces, long nf, long nv, uint32_t flags, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    int fate = -1, nonmanifold = 0;
    if (f < nf) {
        fate = w.fate[f];
        FKey key, other;
        int32_t c[3];
        if (fate == GPNERF_REPAIR_KEPT) {
            face_class(faces, f, nv, w.rep, &key, c);
            if (flags & GPNERF_REPAIR_DROP_DUPLICATES) {
                u64 s = hash_of(key) & w.mask_f;
                int32_t first = (int32_t)f;
                while (true) {
                    const int32_t cur = w.ftab[s];
                    if (cur < 0 || cur == (int32_t)f) break;
                    face_class(faces, cur, nv, w.rep, &other, nullptr);
                    if (same(key, other)) { first = cur; break; }
                    s = (s + 1) & w.mask_f;
                }
                if (first != (int32_t)f) { fate = GPNERF_REPAIR_DUPLICATE; w.fate[f] = (uint8_t)fate; }
            }
        }
        const bool live = fate == GPNERF_REPAIR_KEPT;
        w.fnew[f] = live ? 1 : 0;
        if (live) {
            for (int k = 0; k < 3; ++k) w.vnew[c[k]] = 1;       // (every writer stores the same word)
            if (flags & GPNERF_REPAIR_ORIENT) {
                w.parent[f] = (uint32_t)f << 1;
                for (int k = 0; k < 3; ++k) {
                    const int32_t a = c[k], b = c[(k + 1) % 3];
                    const u64 s = edge_insert(w.ekey, w.mask_e, edge_key(a, b));
                    const int n = atomicAdd(&w.ecnt[s], 1);
                    if (n < 2) w.einc[2 * s + n] = (int32_t)(((uint32_t)f << 1) | (a < b ? 1u : 0u));
                    if (n == 2) ++nonmanifold;
                }
            }
        }
    }
    wave_count(fate == GPNERF_REPAIR_INVALID, &w.hdr[H_F_INVALID]);
    wave_count(fate == GPNERF_REPAIR_UNKEYABLE, &w.hdr[H_F_UNKEYABLE]);
    wave_count(fate == GPNERF_REPAIR_COLLAPSED, &w.hdr[H_F_COLLAPSED]);
    wave_count(fate == GPNERF_REPAIR_DUPLICATE, &w.hdr[H_F_DUPLICATE]);
    const long long nm = wave_sum((long long)nonmanifold);
    if ((threadIdx.x & 63) == 0) stat_add(w.hdr, H_E_NONMANIFOLD, nm);
}

// OUTWARD, a lane per vertex: the float32 bounding box of the output vertices, by integer minimum and maximum of the order-preserving
// image of the bit patterns
DEV uint32_t ordered_of(float x) { const uint32_t b = __float_as_uint(x); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
DEV float float_of(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

__global__ __launch_bounds__(THREADS) void repair_box_kernel(const float* __restrict__ vertices, long nv, Ws w) {
    const long stride = (long)gridDim.x * THREADS;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (long v = (long)blockIdx.x * THREADS + threadIdx.x; v < nv; v += stride) {
        if (w.vnew[v] != 1) continue;
        for (int a = 0; a < 3; ++a) {
            const uint32_t u = ordered_of(vertices[3 * v + a]);
            lo[a] = u < lo[a] ? u : lo[a];
            hi[a] = u > hi[a] ? u : hi[a];
        }
    }
    for (int a = 0; a < 3; ++a) {
        for (int d = 32; d > 0; d >>= 1) {
            const uint32_t ol = __shfl_xor(lo[a], d), oh = __shfl_xor(hi[a], d);
            lo[a] = ol < lo[a] ? ol : lo[a];
            hi[a] = oh > hi[a] ? oh : hi[a];
        }
        // one lane per wavefront, and only where the wavefront would move the bound: a bound read late is one that has moved less, so
        // no atomic that matters is skipped (15 360 wavefronts on six addresses took 0.7 ms of a 1.5 ms call: DESIGN.md 4.22)
        if ((threadIdx.x & 63) == 0) {
            u64* plo = reinterpret_cast<u64*>(&w.hdr[H_BOX_LO + a]);
            u64* phi = reinterpret_cast<u64*>(&w.hdr[H_BOX_HI + a]);
            if ((u64)lo[a] < a_load(plo, 0)) atomicMin(plo, (u64)lo[a]);
            if ((u64)hi[a] > a_load(phi, 0)) atomicMax(phi, (u64)hi[a]);
        }
    }
}

// ---------------------------------------------------------------- patches: the union-find with parities
//
// p[f] = (parent << 1) | parity, parity = s(f) xor s(parent); a root's word is (f << 1).  Every access is an agent-scope atomic (the
// XCDs' L2s are not coherent for plain loads within a kernel: gpnerf_unionfind.h).  The structure is a forest at every moment -- a
// link hangs a root under a lower root of ANOTHER tree, a compression re-hangs a node under a lower ancestor of its own tree -- and
// every word ever written states the relative flip of two faces along the forest's path between them, which neither a later link nor
// a later compression changes.  So a stale word still gives a correct (ancestor, parity); indices strictly decrease along a path, so
// a walk ends; and a link's CAS fails only when somebody else linked that root, of which there are at most (faces - 1).

// the root of i at the time it is read, and the parity of i to it
DEV uint32_t p_find(uint32_t* p, uint32_t i, uint32_t* parity) {
    uint32_t par = 0, word = a_load(p, i);
    while ((word >> 1) != i) { par ^= word & 1u; i = word >> 1; word = a_load(p, i); }
    *parity = par;
    return i;
}

// point the words of i's path at r (found by p_find with parity `par` of i to r) by CAS; a CAS that fails is skipped
DEV void p_compress(uint32_t* p, uint32_t i, uint32_t r, uint32_t par) {
    while (i > r) {
        const uint32_t word = a_load(p, i), q = word >> 1;
        if (q <= r || q == i) return;                        // already at r (or, read late, at something lower); a root
        atomicCAS(&p[i], word, (r << 1) | par);
        par ^= word & 1u;                                    // parity of q to r = (i to r) xor (i to q)
        i = q;
    }
}

// faces f and g with s(f) xor s(g) = pe: linked, or, when they have one root already, CHECKED -- true when the parities disagree.
// Two read-only walks first (most joined pairs of a mesh close a cycle); compression only on the way to a link.  A pair that is
// checked is checked against a relative parity that no later write changes; a pair that is linked holds by construction: the
// patch has a pair that fails exactly when no flips satisfy all of its pairs.
DEV bool unite(uint32_t* p, uint32_t f, uint32_t g, uint32_t pe) {
    while (true) {
        uint32_t pa, pb;
        uint32_t ra = p_find(p, f, &pa), rb = p_find(p, g, &pb);
        if (ra == rb) return ((pa ^ pb) & 1u) != pe;
        p_compress(p, f, ra, pa);
        p_compress(p, g, rb, pb);
        if (ra < rb) { const uint32_t t = ra; ra = rb; rb = t; }
        if (atomicCAS(&p[ra], ra << 1, (rb << 1) | (pa ^ pb ^ pe)) == (ra << 1)) return false;
    }
}

// a lane per live face: for each of its three edges the incidence count m; m == 1 leaves the face's patch open, m >= 3 is looked at
// per patch behind the flattening (repair_shared_*_kernel); of the two faces on an edge with m == 2 the one of the first incidence
// unites the pair, parity 1 when the two half-edges run the same way
__global__ __launch_bounds__(THREADS) void repair_union_kernel(const int32_t* __restrict__ faces, long nf, long nv, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= nf) return;
    if (w.fate[f] != GPNERF_REPAIR_KEPT) { w.fbits[f] = 0; return; }
    int32_t c[3];
    for (int k = 0; k < 3; ++k) c[k] = w.rep[faces[3 * f + k]];
    int bits = 0;
    for (int k = 0; k < 3; ++k) {
        const u64 s = edge_find(w.ekey, w.mask_e, edge_key(c[k], c[(k + 1) % 3]));
        if (w.ekey[s] == EDGE_EMPTY || w.ecnt[s] < 2) { bits |= BIT_OPEN; continue; }
        if (w.ecnt[s] > 2) { bits |= BIT_SHARED; continue; }
        const uint32_t i0 = (uint32_t)w.einc[2 * s], i1 = (uint32_t)w.einc[2 * s + 1];
        if ((i0 >> 1) != (uint32_t)f) continue;
        if (unite(w.parent, (uint32_t)f, i1 >> 1, (i0 & 1u) == (i1 & 1u) ? 1u : 0u)) bits |= BIT_BAD;
    }
    w.fbits[f] = (uint8_t)bits;
}

// Adds val[0 .. N) to columns 0 .. N of row `root` of the patches' table for every lane with root >= 0, with as few atomics as the
// wavefronts' agreement allows (the scheme of gpnerf_meshcomp.hip's component_add: a body mesh is ONE patch, and a lane per face
// adding to one address serialises).  A wavefront whose active lanes share a root sums first; the workgroup's first thread merges
// the runs of wavefronts that agree; a mixed wavefront adds once per distinct root among its lanes.  EVERY thread of the workgroup
// must reach this call.
template <int N>
DEV void patch_add(long long* __restrict__ table, int32_t root, const long long (&val)[N], int32_t (&s_root)[WAVES], long long (&s_val)[WAVES][N]) {
    const int wave = threadIdx.x >> 6;
    const bool active = root >= 0;
    const u64 m = __ballot(active);
    const int32_t r0 = m ? __shfl(root, __ffsll((long long)m) - 1) : -1;
    const bool uniform = __all(!active || root == r0);
    if (uniform) {
        long long sum[N];
        for (int k = 0; k < N; ++k) sum[k] = wave_sum(active ? val[k] : 0ll);
        if ((threadIdx.x & 63) == 0) {
            s_root[wave] = r0;
            for (int k = 0; k < N; ++k) s_val[wave][k] = sum[k];
        }
    } else {
        if ((threadIdx.x & 63) == 0) s_root[wave] = -1;
        u64 todo = m;
        while (todo) {
            const int lead = __ffsll((long long)todo) - 1;
            const int32_t r = __shfl(root, lead);
            const bool mine = active && root == r;
            for (int k = 0; k < N; ++k) {
                const long long sum = wave_sum(mine ? val[k] : 0ll);
                if ((int)(threadIdx.x & 63) == lead && sum) atomicAdd(reinterpret_cast<u64*>(&table[(long)r * PCOLS + k]), (u64)sum);
            }
            todo &= ~__ballot(mine);
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int32_t cur = -1;
    long long acc[N] = {};
    for (int wv = 0; wv <= WAVES; ++wv) {
        const int32_t r = wv < WAVES ? s_root[wv] : -1;
        if (wv < WAVES && r < 0) continue;
        if (r != cur) {
            if (cur >= 0)
                for (int k = 0; k < N; ++k)
                    if (acc[k]) atomicAdd(reinterpret_cast<u64*>(&table[(long)cur * PCOLS + k]), (u64)acc[k]);
            cur = r;
            for (int k = 0; k < N; ++k) acc[k] = 0;
        }
        if (wv < WAVES)
            for (int k = 0; k < N; ++k) acc[k] += s_val[wv][k];
    }
}

// step 6's grid: q_a(x) = rint((double(x) - c_a) * (1048574 / ext)), unfused (the library is built with -ffp-contract=off)
struct Quant { double c[3]; double scale; };
DEV Quant quant_of(const long long* hdr) {
    Quant q;
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = (double)float_of((uint32_t)hdr[H_BOX_LO + a]), hi = (double)float_of((uint32_t)hdr[H_BOX_HI + a]);
        q.c[a] = (lo + hi) / 2.0;
        const double e = hi - lo;
        ext = e > ext ? e : ext;
    }
    q.scale = ext > 0.0 ? 1048574.0 / ext : 0.0;
    return q;
}
DEV long long quantise(const Quant& q, float x, int a) { return q.scale > 0.0 ? (long long)rint(((double)x - q.c[a]) * q.scale) : 0ll; }

// a lane per face, behind the kernel boundary (plain loads: every root is fixed): the root and the parity to it; 1, the parity, the
// open and the mismatch marks and, with OUTWARD, the two words of the signed determinant of the face as the parity winds it, into
// the root's row
__global__ __launch_bounds__(THREADS) void repair_flatten_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces, long nf, long nv,
                                                                 uint32_t flags, Ws w) {
    __shared__ int32_t s_root[WAVES];
    __shared__ long long s_val[WAVES][6];
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    int32_t root = -1;
    long long val[6] = {0, 0, 0, 0, 0, 0};
    if (f < nf && w.fate[f] == GPNERF_REPAIR_KEPT) {
        uint32_t i = (uint32_t)f, par = 0, word = w.parent[i];
        while ((word >> 1) != i) { par ^= word & 1u; i = word >> 1; word = w.parent[i]; }
        root = (int32_t)i;
        w.froot[f] = (i << 1) | par;
        const int bits = w.fbits[f];
        val[P_FACES] = 1;
        val[P_FLIPPED] = par;
        val[P_OPEN] = (bits & BIT_OPEN) ? 1 : 0;
        val[P_BAD] = (bits & BIT_BAD) ? 1 : 0;
        if (flags & GPNERF_REPAIR_OUTWARD) {
            const Quant q = quant_of(w.hdr);
            long long p[3][3];
            for (int k = 0; k < 3; ++k) {
                const long v = w.rep[faces[3 * f + k]];
                for (int a = 0; a < 3; ++a) p[k][a] = quantise(q, vertices[3 * v + a], a);
            }
            long long det = p[0][0] * (p[1][1] * p[2][2] - p[1][2] * p[2][1]) - p[0][1] * (p[1][0] * p[2][2] - p[1][2] * p[2][0]) +
                            p[0][2] * (p[1][0] * p[2][1] - p[1][1] * p[2][0]);
            if (par) det = -det;
            val[P_HI] = det >> 30;
            val[P_LO] = det & (((long long)1 << 30) - 1);
        }
    }
    patch_add<6>(w.ptab, root, val, s_root, s_val);
}

// ---- non-manifold edges: how many of an edge's half-edges are the PATCH's own.  A fourth table of cap_e int32 slots: a slot holds a
// half-edge 3 f + k, its key -- (the packed edge, the root of f's patch) -- read through it; beside it a count.  The first occupant
// stays (no minimum is wanted: only the count is read).
struct HKey { u64 edge; uint32_t root; };
DEV HKey half_key(const int32_t* __restrict__ faces, const Ws& w, int32_t h) {
    const long f = h / 3;
    const int k = h % 3;
    HKey key;
    key.edge = edge_key(w.rep[faces[3 * f + k]], w.rep[faces[3 * f + (k + 1) % 3]]);
    key.root = w.froot[f] >> 1;
    return key;
}
DEV bool same(const HKey& a, const HKey& b) { return a.edge == b.edge && a.root == b.root; }
DEV u64 hash_of(const HKey& a) { return mix64(a.edge + mix64(a.root)); }

// a lane per live face with a non-manifold edge (none in a launch on a mesh without one): its half-edges on such edges counted per (edge, patch)
__global__ __launch_bounds__(THREADS) void repair_shared_insert_kernel(const int32_t* __restrict__ faces, long nf, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    if (w.hdr[H_E_NONMANIFOLD] == 0 || f >= nf || w.fate[f] != GPNERF_REPAIR_KEPT || !(w.fbits[f] & BIT_SHARED)) return;
    for (int k = 0; k < 3; ++k) {
        const int32_t h = (int32_t)(3 * f + k);
        const HKey key = half_key(faces, w, h);
        const u64 e = edge_find(w.ekey, w.mask_e, key.edge);
        if (w.ekey[e] == EDGE_EMPTY || w.ecnt[e] < 3) continue;
        u64 s = hash_of(key) & w.mask_e;
        while (true) {
            int32_t cur = a_load(w.htab, s);
            if (cur < 0) {
                cur = atomicCAS(&w.htab[s], -1, h);
                if (cur < 0) break;
            }
            if (cur == h || same(key, half_key(faces, w, cur))) break;
            s = (s + 1) & w.mask_e;
        }
        atomicAdd(&w.hcnt[s], 1);
    }
}

// behind the kernel boundary: a non-manifold edge that carries other than two half-edges of the face's own patch leaves the patch open
__global__ __launch_bounds__(THREADS) void repair_shared_lookup_kernel(const int32_t* __restrict__ faces, long nf, Ws w) {
    __shared__ int32_t s_root[WAVES];
    __shared__ long long s_val[WAVES][1];
    if (w.hdr[H_E_NONMANIFOLD] == 0) return;                 // (uniform over the launch)
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    int32_t root = -1;
    long long val[1] = {0};
    if (f < nf && w.fate[f] == GPNERF_REPAIR_KEPT && (w.fbits[f] & BIT_SHARED)) {
        root = (int32_t)(w.froot[f] >> 1);
        for (int k = 0; k < 3; ++k) {
            const int32_t h = (int32_t)(3 * f + k);
            const HKey key = half_key(faces, w, h);
            const u64 e = edge_find(w.ekey, w.mask_e, key.edge);
            if (w.ekey[e] == EDGE_EMPTY || w.ecnt[e] < 3) continue;
            u64 s = hash_of(key) & w.mask_e;
            while (w.htab[s] >= 0 && w.htab[s] != h && !same(key, half_key(faces, w, w.htab[s]))) s = (s + 1) & w.mask_e;
            if (w.htab[s] < 0 || w.hcnt[s] != 2) val[0] = 1;
        }
    }
    patch_add<1>(w.ptab, root, val, s_root, s_val);
}

// a lane per face that is its patch's root: the patch's decision (steps 5 and 6) and the patch counts
__global__ __launch_bounds__(THREADS) void repair_patch_kernel(long nf, uint32_t flags, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    bool patch = false, closed = false, bad = false, inverted = false, undecided = false;
    if (f < nf && w.fate[f] == GPNERF_REPAIR_KEPT && (w.froot[f] >> 1) == (uint32_t)f) {
        long long* row = w.ptab + f * PCOLS;
        patch = true;
        closed = row[P_OPEN] == 0;
        bad = row[P_BAD] != 0;
        long long decide = 0;
        if (bad) decide = DECIDE_UNORIENTABLE;
        else {
            bool majority = true;
            if ((flags & GPNERF_REPAIR_OUTWARD) && closed) {
                const long long mask = ((long long)1 << 30) - 1;
                const long long hi = row[P_HI] + (row[P_LO] >> 30), lo = row[P_LO] & mask;     // the sum = hi 2^30 + lo, 0 <= lo < 2^30
                if (hi < 0) { inverted = true; decide = DECIDE_INVERT; majority = false; }
                else if (hi == 0 && lo == 0) undecided = true;
                else majority = false;
            }
            if (majority && 2 * row[P_FLIPPED] > row[P_FACES]) decide = DECIDE_INVERT;
        }
        row[P_DECIDE] = decide;
    }
    wave_count(patch, &w.hdr[H_PATCHES]);
    wave_count(closed, &w.hdr[H_P_CLOSED]);
    wave_count(bad, &w.hdr[H_P_UNORIENTABLE]);
    wave_count(inverted, &w.hdr[H_P_INVERTED]);
    wave_count(undecided, &w.hdr[H_P_UNDECIDED]);
}

// a lane per face: a live face's fate, KEPT or KEPT_FLIPPED
__global__ __launch_bounds__(THREADS) void repair_flip_kernel(long nf, Ws w) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    bool flipped = false;
    if (f < nf && w.fate[f] == GPNERF_REPAIR_KEPT) {
        const uint32_t word = w.froot[f];
        const long long decide = w.ptab[(long)(word >> 1) * PCOLS + P_DECIDE];
        flipped = !(decide & DECIDE_UNORIENTABLE) && ((word & 1u) != (uint32_t)(decide & DECIDE_INVERT));
        if (flipped) w.fate[f] = GPNERF_REPAIR_KEPT_FLIPPED;
    }
    wave_count(flipped, &w.hdr[H_F_FLIPPED]);
}

__global__ void repair_finish_kernel(long nv, long nf, Ws w, int64_t* stats) {
    const long long* h = w.hdr;
    stats[GPNERF_REPAIR_VERTICES_OUT] = h[H_V_OUT];
    stats[GPNERF_REPAIR_FACES_OUT] = h[H_F_OUT];
    stats[GPNERF_REPAIR_VERTICES_WELDED] = h[H_WELDED];
    stats[GPNERF_REPAIR_VERTICES_UNKEYABLE] = h[H_V_UNKEYABLE];
    stats[GPNERF_REPAIR_VERTICES_UNREFERENCED] = nv - h[H_V_OUT] - h[H_WELDED] - h[H_V_UNKEYABLE];
    stats[GPNERF_REPAIR_FACES_INVALID] = h[H_F_INVALID];
    stats[GPNERF_REPAIR_FACES_UNKEYABLE] = h[H_F_UNKEYABLE];
    stats[GPNERF_REPAIR_FACES_COLLAPSED] = h[H_F_COLLAPSED];
    stats[GPNERF_REPAIR_FACES_DUPLICATE] = h[H_F_DUPLICATE];
    stats[GPNERF_REPAIR_FACES_FLIPPED] = h[H_F_FLIPPED];
    stats[GPNERF_REPAIR_EDGES_NONMANIFOLD] = h[H_E_NONMANIFOLD];
    stats[GPNERF_REPAIR_PATCHES] = h[H_PATCHES];
    stats[GPNERF_REPAIR_PATCHES_CLOSED] = h[H_P_CLOSED];
    stats[GPNERF_REPAIR_PATCHES_UNORIENTABLE] = h[H_P_UNORIENTABLE];
    stats[GPNERF_REPAIR_PATCHES_INVERTED] = h[H_P_INVERTED];
    stats[GPNERF_REPAIR_PATCHES_UNDECIDED] = h[H_P_UNDECIDED];
    w.hdr[H_STATUS] = GPNERF_REPAIR_COUNTED;
}

// ---------------------------------------------------------------- emit

// one thread: the sizes the caller brought against those counted
__global__ void repair_emit_check_kernel(Ws w, long nv, long nf, long n_out_v, long n_out_f) {
    const long long st = w.hdr[H_STATUS];
    const bool counted = w.hdr[H_MAGIC] == REPAIR_MAGIC && (st == GPNERF_REPAIR_COUNTED || st == GPNERF_REPAIR_EMITTED || st == GPNERF_REPAIR_MISMATCH);
    if (!counted) { w.hdr[H_STATUS] = GPNERF_REPAIR_NO_COUNT; return; }
    const bool same = w.hdr[H_NV] == nv && w.hdr[H_NF] == nf && w.hdr[H_V_OUT] == n_out_v && w.hdr[H_F_OUT] == n_out_f;
    w.hdr[H_STATUS] = same ? GPNERF_REPAIR_EMITTED : GPNERF_REPAIR_MISMATCH;
}

DEV bool emit_ok(const Ws& w) { return w.hdr[H_MAGIC] == REPAIR_MAGIC && w.hdr[H_STATUS] == GPNERF_REPAIR_EMITTED; }

// a lane per input vertex: vertex_map follows the representative; a kept representative goes to its new number (< VERTICES_OUT, which
// repair_emit_check_kernel found equal to the outputs' size), the three words copied as they are
__global__ __launch_bounds__(THREADS) void repair_emit_vertices_kernel(Ws w, const uint32_t* __restrict__ vertices, long nv, uint32_t* __restrict__ out_vertices,
                                                                       int32_t* __restrict__ vertex_map, int32_t* __restrict__ kept_vertices) {
    const long v = (long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= nv || !emit_ok(w)) return;
    const int32_t r = w.rep[v];
    if (vertex_map) vertex_map[v] = r >= 0 ? w.vnew[r] : -1;
    const int32_t n = w.vnew[v];
    if (n < 0 || r != (int32_t)v) return;
    if (out_vertices)
        for (int k = 0; k < 3; ++k) out_vertices[3 * (long)n + k] = vertices[3 * v + k];
    if (kept_vertices) kept_vertices[n] = (int32_t)v;
}

// a lane per input face: its fate; a live one (its corners in range, their representatives kept) goes to its new number, (a, c, b) when flipped
__global__ __launch_bounds__(THREADS) void repair_emit_faces_kernel(Ws w, const int32_t* __restrict__ faces, long nf, long nv, int32_t* __restrict__ out_faces,
                                                                    int32_t* __restrict__ face_map, uint8_t* __restrict__ face_fate, int32_t* __restrict__ face_patch) {
    const long f = (long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= nf || !emit_ok(w)) return;
    const int fate = w.fate[f];
    if (face_fate) face_fate[f] = (uint8_t)fate;
    const int32_t n = w.fnew[f];
    if (n < 0) return;
    int32_t c[3];
    for (int k = 0; k < 3; ++k) {
        const int32_t i = faces[3 * f + k];
        c[k] = i >= 0 && i < nv && w.rep[i] >= 0 ? w.vnew[w.rep[i]] : -1;
    }
    if (fate == GPNERF_REPAIR_KEPT_FLIPPED) { const int32_t t = c[1]; c[1] = c[2]; c[2] = t; }
    if (out_faces)
        for (int k = 0; k < 3; ++k) out_faces[3 * (long)n + k] = c[k];
    if (face_map) face_map[n] = (int32_t)f;
    if (face_patch) face_patch[n] = (w.hdr[H_FLAGS] & GPNERF_REPAIR_ORIENT) ? (int32_t)(w.froot[f] >> 1) : (int32_t)f;
}

}  // namespace

extern "C" {

size_t gpnerf_mesh_repair_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    return sizes_ok(n_vertices, n_faces) ? layout_of(n_vertices, n_faces).total : 0;
}

int gpnerf_mesh_repair(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, double tol, uint32_t flags,
                       void* workspace, size_t workspace_bytes, int64_t* stats, void* stream) {
    if (!workspace || !stats || !sizes_ok(n_vertices, n_faces) || (!vertices && n_vertices > 0) || (!faces && n_faces > 0)) return GPNERF_E_ARG;
    if ((flags & ~ALL_FLAGS) || ((flags & GPNERF_REPAIR_OUTWARD) && !(flags & GPNERF_REPAIR_ORIENT))) return GPNERF_E_ARG;
    if (!(tol >= 0.0) || !(tol <= 1.7976931348623157e308)) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    const Ws w = ws_of(workspace, l);
    hipStream_t st = S_(stream);
    const long nv = (long)n_vertices, nf = (long)n_faces;
    const dim3 block(THREADS), vgrid(blocks_for(nv, THREADS)), fgrid(blocks_for(nf, THREADS));
    int64_t cells = 0;                                       // the longest of the arrays the clear sweeps
    if (flags & GPNERF_REPAIR_WELD) cells = l.cap_v;
    if ((flags & GPNERF_REPAIR_DROP_DUPLICATES) && l.cap_f > cells) cells = l.cap_f;
    if ((flags & GPNERF_REPAIR_ORIENT) && l.cap_e > cells) cells = l.cap_e;
    if ((flags & GPNERF_REPAIR_ORIENT) && PCOLS * n_faces > cells) cells = PCOLS * n_faces;
    hipLaunchKernelGGL(repair_clear_kernel, dim3(sweep_blocks(cells, THREADS)), block, 0, st, w, nv, nf, flags);
    if (nv > 0) {
        if (flags & GPNERF_REPAIR_WELD) hipLaunchKernelGGL(repair_vertex_insert_kernel, vgrid, block, 0, st, vertices, nv, tol, w);
        hipLaunchKernelGGL(repair_vertex_lookup_kernel, vgrid, block, 0, st, vertices, nv, tol, flags, w);
    }
    if (nf > 0) {
        hipLaunchKernelGGL(repair_face_insert_kernel, fgrid, block, 0, st, faces, nf, nv, flags, w);
        hipLaunchKernelGGL(repair_face_lookup_kernel, fgrid, block, 0, st, faces, nf, nv, flags, w);
        if (flags & GPNERF_REPAIR_ORIENT) {
            if ((flags & GPNERF_REPAIR_OUTWARD) && nv > 0) hipLaunchKernelGGL(repair_box_kernel, dim3(sweep_blocks(nv, THREADS, 1024)), block, 0, st, vertices, nv, w);
            hipLaunchKernelGGL(repair_union_kernel, fgrid, block, 0, st, faces, nf, nv, w);
            hipLaunchKernelGGL(repair_flatten_kernel, fgrid, block, 0, st, vertices, faces, nf, nv, flags, w);
            hipLaunchKernelGGL(repair_shared_insert_kernel, fgrid, block, 0, st, faces, nf, w);
            hipLaunchKernelGGL(repair_shared_lookup_kernel, fgrid, block, 0, st, faces, nf, w);
            hipLaunchKernelGGL(repair_patch_kernel, fgrid, block, 0, st, nf, flags, w);
            hipLaunchKernelGGL(repair_flip_kernel, fgrid, block, 0, st, nf, w);
        }
        scan_launch<RepairScan, 1>(w.fnew, nf, nullptr, w.bsum, &w.hdr[H_F_OUT], nullptr, w.fnew, nullptr, st);
    }
    if (nv > 0) scan_launch<RepairScan, 1>(w.vnew, nv, nullptr, w.bsum, &w.hdr[H_V_OUT], nullptr, w.vnew, nullptr, st);   // (without a face: every mark 0, every number -1)
    hipLaunchKernelGGL(repair_finish_kernel, dim3(1), dim3(1), 0, st, nv, nf, w, stats);
    return launch_status();
}

int gpnerf_mesh_repair_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, void* workspace, size_t workspace_bytes,
                            float* out_vertices, int64_t n_out_vertices, int32_t* out_faces, int64_t n_out_faces, int32_t* vertex_map,
                            int32_t* kept_vertices, int32_t* face_map, uint8_t* face_fate, int32_t* face_patch, void* stream) {
    if (!workspace || !sizes_ok(n_vertices, n_faces) || (!vertices && n_vertices > 0) || (!faces && n_faces > 0)) return GPNERF_E_ARG;
    if (n_out_vertices < 0 || n_out_vertices > n_vertices || n_out_faces < 0 || n_out_faces > n_faces) return GPNERF_E_ARG;
    if ((!out_vertices && n_out_vertices > 0) || (!out_faces && n_out_faces > 0)) return GPNERF_E_ARG;
    const Layout l = layout_of(n_vertices, n_faces);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    const Ws w = ws_of(workspace, l);
    hipStream_t st = S_(stream);
    const long nv = (long)n_vertices, nf = (long)n_faces;
    hipLaunchKernelGGL(repair_emit_check_kernel, dim3(1), dim3(1), 0, st, w, nv, nf, (long)n_out_vertices, (long)n_out_faces);
    if (nv > 0 && (n_out_vertices > 0 || vertex_map))
        hipLaunchKernelGGL(repair_emit_vertices_kernel, dim3(blocks_for(nv, THREADS)), dim3(THREADS), 0, st, w, reinterpret_cast<const uint32_t*>(vertices), nv,
                           reinterpret_cast<uint32_t*>(out_vertices), vertex_map, kept_vertices);
    if (nf > 0 && (n_out_faces > 0 || face_fate))
        hipLaunchKernelGGL(repair_emit_faces_kernel, dim3(blocks_for(nf, THREADS)), dim3(THREADS), 0, st, w, faces, nf, nv, out_faces, face_map, face_fate, face_patch);
    return launch_status();
}

}  // extern "C"
