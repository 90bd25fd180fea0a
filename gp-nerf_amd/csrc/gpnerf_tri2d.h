// gpnerf_tri2d.h -- the exact two-tier walk of a mesh's triangles over a 2-D integer grid, shared by the rasteriser (the grid is a
// view's pixels, gpnerf_raster.hip) and the voxeliser (the grid is the lattice's columns, gpnerf_voxelize.hip).  Included INSIDE the
// including file's unnamed namespace, behind gpnerf_diag.h (DEV) and gpnerf_util.h (wave_count, stat_add).  Device functions and
// small structs only: the kernels stay in their files under their names, and bring the vertex mapping, the rule for a grid point
// on an edge and what a hit does.
//
// Exactness.  A vertex is snapped to 1 / 2^SHIFT of a grid step (8: the rasteriser's 1/256 pixel, 12: the voxeliser's 1/4096 step),
// so the edge functions are int64 products of snapped differences: no rounding, and the same value whichever way a grid point is
// reached -- by edges_at() or by adding the per-step increments, which are exact because the functions are linear.
//
// Two tiers.  The first kernel gives every face ONE lane, which walks the face's clipped box with three additions per grid point
// (lane_walk).  A face whose box holds more than LARGE_BOX points would hold its wavefront's other 63 lanes up: it is appended to
// a list instead (large_append: one counter add per wavefront), and a second launch of fixed grid gives each listed face a whole
// wavefront, 64 points of the box per step (wave_walk).
#ifndef GPNERF_TRI2D_H
#define GPNERF_TRI2D_H

constexpr int LARGE_BOX = 256;                           // grid points in a clipped box above which a face goes to the list (chosen, not tuned)
constexpr int LARGE_BLOCKS = 1024;                       // the list reader's fixed grid: 4096 wavefronts (chosen, not tuned)

struct Mesh {
    const float* vertices; const int32_t* faces;
    long n_vertices, n_faces;
};

struct Snapped { int64_t X, Y; double z; };              // X, Y in 1 / 2^SHIFT of a grid step; z as the including file means it
DEV int64_t lo_of(int64_t a, int64_t b) { return a < b ? a : b; }
DEV int64_t hi_of(int64_t a, int64_t b) { return a > b ? a : b; }

// the values of the first three statistics of both callers: a face counts under its state
enum FaceState { FACE_OK = 0, FACE_BAD_VERTEX = 1, FACE_NO_AREA = 2 };

// the three edge functions at a grid point, or their change over one step
struct Edges {
    int64_t ea, eb, ec;
    DEV void operator+=(const Edges& d) { ea += d.ea; eb += d.eb; ec += d.ec; }
};

enum Inner { INNER_I = 0, INNER_J = 1 };                 // the axis a walk steps through fastest

template <int SHIFT>
struct Setup {
    static constexpr int64_t SNAP = (int64_t)1 << SHIFT; // units per grid step
    Snapped a, b, c;
    int64_t A;                                           // twice the signed area, in units^2
    int i0, i1, j0, j1;                                  // the clipped box, inclusive; empty when i1 < i0 or j1 < j0

    // A from a, b, c, and their box clipped to ni x nj grid points; false, and no box, when the face has no area
    DEV bool fill(int ni, int nj) {
        A = (b.X - a.X) * (c.Y - a.Y) - (b.Y - a.Y) * (c.X - a.X);
        if (A == 0) return false;
        const int64_t x0 = lo_of(a.X, lo_of(b.X, c.X)), x1 = hi_of(a.X, hi_of(b.X, c.X));
        const int64_t y0 = lo_of(a.Y, lo_of(b.Y, c.Y)), y1 = hi_of(a.Y, hi_of(b.Y, c.Y));
        // grid points are the multiples of SNAP: ceil(x0 / SNAP) .. floor(x1 / SNAP), by arithmetic shifts
        i0 = (int)hi_of(0, (x0 + (SNAP - 1)) >> SHIFT); i1 = (int)lo_of(ni - 1, x1 >> SHIFT);
        j0 = (int)hi_of(0, (y0 + (SNAP - 1)) >> SHIFT); j1 = (int)lo_of(nj - 1, y1 >> SHIFT);
        return true;
    }
    DEV long box() const { return i1 >= i0 && j1 >= j0 ? (long)(i1 - i0 + 1) * (j1 - j0 + 1) : 0; }

    // each function is positive on the inner side when A > 0 and negative when A < 0; zero exactly on its edge
    DEV Edges edges_at(int i, int j) const {
        const int64_t px = SNAP * i, py = SNAP * j;
        Edges e;
        e.ea = (c.X - b.X) * (py - b.Y) - (c.Y - b.Y) * (px - b.X);
        e.eb = (a.X - c.X) * (py - c.Y) - (a.Y - c.Y) * (px - c.X);
        e.ec = (b.X - a.X) * (py - a.Y) - (b.Y - a.Y) * (px - a.X);
        return e;
    }
    // the next i adds -SNAP dY, the next j adds SNAP dX (int64: exact)
    DEV Edges step_i() const { return {-SNAP * (c.Y - b.Y), -SNAP * (a.Y - c.Y), -SNAP * (b.Y - a.Y)}; }
    DEV Edges step_j() const { return {SNAP * (c.X - b.X), SNAP * (a.X - c.X), SNAP * (b.X - a.X)}; }
};

// face f's corners through map(p, snapped) -> usable, then A and the box.  The index check: three indices, each >= 0 and < n_vertices.
template <class Map, int SHIFT>
DEV FaceState setup_face(const Mesh& m, long f, int ni, int nj, Map map, Setup<SHIFT>& s) {
    const int32_t ia = m.faces[3 * f], ib = m.faces[3 * f + 1], ic = m.faces[3 * f + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= m.n_vertices || ib >= m.n_vertices || ic >= m.n_vertices) return FACE_BAD_VERTEX;
    const bool ua = map(m.vertices + 3 * (long)ia, s.a);
    const bool ub = map(m.vertices + 3 * (long)ib, s.b);
    const bool uc = map(m.vertices + 3 * (long)ic, s.c);
    if (!(ua && ub && uc)) return FACE_BAD_VERTEX;
    return s.fill(ni, nj) ? FACE_OK : FACE_NO_AREA;
}

// row[state] += the wavefront's live faces of that state: one add per wavefront and counter, and none for a zero
DEV void count_states(bool live, FaceState st, long long* row) {
    const int ok = wave_count(live && st == FACE_OK), bad = wave_count(live && st == FACE_BAD_VERTEX);
    const int flat = wave_count(live && st == FACE_NO_AREA);
    if ((threadIdx.x & 63) == 0) {
        stat_add(row, FACE_OK, ok);
        stat_add(row, FACE_BAD_VERTEX, bad);
        stat_add(row, FACE_NO_AREA, flat);
    }
}

// The large tier: the wavefront's large lanes take consecutive places behind ONE add of their number.  Returns this lane's place
// in the list, or -1 when the lane is not large (or the place lies beyond `cap`, which cannot be: an entry is appended once).
DEV long long large_append(bool large, unsigned long long* list_len, unsigned long long cap) {
    const unsigned long long mask = __ballot(large);
    if (!mask) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((unsigned long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(list_len, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader);
    const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
    return large && at < cap ? (long long)at : -1;
}

// one lane, the whole box: visit(i, j, edges) at every grid point, the edge functions by three additions per point.  (A visitor
// takes the Edges BY VALUE: through a reference the compiler kept a branch per edge test where it now selects.)
template <Inner INNER, int SHIFT, class Visit>
DEV void lane_walk(const Setup<SHIFT>& s, const Visit& visit) {
    const Edges inner = INNER == INNER_I ? s.step_i() : s.step_j(), outer = INNER == INNER_I ? s.step_j() : s.step_i();
    const int in0 = INNER == INNER_I ? s.i0 : s.j0, in1 = INNER == INNER_I ? s.i1 : s.j1;
    const int out0 = INNER == INNER_I ? s.j0 : s.i0, out1 = INNER == INNER_I ? s.j1 : s.i1;
    Edges row = s.edges_at(s.i0, s.j0);
    for (int o = out0; o <= out1; ++o) {
        Edges e = row;
        for (int n = in0; n <= in1; ++n) {
            if (INNER == INNER_I) visit(n, o, e); else visit(o, n, e);
            e += inner;
        }
        row += outer;
    }
}

// one wavefront, a non-empty box: lane `lane` visits the points k = lane, lane + 64, ... of the box, k split by the inner axis's extent
template <Inner INNER, int SHIFT, class Visit>
DEV void wave_walk(const Setup<SHIFT>& s, int lane, const Visit& visit) {
    const int in0 = INNER == INNER_I ? s.i0 : s.j0, out0 = INNER == INNER_I ? s.j0 : s.i0;
    // (unsigned: the extents are at least 1 here, and the division of a long costs less when the compiler need not look at signs)
    const unsigned long bw = (unsigned)((INNER == INNER_I ? s.i1 : s.j1) - in0) + 1u;
    const unsigned long box = bw * ((unsigned)((INNER == INNER_I ? s.j1 : s.i1) - out0) + 1u);
    for (unsigned long k = (unsigned long)lane; k < box; k += 64) {
        const int o = out0 + (int)(k / bw), n = in0 + (int)(k % bw);
        const int i = INNER == INNER_I ? n : o, j = INNER == INNER_I ? o : n;
        const Edges e = s.edges_at(i, j);
        visit(i, j, e);
    }
}

#endif  // GPNERF_TRI2D_H
