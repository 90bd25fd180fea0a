// gpnerf_tridist.h -- THE point-to-triangle distance of the library and its tie rule, shared by the list form (one query per lane
// over a grid of the mesh's faces, gpnerf_meshdist.hip) and the lattice form (one face over the lattice points of its box,
// gpnerf_sdf.hip): both files compile the same functions, so the same (point, face) pair gives the same bits in either.  Included
// INSIDE the including file's unnamed namespace, behind <math.h>, <stdint.h> and gpnerf_diag.h (DEV).  Device functions and small
// structs only.  include/gpnerf_hip.h (gpnerf_mesh_distance) states the definition.
#ifndef GPNERF_TRIDIST_H
#define GPNERF_TRIDIST_H

struct V3 { float x, y, z; };
DEV V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
DEV float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
DEV V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
DEV V3 madd(V3 a, V3 d, float t) { return {a.x + d.x * t, a.y + d.y * t, a.z + d.z * t}; }
DEV V3 load3(const float* p, long i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
DEV bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
DEV float nanf_() { return __int_as_float(0x7fc00000); }
DEV float inff_() { return __int_as_float(0x7f800000); }

// the closest point of segment a + t e, t in [0, 1], to the origin; a zero-length segment is its point
DEV V3 closest_on_segment(V3 a, V3 e) {
    const float ee = dot(e, e);
    float t = 0.f;
    if (ee > 0.f) t = fminf(fmaxf(-dot(a, e) / ee, 0.f), 1.f);
    return madd(a, e, t);
}

// THE distance function, the one every caller uses.  a, b, c: the triangle's vertices RELATIVE TO THE QUERY (vertex - query, one
// rounding each), so the query is the origin; returns the closest point, relative to the query as well.  Ericson's regions
// (Real-Time Collision Detection 5.1.5): vertex a, vertex b, edge ab, vertex c, edge ca, edge bc, interior; an edge's parameter is
// taken as (projection on the edge) / |edge|^2, clamped, rather than from the region's two dot products, whose difference cancels
// for a small triangle far away.  A triangle whose normal is exactly zero (collinear, or all three equal), or whose barycentric
// denominator is not positive, is the nearest of its three segments.  Never NaN for finite input.
DEV V3 closest_on_triangle(V3 a, V3 b, V3 c) {
    const V3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b);
    const V3 n = cross(ab, ac);
    const float nn = dot(n, n);
    bool degenerate = !(nn > 0.f);
    if (!degenerate) {
        const float d1 = -dot(ab, a), d2 = -dot(ac, a);          // ap = -a
        if (d1 <= 0.f && d2 <= 0.f) return a;
        const float d3 = -dot(ab, b), d4 = -dot(ac, b);
        if (d3 >= 0.f && d4 <= d3) return b;
        const float vc = d1 * d4 - d3 * d2;
        if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) return closest_on_segment(a, ab);
        const float d5 = -dot(ab, c), d6 = -dot(ac, c);
        if (d6 >= 0.f && d5 <= d6) return c;
        const float vb = d5 * d2 - d1 * d6;
        if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) return closest_on_segment(a, ac);
        const float va = d3 * d6 - d5 * d4;
        if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) return closest_on_segment(b, bc);
        const float den = (va + vb) + vc;
        if (den > 0.f) {
            const float v = vb / den, w = vc / den;
            return madd(madd(a, ab, v), ac, w);
        }
        degenerate = true;
    }
    const V3 p0 = closest_on_segment(a, ab), p1 = closest_on_segment(b, bc), p2 = closest_on_segment(a, ac);
    const float q0 = dot(p0, p0), q1 = dot(p1, p1), q2 = dot(p2, p2);
    V3 best = p0;
    float q = q0;
    if (q1 < q) { best = p1; q = q1; }
    if (q2 < q) { best = p2; }
    return best;
}

struct Best { float d; int32_t f; V3 cp; };

// one face against one query: the tie rule lives here (bit-equal distance: the lower face index)
DEV void test_face(Best& best, V3 p, V3 a, V3 b, V3 c, int32_t f) {
    const V3 cp = closest_on_triangle(sub(a, p), sub(b, p), sub(c, p));
    const float d = sqrtf(dot(cp, cp));
    if (d < best.d || (d == best.d && f < best.f)) { best.d = d; best.f = f; best.cp = cp; }
}

DEV bool face_valid(const float* __restrict__ vertices, int64_t n_vertices, const int32_t* __restrict__ faces, long f, V3& a, V3& b, V3& c) {
    const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) return false;
    a = load3(vertices, i0); b = load3(vertices, i1); c = load3(vertices, i2);
    return finite3(a) && finite3(b) && finite3(c);
}

#endif  // GPNERF_TRIDIST_H
