// gpnerf_rasterface.h -- a mesh face in a calibrated view as gpnerf_mesh_rasterize defines it (include/gpnerf_hip.h): the projection
// of a vertex and its snap to 1/256 pixel, the face's setup, the inclusive edge rule and the perspective-correct terms of a covered
// pixel.  Shared by the rasteriser (gpnerf_raster.hip: the draw and the interpolation) and the texture atlas's draw (gpnerf_atlas.hip),
// which shade the SAME pixels from the same numbers.  Included INSIDE the including file's unnamed namespace, behind gpnerf_diag.h
// (DEV) and gpnerf_tri2d.h (Mesh, Snapped, Setup, Edges, setup_face).  Device functions, small structs and one host helper: no kernel.
#ifndef GPNERF_RASTERFACE_H
#define GPNERF_RASTERFACE_H

constexpr int RASTER_VIEWS = 8;                          // the cameras of one call, at most
constexpr int SNAP_SHIFT = 8;                            // 256 sub-pixel units per pixel
constexpr double GUARD = 1048576.0;                      // 2^20 pixels

using Setup8 = Setup<SNAP_SHIFT>;

struct Cams { double cam[RASTER_VIEWS][21]; };           // K 3x3 row-major, RT 3x4 row-major: gpnerf_visual_hull's layout

// one vertex in one view: the hull's projection (float64, multiply then add, unfused), the usable test, the snap to 1/256 pixel
DEV bool project_vertex(const double* __restrict__ cam, const float* __restrict__ p, double z_near, Snapped& s) {
    const double* K = cam;
    const double* RT = cam + 9;
    const double p0 = (double)p[0], p1 = (double)p[1], p2 = (double)p[2];
    const double c0 = ((p0 * RT[0] + p1 * RT[1]) + p2 * RT[2]) + RT[3];
    const double c1 = ((p0 * RT[4] + p1 * RT[5]) + p2 * RT[6]) + RT[7];
    const double c2 = ((p0 * RT[8] + p1 * RT[9]) + p2 * RT[10]) + RT[11];
    const double h0 = (c0 * K[0] + c1 * K[1]) + c2 * K[2];
    const double h1 = (c0 * K[3] + c1 * K[4]) + c2 * K[5];
    const double h2 = (c0 * K[6] + c1 * K[7]) + c2 * K[8];
    const double x = h0 / h2, y = h1 / h2;
    // (every comparison is false for a NaN; an infinite x or y fails the guard band, an infinite z is named)
    if (!(h2 >= z_near) || !(h2 < (double)INFINITY) || !(fabs(x) <= GUARD) || !(fabs(y) <= GUARD)) return false;
    s.X = (int64_t)rint(256.0 * x);
    s.Y = (int64_t)rint(256.0 * y);
    s.z = h2;
    return true;
}

// face f in the view of `cam`: its corners projected, A and the pixel box clipped to the image
DEV FaceState raster_setup(const Mesh& m, const double* __restrict__ cam, double z_near, long f, int H, int W, Setup8& s) {
    return setup_face(m, f, W, H, [&](const float* p, Snapped& v) { return project_vertex(cam, p, z_near, v); }, s);
}

// the edge functions each multiplied by sign(A): covered iff none is negative (a pixel exactly on an edge is covered)
DEV bool covers(const Setup8& s, const Edges& e) {
    return s.A > 0 ? (e.ea >= 0 && e.eb >= 0 && e.ec >= 0) : (e.ea <= 0 && e.eb <= 0 && e.ec <= 0);
}

// perspective-correct depth terms of a covered pixel: wk = Ek / A, q = (wa / za + wb / zb) + wc / zc
struct Persp { double ta, tb, tc, q; };                 // tk = wk / zk

DEV Persp persp_of(const Setup8& s, const Edges& e) {
    const double A = (double)s.A;
    Persp p;
    p.ta = ((double)e.ea / A) / s.a.z;
    p.tb = ((double)e.eb / A) / s.b.z;
    p.tc = ((double)e.ec / A) / s.c.z;
    p.q = (p.ta + p.tb) + p.tc;
    return p;
}

void cams_of(const double* cams, int n_views, Cams& c) {
    for (int v = 0; v < RASTER_VIEWS; ++v)
        for (int e = 0; e < 21; ++e) c.cam[v][e] = v < n_views ? cams[v * 21 + e] : 0.0;
}

#endif  // GPNERF_RASTERFACE_H
