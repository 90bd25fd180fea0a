// gpnerf_raytri.h -- THE ray / triangle intersection of the library and its tie rule, shared by the two forms of gpnerf_mesh_raycast
// (every face through LDS; the faces of the cells a ray walks): both compile the same functions, so the same (ray, face) pair gives
// the same bits in either.  Included INSIDE the including file's unnamed namespace, behind <math.h>, <stdint.h>, gpnerf_diag.h (DEV)
// and gpnerf_tridist.h (V3, sub, finite3, nanf_, inff_).  Device functions and small structs only.  include/gpnerf_hip.h
// (gpnerf_mesh_raycast, THE INTERSECTION) states the definition; this is the watertight test of Woop, Benthin and Wald (Watertight
// Ray/Triangle Intersection, JCGT 2(1), 2013) in float32, unfused (the build has -ffp-contract=off).
//
// WATERTIGHT.  Write P' for a vertex's sheared (x, y) pair as computed below: two float32 numbers that depend on the ray and on that
// vertex alone, so two faces that share a vertex see the same P'.
//   1. f(P, Q) = fl(fl(Px Qy) - fl(Py Qx)) is exactly antisymmetric: f(Q, P) = fl(fl(Qx Py) - fl(Qy Px)) takes the same two
//      products (a float32 product commutes) in the other order, and fl(m2 - m1) = -fl(m1 - m2).  So the edge function of a shared
//      edge is, bit for bit, the negative in one face of what it is in the other.
//   2. A nonzero float32 f has the sign of the exact Px Qy - Py Qx: rounding is monotone, so Px Qy > Py Qx gives fl(Px Qy) >= fl(Py
//      Qx), and a float32 difference is zero only for equal operands.  Where an f is exactly 0 the three are recomputed in float64,
//      where both products are exact (24 + 24 bits) and the difference of two doubles has its exact sign.  Either way the signs tested
//      are the signs of the exact edge functions of the triangle A'B'C'.
//   3. So a face is accepted (up to det and the range of t) iff the origin of the sheared plane lies in the CLOSED exact triangle
//      A'B'C' -- edges and vertices included.  The triangles A'B'C' of the faces around an edge or a vertex tile a neighbourhood of
//      it in the sheared plane exactly as the faces do (the same P' from either side), so there is no gap between them for the
//      origin to fall into: a ray through a closed surface hits a face of it.
#ifndef GPNERF_RAYTRI_H
#define GPNERF_RAYTRI_H

constexpr int RAYCAST_NEAREST = GPNERF_RAYCAST_NEAREST, RAYCAST_ANY = GPNERF_RAYCAST_ANY;

struct Ray { V3 o, d; float tmin, tmax; };
// what THE INTERSECTION derives from the direction alone: the axes and the shear
struct RayAxes { int kx, ky, kz; float Sx, Sy, Sz; };
struct RayBest { float t; int32_t f; float wb, wc; };

DEV float pick(V3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

DEV Ray load_ray(const float* __restrict__ rays, long i) {
    const float* r = rays + 8 * i;
    return {{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, r[6], r[7]};
}

// a ray the call answers: finite origin and direction, a direction that is not zero, bounds that are not NaN and not crossed
DEV bool ray_valid(const Ray& r) {
    return finite3(r.o) && finite3(r.d) && (r.d.x != 0.f || r.d.y != 0.f || r.d.z != 0.f) && r.tmin <= r.tmax;     // (a NaN bound fails <=)
}

DEV RayAxes ray_axes(V3 d) {
    const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
    RayAxes k;
    k.kz = 0;                                            // the largest |d|, the lowest index on a tie
    if (ay > ax) k.kz = 1;
    if (az > fmaxf(ax, ay)) k.kz = 2;
    k.kx = k.kz == 2 ? 0 : k.kz + 1;
    k.ky = k.kx == 2 ? 0 : k.kx + 1;
    const float dz = pick(d, k.kz);
    if (dz < 0.f) { const int s = k.kx; k.kx = k.ky; k.ky = s; }
    k.Sx = pick(d, k.kx) / dz;
    k.Sy = pick(d, k.ky) / dz;
    k.Sz = 1.f / dz;
    return k;
}

// THE INTERSECTION.  True iff the ray hits the face with tmin <= t <= tmax; t, and the barycentric weights of b and c, are then set.
DEV bool ray_triangle(V3 o, const RayAxes& k, float tmin, float tmax, V3 a, V3 b, V3 c, float& t, float& wb, float& wc) {
    const V3 A = sub(a, o), B = sub(b, o), C = sub(c, o);
    const float Akz = pick(A, k.kz), Bkz = pick(B, k.kz), Ckz = pick(C, k.kz);
    const float Ax = pick(A, k.kx) - k.Sx * Akz, Ay = pick(A, k.ky) - k.Sy * Akz, Az = k.Sz * Akz;
    const float Bx = pick(B, k.kx) - k.Sx * Bkz, By = pick(B, k.ky) - k.Sy * Bkz, Bz = k.Sz * Bkz;
    const float Cx = pick(C, k.kx) - k.Sx * Ckz, Cy = pick(C, k.ky) - k.Sy * Ckz, Cz = k.Sz * Ckz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (U == 0.f || V == 0.f || W == 0.f) {              // on an edge or a vertex within float32: the exact signs decide
        const double Ud = (double)Cx * (double)By - (double)Cy * (double)Bx, Vd = (double)Ax * (double)Cy - (double)Ay * (double)Cx,
                     Wd = (double)Bx * (double)Ay - (double)By * (double)Ax;
        if ((Ud < 0.0 || Vd < 0.0 || Wd < 0.0) && (Ud > 0.0 || Vd > 0.0 || Wd > 0.0)) return false;
        U = (float)Ud; V = (float)Vd; W = (float)Wd;
    } else if ((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f)) {
        return false;
    }
    const float det = (U + V) + W;
    if (det == 0.f) return false;
    const float T = (U * Az + V * Bz) + W * Cz;
    const float th = T / det;
    if (!(th >= tmin && th <= tmax)) return false;        // both ends inclusive; a NaN fails
    t = th; wb = V / det; wc = W / det;
    return true;
}

// one face against one ray: the tie rule lives here (bit-equal t: the lower face index).  True iff the face was accepted.
DEV bool test_ray_face(RayBest& best, const Ray& r, const RayAxes& k, V3 a, V3 b, V3 c, int32_t f) {
    float t, wb, wc;
    if (!ray_triangle(r.o, k, r.tmin, r.tmax, a, b, c, t, wb, wc)) return false;
    if (t < best.t || (t == best.t && (best.f < 0 || f < best.f))) { best.t = t; best.f = f; best.wb = wb; best.wc = wc; }
    return true;
}

#endif  // GPNERF_RAYTRI_H
