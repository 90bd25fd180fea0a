// gpnerf_align.hip -- registering a mesh onto a scan on gfx950: the weighted least-squares rigid / similarity fit of given pairs
// (Horn's quaternion form, solved by cyclic Jacobi), the transform of a point list by the slot's matrix, and one trimmed
// point-to-plane Gauss-Newton step on the correspondences gpnerf_mesh_distance wrote.  include/gpnerf_hip.h states the definitions,
// the summation order and the slot; tests/align_cases.py restates them in numpy, operation for operation.
//
// Kernel launches only, on the caller's stream; nothing allocated, nothing waited for; every launch sized from constants (the sums
// always run on ALIGN_BLOCKS workgroups); every data-dependent decision (few pairs, a singular system) is taken on the device and
// leaves a status in the slot.  No atomics at all: a workgroup writes its own row of partial sums, and a later launch folds the rows.
//
// All arithmetic is double, unfused (the Makefile's -ffp-contract=off), from the float32 inputs converted exactly; every sum has ONE
// association: pair i belongs to thread i % 256 of workgroup (i / 256) % 64, a thread adds its pairs in ascending order onto zero,
// 256 partials fold by the halving tree x[t] += x[t + s], s = 128 .. 1 (distance_stats_kernel's tree), the 64 rows by the same tree
// from s = 32.  A pair that is skipped or trimmed adds nothing, which is adding exact zeros: an accumulator that starts at +0 never
// becomes -0.  The counts are integers (any association gives the same sums).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // S_, launch_status, blocks_for, wave_sum

constexpr int THREADS = GPNERF_ALIGN_THREADS, BLOCKS = GPNERF_ALIGN_BLOCKS;
constexpr int K_MAX = 29;                                // the widest row: the plane step's 21 + 6 + 1 + 1
constexpr int K_FIT1 = 7, K_FIT2 = 11, K_STEP = 29;
constexpr int N_COUNTS = 4;                              // used, skipped, trimmed, (spare)
constexpr int64_t MAX_PAIRS = (int64_t)INT32_MAX * THREADS;
constexpr int POINT_THREADS = 256;

static_assert(GPNERF_ALIGN_WS_ROWS + BLOCKS * K_MAX == GPNERF_ALIGN_WS_COUNT_ROWS, "the header's workspace layout");
static_assert(GPNERF_ALIGN_WS_COUNT_ROWS + BLOCKS * N_COUNTS == GPNERF_ALIGN_WS_DOUBLES, "the header's workspace layout");
static_assert(sizeof(double) * K_MAX * THREADS <= 60 * 1024, "the fold's LDS stays under the static limit");

struct Ws { double* d; long long* counts; double* rows; long long* count_rows; };

Ws ws_of(void* workspace) {
    Ws w;
    w.d = static_cast<double*>(workspace);
    w.counts = reinterpret_cast<long long*>(w.d + GPNERF_ALIGN_WS_COUNTS);
    w.rows = w.d + GPNERF_ALIGN_WS_ROWS;
    w.count_rows = reinterpret_cast<long long*>(w.d + GPNERF_ALIGN_WS_COUNT_ROWS);
    return w;
}

struct D3 { double x, y, z; };
DEV D3 load3d(const float* p, long i) { return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]}; }
DEV bool finite3(D3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
DEV D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
DEV double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
DEV D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
DEV double nan_() { return __longlong_as_double(0x7ff8000000000000ll); }

// the workgroup's K partial sums and its counts, written to its row: the halving tree over the 256 threads
template <int K>
DEV void block_fold(const double (&acc)[K], const long long (&cnt)[N_COUNTS], double* s, Ws w) {
    __shared__ long long s_cnt[N_COUNTS][THREADS / 64];
    const int t = threadIdx.x;
    for (int k = 0; k < K; ++k) s[k * THREADS + t] = acc[k];
    for (int k = 0; k < N_COUNTS; ++k) {
        const long long c = wave_sum(cnt[k]);
        if ((t & 63) == 0) s_cnt[k][t >> 6] = c;
    }
    __syncthreads();
    for (int st = THREADS / 2; st > 0; st >>= 1) {
        if (t < st)
            for (int k = 0; k < K; ++k) s[k * THREADS + t] += s[k * THREADS + t + st];
        __syncthreads();
    }
    if (t < K) w.rows[(long)blockIdx.x * K_MAX + t] = s[t * THREADS];
    if (t < N_COUNTS) {
        long long c = 0;
        for (int j = 0; j < THREADS / 64; ++j) c += s_cnt[t][j];
        w.count_rows[(long)blockIdx.x * N_COUNTS + t] = c;
    }
}

// the 64 rows' K sums, by the same tree from s = 32, left in out[0 .. K); one workgroup of BLOCKS threads, every thread must call.
// s: LDS, K * BLOCKS doubles.  Behind the call every thread may read out[] (a __syncthreads ends it).
template <int K>
DEV void rows_fold(Ws w, double* s, double* out, long long* counts_out) {
    const int b = threadIdx.x;
    for (int k = 0; k < K; ++k) s[k * BLOCKS + b] = w.rows[(long)b * K_MAX + k];
    __syncthreads();
    for (int st = BLOCKS / 2; st > 0; st >>= 1) {
        if (b < st)
            for (int k = 0; k < K; ++k) s[k * BLOCKS + b] += s[k * BLOCKS + b + st];
        __syncthreads();
    }
    if (b < K) out[b] = s[b * BLOCKS];
    if (counts_out && b < N_COUNTS) {
        long long c = 0;
        for (int j = 0; j < BLOCKS; ++j) c += w.count_rows[(long)j * N_COUNTS + b];
        counts_out[b] = c;
    }
    __syncthreads();
}

// a pair of the closed-form fit: both points finite, the weight (1 without a list) finite and positive
DEV bool fit_pair(const float* __restrict__ src, const float* __restrict__ dst, const float* __restrict__ weights, long i, D3& a, D3& b,
                  double& wt) {
    a = load3d(src, i);
    b = load3d(dst, i);
    wt = weights ? (double)weights[i] : 1.0;
    return finite3(a) && finite3(b) && isfinite(wt) && wt > 0.0;
}

// pass 1: W, sum w src, sum w dst; the counts
__global__ __launch_bounds__(THREADS) void fit_sums1_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                            const float* __restrict__ weights, long n, Ws w) {
    __shared__ double s[K_FIT1 * THREADS];
    double acc[K_FIT1] = {};
    long long cnt[N_COUNTS] = {};
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long)BLOCKS * THREADS) {
        D3 a, b;
        double wt;
        if (!fit_pair(src, dst, weights, i, a, b, wt)) { ++cnt[1]; continue; }
        ++cnt[0];
        acc[0] += wt;
        acc[1] += wt * a.x; acc[2] += wt * a.y; acc[3] += wt * a.z;
        acc[4] += wt * b.x; acc[5] += wt * b.y; acc[6] += wt * b.z;
    }
    block_fold<K_FIT1>(acc, cnt, s, w);
}

// one workgroup: pass 1's rows folded, the centroids (zero when nothing was used)
__global__ __launch_bounds__(BLOCKS) void fit_centroids_kernel(Ws w) {
    __shared__ double s[K_FIT1 * BLOCKS];
    rows_fold<K_FIT1>(w, s, w.d + GPNERF_ALIGN_WS_SUMS1, w.counts);
    if (threadIdx.x != 0) return;
    const double* m = w.d + GPNERF_ALIGN_WS_SUMS1;
    const bool any = w.counts[0] > 0;
    for (int k = 0; k < 6; ++k) w.d[GPNERF_ALIGN_WS_CENTROIDS + k] = any ? m[1 + k] / m[0] : 0.0;
}

// pass 2, about the centroids: S = sum w a b^T (row-major), sum w |a|^2, and sum w |dst - src|^2 of the pairs as given
__global__ __launch_bounds__(THREADS) void fit_sums2_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                            const float* __restrict__ weights, long n, Ws w) {
    __shared__ double s[K_FIT2 * THREADS];
    const double* c = w.d + GPNERF_ALIGN_WS_CENTROIDS;
    const D3 cs = {c[0], c[1], c[2]}, cd = {c[3], c[4], c[5]};
    double acc[K_FIT2] = {};
    const long long cnt[N_COUNTS] = {};
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long)BLOCKS * THREADS) {
        D3 p, q;
        double wt;
        if (!fit_pair(src, dst, weights, i, p, q, wt)) continue;
        const D3 a = sub(p, cs), b = sub(q, cd), e = sub(q, p);
        const double wa[3] = {wt * a.x, wt * a.y, wt * a.z}, bb[3] = {b.x, b.y, b.z};
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) acc[3 * r + k] += wa[r] * bb[k];
        acc[9] += wt * dot(a, a);
        acc[10] += wt * dot(e, e);
    }
    block_fold<K_FIT2>(acc, cnt, s, w);
}

// (w, x, y, z), unit -> R, row-major
DEV void quat_to_R(const double* q, double* R) {
    const double ww = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = ww * x, wy = ww * y, wz = ww * z;
    R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
    R[3] = 2.0 * (xy + wz);       R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
    R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = 1.0 - 2.0 * (xx + yy);
}

// cyclic Jacobi on a symmetric 4 x 4: 8 sweeps, the pairs (p, q), p < q, in row-major order; V's columns become the eigenvectors
DEV void jacobi4(double (&A)[4][4], double (&V)[4][4]) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 8; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double den = fabs(theta) + sqrt(theta * theta + 1.0);
                const double t = theta < 0.0 ? -1.0 / den : 1.0 / den;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {            // A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {            // J^T (A J)
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                A[p][q] = 0.0;
                A[q][p] = 0.0;
                for (int k = 0; k < 4; ++k) {            // V J
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
}

DEV void write_identity(double* slot) {
    for (int k = 0; k < 12; ++k) slot[GPNERF_XFORM_M + k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
    slot[GPNERF_XFORM_SCALE] = 1.0;
}

// one workgroup: pass 2's rows folded, then thread 0 solves
__global__ __launch_bounds__(BLOCKS) void fit_solve_kernel(Ws w, int with_scale, double* slot) {
    __shared__ double s[K_FIT2 * BLOCKS];
    rows_fold<K_FIT2>(w, s, w.d + GPNERF_ALIGN_WS_SUMS2, nullptr);
    if (threadIdx.x != 0) return;
    const double* S = w.d + GPNERF_ALIGN_WS_SUMS2;
    const double saa = S[9], see = S[10], W = w.d[GPNERF_ALIGN_WS_SUMS1];
    const double* c = w.d + GPNERF_ALIGN_WS_CENTROIDS;
    const long long used = w.counts[0], skipped = w.counts[1];
    int status = GPNERF_ALIGN_OK;
    double M[12], scale = 1.0;
    if (used < 3) status = GPNERF_ALIGN_FEW;
    else if (!(saa > 0.0) || !isfinite(saa)) status = GPNERF_ALIGN_SINGULAR;
    else {
        double A[4][4], V[4][4];
        A[0][0] = (S[0] + S[4]) + S[8];
        A[1][1] = (S[0] - S[4]) - S[8];
        A[2][2] = (S[4] - S[0]) - S[8];
        A[3][3] = (S[8] - S[0]) - S[4];
        A[0][1] = A[1][0] = S[5] - S[7];
        A[0][2] = A[2][0] = S[6] - S[2];
        A[0][3] = A[3][0] = S[1] - S[3];
        A[1][2] = A[2][1] = S[1] + S[3];
        A[1][3] = A[3][1] = S[6] + S[2];
        A[2][3] = A[3][2] = S[5] + S[7];
        jacobi4(A, V);
        int best = 0;
        for (int j = 1; j < 4; ++j)
            if (A[j][j] > A[best][best]) best = j;
        if (A[0][0] == A[1][1] && A[1][1] == A[2][2] && A[2][2] == A[3][3]) status = GPNERF_ALIGN_SINGULAR;
        else {
            double q[4] = {V[0][best], V[1][best], V[2][best], V[3][best]};
            const double len = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
            for (int k = 0; k < 4; ++k) q[k] = q[k] / len;
            if (q[0] < 0.0)
                for (int k = 0; k < 4; ++k) q[k] = -q[k];
            double R[9];
            quat_to_R(q, R);
            if (with_scale) {
                double num = 0.0;
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) num += R[3 * i + j] * S[3 * j + i];
                scale = num / saa;
            }
            bool ok = isfinite(scale) && scale > 0.0;
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) M[4 * i + j] = scale * R[3 * i + j];
                M[4 * i + 3] = c[3 + i] - scale * ((R[3 * i] * c[0] + R[3 * i + 1] * c[1]) + R[3 * i + 2] * c[2]);
            }
            for (int k = 0; k < 12; ++k) ok = ok && isfinite(M[k]);
            if (!ok) status = GPNERF_ALIGN_SINGULAR;
        }
    }
    if (status == GPNERF_ALIGN_OK) {
        for (int k = 0; k < 12; ++k) slot[GPNERF_XFORM_M + k] = M[k];
        slot[GPNERF_XFORM_SCALE] = scale;
    } else {
        write_identity(slot);                            // (the call writes the slot absolutely: a fit that fails is the identity)
    }
    slot[GPNERF_XFORM_STATUS] = (double)status;
    slot[GPNERF_XFORM_USED] = (double)used;
    slot[GPNERF_XFORM_SKIPPED] = (double)skipped;
    slot[GPNERF_XFORM_TRIMMED] = 0.0;
    slot[GPNERF_XFORM_WSUM] = W;
    slot[GPNERF_XFORM_RMS] = used > 0 ? sqrt(see / W) : nan_();
    for (int k = 0; k < 3; ++k) slot[GPNERF_XFORM_PIVOT + k] = c[k];
    for (int k = GPNERF_XFORM_PIVOT + 3; k < GPNERF_XFORM_DOUBLES; ++k) slot[k] = 0.0;
}

struct Init { double m[12]; double scale; };

// one workgroup: the point sums folded (fit_sums1_kernel with src = dst = points, no weights), the slot initialised
__global__ __launch_bounds__(BLOCKS) void init_kernel(Ws w, Init init, double* slot) {
    __shared__ double s[K_FIT1 * BLOCKS];
    rows_fold<K_FIT1>(w, s, w.d + GPNERF_ALIGN_WS_SUMS1, w.counts);
    if (threadIdx.x != 0) return;
    const double* m = w.d + GPNERF_ALIGN_WS_SUMS1;
    const long long used = w.counts[0];
    for (int k = 0; k < 12; ++k) slot[GPNERF_XFORM_M + k] = init.m[k];
    slot[GPNERF_XFORM_SCALE] = init.scale;
    slot[GPNERF_XFORM_STATUS] = (double)GPNERF_ALIGN_OK;
    slot[GPNERF_XFORM_USED] = (double)used;
    slot[GPNERF_XFORM_SKIPPED] = (double)w.counts[1];
    slot[GPNERF_XFORM_TRIMMED] = 0.0;
    slot[GPNERF_XFORM_WSUM] = m[0];
    slot[GPNERF_XFORM_RMS] = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double ck = used > 0 ? m[1 + k] / m[0] : 0.0;
        slot[GPNERF_XFORM_PIVOT + k] = ck;
        w.d[GPNERF_ALIGN_WS_CENTROIDS + k] = ck;
        w.d[GPNERF_ALIGN_WS_CENTROIDS + 3 + k] = ck;
    }
    for (int k = GPNERF_XFORM_PIVOT + 3; k < GPNERF_XFORM_DOUBLES; ++k) slot[k] = 0.0;
}

// out = float32(M p), each coordinate ((m0 x + m1 y) + m2 z) + m3 in double; vectors: M's 3 x 3 / SCALE, no translation
__global__ __launch_bounds__(POINT_THREADS) void transform_kernel(const float* points, long n, const double* __restrict__ slot, int vectors,
                                                                  float* out) {
    const long i = (long)blockIdx.x * POINT_THREADS + threadIdx.x;
    if (i >= n) return;
    const D3 p = load3d(points, i);                      // (read before the write: in place is allowed)
    float r[3];
    const double scale = slot[GPNERF_XFORM_SCALE];
    for (int k = 0; k < 3; ++k) {
        const double* m = slot + GPNERF_XFORM_M + 4 * k;
        double v;
        if (vectors) v = ((m[0] / scale) * p.x + (m[1] / scale) * p.y) + (m[2] / scale) * p.z;
        else v = ((m[0] * p.x + m[1] * p.y) + m[2] * p.z) + m[3];
        r[k] = (float)v;
    }
    const bool ok = finite3(p);
    for (int k = 0; k < 3; ++k) out[3 * i + k] = ok ? r[k] : __int_as_float(0x7fc00000);
}

DEV void pivot_image(const double* __restrict__ slot, double* cp) {
    const double* piv = slot + GPNERF_XFORM_PIVOT;
    for (int k = 0; k < 3; ++k) {
        const double* m = slot + GPNERF_XFORM_M + 4 * k;
        cp[k] = ((m[0] * piv[0] + m[1] * piv[1]) + m[2] * piv[2]) + m[3];
    }
}

// the plane step's sums: the 21 entries of J J^T on and above the diagonal (row-major), the 6 of J r, r^2, and the pairs' count as W
__global__ __launch_bounds__(THREADS) void step_sums_kernel(const float* __restrict__ cur, const float* __restrict__ closest,
                                                            const int32_t* __restrict__ face, const float* __restrict__ dist, long n,
                                                            const float* __restrict__ vertices, int64_t n_vertices,
                                                            const int32_t* __restrict__ faces, int64_t n_faces, float max_dist,
                                                            const double* __restrict__ slot, Ws w) {
    __shared__ double s[K_STEP * THREADS];
    double cp[3];
    pivot_image(slot, cp);
    double acc[K_STEP] = {};
    long long cnt[N_COUNTS] = {};
    for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < n; i += (long)BLOCKS * THREADS) {
        const D3 p = load3d(cur, i);
        const float d = dist[i];
        if (d != d || !finite3(p)) { ++cnt[1]; continue; }
        if (d > max_dist) { ++cnt[2]; continue; }
        const int32_t f = face[i];
        const D3 q = load3d(closest, i);
        if (f < 0 || f >= n_faces || !isfinite(d) || !finite3(q)) { ++cnt[1]; continue; }
        const int32_t i0 = faces[3 * (long)f], i1 = faces[3 * (long)f + 1], i2 = faces[3 * (long)f + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) { ++cnt[1]; continue; }
        const D3 a = load3d(vertices, i0), b = load3d(vertices, i1), c = load3d(vertices, i2);
        if (!finite3(a) || !finite3(b) || !finite3(c)) { ++cnt[1]; continue; }
        const D3 nn = cross(sub(b, a), sub(c, a));
        const double len = sqrt(dot(nn, nn));
        if (!(len > 0.0) || !isfinite(len)) { ++cnt[1]; continue; }
        ++cnt[0];
        const D3 nf = {nn.x / len, nn.y / len, nn.z / len};
        const D3 rel = {p.x - cp[0], p.y - cp[1], p.z - cp[2]};
        const D3 m = cross(rel, nf);
        const double J[6] = {m.x, m.y, m.z, nf.x, nf.y, nf.z};
        const double r = dot(sub(q, p), nf);
        int at = 0;
        for (int u = 0; u < 6; ++u)
            for (int v = u; v < 6; ++v) acc[at++] += J[u] * J[v];
        for (int u = 0; u < 6; ++u) acc[21 + u] += J[u] * r;
        acc[27] += r * r;
        acc[28] += 1.0;
    }
    block_fold<K_STEP>(acc, cnt, s, w);
}

// one workgroup: the rows folded; thread 0 solves the 6 x 6 system by Cholesky and composes the step onto M
__global__ __launch_bounds__(BLOCKS) void step_solve_kernel(Ws w, double* slot, double* history_row) {
    __shared__ double s[K_STEP * BLOCKS];
    rows_fold<K_STEP>(w, s, w.d + GPNERF_ALIGN_WS_STEP, w.counts);
    if (threadIdx.x != 0) return;
    const double* sums = w.d + GPNERF_ALIGN_WS_STEP;
    const long long used = w.counts[0], skipped = w.counts[1], trimmed = w.counts[2];
    int status = used < 6 ? GPNERF_ALIGN_FEW : GPNERF_ALIGN_OK;
    double Mn[12];
    if (status == GPNERF_ALIGN_OK) {
        double A[6][6], Lm[6][6], g[6], y[6], x[6];
        int at = 0;
        for (int u = 0; u < 6; ++u)
            for (int v = u; v < 6; ++v) { A[u][v] = sums[at]; A[v][u] = sums[at]; ++at; }
        for (int u = 0; u < 6; ++u) g[u] = sums[21 + u];
        for (int j = 0; j < 6 && status == GPNERF_ALIGN_OK; ++j) {
            double dj = A[j][j];
            for (int k = 0; k < j; ++k) dj = dj - Lm[j][k] * Lm[j][k];
            if (!(dj > 9.313225746154785e-10 * A[j][j])) { status = GPNERF_ALIGN_SINGULAR; break; }      // 2^-30
            Lm[j][j] = sqrt(dj);
            for (int i = j + 1; i < 6; ++i) {
                double v = A[i][j];
                for (int k = 0; k < j; ++k) v = v - Lm[i][k] * Lm[j][k];
                Lm[i][j] = v / Lm[j][j];
            }
        }
        if (status == GPNERF_ALIGN_OK) {
            for (int i = 0; i < 6; ++i) {
                double v = g[i];
                for (int k = 0; k < i; ++k) v = v - Lm[i][k] * y[k];
                y[i] = v / Lm[i][i];
            }
            for (int i = 5; i >= 0; --i) {
                double v = y[i];
                for (int k = i + 1; k < 6; ++k) v = v - Lm[k][i] * x[k];
                x[i] = v / Lm[i][i];
            }
            // the rotation of the update without trigonometry (Cayley): q = (1, omega / 2), normalised
            const double h[3] = {x[0] / 2.0, x[1] / 2.0, x[2] / 2.0};
            const double inv = 1.0 / sqrt(1.0 + ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]));
            const double q[4] = {inv, h[0] * inv, h[1] * inv, h[2] * inv};
            double R[9], cp[3], ts[3];
            quat_to_R(q, R);
            pivot_image(slot, cp);
            for (int i = 0; i < 3; ++i) ts[i] = (cp[i] + x[3 + i]) - ((R[3 * i] * cp[0] + R[3 * i + 1] * cp[1]) + R[3 * i + 2] * cp[2]);
            const double* M = slot + GPNERF_XFORM_M;
            bool ok = true;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 4; ++j) {
                    double v = (R[3 * i] * M[j] + R[3 * i + 1] * M[4 + j]) + R[3 * i + 2] * M[8 + j];
                    if (j == 3) v = v + ts[i];
                    Mn[4 * i + j] = v;
                    ok = ok && isfinite(v);
                }
            if (!ok) status = GPNERF_ALIGN_SINGULAR;
        }
    }
    if (status == GPNERF_ALIGN_OK)
        for (int k = 0; k < 12; ++k) slot[GPNERF_XFORM_M + k] = Mn[k];
    const double rms = used > 0 ? sqrt(sums[27] / sums[28]) : nan_();
    slot[GPNERF_XFORM_STATUS] = (double)status;
    slot[GPNERF_XFORM_USED] = (double)used;
    slot[GPNERF_XFORM_SKIPPED] = (double)skipped;
    slot[GPNERF_XFORM_TRIMMED] = (double)trimmed;
    slot[GPNERF_XFORM_WSUM] = sums[28];
    slot[GPNERF_XFORM_RMS] = rms;
    if (history_row) {
        history_row[0] = rms;
        history_row[1] = (double)used;
        history_row[2] = (double)trimmed;
        history_row[3] = (double)status;
    }
}

bool ws_ok(const void* ws, size_t bytes) { return ws && bytes >= sizeof(double) * GPNERF_ALIGN_WS_DOUBLES; }

}  // namespace

extern "C" {

size_t gpnerf_align_workspace_bytes(void) { return sizeof(double) * GPNERF_ALIGN_WS_DOUBLES; }

int gpnerf_rigid_fit(const float* src, const float* dst, const float* weights, int64_t n, int32_t with_scale, double* slot, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (!slot || n < 0 || n > MAX_PAIRS || !ws_ok(workspace, workspace_bytes) || !src || !dst) return GPNERF_E_ARG;
    const Ws w = ws_of(workspace);
    hipLaunchKernelGGL(fit_sums1_kernel, dim3(BLOCKS), dim3(THREADS), 0, S_(stream), src, dst, weights, (long)n, w);
    hipLaunchKernelGGL(fit_centroids_kernel, dim3(1), dim3(BLOCKS), 0, S_(stream), w);
    hipLaunchKernelGGL(fit_sums2_kernel, dim3(BLOCKS), dim3(THREADS), 0, S_(stream), src, dst, weights, (long)n, w);
    hipLaunchKernelGGL(fit_solve_kernel, dim3(1), dim3(BLOCKS), 0, S_(stream), w, (int)(with_scale != 0), slot);
    return launch_status();
}

int gpnerf_align_init(const float* points, int64_t n, const double* init_matrix12, double* slot, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (!slot || n < 0 || n > MAX_PAIRS || !ws_ok(workspace, workspace_bytes) || !points) return GPNERF_E_ARG;
    Init init = {{1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0}, 1.0};
    if (init_matrix12) {
        for (int k = 0; k < 12; ++k) {
            if (!isfinite(init_matrix12[k])) return GPNERF_E_ARG;
            init.m[k] = init_matrix12[k];
        }
        init.scale = sqrt((init.m[0] * init.m[0] + init.m[1] * init.m[1]) + init.m[2] * init.m[2]);
        if (!(init.scale > 0.0) || !isfinite(init.scale)) return GPNERF_E_ARG;
    }
    const Ws w = ws_of(workspace);
    hipLaunchKernelGGL(fit_sums1_kernel, dim3(BLOCKS), dim3(THREADS), 0, S_(stream), points, points, (const float*)nullptr, (long)n, w);
    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(BLOCKS), 0, S_(stream), w, init, slot);
    return launch_status();
}

int gpnerf_transform_points(const float* points, int64_t n, const double* slot, int32_t vectors, float* out, void* stream) {
    if (!slot || n < 0 || n > MAX_PAIRS || !points || !out) return GPNERF_E_ARG;
    if (n == 0) return GPNERF_OK;
    hipLaunchKernelGGL(transform_kernel, dim3(blocks_for(n, POINT_THREADS)), dim3(POINT_THREADS), 0, S_(stream), points, (long)n, slot,
                       (int)(vectors != 0), out);
    return launch_status();
}

int gpnerf_align_step(const float* cur, const float* closest, const int32_t* face, const float* dist, int64_t n, const float* vertices,
                      int64_t n_vertices, const int32_t* faces, int64_t n_faces, float max_dist, double* slot, double* history_row,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!slot || n < 0 || n > MAX_PAIRS || !ws_ok(workspace, workspace_bytes) || !cur || !closest || !face || !dist) return GPNERF_E_ARG;
    if (!vertices || !faces || n_vertices < 0 || n_faces < 1 || n_faces > INT32_MAX || !(max_dist > 0.f)) return GPNERF_E_ARG;
    const Ws w = ws_of(workspace);
    hipLaunchKernelGGL(step_sums_kernel, dim3(BLOCKS), dim3(THREADS), 0, S_(stream), cur, closest, face, dist, (long)n, vertices, n_vertices,
                       faces, n_faces, max_dist, slot, w);
    hipLaunchKernelGGL(step_solve_kernel, dim3(1), dim3(BLOCKS), 0, S_(stream), w, slot, history_row);
    return launch_status();
}

}  // extern "C"
