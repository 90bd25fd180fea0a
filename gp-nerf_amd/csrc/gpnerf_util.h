// gpnerf_util.h -- the small helpers every translation unit of the library had a copy of: the launchers' host helpers and the
// per-wavefront counts and sums behind the integer statistics.  Included INSIDE the including file's unnamed namespace, behind
// <hip/hip_runtime.h>, <stdint.h>, include/gpnerf_hip.h (GPNERF_OK, GPNERF_E_LAUNCH) and gpnerf_diag.h (DEV).  No kernel lives
// here; a helper a file does not call leaves nothing in its object.  A file whose helper of one of these names means something
// else keeps it under a name of its own (gpnerf_mesh.hip: wave_sum_lane0).
#ifndef GPNERF_UTIL_H
#define GPNERF_UTIL_H

// ---- host
constexpr size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
hipStream_t S_(void* s) { return reinterpret_cast<hipStream_t>(s); }
int launch_status() { return hipGetLastError() == hipSuccess ? GPNERF_OK : GPNERF_E_LAUNCH; }
unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
// a grid-stride launch over `items`, `per` of them per block and step: at least one block, at most `cap`
constexpr int SWEEP_BLOCKS_MAX = 4096;
unsigned sweep_blocks(int64_t items, int per, int cap = SWEEP_BLOCKS_MAX) {
    const int64_t b = (items + per - 1) / per;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

bool mesh_ok(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces) {
    return n_vertices >= 0 && n_vertices <= INT32_MAX && n_faces >= 0 && n_faces <= INT32_MAX && (vertices || n_vertices == 0) &&
           (faces || n_faces == 0);
}

// ---- device.  Every lane of the wavefront must reach these calls.
DEV int wave_count(bool flag) { return __popcll(__ballot(flag)); }

// one add per wavefront, by its first lane with the flag, and none for a zero
DEV void wave_count(bool flag, long long* counter) {
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1))
        atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)__popcll(m));
}

// the sum over the wavefront, in every lane (integers: any association gives the same result)
template <class T>
DEV T wave_sum(T v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// stats[which] += n, unless n is zero: for one lane of a wavefront, behind a wave_count or a wave_sum
DEV void stat_add(long long* stats, int which, long long n) {
    if (n) atomicAdd(reinterpret_cast<unsigned long long*>(stats + which), (unsigned long long)n);
}

#endif  // GPNERF_UTIL_H
