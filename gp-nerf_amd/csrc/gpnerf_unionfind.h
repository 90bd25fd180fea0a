// gpnerf_unionfind.h -- the lock-free min-label union-find on a global parent array, shared by gpnerf_mesh.hip (the alpha cube's
// components across bricks, cc_merge_kernel) and gpnerf_meshcomp.hip (a mesh's components over its faces).  Device functions only;
// included INSIDE the including file's unnamed namespace, behind <hip/hip_runtime.h>, so that every translation unit carries code of
// its own (no device code crosses files).
//
// The eight XCDs' L2s are not coherent for plain loads within one kernel, so EVERY access here is an agent-scope atomic: relaxed
// loads (they bypass the stale levels) and atomicMin.  A parent that is read late is harmless all the same, and that is what the
// walk relies on between its load and its use: a word only ever decreases, from a member of the set to a lower member of the same
// set, so an old value is still an ancestor-or-self on a path to the current root.  No lane ever waits for a value another lane has
// yet to write: a walk ends because indices strictly decrease along a path, and g_union retries only after somebody else's link
// succeeded, of which there are at most (number of elements - 1).  The kernel that unites is followed by a kernel boundary before
// anything reads the array with plain loads.
#ifndef GPNERF_UNIONFIND_H
#define GPNERF_UNIONFIND_H

__device__ __forceinline__ int g_load(int* p, long i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(int* p, int i) {
    int q = g_load(p, i);
    while (q != i) { i = q; q = g_load(p, i); }
    return i;
}
// find, then point every word of the walked path at the root found (a lower member of the same set: the invariant above holds)
__device__ __forceinline__ int g_find_compress(int* p, int i) {
    const int r = g_find(p, i);
    int q = g_load(p, i);
    while (q > r) { atomicMin(&p[i], r); i = q; q = g_load(p, i); }
    return r;
}
__device__ __forceinline__ void g_union(int* p, int a, int b) {
    while (true) {
        a = g_find_compress(p, a); b = g_find_compress(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&p[a], b);      // a was a root when read; if it still is, it now hangs below b
        if (old == a) return;
        a = old;                                   // somebody linked a first (to old < a): old and b still have to meet
    }
}

#endif  // GPNERF_UNIONFIND_H
