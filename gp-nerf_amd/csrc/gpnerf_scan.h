// gpnerf_scan.h -- the three-launch integer scan shared by gpnerf_simplify.hip and gpnerf_meshtopo.hip: block sums, their exclusive
// prefix in one workgroup, the prefix applied.  Integer sums: any association gives the same result.  Included INSIDE the including
// file's unnamed namespace, behind <hip/hip_runtime.h> and <stdint.h>, so that every translation unit carries kernels of its own (no
// device code crosses files).  Every kernel is a template over a tag type that the including file names after itself, so that the
// library's code objects hold no two kernels of one name.  The caller owns `bsum`: at least ceil(n / SCAN_CHUNK) 64-bit words.
#ifndef GPNERF_SCAN_H
#define GPNERF_SCAN_H

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;                                 // per thread
constexpr int SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;         // 2048 items per block of the scans
constexpr int SCAN_TOP_THREADS = 1024;

// the items at or beyond *n_dev (when given) count as 0
__device__ __forceinline__ int scan_item(const int32_t* __restrict__ in, long i, long n, long n_live) { return (i < n && i < n_live) ? in[i] : 0; }

template <class Tag>
__global__ __launch_bounds__(SCAN_THREADS) void scan_sums_kernel(const int32_t* __restrict__ in, long n, const long long* n_dev, long long* bsum) {
    __shared__ long long s_sum[SCAN_THREADS];
    const int t = threadIdx.x;
    const long n_live = n_dev ? (long)*n_dev : n, i0 = (long)blockIdx.x * SCAN_CHUNK + (long)t * SCAN_ITEMS;
    long long sum = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) sum += scan_item(in, i0 + k, n, n_live);
    s_sum[t] = sum;
    __syncthreads();
    for (int s = SCAN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) s_sum[t] += s_sum[t + s];
        __syncthreads();
    }
    if (t == 0) bsum[blockIdx.x] = s_sum[0];
}

// one workgroup: the block sums become their exclusive prefix, the total goes to *total_out
template <class Tag>
__global__ __launch_bounds__(SCAN_TOP_THREADS) void scan_top_kernel(long long* bsum, long nb, long long* total_out) {
    __shared__ long long s_sum[SCAN_TOP_THREADS];
    const int t = threadIdx.x;
    const long per = (nb + SCAN_TOP_THREADS - 1) / SCAN_TOP_THREADS, b0 = min((long)t * per, nb), b1 = min(b0 + per, nb);
    long long sum = 0;
    for (long b = b0; b < b1; ++b) sum += bsum[b];
    s_sum[t] = sum;
    __syncthreads();
    for (int off = 1; off < SCAN_TOP_THREADS; off <<= 1) {    // inclusive scan over the threads, ten doubling steps
        const long long left = t >= off ? s_sum[t - off] : 0;
        __syncthreads();
        s_sum[t] += left;
        __syncthreads();
    }
    long long before = s_sum[t] - sum;
    const long long total = s_sum[SCAN_TOP_THREADS - 1];
    for (long b = b0; b < b1; ++b) {
        const long long c = bsum[b];
        bsum[b] = before;
        before += c;
    }
    if (t == 0) *total_out = total;
}

// MODE 0: out64[i] = the exclusive prefix.  MODE 1: `in` holds flags and out32 (which may be `in`) receives the prefix where the flag
// is set and -1 elsewhere; inverse[prefix] = i where given.
template <class Tag, int MODE>
__global__ __launch_bounds__(SCAN_THREADS) void scan_apply_kernel(const int32_t* in, long n, const long long* n_dev, const long long* __restrict__ bsum,
                                                                  long long* out64, int32_t* out32, int32_t* inverse) {
    __shared__ long long s_sum[SCAN_THREADS];
    const int t = threadIdx.x;
    const long n_live = n_dev ? (long)*n_dev : n, i0 = (long)blockIdx.x * SCAN_CHUNK + (long)t * SCAN_ITEMS;
    int item[SCAN_ITEMS];
    long long sum = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) { item[k] = scan_item(in, i0 + k, n, n_live); sum += item[k]; }
    s_sum[t] = sum;
    __syncthreads();                                     // (every item of the block has been read: out32 may alias in)
    long long before = bsum[blockIdx.x];
    for (int k = 0; k < t; ++k) before += s_sum[k];
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const long i = i0 + k;
        if (i < n) {
            if (MODE == 0) out64[i] = before;
            else {
                out32[i] = item[k] ? (int32_t)before : -1;
                if (inverse && item[k]) inverse[before] = (int32_t)i;
            }
        }
        before += item[k];
    }
}

// the three launches of a scan over n items (n >= 1, host-known)
template <class Tag, int MODE>
void scan_launch(const int32_t* in, int64_t n, const long long* n_dev, long long* bsum, long long* total_out, long long* out64, int32_t* out32,
                 int32_t* inverse, hipStream_t st) {
    const unsigned nb = (unsigned)((n + SCAN_CHUNK - 1) / SCAN_CHUNK);
    hipLaunchKernelGGL(scan_sums_kernel<Tag>, dim3(nb), dim3(SCAN_THREADS), 0, st, in, (long)n, n_dev, bsum);
    hipLaunchKernelGGL(scan_top_kernel<Tag>, dim3(1), dim3(SCAN_TOP_THREADS), 0, st, bsum, (long)nb, total_out);
    hipLaunchKernelGGL((scan_apply_kernel<Tag, MODE>), dim3(nb), dim3(SCAN_THREADS), 0, st, in, (long)n, n_dev, (const long long*)bsum, out64, out32, inverse);
}

#endif  // GPNERF_SCAN_H
