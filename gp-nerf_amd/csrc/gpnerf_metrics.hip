// gpnerf_metrics.hip -- the evaluator's per-frame metrics on gfx950 (libs/evaluators/if_nerf.py:15-63: MSE / PSNR over the
// mask_at_box pixels, SSIM on the mask's bounding-rectangle crop with both images zero outside the mask), the definition
// gp-nerf_amd/evaluator.py computes with float64 torch ops; include/gpnerf_hip.h states the output's specification.
//
// Four launches, each sized from H and W alone, nothing allocated and nothing waited for; no workgroup reads what another
// workgroup of the same launch wrote, and there is no atomic at all, so a frame's slot is a function of its inputs alone:
//   1. metrics_rows_kernel: one wavefront per image row -- the row's mask as 64-pixel ballot words with the count of set pixels in
//      front of each word, the row's count, first and last set column; and share `row` of the squared error over the 3n values
//      (pred and gt are compact lists, so that sum does not need the mask);
//   2. metrics_scan_kernel (one workgroup): the rows' exclusive offsets, the bounding rectangle, the population, the status;
//   3. metrics_ssim_kernel: one workgroup per 32x8 tile of 7x7 windows, anchored at the rectangle's origin (tiles beyond the
//      rectangle exit, as does every tile of a frame with a status): ranks its 38x14 pixels from the ballot words, gathers them,
//      sums the five window quantities separably in double and leaves one partial per tile and channel;
//   4. metrics_finish_kernel (one workgroup): adds the partials in a fixed order and writes the slot.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gpnerf_hip.h"

namespace {

#include "gpnerf_diag.h"       // the lab's hook points, empty in the product (csrc/nodiag/)
#include "gpnerf_util.h"       // align256, S_, launch_status

constexpr int WIN = 7;                                   // skimage's default window
constexpr int TILE_W = 32, TILE_H = 8;                   // windows per tile
constexpr int REG_W = TILE_W + WIN - 1, REG_H = TILE_H + WIN - 1, REG_N = REG_W * REG_H;   // the pixels under them: 38 x 14
constexpr int THREADS = TILE_W * TILE_H;                 // 256: one window per thread
constexpr int ST_OK = 0, ST_COUNT = 1, ST_EMPTY = 2, ST_SMALL = 3;
// the header metrics_scan_kernel leaves for the two kernels behind it
enum { HDR_X, HDR_Y, HDR_W, HDR_H, HDR_POP, HDR_STATUS, HDR_INTS = 8 };

struct Layout {
    int H, W, nblk, gtx, gty;                            // 64-pixel words per row; the grid of window tiles
    size_t hdr, rowinfo, rowoff, bits, pre, sqpart, part, total;
};

Layout layout_of(int32_t H, int32_t W) {
    Layout l;
    l.H = H; l.W = W;
    l.nblk = (W + 63) / 64;
    l.gtx = W >= WIN ? (W - WIN + 1 + TILE_W - 1) / TILE_W : 1;
    l.gty = H >= WIN ? (H - WIN + 1 + TILE_H - 1) / TILE_H : 1;
    size_t o = 0;
    l.hdr = o;     o += align256(sizeof(int32_t) * HDR_INTS);
    l.rowinfo = o; o += align256(sizeof(int32_t) * 4 * (size_t)H);           // {count, first, last, -}
    l.rowoff = o;  o += align256(sizeof(int32_t) * (size_t)H);
    l.bits = o;    o += align256(sizeof(uint64_t) * (size_t)H * l.nblk);
    l.pre = o;     o += align256(sizeof(int32_t) * (size_t)H * l.nblk);
    l.sqpart = o;  o += align256(sizeof(double) * (size_t)H);
    l.part = o;    o += align256(sizeof(double) * 3 * (size_t)l.gtx * l.gty);
    l.total = o;
    return l;
}

bool dims_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && (int64_t)H * W <= (int64_t)INT32_MAX; }

struct Ws {
    int32_t* hdr; int32_t* rowinfo; int32_t* rowoff; uint64_t* bits; int32_t* pre; double* sqpart; double* part;
};

// the sum of v over the workgroup's threads in a fixed tree; every thread gets it.  `red` holds blockDim.x doubles.
__device__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();                                     // (the previous use of `red` is over)
    red[t] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(64) void metrics_rows_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                          const uint8_t* __restrict__ mask, int H, int W, int nblk, long n3, Ws ws) {
    const int row = blockIdx.x, lane = threadIdx.x;
    int count = 0, first = W, last = -1;
    for (int b = 0; b < nblk; ++b) {
        const int col = b * 64 + lane;
        const bool m = col < W && mask[(long)row * W + col] != 0;
        const unsigned long long word = __ballot(m);
        if (lane == 0) {
            ws.bits[(long)row * nblk + b] = word;
            ws.pre[(long)row * nblk + b] = count;
        }
        if (word) {
            first = min(first, b * 64 + __ffsll(word) - 1);
            last = b * 64 + 63 - __clzll(word);
            count += __popcll(word);
        }
    }
    if (lane == 0) {
        ws.rowinfo[4 * row] = count;
        ws.rowinfo[4 * row + 1] = first;
        ws.rowinfo[4 * row + 2] = last;
        ws.rowinfo[4 * row + 3] = 0;
    }
    // share `row` of the 3n squared differences: a contiguous chunk, lane-strided, then the wavefront's fixed shuffle tree
    const long chunk = (n3 + H - 1) / H, lo = row * chunk, hi = min(lo + chunk, n3);
    double s = 0.0;
    for (long i = lo + lane; i < hi; i += 64) {
        const double d = (double)pred[i] - (double)gt[i];
        s += d * d;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) ws.sqpart[row] = s;
}

__global__ __launch_bounds__(THREADS) void metrics_scan_kernel(int H, int W, long n, Ws ws) {
    __shared__ int s_cnt[THREADS], s_y0[THREADS], s_y1[THREADS], s_x0[THREADS], s_x1[THREADS];
    const int t = threadIdx.x;
    const int per = (H + THREADS - 1) / THREADS, r0 = min(t * per, H), r1 = min(r0 + per, H);     // consecutive rows per thread
    int cnt = 0, y0 = H, y1 = -1, x0 = W, x1 = -1;
    for (int r = r0; r < r1; ++r) {
        const int c = ws.rowinfo[4 * r];
        if (c) {
            y0 = min(y0, r); y1 = r;
            x0 = min(x0, ws.rowinfo[4 * r + 1]); x1 = max(x1, ws.rowinfo[4 * r + 2]);
        }
        cnt += c;
    }
    s_cnt[t] = cnt; s_y0[t] = y0; s_y1[t] = y1; s_x0[t] = x0; s_x1[t] = x1;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < t; ++k) before += s_cnt[k];
    for (int r = r0; r < r1; ++r) {
        ws.rowoff[r] = before;
        before += ws.rowinfo[4 * r];
    }
    if (t == 0) {
        int pop = 0;
        for (int k = 0; k < THREADS; ++k) {
            pop += s_cnt[k];
            y0 = min(y0, s_y0[k]); y1 = max(y1, s_y1[k]); x0 = min(x0, s_x0[k]); x1 = max(x1, s_x1[k]);
        }
        const int w = pop ? x1 - x0 + 1 : 0, h = pop ? y1 - y0 + 1 : 0;
        ws.hdr[HDR_X] = pop ? x0 : 0;
        ws.hdr[HDR_Y] = pop ? y0 : 0;
        ws.hdr[HDR_W] = w;
        ws.hdr[HDR_H] = h;
        ws.hdr[HDR_POP] = pop;
        ws.hdr[HDR_STATUS] = (long)pop != n ? ST_COUNT : pop == 0 ? ST_EMPTY : (w < WIN || h < WIN) ? ST_SMALL : ST_OK;
    }
}

__global__ __launch_bounds__(THREADS) void metrics_ssim_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int nblk,
                                                               int gtx, Ws ws) {
    __shared__ float s_p[3][REG_N], s_g[3][REG_N];
    __shared__ double s_h[5][REG_H][TILE_W];             // the horizontal 7-sums of x, y, xx, yy, xy of one channel
    __shared__ double s_red[THREADS];
    if (ws.hdr[HDR_STATUS] != ST_OK) return;             // (uniform: the whole launch leaves)
    const int x0 = ws.hdr[HDR_X], y0 = ws.hdr[HDR_Y], w = ws.hdr[HDR_W], h = ws.hdr[HDR_H];
    const int tx = blockIdx.x % gtx, ty = blockIdx.x / gtx;
    const int wx0 = tx * TILE_W, wy0 = ty * TILE_H;      // the tile's first window, relative to the rectangle
    if (wx0 > w - WIN || wy0 > h - WIN) return;          // no window of this tile lies in the rectangle
    const int t = threadIdx.x;
    for (int i = t; i < REG_N; i += THREADS) {
        const int rx = wx0 + i % REG_W, ry = wy0 + i / REG_W;
        float p[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f};
        if (rx < w && ry < h) {                          // inside the rectangle, hence inside the image
            const int gx = x0 + rx, gy = y0 + ry, b = gx >> 6, k = gx & 63;
            const unsigned long long word = ws.bits[(long)gy * nblk + b];
            if ((word >> k) & 1ull) {
                // the pixel's place in the compact lists: status 0 means the population is n, so rank < n
                const long rank = (long)ws.rowoff[gy] + ws.pre[(long)gy * nblk + b] + __popcll(word & ((1ull << k) - 1ull));
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    p[c] = pred[3 * rank + c];
                    g[c] = gt[3 * rank + c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s_p[c][i] = p[c];
            s_g[c][i] = g[c];
        }
    }
    const int wx = t % TILE_W, wy = t / TILE_W;
    const bool valid = wx0 + wx <= w - WIN && wy0 + wy <= h - WIN;
    const double c1 = (0.01 * 2.0) * (0.01 * 2.0), c2 = (0.03 * 2.0) * (0.03 * 2.0);
    const double area = (double)(WIN * WIN), norm = area / (area - 1.0);
    for (int c = 0; c < 3; ++c) {
        __syncthreads();                                 // the region is loaded / the previous channel's s_h has been read
        for (int i = t; i < REG_H * TILE_W; i += THREADS) {
            const int col = i % TILE_W, r = i / TILE_W;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const double x = (double)s_p[c][r * REG_W + col + k], y = (double)s_g[c][r * REG_W + col + k];
                sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
            }
            s_h[0][r][col] = sx; s_h[1][r][col] = sy; s_h[2][r][col] = sxx; s_h[3][r][col] = syy; s_h[4][r][col] = sxy;
        }
        __syncthreads();
        double q[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) s += s_h[j][wy + k][wx];
            q[j] = s / area;
        }
        const double ux = q[0], uy = q[1];
        const double vx = norm * (q[2] - ux * ux), vy = norm * (q[3] - uy * uy), vxy = norm * (q[4] - ux * uy);
        const double ssim = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
        const double sum = block_sum(valid ? ssim : 0.0, s_red);
        if (t == 0) ws.part[3 * (long)blockIdx.x + c] = sum;
    }
}

__global__ __launch_bounds__(THREADS) void metrics_finish_kernel(int H, int gtx, long n3, Ws ws, double* __restrict__ out) {
    __shared__ double s_red[THREADS];
    const int t = threadIdx.x;
    const int status = ws.hdr[HDR_STATUS], w = ws.hdr[HDR_W], h = ws.hdr[HDR_H];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double mse = nan, ssim = nan;
    if (status == ST_OK || status == ST_SMALL) {
        double s = 0.0;
        for (int r = t; r < H; r += THREADS) s += ws.sqpart[r];
        mse = block_sum(s, s_red) / (double)n3;
    }
    if (status == ST_OK) {
        const int ntx = (w - WIN + 1 + TILE_W - 1) / TILE_W, nty = (h - WIN + 1 + TILE_H - 1) / TILE_H;    // the tiles that wrote
        const double windows = (double)(w - WIN + 1) * (double)(h - WIN + 1);
        double mean = 0.0;
        for (int c = 0; c < 3; ++c) {
            double s = 0.0;
            for (int k = t; k < ntx * nty; k += THREADS) s += ws.part[3 * ((long)(k / ntx) * gtx + k % ntx) + c];
            mean += block_sum(s, s_red) / windows;
        }
        ssim = mean / 3.0;
    }
    if (t == 0) {
        out[GPNERF_METRICS_MSE] = mse;
        out[GPNERF_METRICS_SSIM] = ssim;
        out[GPNERF_METRICS_X] = (double)ws.hdr[HDR_X];
        out[GPNERF_METRICS_Y] = (double)ws.hdr[HDR_Y];
        out[GPNERF_METRICS_W] = (double)w;
        out[GPNERF_METRICS_H] = (double)h;
        out[GPNERF_METRICS_POPULATION] = (double)ws.hdr[HDR_POP];
        out[GPNERF_METRICS_STATUS] = (double)status;
    }
}

}  // namespace

extern "C" {

size_t gpnerf_metrics_workspace_bytes(int32_t H, int32_t W) {
    if (!dims_ok(H, W)) return 0;
    return layout_of(H, W).total;
}

int gpnerf_image_metrics(const float* pred, const float* gt, const uint8_t* mask, int32_t H, int32_t W, int64_t n, void* workspace,
                         size_t workspace_bytes, double* out, void* stream) {
    if (!pred || !gt || !mask || !workspace || !out || !dims_ok(H, W) || n < 0 || n > (int64_t)H * W) return GPNERF_E_ARG;
    const Layout l = layout_of(H, W);
    if (workspace_bytes < l.total) return GPNERF_E_ARG;
    char* base = static_cast<char*>(workspace);
    Ws ws;
    ws.hdr = reinterpret_cast<int32_t*>(base + l.hdr);
    ws.rowinfo = reinterpret_cast<int32_t*>(base + l.rowinfo);
    ws.rowoff = reinterpret_cast<int32_t*>(base + l.rowoff);
    ws.bits = reinterpret_cast<uint64_t*>(base + l.bits);
    ws.pre = reinterpret_cast<int32_t*>(base + l.pre);
    ws.sqpart = reinterpret_cast<double*>(base + l.sqpart);
    ws.part = reinterpret_cast<double*>(base + l.part);
    const long n3 = 3 * (long)n;
    hipLaunchKernelGGL(metrics_rows_kernel, dim3((unsigned)H), dim3(64), 0, S_(stream), pred, gt, mask, (int)H, (int)W, l.nblk, n3, ws);
    hipLaunchKernelGGL(metrics_scan_kernel, dim3(1), dim3(THREADS), 0, S_(stream), (int)H, (int)W, (long)n, ws);
    hipLaunchKernelGGL(metrics_ssim_kernel, dim3((unsigned)(l.gtx * l.gty)), dim3(THREADS), 0, S_(stream), pred, gt, l.nblk, l.gtx, ws);
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(THREADS), 0, S_(stream), (int)H, l.gtx, n3, ws, out);
    return launch_status();
}

}  // extern "C"
