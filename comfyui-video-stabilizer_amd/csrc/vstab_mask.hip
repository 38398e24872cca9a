// vstab_mask.hip -- estimation mask: per-frame subject masks at full resolution -> which grid samples of the dense flow the
// model fit may use (vstab_sample_fit_batch_masked).  Not a reference feature; the rule is stated in include/vstab.h.
//
// Everything is an OR over a box: a grid sample is blocked iff a subject pixel lies in the rectangle of source pixels that
// its margin square of working pixels covers, and a rectangle's OR separates into rows and columns.  Two kernels:
//
//   mask_rows_kernel   one workgroup per (mask, working row Y): reads the source rows of Y's INTER_AREA footprint (the only
//                      full-resolution traffic: 4 B per mask value, 16-byte non-temporal loads -- read once, never again),
//                      ORs them per source column into LDS, folds columns into the covered working row, dilates that row by
//                      `margin` and keeps every `step`-th column: gw bytes per working row.
//   mask_cols_kernel   one lane per (mask, grid sample): OR of those bytes over the working rows |Y - gy*step| <= margin.
//                      A broadcast mask (n_masks == 1) is reduced once; its lanes write the result to every frame.
//
// The footprints of neighbouring working rows are disjoint for integer ratios (1080p -> 540 rows: two source rows each) and
// share one source row otherwise, which the second workgroup finds in L2.  Between the kernels travel work_h * gw bytes per
// mask (65 KB for 960x540, step 8) against 8.3 MB of mask values.  No atomics; nothing but the rows' bytes is kept.
#include "vstab_internal.h"
#include <cmath>

namespace {

constexpr int MASK_MAX_COLS = 8192;   // source columns of a row (LDS: one byte per source column + one per working column)

// `> 0.5` or not finite (NaN fails `<=`; -inf passes it and is caught by name)
__device__ __forceinline__ unsigned subject(float v) { return (!(v <= 0.5f) || v == -INFINITY) ? 1u : 0u; }

// floor(a * num / den), ceil(a * num / den) for non-negative ints whose product fits 64 bits
__host__ __device__ __forceinline__ int floor_ratio(int a, int num, int den) { return (int)(((long long)a * num) / den); }
__host__ __device__ __forceinline__ int ceil_ratio(int a, int num, int den) { return (int)(((long long)a * num + den - 1) / den); }

// VEC: src_w % 4 == 0 and the base 16-byte aligned (every row then is): four columns per lane and load
template <bool VEC>
__global__ __launch_bounds__(512) void mask_rows_kernel(const float* __restrict__ mask, uint8_t* __restrict__ rows, int src_h, int src_w,
                                                        int work_h, int work_w, int gw, int step, int margin)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_sub[MASK_MAX_COLS];   // per source column: subject in any row of the footprint
    __shared__ uint8_t s_cov[MASK_MAX_COLS];                                // per working column: covered
    const int Y = (int)blockIdx.x % work_h, m = (int)blockIdx.x / work_h;
    const int y0 = floor_ratio(Y, src_h, work_h), y1 = min(src_h, ceil_ratio(Y + 1, src_h, work_h));
    const float* __restrict__ M = mask + ((size_t)m * src_h + y0) * src_w;
    if (VEC) {
        typedef float f4_t __attribute__((ext_vector_type(4)));
        const int nvec = src_w >> 2;
        for (int k = threadIdx.x; k < nvec; k += blockDim.x) {
            unsigned a = 0, b = 0, c = 0, d = 0;
            for (int y = 0; y < y1 - y0; y++) {
                const f4_t v = __builtin_nontemporal_load(reinterpret_cast<const f4_t*>(M + (size_t)y * src_w) + k);
                a |= subject(v.x); b |= subject(v.y); c |= subject(v.z); d |= subject(v.w);
            }
            reinterpret_cast<unsigned*>(s_sub)[k] = a | (b << 8) | (c << 16) | (d << 24);
        }
    } else {
        for (int x = threadIdx.x; x < src_w; x += blockDim.x) {
            unsigned a = 0;
            for (int y = 0; y < y1 - y0; y++) a |= subject(__builtin_nontemporal_load(M + (size_t)y * src_w + x));
            s_sub[x] = (uint8_t)a;
        }
    }
    __syncthreads();
    for (int X = threadIdx.x; X < work_w; X += blockDim.x) {
        const int x0 = floor_ratio(X, src_w, work_w), x1 = min(src_w, ceil_ratio(X + 1, src_w, work_w));
        unsigned a = 0;
        for (int x = x0; x < x1; x++) a |= s_sub[x];
        s_cov[X] = (uint8_t)a;
    }
    __syncthreads();
    uint8_t* __restrict__ R = rows + ((size_t)m * work_h + Y) * gw;
    for (int gx = threadIdx.x; gx < gw; gx += blockDim.x) {
        const int X0 = max(0, gx * step - margin), X1 = min(work_w - 1, gx * step + margin);
        unsigned a = 0;
        for (int X = X0; X <= X1; X++) a |= s_cov[X];
        R[gx] = (uint8_t)a;
    }
}

__global__ __launch_bounds__(256) void mask_cols_kernel(const uint8_t* __restrict__ rows, uint8_t* __restrict__ blocked, int n_masks,
                                                        int n_frames, int work_h, int gh, int gw, int step, int margin)
{
    const int per = gh * gw;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)n_masks * per) return;
    const int m = (int)(t / per), g = (int)(t - (long long)m * per);
    const int gy = g / gw, gx = g - gy * gw;
    const int Y0 = max(0, gy * step - margin), Y1 = min(work_h - 1, gy * step + margin);
    const uint8_t* __restrict__ R = rows + (size_t)m * work_h * gw + gx;
    unsigned a = 0;
    for (int Y = Y0; Y <= Y1; Y++) a |= R[(size_t)Y * gw];
    if (n_masks == 1) {
        for (int f = 0; f < n_frames; f++) blocked[(size_t)f * per + g] = (uint8_t)a;
    } else {
        blocked[(size_t)m * per + g] = (uint8_t)a;
    }
}

}  // namespace

extern "C" int vstab_mask_block_grid(vstab_ctx* ctx, const float* mask, int n_masks, int n_frames, int src_h, int src_w, int work_h,
                                     int work_w, int step, int margin, uint8_t* blocked)
{
    VSTAB_REQUIRE(ctx != nullptr, "vstab_mask_block_grid: ctx is NULL");
    VSTAB_REQUIRE(mask && blocked, "vstab_mask_block_grid: NULL pointer argument");
    VSTAB_REQUIRE(n_frames > 0 && src_h > 0 && src_w > 0 && work_h > 0 && work_w > 0 && step > 0, "vstab_mask_block_grid: non-positive size");
    VSTAB_REQUIRE(n_masks == 1 || n_masks == n_frames, "vstab_mask_block_grid: %d masks for %d frames (expected 1 or %d)", n_masks, n_frames, n_frames);
    VSTAB_REQUIRE(work_h <= src_h && work_w <= src_w, "vstab_mask_block_grid: working size %dx%d larger than source %dx%d", work_w, work_h, src_w, src_h);
    VSTAB_REQUIRE(src_w <= MASK_MAX_COLS, "vstab_mask_block_grid: %d source columns exceed the supported %d", src_w, MASK_MAX_COLS);
    VSTAB_REQUIRE(margin >= 0 && margin <= 64, "vstab_mask_block_grid: margin %d outside [0, 64]", margin);
    const int gh = (work_h + step - 1) / step, gw = (work_w + step - 1) / step;
    VSTAB_REQUIRE((long long)n_masks * work_h < 0x7fffffffLL, "vstab_mask_block_grid: clip too large");
    VSTAB_HIP(hipSetDevice(ctx->device));
    if (ctx->d_mask_rows.reserve((size_t)n_masks * work_h * gw)) return 1;
    uint8_t* rows = static_cast<uint8_t*>(ctx->d_mask_rows.ptr);
    KernelTimer timer(ctx, "mask");
    const bool vec = (src_w % 4 == 0) && (reinterpret_cast<uintptr_t>(mask) % 16 == 0);
    // lanes for one pass over the row's loads where that fits (1920 columns: 480 loads of 16 bytes -> 512 lanes)
    const int items = vec ? src_w / 4 : src_w;
    const int threads = items >= 512 ? 512 : (items > 256 ? 512 : 256);
    const dim3 grid((unsigned)(n_masks * work_h));
    if (vec) hipLaunchKernelGGL(mask_rows_kernel<true>, grid, dim3(threads), 0, ctx->stream, mask, rows, src_h, src_w, work_h, work_w, gw, step, margin);
    else hipLaunchKernelGGL(mask_rows_kernel<false>, grid, dim3(threads), 0, ctx->stream, mask, rows, src_h, src_w, work_h, work_w, gw, step, margin);
    VSTAB_HIP(hipGetLastError());
    const long long lanes = (long long)n_masks * gh * gw;
    hipLaunchKernelGGL(mask_cols_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, ctx->stream, rows, blocked, n_masks, n_frames,
                       work_h, gh, gw, step, margin);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
