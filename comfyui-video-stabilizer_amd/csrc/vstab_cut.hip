// vstab_cut.hip -- scene cuts: the motion-compensated residual of every consecutive pair of estimation images
// (vstab_pair_residual_batch).  Not a reference feature; the rule is stated in include/vstab.h.
//
// One kernel.  A workgroup owns CUT_ROWS rows of one pair; a lane takes 16 pixels of a row of the FROM image with one
// 16-byte load, maps each through the pair's transition (fp64 from the float32 matrix, the rule's association), rounds
// half-to-even and looks the TO image up there with a byte load.  A shake-sized transition keeps those lookups within a
// few rows of the pixel, so both images of a pair cross HBM about once: ~2 * h * w bytes per pair.  Everything that is
// summed is an integer (|a - b| <= 255, counts): lane sums (u32) -> BlockSums (vstab_internal.h), totalled in 64 bits ->
// one atomic per workgroup and array, skipped where the workgroup counted nothing.
#include "vstab_internal.h"

namespace {

constexpr int CUT_ROWS = 16;      // rows of a pair per workgroup (960x540: 34 workgroups per pair, 3.75 loads per lane)
constexpr int CUT_THREADS = 256;

// (the mapping of one pixel, vstab_pair_lookup, is in vstab_internal.h: the deflicker measures through the same one)

// VEC: w % 16 == 0 and the base 16-byte aligned (every row then is)
template <bool VEC>
__global__ __launch_bounds__(CUT_THREADS) void pair_residual_kernel(const uint8_t* __restrict__ gray, const float* __restrict__ mats,
                                                                    int h, int w, int tiles, unsigned long long* __restrict__ sum_abs,
                                                                    unsigned* __restrict__ inside)
{
    __shared__ BlockSums<unsigned, 2, CUT_THREADS> s_sums;      // |a - b|, inside
    const int pair = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - pair * tiles;
    const int y0 = tile * CUT_ROWS, rows = min(CUT_ROWS, h - y0);
    PairMatrix A;
    for (int k = 0; k < 9; k++) A.m[k] = (double)mats[(size_t)pair * 9 + k];
    const uint8_t* __restrict__ from = gray + (size_t)pair * h * w;
    const uint8_t* __restrict__ to = from + (size_t)h * w;
    const int chunks = (w + 15) >> 4;                   // 16-pixel pieces of a row
    unsigned acc = 0, cnt = 0;                          // <= 255 * 16 * (CUT_ROWS * chunks / CUT_THREADS + 1): far below 2^32
    for (int item = threadIdx.x; item < rows * chunks; item += CUT_THREADS) {
        const int r = item / chunks, c = item - r * chunks;
        const int y = y0 + r, x0 = c << 4;
        const uint8_t* __restrict__ row = from + (size_t)y * w;
        if (VEC) {
            const uint4 v = *reinterpret_cast<const uint4*>(row + x0);
            const unsigned word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++) {
                int q;
                if (vstab_pair_lookup(A, x0 + k, y, h, w, &q)) {
                    const int a = (int)((word[k >> 2] >> ((k & 3) * 8)) & 0xffu), b = (int)to[q];
                    acc += (unsigned)abs(a - b);
                    cnt += 1;
                }
            }
        } else {
            const int x1 = min(w, x0 + 16);
            for (int x = x0; x < x1; x++) {
                int q;
                if (vstab_pair_lookup(A, x, y, h, w, &q)) {
                    acc += (unsigned)abs((int)row[x] - (int)to[q]);
                    cnt += 1;
                }
            }
        }
    }
    s_sums.put({acc, cnt});
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned count = s_sums.total(1);
        if (count) {
            atomicAdd(&sum_abs[pair], s_sums.total<unsigned long long>(0));
            atomicAdd(&inside[pair], count);
        }
    }
}

}  // namespace

extern "C" int vstab_pair_residual_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const float* transitions,
                                         uint64_t* sum_abs, uint32_t* inside)
{
    VSTAB_REQUIRE(ctx != nullptr, "vstab_pair_residual_batch: ctx is NULL");
    VSTAB_REQUIRE(gray && transitions && sum_abs && inside, "vstab_pair_residual_batch: NULL pointer argument");
    VSTAB_REQUIRE(n >= 2 && h > 0 && w > 0, "vstab_pair_residual_batch: needs at least two frames of a positive size (n=%d, %dx%d)", n, w, h);
    VSTAB_REQUIRE((long long)h * w < 0x7fffffffLL, "vstab_pair_residual_batch: %dx%d image too large", w, h);
    const int pairs = n - 1, tiles = (h + CUT_ROWS - 1) / CUT_ROWS;
    VSTAB_REQUIRE((long long)pairs * tiles < 0x7fffffffLL, "vstab_pair_residual_batch: clip too large");
    VSTAB_HIP(hipSetDevice(ctx->device));
    void* d_mats = nullptr;
    if (int rc = vstab_stage_params(ctx, transitions, (size_t)pairs * 9 * sizeof(float), &d_mats)) return rc;
    VSTAB_HIP(hipMemsetAsync(sum_abs, 0, (size_t)pairs * sizeof(uint64_t), ctx->stream));
    VSTAB_HIP(hipMemsetAsync(inside, 0, (size_t)pairs * sizeof(uint32_t), ctx->stream));
    KernelTimer timer(ctx, "cut");
    const bool vec = (w % 16 == 0) && (reinterpret_cast<uintptr_t>(gray) % 16 == 0);
    const dim3 grid((unsigned)(pairs * tiles)), block(CUT_THREADS);
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(sum_abs);
    if (vec) hipLaunchKernelGGL(pair_residual_kernel<true>, grid, block, 0, ctx->stream, gray, static_cast<const float*>(d_mats), h, w, tiles, sums, inside);
    else hipLaunchKernelGGL(pair_residual_kernel<false>, grid, block, 0, ctx->stream, gray, static_cast<const float*>(d_mats), h, w, tiles, sums, inside);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
