// vstab_sharp.hip -- sharpness transfer: the gradient energy of every frame of a clip as one exact 64-bit integer (the rule:
// include/vstab.h, vstab_frame_sharpness_batch).  The transfer itself is a warp kernel and lives in vstab_neighbour.hip.
//
//   frame_sharpness_kernel  one workgroup = one 64 x 32 tile of one frame.  Y = (q(r) + 2 q(g) + q(b)) >> 2 of the tile's pixels
//                           and of one more column and row (the halo the forward differences reach into) is computed once per
//                           pixel into LDS as 32-bit words, rows 65 words apart so that the lanes of a wavefront, which read
//                           consecutive words, never share a bank.  Both differences come from LDS.  A thread sums its 8
//                           pixels in 64 bits -> BlockSums (vstab_internal.h) -> one 64-bit atomic add per workgroup and
//                           frame, skipped where the tile is flat.  Nothing waits for another workgroup.
// The pixel loads are non-temporal: a frame is read once by this pass, 12 B per pixel plus the halo (65 * 33 / (64 * 32) =
// 1.05 reads per pixel, the halo from the cache).  The mask moments measured a tenth in their favour;
// VSTAB_SHARPNESS_PLAIN (a build flag) restores plain loads for an A/B.  A pixel is three dwords at a 4-byte alignment,
// whatever the frame's start: no wider vector, so no head or tail.  40 VGPRs (nine dwordx3 loads in flight per thread), no
// scratch, 8 waves per SIMD (-Rpass-analysis=kernel-resource-usage).
#include "vstab_internal.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_TW = 64, SH_TH = 32;                  // the tile: 2048 pixels, 8 per thread
constexpr int SH_LW = SH_TW + 1, SH_LH = SH_TH + 1;    // with the halo column and row
constexpr int SH_WORDS = SH_LW * SH_LH;                // 2145 words = 8.4 KiB

__device__ __forceinline__ float sh_load(const float* p)
{
#ifdef VSTAB_SHARPNESS_PLAIN
    return *p;
#else
    return __builtin_nontemporal_load(p);
#endif
}

// q of the blended fill's gain sums (vstab_neighbour.hip: gain_q): 16 fractional bits, truncated; below 0 and NaN give 0, 1 and
// above give 65536.
__device__ __forceinline__ unsigned sh_q(float v)
{
    return v > 0.f ? (v < 1.f ? (unsigned)(v * 65536.0f) : 65536u) : 0u;
}

// grid (tiles_x * tiles_y * n), 256 threads; h * w <= 2^30, w >= 2, h >= 2
__global__ __launch_bounds__(SH_THREADS) void frame_sharpness_kernel(const float* __restrict__ frames, int h, int w, unsigned tiles_x,
                                                                     unsigned tiles_per_frame, unsigned long long* __restrict__ energy)
{
    __shared__ unsigned s_y[SH_WORDS];
    __shared__ BlockSums<unsigned long long, 1, SH_THREADS> s_energy;
    const unsigned t = threadIdx.x;
    const unsigned frame = blockIdx.x / tiles_per_frame, tile = blockIdx.x - frame * tiles_per_frame;
    const unsigned tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int x0 = (int)tile_x * SH_TW, y0 = (int)tile_y * SH_TH;
    const float* __restrict__ f = frames + (size_t)frame * (size_t)h * (size_t)w * 3;

    // Y of the tile and its halo, the loads of all nine rounds first; a word outside the frame is 0 and is never read back
    // (the differences stop at w - 2, h - 2)
    constexpr int ROUNDS = (SH_WORDS + SH_THREADS - 1) / SH_THREADS;
    float v[ROUNDS][3];
#pragma unroll
    for (int j = 0; j < ROUNDS; j++) {
        const unsigned i = t + (unsigned)j * SH_THREADS;
        const unsigned ly = i / (unsigned)SH_LW, lx = i - ly * (unsigned)SH_LW;
        const int x = x0 + (int)lx, y = y0 + (int)ly;
        v[j][0] = v[j][1] = v[j][2] = 0.f;
        if (i < (unsigned)SH_WORDS && x < w && y < h) {
            const float* p = f + ((unsigned)y * (unsigned)w + (unsigned)x) * 3u;     // 3 h w <= 3 * 2^30 < 2^32
            v[j][0] = sh_load(p); v[j][1] = sh_load(p + 1); v[j][2] = sh_load(p + 2);
        }
    }
#pragma unroll
    for (int j = 0; j < ROUNDS; j++) {
        const unsigned i = t + (unsigned)j * SH_THREADS;
        if (i < (unsigned)SH_WORDS) s_y[i] = (sh_q(v[j][0]) + 2u * sh_q(v[j][1]) + sh_q(v[j][2])) >> 2;   // <= 65536
    }
    __syncthreads();

    unsigned long long sum = 0ull;
    const unsigned lx = t & (SH_TW - 1);
    const int x = x0 + (int)lx;
#pragma unroll
    for (int r = 0; r < SH_TH / (SH_THREADS / SH_TW); r++) {
        const unsigned ly = (t >> 6) + (unsigned)r * (SH_THREADS / SH_TW);
        const int y = y0 + (int)ly;
        if (x < w - 1 && y < h - 1) {
            const int c = (int)s_y[ly * SH_LW + lx];
            const int gx = (int)s_y[ly * SH_LW + lx + 1] - c, gy = (int)s_y[(ly + 1) * SH_LW + lx] - c;   // |g| <= 65536
            sum += (unsigned long long)((long long)gx * gx) + (unsigned long long)((long long)gy * gy);   // <= 2^33 a pixel
        }
    }

    s_energy.put({sum});
    __syncthreads();
    if (t == 0) {
        const unsigned long long total = s_energy.total(0);   // <= 2^11 * 2^33
        if (total) atomicAdd(energy + frame, total);
    }
}

}  // namespace

extern "C" int vstab_frame_sharpness_batch(vstab_ctx* ctx, const float* frames, int n, int h, int w, uint64_t* energy)
{
    const char* who = "vstab_frame_sharpness_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(frames != nullptr && energy != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE((long long)h * w <= (1ll << 30), "%s: %d x %d pixels per frame, the limit is 2^30 (a pixel adds up to 2^33 to a "
                  "64-bit sum)", who, w, h);
    VSTAB_REQUIRE(((uintptr_t)frames & 3) == 0 && ((uintptr_t)energy & 7) == 0, "%s: a pointer argument is not aligned to its element size", who);
    const unsigned tiles_x = ((unsigned)w + SH_TW - 1) / SH_TW, tiles_y = ((unsigned)h + SH_TH - 1) / SH_TH;
    const unsigned long long blocks = (unsigned long long)tiles_x * tiles_y * (unsigned long long)n;
    VSTAB_REQUIRE(blocks <= 0x7fffffffull, "%s: n=%d frames of %d x %d exceed the grid", who, n, w, h);

    VSTAB_HIP(hipSetDevice(ctx->device));
    KernelTimer timer(ctx, "sharpness");
    VSTAB_HIP(hipMemsetAsync(energy, 0, sizeof(uint64_t) * (size_t)n, ctx->stream));
    if (w == 1 || h == 1) return 0;                     // no pixel has both differences: every energy is zero
    hipLaunchKernelGGL(frame_sharpness_kernel, dim3((unsigned)blocks), dim3(SH_THREADS), 0, ctx->stream, frames, h, w, tiles_x,
                       tiles_x * tiles_y, reinterpret_cast<unsigned long long*>(energy));
    VSTAB_HIP(hipGetLastError());
    return 0;
}
