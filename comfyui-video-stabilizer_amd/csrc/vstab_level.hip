// vstab_level.hip -- horizon level: the histogram of gradient orientations of every estimation image, folded modulo 90
// degrees, weighted by the squared gradient magnitude, as exact integers (vstab_orientation_hist_batch).  Not a reference
// feature; the rule is stated in include/vstab.h.
//
// One kernel.  A workgroup owns LEVEL_ROWS rows of one frame; a lane takes 16 pixels of a row with one 16-byte load per
// row of the 3x3 support (the rows above and below are another lane's own row: they come from L2, so a frame crosses HBM
// about once) plus one halo byte on either side.  Everything is an integer: the Scharr gradients, m2 = gx^2 + gy^2
// (< 2^32), the bin (one division of numbers below 2^24, done with v_rcp_f32 and an exact correction step).
//
// Where the mass goes: a lane walks its pixels in order and merges a run of equal bins in registers (64 bits wide from the
// start), so axis-aligned content -- nearly every counted pixel in bin K, one LDS address -- costs one LDS atomic per lane
// and not one per pixel; what a lane does flush goes into its WAVE's copy of the histogram in LDS (ds_add_u64), so the four
// waves never meet on an address.  Behind a barrier the copies are added and every non-zero bin goes out with one 64-bit
// global atomic per workgroup and frame.
#include "vstab_internal.h"

namespace {

constexpr int LEVEL_K = VSTAB_ORIENTATION_K;        // bins: -K .. K
constexpr int LEVEL_BINS = 2 * LEVEL_K + 1;
constexpr int LEVEL_ROWS = 16;     // rows of a frame per workgroup (960x540: 34 workgroups per frame, 3.75 items per lane)
constexpr int LEVEL_THREADS = 256;
#ifdef VSTAB_LEVEL_ONE_COPY      // (a build flag for the A/B of DESIGN 8o: one histogram per workgroup instead of one per wave)
constexpr int LEVEL_COPIES = 1;
#else
constexpr int LEVEL_COPIES = LEVEL_THREADS / 64;
#endif

// floor(num / den) for 0 <= num < 2^24, 0 < den < 2^24 and a quotient below 2^10: both convert to float exactly, v_rcp_f32 is
// within 1 ulp, so the product is within 1 of the quotient and one step either way makes it exact.
__device__ __forceinline__ unsigned div_small(unsigned num, unsigned den)
{
    unsigned q = (unsigned)((float)num * __builtin_amdgcn_rcpf((float)den));
    const int r = (int)num - (int)(q * den);
    if (r < 0) q -= 1u;
    else if ((unsigned)r >= den) q += 1u;
    return q;
}

// a lane's run of equal bins, and where it goes when the bin changes
struct Run {
    int bin = -1;
    unsigned long long mass = 0ull;

    __device__ __forceinline__ void flush(unsigned long long* hist)
    {
        if (bin >= 0) atomicAdd(&hist[bin], mass);
    }
    __device__ __forceinline__ void add(int b, unsigned m2, unsigned long long* hist)
    {
        if (b != bin) {
            flush(hist);
            bin = b;
            mass = 0ull;
        }
        mass += m2;
    }
};

// VEC: w % 16 == 0 and the base 16-byte aligned (every row of every frame then is)
template <bool VEC>
__global__ __launch_bounds__(LEVEL_THREADS) void orientation_hist_kernel(const uint8_t* __restrict__ gray, int h, int w, int tiles,
                                                                         unsigned min_mag2, unsigned long long* __restrict__ hist)
{
    __shared__ unsigned long long s_hist[LEVEL_COPIES][LEVEL_BINS];
    for (int b = threadIdx.x; b < LEVEL_COPIES * LEVEL_BINS; b += LEVEL_THREADS) (&s_hist[0][0])[b] = 0ull;
    __syncthreads();
    unsigned long long* mine = s_hist[(threadIdx.x >> 6) % LEVEL_COPIES];

    const int frame = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - frame * tiles;
    const int y0 = max(1, tile * LEVEL_ROWS), y1 = min(h - 1, (tile + 1) * LEVEL_ROWS);   // rows [y0, y1) have both neighbours
    const int rows = max(0, y1 - y0);
    const uint8_t* __restrict__ img = gray + (size_t)frame * h * w;
    const int chunks = (w + 15) >> 4;                   // 16-pixel pieces of a row
    Run run;
    for (int item = threadIdx.x; item < rows * chunks; item += LEVEL_THREADS) {
        const int r = item / chunks, c = item - r * chunks;
        const int y = y0 + r, x0 = c << 4;
        // p[j][i]: the pixel at (x0 - 1 + i, y - 1 + j); 0 where that is outside the row (never used: see the x range below)
        int p[3][18];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const uint8_t* __restrict__ row = img + (size_t)(y - 1 + j) * w;
            if (VEC) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + x0);
                const unsigned word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 16; i++) p[j][i + 1] = (int)((word[i >> 2] >> ((i & 3) * 8)) & 0xffu);
                p[j][0] = x0 > 0 ? (int)row[x0 - 1] : 0;
                p[j][17] = x0 + 16 < w ? (int)row[x0 + 16] : 0;
            } else {
#pragma unroll
                for (int i = 0; i < 18; i++) {
                    const int x = x0 - 1 + i;
                    p[j][i] = (x >= 0 && x < w) ? (int)row[x] : 0;
                }
            }
        }
#pragma unroll
        for (int i = 1; i <= 16; i++) {
            const int x = x0 + i - 1;
            if (x < 1 || x > w - 2) continue;
            const int gx = 3 * (p[0][i + 1] - p[0][i - 1]) + 10 * (p[1][i + 1] - p[1][i - 1]) + 3 * (p[2][i + 1] - p[2][i - 1]);
            const int gy = 3 * (p[2][i - 1] - p[0][i - 1]) + 10 * (p[2][i] - p[0][i]) + 3 * (p[2][i + 1] - p[0][i + 1]);
            const unsigned m2 = (unsigned)(gx * gx + gy * gy);      // <= 2 * 4080^2
            if (m2 == 0u || m2 < min_mag2) continue;
            const unsigned a = (unsigned)abs(gx), b = (unsigned)abs(gy);
            const unsigned lo = min(a, b), hi = max(a, b);          // hi > 0
            const int j = (int)div_small(2u * LEVEL_K * lo + hi, 2u * hi);   // 0 .. K
            const bool negative = ((gx ^ gy) < 0) != (a < b);       // sign(gx * gy) * (a >= b ? 1 : -1) < 0; j == 0 where a product is 0
            run.add(LEVEL_K + (negative ? -j : j), m2, mine);
        }
    }
    run.flush(mine);
    __syncthreads();
    unsigned long long* __restrict__ out = hist + (size_t)frame * LEVEL_BINS;
    for (int b = threadIdx.x; b < LEVEL_BINS; b += LEVEL_THREADS) {
        unsigned long long s = 0ull;
#pragma unroll
        for (int k = 0; k < LEVEL_COPIES; k++) s += s_hist[k][b];
        if (s) atomicAdd(&out[b], s);
    }
}

}  // namespace

extern "C" int vstab_orientation_hist_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, uint32_t min_mag2, uint64_t* hist)
{
    const char* who = "vstab_orientation_hist_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(gray != nullptr && hist != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(((uintptr_t)hist & 7) == 0, "%s: hist is not aligned to 8 bytes", who);
    VSTAB_REQUIRE(w <= 32768 && h <= 32768, "%s: %d x %d pixels, the limit is 32768 per axis", who, w, h);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    const int tiles = (h + LEVEL_ROWS - 1) / LEVEL_ROWS;
    VSTAB_REQUIRE((long long)n * tiles < 0x7fffffffLL, "%s: n=%d frames exceed the grid", who, n);
    VSTAB_HIP(hipSetDevice(ctx->device));
    VSTAB_HIP(hipMemsetAsync(hist, 0, (size_t)n * LEVEL_BINS * sizeof(uint64_t), ctx->stream));
    if (h < 3 || w < 3) return 0;      // no pixel has all eight neighbours
    KernelTimer timer(ctx, "orientation_hist");
    const bool vec = (w % 16 == 0) && (reinterpret_cast<uintptr_t>(gray) % 16 == 0);
    const dim3 grid((unsigned)(n * tiles)), block(LEVEL_THREADS);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(hist);
    if (vec) hipLaunchKernelGGL(orientation_hist_kernel<true>, grid, block, 0, ctx->stream, gray, h, w, tiles, (unsigned)min_mag2, out);
    else hipLaunchKernelGGL(orientation_hist_kernel<false>, grid, block, 0, ctx->stream, gray, h, w, tiles, (unsigned)min_mag2, out);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
