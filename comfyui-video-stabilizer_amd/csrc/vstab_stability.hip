// vstab_stability.hip -- masked squared error between frames as exact integers (the rule: include/vstab.h).
//
//   sse_zero_kernel   the call zeroes its own outputs (one launch instead of two fills on the stream)
//   frame_sse_kernel  one launch over all pairs: per thread -> two BlockSums (vstab_internal.h) behind one barrier -> one
//                     64-bit and one 32-bit atomic per workgroup and pair, skipped when the workgroup counted nothing
// A frame is read as the flat float array it is, in tiles of 3072 floats (1024 pixels), so that consecutive lanes load
// consecutive addresses whatever the pixel stride (the warp kernel's lesson): float4 per lane where frame a[k] and
// frame b[k] sit at the same offset from a 16-byte boundary (up to 3 head and 3 tail floats go one by one), one float per
// lane where they do not (frame k >= 1 of a clip whose frame size is no multiple of 16 bytes, compared with its neighbour).
#include "vstab_internal.h"

namespace {

constexpr int SSE_THREADS = 256;
constexpr unsigned SSE_TILE_FLOATS = 3072;            // 1024 pixels: 768 float4, three per thread
constexpr unsigned SSE_TILE_VECS = SSE_TILE_FLOATS / 4;
constexpr unsigned SSE_TILE_PIXELS = SSE_TILE_FLOATS / 3;
constexpr unsigned SSE_TARGET_BLOCKS = 4096;          // 256 CUs x 8 workgroups x 2: the rest is a grid-stride loop per pair

__device__ __forceinline__ bool sse_valid(const float* mask, size_t p) { return mask == nullptr || mask[p] <= 0.5f; }

// one channel of one counting pixel: d in float32, the square in fp64 (exact), capped at 4, scaled by 2^32 (exact), truncated
__device__ __forceinline__ unsigned long long sse_term(float x, float y)
{
    const float d = x - y;
    double e = (double)d * (double)d;
    e = (e < 4.0) ? e : 4.0;             // a NaN or inf difference takes the cap
    return (unsigned long long)(e * 4294967296.0);
}

__global__ void sse_zero_kernel(unsigned long long* __restrict__ sse, unsigned* __restrict__ count, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        sse[i] = 0ull;
        count[i] = 0u;
    }
}

// grid (blocks_per_pair * n), 256 threads; px = h * w < 2^31
__global__ __launch_bounds__(SSE_THREADS) void frame_sse_kernel(const float* a, const float* mask_a, const float* b, const float* mask_b,
                                                                unsigned px, unsigned blocks_per_pair,
                                                                unsigned long long* __restrict__ sse_out, unsigned* __restrict__ count_out)
{
    __shared__ BlockSums<unsigned long long, 1, SSE_THREADS> s_sse;
    __shared__ BlockSums<unsigned, 1, SSE_THREADS> s_count;
    const unsigned t = threadIdx.x;
    const unsigned pair = blockIdx.x / blocks_per_pair, slot = blockIdx.x - pair * blocks_per_pair;
    const size_t floats = (size_t)px * 3;
    const float* fa = a + (size_t)pair * floats;
    const float* fb = b + (size_t)pair * floats;
    const float* ma = mask_a ? mask_a + (size_t)pair * px : nullptr;
    const float* mb = mask_b ? mask_b + (size_t)pair * px : nullptr;

    unsigned long long sse = 0ull;
    unsigned count = 0u;
    const unsigned ra = (unsigned)(((uintptr_t)fa >> 2) & 3), rb = (unsigned)(((uintptr_t)fb >> 2) & 3);
    if (ra == rb) {
        // ---- both frames at the same offset from a 16-byte boundary: aligned float4 loads behind a head of 0..3 floats ----
        const unsigned head = (4u - ra) & 3u;
        const unsigned vecs = floats > head ? (unsigned)((floats - head) >> 2) : 0u;   // < 3 * 2^29
        const float4* va = reinterpret_cast<const float4*>(fa + head);
        const float4* vb = reinterpret_cast<const float4*>(fb + head);
        const unsigned tiles = (vecs + SSE_TILE_VECS - 1) / SSE_TILE_VECS;
        for (unsigned tile = slot; tile < tiles; tile += blocks_per_pair) {
            const unsigned v0 = tile * SSE_TILE_VECS;
#pragma unroll
            for (unsigned r = 0; r < SSE_TILE_VECS / SSE_THREADS; r++) {
                const unsigned vl = t + r * SSE_THREADS;   // float4 within the tile
                if (v0 + vl >= vecs) break;
                // the float4 holds the floats head + 4 * (v0 + vl) + {0..3} of the frame: the last 3 - c0 channels of pixel
                // p0 and the first c0 + 1 of pixel p0 + 1
                const unsigned jl = head + 4u * vl;
                const unsigned pl = jl / 3u, c0 = jl - 3u * pl;
                const size_t p0 = (size_t)tile * SSE_TILE_PIXELS + pl;
                const float4 x = va[v0 + vl], y = vb[v0 + vl];
                const bool k0 = sse_valid(ma, p0) && sse_valid(mb, p0);
                const bool k1 = sse_valid(ma, p0 + 1) && sse_valid(mb, p0 + 1);   // (the float4's last float is of p0 + 1: inside)
                const unsigned split = 3u - c0;   // floats [0, split) are of p0; float `split` is channel 0 of p0 + 1
                const unsigned long long q0 = sse_term(x.x, y.x), q1 = sse_term(x.y, y.y), q2 = sse_term(x.z, y.z), q3 = sse_term(x.w, y.w);
                sse += k0 ? q0 : 0ull;
                sse += (split > 1u ? k0 : k1) ? q1 : 0ull;
                sse += (split > 2u ? k0 : k1) ? q2 : 0ull;
                sse += k1 ? q3 : 0ull;
                count += (c0 == 0u && k0) ? 1u : 0u;
                count += k1 ? 1u : 0u;
            }
        }
        // the floats in front of and behind the float4s: at most 6, by the pair's first workgroup
        if (slot == 0 && t < 6) {
            const size_t tail0 = (size_t)head + 4 * (size_t)vecs;
            const size_t j = t < 3 ? (size_t)t : tail0 + (t - 3);
            const bool mine = t < 3 ? (t < head && j < floats) : (j < floats);
            if (mine) {
                const size_t p = j / 3;
                if (sse_valid(ma, p) && sse_valid(mb, p)) {
                    sse += sse_term(fa[j], fb[j]);
                    count += (j - 3 * p == 0) ? 1u : 0u;
                }
            }
        }
    } else {
        // ---- the two frames sit at different offsets: one float per lane, consecutive lanes on consecutive floats ----
        const unsigned tiles = (unsigned)((floats + SSE_TILE_FLOATS - 1) / SSE_TILE_FLOATS);
        for (unsigned tile = slot; tile < tiles; tile += blocks_per_pair) {
            const size_t j0 = (size_t)tile * SSE_TILE_FLOATS;
#pragma unroll 4
            for (unsigned r = 0; r < SSE_TILE_FLOATS / SSE_THREADS; r++) {
                const unsigned jl = t + r * SSE_THREADS;
                if (j0 + jl >= floats) break;
                const unsigned pl = jl / 3u, c = jl - 3u * pl;
                const size_t p = (size_t)tile * SSE_TILE_PIXELS + pl;
                if (sse_valid(ma, p) && sse_valid(mb, p)) {
                    sse += sse_term(fa[j0 + jl], fb[j0 + jl]);
                    count += (c == 0u) ? 1u : 0u;
                }
            }
        }
    }

    // one pair of atomics per workgroup -- none if it counted nothing (its sum is 0 then)
    s_sse.put({sse});
    s_count.put({count});
    __syncthreads();
    if (t == 0) {
        const unsigned total = s_count.total(0);
        if (total) {
            atomicAdd(&sse_out[pair], s_sse.total(0));
            atomicAdd(&count_out[pair], total);
        }
    }
}

}  // namespace

extern "C" int vstab_frame_sse_batch(vstab_ctx* ctx, const float* a, const float* mask_a, const float* b, const float* mask_b,
                                     int n, int h, int w, uint64_t* sse, uint32_t* count)
{
    const char* who = "vstab_frame_sse_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(a != nullptr && b != nullptr && sse != nullptr && count != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)mask_a | (uintptr_t)mask_b) & 3) == 0 && ((uintptr_t)sse & 7) == 0 &&
                      ((uintptr_t)count & 3) == 0,
                  "%s: a pointer argument is not aligned to its element size", who);

    const unsigned px = (unsigned)((long long)h * w);
    const size_t floats = (size_t)px * 3;
    // workgroups per pair: a tile each at most, and no more over all pairs than keep every CU busy (the rest is the kernel's loop)
    const size_t tiles = (floats + SSE_TILE_FLOATS - 1) / SSE_TILE_FLOATS;
    size_t per_pair = (SSE_TARGET_BLOCKS + (size_t)n - 1) / (size_t)n;
    if (per_pair > tiles) per_pair = tiles;
    VSTAB_REQUIRE(per_pair * (size_t)n <= 0x7fffffffull, "%s: n=%d pairs exceed the grid", who, n);

    VSTAB_HIP(hipSetDevice(ctx->device));
    KernelTimer timer(ctx, "stability");
    unsigned long long* sse_dev = reinterpret_cast<unsigned long long*>(sse);
    hipLaunchKernelGGL(sse_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, sse_dev, count, n);
    hipLaunchKernelGGL(frame_sse_kernel, dim3((unsigned)(per_pair * (size_t)n)), dim3(SSE_THREADS), 0, ctx->stream, a, mask_a, b, mask_b,
                       px, (unsigned)per_pair, sse_dev, count);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
