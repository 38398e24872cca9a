// vstab_subject.hip -- subject lock: count, coordinate sums and bounding box of a mask's subject pixels, per frame, as exact
// integers (the rule: include/vstab.h, vstab_mask_moments_batch).
//
//   moments_preset_kernel  the call presets its own outputs: sums 0, bbox four times 0xFFFFFFFF (== -1)
//   mask_moments_kernel    one launch over all frames: per thread -> wave shuffle -> LDS -> one set of atomics per workgroup
//                          and frame (three 64-bit adds, two unsigned minima, two signed maxima), skipped when the workgroup
//                          counted nothing
// Shaped as frame_sse_kernel is (vstab_stability.hip): a frame is read as the flat float array it is, in tiles of
// 4096 floats, consecutive lanes on consecutive float4s (four per thread and tile) behind a head of 0..3 floats where the
// frame does not start on a 16-byte boundary (frame k of a clip whose h*w is no multiple of 4), up to 3 tail floats; head and
// tail go one by one by the frame's first workgroup.  (x, y) of a float4's first pixel come from one division per vector,
// the other three by stepping with wrap.
// The float4 loads are non-temporal: the mask is read once by this pass, and measured against plain loads they are about a
// tenth faster (profiles/r15_subject_lock.md).  VSTAB_MASK_MOMENTS_PLAIN (a build flag) restores plain loads for
// that A/B.
#include "vstab_internal.h"

namespace {

typedef float mm_f4 __attribute__((ext_vector_type(4)));

constexpr int MM_THREADS = 256;
constexpr unsigned MM_TILE_VECS = 1024;               // 4096 floats = 16 KiB, four float4 per thread
constexpr unsigned MM_TARGET_BLOCKS = 4096;           // 256 CUs x 8 workgroups x 2: the rest is a grid-stride loop per frame

__device__ __forceinline__ mm_f4 mm_load(const mm_f4* p)
{
#ifdef VSTAB_MASK_MOMENTS_PLAIN
    return *p;
#else
    return __builtin_nontemporal_load(p);
#endif
}

// what one thread (then one wave, then one workgroup) knows of its frame
struct Moments {
    unsigned long long count, sum_x, sum_y;
    unsigned x0, y0;   // unsigned minima
    int x1, y1;        // signed maxima

    __device__ __forceinline__ void pixel(float m, unsigned x, unsigned y)
    {
        if (m > 0.5f) {   // false for a NaN, true for +inf
            count += 1ull;
            sum_x += x;
            sum_y += y;
            x0 = min(x0, x);
            y0 = min(y0, y);
            x1 = max(x1, (int)x);
            y1 = max(y1, (int)y);
        }
    }
    __device__ __forceinline__ void merge(const Moments& o)
    {
        count += o.count;
        sum_x += o.sum_x;
        sum_y += o.sum_y;
        x0 = min(x0, o.x0);
        y0 = min(y0, o.y0);
        x1 = max(x1, o.x1);
        y1 = max(y1, o.y1);
    }
};

__device__ __forceinline__ Moments moments_empty() { return Moments{0ull, 0ull, 0ull, 0xFFFFFFFFu, 0xFFFFFFFFu, -1, -1}; }

__global__ void moments_preset_kernel(unsigned long long* __restrict__ sums, unsigned* __restrict__ bbox, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // one of the n * 4 bbox words; the first n * 3 also zero a sum
    if (i < n * 4) bbox[i] = 0xFFFFFFFFu;
    if (i < n * 3) sums[i] = 0ull;
}

// grid (blocks_per_frame * n), 256 threads; px = h * w < 2^31, w, h <= 32768
__global__ __launch_bounds__(MM_THREADS) void mask_moments_kernel(const float* __restrict__ mask, unsigned px, unsigned w,
                                                                  unsigned blocks_per_frame, unsigned long long* __restrict__ sums,
                                                                  unsigned* __restrict__ bbox)
{
    __shared__ Moments wave_part[MM_THREADS / 64];
    const unsigned t = threadIdx.x;
    const unsigned frame = blockIdx.x / blocks_per_frame, slot = blockIdx.x - frame * blocks_per_frame;
    const float* f = mask + (size_t)frame * px;

    Moments m = moments_empty();
    // ---- aligned float4 loads behind a head of 0..3 floats ----
    const unsigned head = (4u - (unsigned)(((uintptr_t)f >> 2) & 3)) & 3u;
    const unsigned vecs = px > head ? (px - head) >> 2 : 0u;
    const mm_f4* v4 = reinterpret_cast<const mm_f4*>(f + head);
    const unsigned tiles = (vecs + MM_TILE_VECS - 1) / MM_TILE_VECS;
    for (unsigned tile = slot; tile < tiles; tile += blocks_per_frame) {
        const unsigned v0 = tile * MM_TILE_VECS;
        mm_f4 val[MM_TILE_VECS / MM_THREADS];
#pragma unroll
        for (unsigned r = 0; r < MM_TILE_VECS / MM_THREADS; r++) {   // the tile's loads first, then the arithmetic
            const unsigned v = v0 + t + r * MM_THREADS;
            val[r] = v < vecs ? mm_load(v4 + v) : mm_f4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (unsigned r = 0; r < MM_TILE_VECS / MM_THREADS; r++) {
            const unsigned v = v0 + t + r * MM_THREADS;
            if (v >= vecs) break;
            const unsigned p = head + 4u * v;     // the float4's first pixel; p + 3 < px
            unsigned y = p / w, x = p - y * w;
            m.pixel(val[r].x, x, y);
            if (++x == w) { x = 0u; y++; }
            m.pixel(val[r].y, x, y);
            if (++x == w) { x = 0u; y++; }
            m.pixel(val[r].z, x, y);
            if (++x == w) { x = 0u; y++; }
            m.pixel(val[r].w, x, y);
        }
    }
    // the floats in front of and behind the float4s: at most 6, by the frame's first workgroup
    if (slot == 0 && t < 6) {
        const unsigned tail0 = head + 4u * vecs;
        const unsigned p = t < 3 ? t : tail0 + (t - 3);
        const bool mine = t < 3 ? (t < head && p < px) : (p < px);
        if (mine) {
            const unsigned y = p / w;
            m.pixel(f[p], p - y * w, y);
        }
    }

    // wave shuffle, LDS over the four waves, one set of atomics per workgroup -- none if it counted nothing
    for (int s = 32; s > 0; s >>= 1) {
        Moments o;
        o.count = __shfl_down(m.count, s, 64);
        o.sum_x = __shfl_down(m.sum_x, s, 64);
        o.sum_y = __shfl_down(m.sum_y, s, 64);
        o.x0 = __shfl_down(m.x0, s, 64);
        o.y0 = __shfl_down(m.y0, s, 64);
        o.x1 = __shfl_down(m.x1, s, 64);
        o.y1 = __shfl_down(m.y1, s, 64);
        m.merge(o);
    }
    if ((t & 63) == 0) wave_part[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
        m.merge(wave_part[1]);
        m.merge(wave_part[2]);
        m.merge(wave_part[3]);
        if (m.count) {
            unsigned long long* s = sums + (size_t)frame * 3;
            unsigned* b = bbox + (size_t)frame * 4;
            atomicAdd(&s[0], m.count);
            atomicAdd(&s[1], m.sum_x);
            atomicAdd(&s[2], m.sum_y);
            atomicMin(&b[0], m.x0);
            atomicMin(&b[1], m.y0);
            atomicMax(reinterpret_cast<int*>(&b[2]), m.x1);
            atomicMax(reinterpret_cast<int*>(&b[3]), m.y1);
        }
    }
}

}  // namespace

extern "C" int vstab_mask_moments_batch(vstab_ctx* ctx, const float* mask, int n, int h, int w, uint64_t* sums, int32_t* bbox)
{
    const char* who = "vstab_mask_moments_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(mask != nullptr && sums != nullptr && bbox != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(w <= 32768 && h <= 32768, "%s: %d x %d pixels, the limit is 32768 per axis", who, w, h);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE(((uintptr_t)mask & 3) == 0 && ((uintptr_t)sums & 7) == 0 && ((uintptr_t)bbox & 3) == 0,
                  "%s: a pointer argument is not aligned to its element size", who);
    VSTAB_REQUIRE(n <= 0x7fffffff / 4, "%s: n=%d frames exceed the preset grid", who, n);

    const unsigned px = (unsigned)((long long)h * w);
    // workgroups per frame: a tile each at most, and no more over all frames than keep every CU busy (the rest is the kernel's loop)
    size_t tiles = ((size_t)(px >> 2) + MM_TILE_VECS - 1) / MM_TILE_VECS;
    if (tiles < 1) tiles = 1;   // (a frame of fewer than 4 pixels is head and tail alone)
    size_t per_frame = (MM_TARGET_BLOCKS + (size_t)n - 1) / (size_t)n;
    if (per_frame > tiles) per_frame = tiles;
    VSTAB_REQUIRE(per_frame * (size_t)n <= 0x7fffffffull, "%s: n=%d frames exceed the grid", who, n);

    VSTAB_HIP(hipSetDevice(ctx->device));
    KernelTimer timer(ctx, "mask_moments");
    unsigned long long* sums_dev = reinterpret_cast<unsigned long long*>(sums);
    unsigned* bbox_dev = reinterpret_cast<unsigned*>(bbox);
    hipLaunchKernelGGL(moments_preset_kernel, dim3((unsigned)((n * 4 + 255) / 256)), dim3(256), 0, ctx->stream, sums_dev, bbox_dev, n);
    hipLaunchKernelGGL(mask_moments_kernel, dim3((unsigned)(per_frame * (size_t)n)), dim3(MM_THREADS), 0, ctx->stream, mask, px,
                       (unsigned)w, (unsigned)per_frame, sums_dev, bbox_dev);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
