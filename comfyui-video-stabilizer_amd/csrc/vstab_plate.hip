// vstab_plate.hip -- clean plate: the per-pixel temporal median of a registered shot (vstab_plate_median_batch), the fill of
// what is still padding from it (vstab_plate_fill_batch) and the difference matte (vstab_plate_matte_batch).  Not a reference
// feature; the three rules are stated in include/vstab.h.
//
//   plate_median_reg_kernel<CAP>   rows of up to CAP = 4 / 8 / 16 / 32 / 64 samples: a lane takes one flat element of [h, w, 3], its
//                                  samples' order keys stay in registers (fully unrolled), consecutive lanes load consecutive
//                                  floats of one frame
//   plate_median_lds_kernel<CAP>   rows of up to CAP = 128 / 256 samples: a workgroup takes 64 flat elements, wave k loads
//                                  the samples k, k + 4, ... (256 contiguous bytes per load instruction) and stages their keys in
//                                  LDS as [sample][element]; then 16 lanes x 4 quarters of the samples work on every element
//   plate_fill_kernel<VEC>, plate_matte_kernel<VEC>   streaming, shaped as apply_gain_kernel's launch: workgroups per frame, a
//                                  lane takes 4 whole pixels with 16-byte accesses (VEC) or one pixel
// Both median kernels select by the same rule: the key of rank r is the largest v with #{key < v} <= r, built from the top
// bit down (32 counting passes over the samples).  A sample that is not valid is staged as the largest key, where it cannot
// be reached: r < count.  No arithmetic touches a value, so nothing here depends on -ffp-contract.
#include "vstab_internal.h"

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_TILE = 64;                      // flat elements per workgroup of the LDS form
constexpr unsigned PL_TOP = 0xFFFFFFFFu;         // the key of every NaN and of every sample that is not valid
constexpr unsigned PL_TARGET_BLOCKS = 4096;      // fill / matte: over all frames; beyond it a workgroup's loop takes the rest

// the order key of a float32: -0.0f below +0.0f (the mask hand-off's order, as an unsigned number), every NaN on top
__device__ __forceinline__ unsigned pl_key(float v)
{
    const unsigned b = __float_as_uint(v);
    return (v != v) ? PL_TOP : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
}
__device__ __forceinline__ float pl_unkey(unsigned k)
{
    return __uint_as_float(k == PL_TOP ? 0x7FC00000u : ((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k));
}
// the stability report's convention; a NaN is not valid
__device__ __forceinline__ bool pl_valid(float m) { return m <= 0.5f; }

struct PlateArgs {
    const float* frames;
    const float* mask;        // or nullptr
    const int* tab;           // [shots, S]
    float* plate;
    int* count;
    size_t elems;             // h * w * 3
    size_t px;                // h * w
    int S;                    // row pitch of tab
    int cols;                 // the widest row: columns behind it hold -1 everywhere
    unsigned tiles_per_shot;
};

// grid (tiles_per_shot * shots); a lane per flat element
template <int CAP>
__global__ __launch_bounds__(PL_THREADS) void plate_median_reg_kernel(PlateArgs a)
{
    const unsigned shot = blockIdx.x / a.tiles_per_shot, tile = blockIdx.x - shot * a.tiles_per_shot;
    const size_t e = (size_t)tile * PL_THREADS + threadIdx.x;
    if (e >= a.elems) return;
    const size_t p = e / 3;
    const int* __restrict__ row = a.tab + (size_t)shot * a.S;
    unsigned key[CAP];
    unsigned cnt = 0u;
#pragma unroll
    for (int j = 0; j < CAP; j++) {
        const int f = j < a.cols ? row[j] : -1;       // uniform
        unsigned k = PL_TOP;
        if (f >= 0) {
            const float v = a.frames[(size_t)f * a.elems + e];
            const bool ok = a.mask == nullptr || pl_valid(a.mask[(size_t)f * a.px + p]);
            if (ok) {
                k = pl_key(v);
                cnt += 1u;
            }
        }
        key[j] = k;
    }
    const unsigned rank = (cnt - 1u) >> 1;
    unsigned prefix = 0u;
    for (int b = 31; b >= 0; b--) {
        const unsigned cand = prefix | (1u << b);
        unsigned below = 0u;
#pragma unroll
        for (int j = 0; j < CAP; j++) below += key[j] < cand ? 1u : 0u;
        if (below <= rank) prefix = cand;
    }
    a.plate[(size_t)shot * a.elems + e] = cnt ? pl_unkey(prefix) : 0.0f;
    if (e == 3 * p) a.count[(size_t)shot * a.px + p] = (int)cnt;
}

// grid (tiles_per_shot * shots); a workgroup per PL_TILE flat elements.  LDS: CAP rows of 64 keys (64 KiB at CAP = 256) and the
// four waves' valid counts: two workgroups per CU stay resident at CAP = 256, four at CAP = 128.  Row j is rotated by 16 columns
// where j is odd: the 16 lanes of quarter q read row j = q (mod 4), so the two quarters of a ds_read_b32's 32-lane group hit
// the two halves of the 32 banks.
template <int CAP>
__global__ __launch_bounds__(PL_THREADS) void plate_median_lds_kernel(PlateArgs a)
{
    __shared__ unsigned s_key[CAP * PL_TILE];
    __shared__ unsigned s_cnt[4][PL_TILE];
    const unsigned t = threadIdx.x, l = t & 63u;
    const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane((int)(t >> 6));
    const unsigned shot = blockIdx.x / a.tiles_per_shot, tile = blockIdx.x - shot * a.tiles_per_shot;
    const size_t e0 = (size_t)tile * PL_TILE;
    const int* __restrict__ row = a.tab + (size_t)shot * a.S;
    const int rows = (a.cols + 3) & ~3;              // <= CAP: the host chose CAP >= cols, CAP % 4 == 0
    {
        const size_t e = e0 + l;
        const bool in = e < a.elems;
        const size_t p = in ? e / 3 : 0;
        unsigned cnt = 0u;
#pragma unroll 4
        for (int j = (int)w; j < rows; j += 4) {
            const int f = j < a.cols ? row[j] : -1;   // uniform over the wave
            unsigned k = PL_TOP;
            if (f >= 0 && in) {
                const float v = a.frames[(size_t)f * a.elems + e];
                const bool ok = a.mask == nullptr || pl_valid(a.mask[(size_t)f * a.px + p]);
                if (ok) {
                    k = pl_key(v);
                    cnt += 1u;
                }
            }
            s_key[j * PL_TILE + ((l + (((unsigned)j & 1u) << 4)) & 63u)] = k;
        }
        s_cnt[w][l] = cnt;
    }
    __syncthreads();
    const unsigned el = (w << 4) | (l & 15u), q = l >> 4;
    const unsigned cnt = s_cnt[0][el] + s_cnt[1][el] + s_cnt[2][el] + s_cnt[3][el];
    const unsigned rank = (cnt - 1u) >> 1;
    const unsigned* __restrict__ col = s_key + ((el + ((q & 1u) << 4)) & 63u);      // (j & 1 == q & 1 for every row of this lane)
    unsigned prefix = 0u;
    for (int b = 31; b >= 0; b--) {
        const unsigned cand = prefix | (1u << b);
        unsigned below = 0u;
#pragma unroll 8
        for (int j = (int)q; j < rows; j += 4) below += col[j * PL_TILE] < cand ? 1u : 0u;
        below += __shfl_xor(below, 16);
        below += __shfl_xor(below, 32);
        if (below <= rank) prefix = cand;
    }
    const size_t e = e0 + el;
    if (q == 0u && e < a.elems) {
        const size_t p = e / 3;
        a.plate[(size_t)shot * a.elems + e] = cnt ? pl_unkey(prefix) : 0.0f;
        if (e == 3 * p) a.count[(size_t)shot * a.px + p] = (int)cnt;
    }
}

// ---- fill and matte ------------------------------------------------------------------------------------------------------
// A lane's pixels: 4 (three float4 of colour, one of mask, one int4 of counts) or 1.  The four pixels of a lane lie in the
// three float4 a, b, c as  a.x a.y a.z | a.w b.x b.y | b.z b.w c.x | c.y c.z c.w.
struct PlPixels4 {
    float4 a, b, c;
};

// grid (per_frame * n); px = h * w < 2^31; VEC: px % 4 == 0 and every pointer is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(PL_THREADS) void plate_fill_kernel(float* __restrict__ dst, float* __restrict__ mask,
                                                                const float* __restrict__ plate, const int* __restrict__ count,
                                                                const int* __restrict__ shot_of, unsigned px, unsigned per_frame,
                                                                int min_count, unsigned* __restrict__ filled_out)
{
    const unsigned t = threadIdx.x;
    const unsigned frame = blockIdx.x / per_frame, slot = blockIdx.x - frame * per_frame;
    const int shot = shot_of ? shot_of[frame] : 0;
    float* __restrict__ f = dst + (size_t)frame * px * 3;
    float* __restrict__ m = mask + (size_t)frame * px;
    const float* __restrict__ pl = plate + (size_t)shot * px * 3;
    const int* __restrict__ cn = count + (size_t)shot * px;
    unsigned filled[1] = {0u};
    const unsigned groups = VEC ? px >> 2 : px;
    for (unsigned g = slot * PL_THREADS + t; g < groups; g += per_frame * PL_THREADS) {
        if (VEC) {
            float4 mk = reinterpret_cast<const float4*>(m)[g];
            const bool n0 = !pl_valid(mk.x), n1 = !pl_valid(mk.y), n2 = !pl_valid(mk.z), n3 = !pl_valid(mk.w);
            if (!(n0 || n1 || n2 || n3)) continue;           // nothing is padding: neither the plate nor the frame is read
            const int4 c = reinterpret_cast<const int4*>(cn)[g];
            const bool f0 = n0 && c.x >= min_count, f1 = n1 && c.y >= min_count, f2 = n2 && c.z >= min_count, f3 = n3 && c.w >= min_count;
            if (!(f0 || f1 || f2 || f3)) continue;
            float4* __restrict__ F = reinterpret_cast<float4*>(f) + (size_t)g * 3;
            const float4* __restrict__ P = reinterpret_cast<const float4*>(pl) + (size_t)g * 3;
            PlPixels4 x = {F[0], F[1], F[2]};
            const PlPixels4 y = {P[0], P[1], P[2]};
            if (f0) { x.a.x = y.a.x; x.a.y = y.a.y; x.a.z = y.a.z; mk.x = 0.0f; }
            if (f1) { x.a.w = y.a.w; x.b.x = y.b.x; x.b.y = y.b.y; mk.y = 0.0f; }
            if (f2) { x.b.z = y.b.z; x.b.w = y.b.w; x.c.x = y.c.x; mk.z = 0.0f; }
            if (f3) { x.c.y = y.c.y; x.c.z = y.c.z; x.c.w = y.c.w; mk.w = 0.0f; }
            filled[0] += (f0 ? 1u : 0u) + (f1 ? 1u : 0u) + (f2 ? 1u : 0u) + (f3 ? 1u : 0u);
            F[0] = x.a; F[1] = x.b; F[2] = x.c;
            reinterpret_cast<float4*>(m)[g] = mk;
        } else {
            if (pl_valid(m[g]) || cn[g] < min_count) continue;
            const size_t j = (size_t)g * 3;
            f[j] = pl[j]; f[j + 1] = pl[j + 1]; f[j + 2] = pl[j + 2];
            m[g] = 0.0f;
            filled[0] += 1u;
        }
    }
    if (filled_out != nullptr) block_count_add<1>(filled, {filled_out}, (int)frame);
}

// one pixel of the matte rule: own, counted, and some channel differs (a NaN on either side differs)
__device__ __forceinline__ bool pl_matte(bool own, int c, int min_count, float f0, float f1, float f2, float p0, float p1, float p2,
                                         float thr)
{
    const bool same = __builtin_fabsf(f0 - p0) <= thr && __builtin_fabsf(f1 - p1) <= thr && __builtin_fabsf(f2 - p2) <= thr;
    return own && c >= min_count && !same;
}

template <bool VEC>
__global__ __launch_bounds__(PL_THREADS) void plate_matte_kernel(const float* __restrict__ frames, const float* __restrict__ mask,
                                                                 const float* __restrict__ plate, const int* __restrict__ count,
                                                                 const int* __restrict__ shot_of, unsigned px, unsigned per_frame,
                                                                 float thr, int min_count, float* __restrict__ matte,
                                                                 unsigned* __restrict__ matte_out)
{
    const unsigned t = threadIdx.x;
    const unsigned frame = blockIdx.x / per_frame, slot = blockIdx.x - frame * per_frame;
    const int shot = shot_of ? shot_of[frame] : 0;
    const float* __restrict__ f = frames + (size_t)frame * px * 3;
    const float* __restrict__ m = mask ? mask + (size_t)frame * px : nullptr;
    const float* __restrict__ pl = plate + (size_t)shot * px * 3;
    const int* __restrict__ cn = count + (size_t)shot * px;
    float* __restrict__ out = matte + (size_t)frame * px;
    unsigned marked[1] = {0u};
    const unsigned groups = VEC ? px >> 2 : px;
    for (unsigned g = slot * PL_THREADS + t; g < groups; g += per_frame * PL_THREADS) {
        if (VEC) {
            const float4 mk = m ? reinterpret_cast<const float4*>(m)[g] : make_float4(0.f, 0.f, 0.f, 0.f);
            const int4 c = reinterpret_cast<const int4*>(cn)[g];
            const float4* __restrict__ F = reinterpret_cast<const float4*>(f) + (size_t)g * 3;
            const float4* __restrict__ P = reinterpret_cast<const float4*>(pl) + (size_t)g * 3;
            const PlPixels4 x = {F[0], F[1], F[2]}, y = {P[0], P[1], P[2]};
            const bool s0 = pl_matte(pl_valid(mk.x), c.x, min_count, x.a.x, x.a.y, x.a.z, y.a.x, y.a.y, y.a.z, thr);
            const bool s1 = pl_matte(pl_valid(mk.y), c.y, min_count, x.a.w, x.b.x, x.b.y, y.a.w, y.b.x, y.b.y, thr);
            const bool s2 = pl_matte(pl_valid(mk.z), c.z, min_count, x.b.z, x.b.w, x.c.x, y.b.z, y.b.w, y.c.x, thr);
            const bool s3 = pl_matte(pl_valid(mk.w), c.w, min_count, x.c.y, x.c.z, x.c.w, y.c.y, y.c.z, y.c.w, thr);
            reinterpret_cast<float4*>(out)[g] = make_float4(s0 ? 1.f : 0.f, s1 ? 1.f : 0.f, s2 ? 1.f : 0.f, s3 ? 1.f : 0.f);
            marked[0] += (s0 ? 1u : 0u) + (s1 ? 1u : 0u) + (s2 ? 1u : 0u) + (s3 ? 1u : 0u);
        } else {
            const size_t j = (size_t)g * 3;
            const bool s = pl_matte(m == nullptr || pl_valid(m[g]), cn[g], min_count, f[j], f[j + 1], f[j + 2], pl[j], pl[j + 1], pl[j + 2], thr);
            out[g] = s ? 1.f : 0.f;
            marked[0] += s ? 1u : 0u;
        }
    }
    if (matte_out != nullptr) block_count_add<1>(marked, {matte_out}, (int)frame);
}

// What fill and matte check alike, and their launch geometry.  *d_shot: the staged shot table, or nullptr for one shot.
int plate_stream_prepare(vstab_ctx* ctx, const char* who, int n, int h, int w, const void* const* ptrs, int nptrs, const int32_t* shot,
                         int shots, int min_count, uint32_t* counter, const int** d_shot, unsigned* per_frame, bool* vec)
{
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(shots >= 1, "%s: shots=%d, at least one is needed", who, shots);
    uintptr_t bits = (uintptr_t)counter;
    for (int k = 0; k < nptrs; k++) {
        VSTAB_REQUIRE(ptrs[k] != nullptr, "%s: NULL pointer argument", who);
        bits |= (uintptr_t)ptrs[k];
    }
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE((bits & 3) == 0, "%s: a pointer argument is not aligned to its element size", who);
    VSTAB_REQUIRE(min_count >= 1 && min_count <= VSTAB_PLATE_SAMPLES_MAX, "%s: min_count=%d outside 1..%d", who, min_count,
                  VSTAB_PLATE_SAMPLES_MAX);
    if (shot != nullptr) {
        for (int k = 0; k < n; k++) {
            VSTAB_REQUIRE(shot[k] >= 0 && shot[k] < shots, "%s: shot[%d]=%d outside 0..%d", who, k, shot[k], shots - 1);
            VSTAB_REQUIRE(k == 0 || shot[k] >= shot[k - 1], "%s: shot is not non-decreasing at frame %d", who, k);
        }
    }
    const unsigned px = (unsigned)((long long)h * w);
    *vec = (px & 3u) == 0u && (bits & 15) == 0;
    const size_t groups = *vec ? px >> 2 : px;
    size_t pf = (PL_TARGET_BLOCKS + (size_t)n - 1) / (size_t)n;
    const size_t tiles = (groups + PL_THREADS - 1) / PL_THREADS;
    if (pf > tiles) pf = tiles;
    VSTAB_REQUIRE(pf * (size_t)n <= 0x7fffffffull, "%s: n=%d frames exceed the grid", who, n);
    *per_frame = (unsigned)pf;
    VSTAB_HIP(hipSetDevice(ctx->device));
    if (counter != nullptr) VSTAB_HIP(hipMemsetAsync(counter, 0, (size_t)n * sizeof(uint32_t), ctx->stream));
    *d_shot = nullptr;
    if (shot != nullptr) {
        void* d = nullptr;
        if (int rc = vstab_stage_params(ctx, shot, (size_t)n * sizeof(int32_t), &d)) return rc;
        *d_shot = static_cast<const int*>(d);
    }
    return 0;
}

}  // namespace

extern "C" int vstab_plate_median_batch(vstab_ctx* ctx, const float* frames, const float* mask, int n, int h, int w,
                                        const int32_t* sample_frame, int shots, int S, float* plate, int32_t* count)
{
    const char* who = "vstab_plate_median_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(shots >= 1, "%s: shots=%d, at least one is needed", who, shots);
    VSTAB_REQUIRE(S >= 1 && S <= VSTAB_PLATE_SAMPLES_MAX, "%s: S=%d samples per shot outside 1..%d", who, S, VSTAB_PLATE_SAMPLES_MAX);
    VSTAB_REQUIRE(frames != nullptr && sample_frame != nullptr && plate != nullptr && count != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE((((uintptr_t)frames | (uintptr_t)mask | (uintptr_t)plate | (uintptr_t)count) & 3) == 0,
                  "%s: a pointer argument is not aligned to its element size", who);
    int cols = 0;
    for (int s = 0; s < shots; s++) {
        const int32_t* row = sample_frame + (size_t)s * S;
        VSTAB_REQUIRE(row[0] != -1, "%s: sample_frame row %d is empty", who, s);
        int len = 0;
        for (int j = 0; j < S; j++) {
            if (row[j] == -1) continue;
            VSTAB_REQUIRE(row[j] >= 0 && row[j] < n, "%s: sample_frame[%d][%d]=%d is not a frame index in 0..%d", who, s, j, row[j], n - 1);
            VSTAB_REQUIRE(len == j, "%s: sample_frame row %d holds the index %d behind its -1 padding", who, s, row[j]);
            VSTAB_REQUIRE(j == 0 || row[j] > row[j - 1], "%s: sample_frame row %d is not strictly increasing at column %d (%d after %d)",
                          who, s, j, row[j], row[j - 1]);
            len = j + 1;
        }
        if (len > cols) cols = len;
    }
    PlateArgs a;
    a.frames = frames;
    a.mask = mask;
    a.plate = plate;
    a.count = count;
    a.px = (size_t)h * w;
    a.elems = a.px * 3;
    a.S = S;
    a.cols = cols;
    const bool reg = cols <= VSTAB_PLATE_REGISTER_MAX;
    const size_t tile = reg ? PL_THREADS : PL_TILE;
    const size_t tiles = (a.elems + tile - 1) / tile;
    VSTAB_REQUIRE(tiles * (size_t)shots <= 0x7fffffffull, "%s: %d shots of %d x %d pixels exceed the grid", who, shots, w, h);
    a.tiles_per_shot = (unsigned)tiles;
    VSTAB_HIP(hipSetDevice(ctx->device));
    void* d_tab = nullptr;
    if (int rc = vstab_stage_params(ctx, sample_frame, (size_t)shots * S * sizeof(int32_t), &d_tab)) return rc;
    a.tab = static_cast<const int*>(d_tab);
    const dim3 grid((unsigned)(tiles * (size_t)shots)), block(PL_THREADS);
    KernelTimer timer(ctx, "plate_median");
    if (cols <= 4) hipLaunchKernelGGL(plate_median_reg_kernel<4>, grid, block, 0, ctx->stream, a);
    else if (cols <= 8) hipLaunchKernelGGL(plate_median_reg_kernel<8>, grid, block, 0, ctx->stream, a);
    else if (cols <= 16) hipLaunchKernelGGL(plate_median_reg_kernel<16>, grid, block, 0, ctx->stream, a);
    else if (cols <= 32) hipLaunchKernelGGL(plate_median_reg_kernel<32>, grid, block, 0, ctx->stream, a);
    else if (reg) hipLaunchKernelGGL(plate_median_reg_kernel<VSTAB_PLATE_REGISTER_MAX>, grid, block, 0, ctx->stream, a);
    else if (cols <= 128) hipLaunchKernelGGL(plate_median_lds_kernel<128>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(plate_median_lds_kernel<VSTAB_PLATE_SAMPLES_MAX>, grid, block, 0, ctx->stream, a);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

extern "C" int vstab_plate_fill_batch(vstab_ctx* ctx, float* dst, float* mask, int n, int h, int w, const float* plate,
                                      const int32_t* count, const int32_t* shot, int shots, int min_count, uint32_t* filled_count)
{
    const char* who = "vstab_plate_fill_batch";
    const void* ptrs[] = {dst, mask, plate, count};
    const int* d_shot = nullptr;
    unsigned per_frame = 0;
    bool vec = false;
    if (int rc = plate_stream_prepare(ctx, who, n, h, w, ptrs, 4, shot, shots, min_count, filled_count, &d_shot, &per_frame, &vec)) return rc;
    const unsigned px = (unsigned)((long long)h * w);
    const dim3 grid(per_frame * (unsigned)n), block(PL_THREADS);
    KernelTimer timer(ctx, "plate_fill");
    if (vec) hipLaunchKernelGGL(plate_fill_kernel<true>, grid, block, 0, ctx->stream, dst, mask, plate, count, d_shot, px, per_frame, min_count, filled_count);
    else hipLaunchKernelGGL(plate_fill_kernel<false>, grid, block, 0, ctx->stream, dst, mask, plate, count, d_shot, px, per_frame, min_count, filled_count);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

extern "C" int vstab_plate_matte_batch(vstab_ctx* ctx, const float* frames, const float* mask, int n, int h, int w, const float* plate,
                                       const int32_t* count, const int32_t* shot, int shots, float threshold, int min_count,
                                       float* matte, uint32_t* matte_count)
{
    const char* who = "vstab_plate_matte_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(threshold >= 0.0f && threshold <= 3.4028234663852886e38f, "%s: threshold=%g is not finite and >= 0", who, (double)threshold);
    VSTAB_REQUIRE((((uintptr_t)mask) & 3) == 0, "%s: a pointer argument is not aligned to its element size", who);
    const void* ptrs[] = {frames, plate, count, matte};
    const int* d_shot = nullptr;
    unsigned per_frame = 0;
    bool vec = false;
    if (int rc = plate_stream_prepare(ctx, who, n, h, w, ptrs, 4, shot, shots, min_count, matte_count, &d_shot, &per_frame, &vec)) return rc;
    vec = vec && (((uintptr_t)mask) & 15) == 0;
    const unsigned px = (unsigned)((long long)h * w);
    if (!vec) {   // the geometry of the one-pixel form
        size_t pf = (PL_TARGET_BLOCKS + (size_t)n - 1) / (size_t)n;
        const size_t tiles = ((size_t)px + PL_THREADS - 1) / PL_THREADS;
        per_frame = (unsigned)(pf > tiles ? tiles : pf);
    }
    const dim3 grid(per_frame * (unsigned)n), block(PL_THREADS);
    KernelTimer timer(ctx, "plate_matte");
    if (vec) hipLaunchKernelGGL(plate_matte_kernel<true>, grid, block, 0, ctx->stream, frames, mask, plate, count, d_shot, px, per_frame, threshold, min_count, matte, matte_count);
    else hipLaunchKernelGGL(plate_matte_kernel<false>, grid, block, 0, ctx->stream, frames, mask, plate, count, d_shot, px, per_frame, threshold, min_count, matte, matte_count);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
