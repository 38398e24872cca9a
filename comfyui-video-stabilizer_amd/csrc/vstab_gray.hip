// vstab_gray.hip -- F2: RGB f32 -> gray u8 (truncating) -> INTER_AREA downscale to the working size.
//
// Replaces nodes/stabilizer_utils.py:236-242 (_make_gray) and :271-276 (cv2.resize INTER_AREA).
// This is the only estimation-stage pass that touches full-resolution data: 24.9 MB read per
// 1080p frame, 0.5 MB written -> HBM-bound, one fused pass for the integer-ratio cases
// (1080p -> 960x540 is 2x2, 4K -> 960x540 is 4x4): a lane per source pixel column, see gray_area_int_kernel.
//
// Gray arithmetic follows OpenCV's RGB2Gray<float>: an 8-lane FMA body
// fma(b, 0.114, fma(g, 0.587, r*0.299)) and an unfused scalar tail for the last (w % 8) pixels
// of a row; then v = gray*255 (f32), clip to [0,255], truncate.
#include "vstab_internal.h"
#include "vstab_area.h"
#include "vstab_wait.h"
#include <algorithm>

namespace {

__device__ __forceinline__ int gray_u8(float r, float g, float b, bool fused)
{
    const float k0 = 0.299f, k1 = 0.587f, k2 = 0.114f;
    float y;
    if (fused) y = __builtin_fmaf(b, k2, __builtin_fmaf(g, k1, r * k0));
    else y = r * k0 + g * k1 + b * k2;
    float v = y * 255.0f;
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    return (int)v;
}

// Integer-ratio INTER_AREA (K x K boxes) fused with the gray conversion. K == 1: gray only.
// One workgroup per output row, one SOURCE pixel column per lane: a lane reads its pixel (12 B) from each of the K rows
// of the box and the K lanes of a box add up over DPP, so every load instruction of a wavefront covers 768 contiguous
// bytes with no holes.  The frames are read once and never again by this pass: non-temporal loads (measured on
// MI355X, profiles/r02_gray_forms.md: 256 x 1080p 1.09 -> 0.96 ms, 6.6 TB/s; 4K 0.82 -> 0.71 ms).  The launch picks a
// workgroup size that divides the row into whole passes (640 threads for 1920 and 3840 columns).
//
// RANGE: the same pass also yields the largest sample of the source rows it reads (NaN if they hold one, as numpy's
// max does) -- the value-range sniff of nodes/stabilizer_utils.py:127-131 (`float(arr.max()) > 1.5` per frame) --
// instead of a second 24.9 MB read per frame.  Every wavefront writes its own partial to
// row_max[((f * groups + g) * waves + wave)]: a DPP maximum (wave_max_lane63) and a ballot of the NaN flag, no LDS, no
// barrier; frame_max_kernel reduces the groups * waves partials of a frame.  Only valid when the K x K boxes tile the
// whole source (the host checks dh * K == sh and dw * K == sw).
// G: consecutive output rows of one frame that a workgroup walks (the last group of a frame may be shorter); the
// partial is then written once per G rows.
// Measured on MI355X, 256 x 1080p (profiles/r28_range_tail.md): the probe is 19 VALU instructions per loop trip (97
// against 78); stand-alone the sniff costs 0.03 ms (0.97-0.98 against 0.94 ms).  Inside the Flow step the RANGE pass with
// G = 2 takes 1.00-1.08 ms, 40-70 us less than the earlier tail (two shuffle chains, LDS, a barrier and thread 0's loop
// over the wavefronts, one row per workgroup); G = 2 is 16-50 us under G = 1 there and level with 4 and 6.  Without RANGE
// two rows per workgroup are slower than one (0.97 against 0.94 ms), so that instantiation runs with G = 1.
template <int K, bool RANGE, int G>
__global__ __launch_bounds__(1024) void gray_area_int_kernel(const float* __restrict__ frames, uint8_t* __restrict__ out,
                                                             int n, int sh, int sw, int dh, int dw, int body,
                                                             float* __restrict__ row_max)
{
    const int groups = (dh + G - 1) / G;
    const int g = (int)blockIdx.x % groups, f = (int)blockIdx.x / groups;
    const int y_end = (g * G + G < dh) ? g * G + G : dh;
    float vmax = -INFINITY;
    int has_nan = 0;
    const int used = dw * K;   // == sw on the fused path
    constexpr int U = 4 / K;   // columns per thread and pass: four 12-B loads in flight
    typedef float f3_t __attribute__((ext_vector_type(3), aligned(4)));
    int y = g * G;
    do {
        const float* rowbase = frames + ((size_t)f * sh + (size_t)y * K) * sw * 3;
        uint8_t* D = out + ((size_t)f * dh + y) * dw;
        for (int sx0 = threadIdx.x; sx0 < used; sx0 += U * blockDim.x) {
            f3_t px[U][K];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int sx = sx0 + u * blockDim.x;
                if (sx < used) {
#pragma unroll
                    for (int j = 0; j < K; j++)
                        px[u][j] = __builtin_nontemporal_load(reinterpret_cast<const f3_t*>(rowbase + (size_t)j * sw * 3 + (size_t)sx * 3));
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int sx = sx0 + u * blockDim.x;
                if (sx < used) {
                    const bool fused = sx < body;
                    int sum = 0;
#pragma unroll
                    for (int j = 0; j < K; j++) {
                        const float cr = px[u][j].x, cg = px[u][j].y, cb = px[u][j].z;
                        sum += gray_u8(cr, cg, cb, fused);
                        if (RANGE) {
                            vmax = __builtin_fmaxf(vmax, __builtin_fmaxf(__builtin_fmaxf(cr, cg), cb));
                            // per component: a sum probe would also fire on +inf next to -inf, where numpy's max is +inf.
                            // (Round 5 tried the NaN-propagating v_maximum3_f32 and v_max3_f32 + a wavefront NaN mask through
                            // inline asm: both SLOWER, 1.27 vs 1.13 ms per 256 x 1080p on one box; the asm statements keep the
                            // compiler from overlapping the next loads with this arithmetic, which is what the pass lives on.
                            // profiles/r05_dis_small_steps.md)
                            has_nan |= ((cr != cr) | (cg != cg) | (cb != cb)) ? 1 : 0;
                        }
                    }
                    // the K lanes of a box sit in one quad (blockDim.x and `used` are multiples of K): integer adds, any order
                    if (K >= 2) sum += __builtin_amdgcn_update_dpp(0, sum, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
                    if (K == 4) sum += __builtin_amdgcn_update_dpp(0, sum, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
                    if ((sx & (K - 1)) == 0) {
                        int o;
                        if (K == 1) o = sum;
                        else if (K == 2) o = (sum + 2) >> 2;
                        else o = sat_u8_round(sum * (1.f / (K * K)));
                        D[sx / K] = (uint8_t)o;
                    }
                }
            }
        }
    } while (G > 1 && ++y < y_end);
    if (RANGE) {
        // every lane of the wavefront is here (blockDim.x is a multiple of 64); lanes without a pixel hold -inf and 0
        const float m = wave_max_lane63(vmax);
        const bool any_nan = __ballot(has_nan) != 0;
        const int waves = (int)blockDim.x >> 6, wave = (int)threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 63) row_max[((size_t)f * groups + g) * waves + wave] = any_nan ? NAN : m;
    }
}

// per-frame maximum of the range passes' partial maxima, `rows` of them per frame (NaN wins, as in numpy): one workgroup per frame
// host_max (optional): the maxima also go to coherent host memory -- by the LAST workgroup to finish (a device-scope count
// finds it), as one coalesced store of all `gridDim.x` values followed by a release store of `target` into host_flag.  (One
// store + one system-scope atomic per workgroup, the first form of this, serialised 256 PCIe round trips: 276 us.)
__global__ __launch_bounds__(256) void frame_max_kernel(const float* __restrict__ row_max, float* __restrict__ frame_max, int rows,
                                                        float* host_max, unsigned* host_flag, unsigned* dev_count, unsigned target)
{
    __shared__ float s_max[4];
    __shared__ int s_nan[4];
    __shared__ int s_last;
    const float* R = row_max + (size_t)blockIdx.x * rows;
    float vmax = -INFINITY;
    int has_nan = 0;
    for (int k = threadIdx.x; k < rows; k += 256) {
        const float v = R[k];
        has_nan |= (v != v) ? 1 : 0;
        vmax = __builtin_fmaxf(vmax, v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        vmax = __builtin_fmaxf(vmax, __shfl_down(vmax, off));
        has_nan |= __shfl_down(has_nan, off);
    }
    if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = vmax; s_nan[threadIdx.x >> 6] = has_nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float m = __builtin_fmaxf(__builtin_fmaxf(s_max[0], s_max[1]), __builtin_fmaxf(s_max[2], s_max[3]));
        frame_max[blockIdx.x] = (s_nan[0] | s_nan[1] | s_nan[2] | s_nan[3]) ? NAN : m;
        s_last = 0;
        if (host_max != nullptr) {
            // release the value, count this workgroup; the one that completes the pass's count mirrors all of them
            const unsigned prev = __hip_atomic_fetch_add(dev_count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (prev + 1u == target) ? 1 : 0;
        }
    }
    if (host_max == nullptr) return;
    __syncthreads();
    if (s_last) {
        for (int i = threadIdx.x; i < (int)gridDim.x; i += 256)
            host_max[i] = __hip_atomic_load(frame_max + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(host_flag, target, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// stabilizer_utils.py:127-131 applied to a clip: frames whose maximum exceeds 1.5 are divided by 255 (IEEE f32
// division, as numpy's `arr /= 255.0`), the others are copied; NaN maxima compare False.  Out of place: the caller's
// tensor is never modified.
__global__ __launch_bounds__(256) void value_range_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          const float* __restrict__ frame_max, long long per_frame, long long total)
{
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const float v = src[t];
        dst[t] = (frame_max[t / per_frame] > 1.5f) ? v / 255.0f : v;
    }
}

// per-row maxima of a clip without producing gray (Motion Apply has no estimation pass): one workgroup of 4 wavefronts
// per source row, one partial per wavefront in row_max[4 * row + wave]
// VEC: pieces are a multiple of 4 floats and 16-B aligned (checked by the host); otherwise plain 4-B loads
template <bool VEC>
__global__ __launch_bounds__(256) void row_max_kernel(const float* __restrict__ frames, float* __restrict__ row_max, int row_floats)
{
    const float* S = frames + (size_t)blockIdx.x * row_floats;
    float vmax = -INFINITY;
    int has_nan = 0;
    if (VEC) {
        typedef float f4_t __attribute__((ext_vector_type(4)));
        const f4_t* R = reinterpret_cast<const f4_t*>(S);
        const int nvec = row_floats / 4;
#pragma unroll 4
        for (int k = threadIdx.x; k < nvec; k += 256) {
            const f4_t v = __builtin_nontemporal_load(R + k);   // read once by this pass (see gray_area_int_kernel)
            vmax = __builtin_fmaxf(__builtin_fmaxf(vmax, __builtin_fmaxf(v.x, v.y)), __builtin_fmaxf(v.z, v.w));
            has_nan |= ((v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w)) ? 1 : 0;
        }
    } else {
        for (int k = threadIdx.x; k < row_floats; k += 256) {
            const float v = S[k];
            vmax = __builtin_fmaxf(vmax, v);
            has_nan |= (v != v) ? 1 : 0;
        }
    }
    // one partial per wavefront, as in gray_area_int_kernel: no LDS, no barrier
    const float m = wave_max_lane63(vmax);
    const bool any_nan = __ballot(has_nan) != 0;
    if ((threadIdx.x & 63) == 63) row_max[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = any_nan ? NAN : m;
}

}  // namespace

static int gray_run(vstab_ctx* ctx, const float* frames, int n, int src_h, int src_w, int work_h, int work_w, uint8_t* gray,
                    float* frame_max)
{
    VSTAB_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int body = src_w & ~7;
    KernelTimer timer(ctx, "gray");
    float* row_max = nullptr;
    int range_rows = 0;   // entries of row_max per frame once the gray pass has filled it

    // workgroup size: the multiple of 64 (<= 1024) that covers a row of `cols` columns in whole passes with the fewest
    // idle lane slots; ties go to the size nearest 640 (measured best for 1920 / 3840 columns)
    auto threads_for = [](int cols) {
        int best = 256;
        long long best_cost = -1;
        for (int t = 256; t <= 1024; t += 64) {
            const long long cost = (long long)((cols + t - 1) / t) * t;
            if (best_cost < 0 || cost < best_cost || (cost == best_cost && std::abs(t - 640) < std::abs(best - 640))) { best = t; best_cost = cost; }
        }
        // A/B measurement (tools/gray_forms.py); whole wavefronts, as the kernel's quads and its per-wavefront partials need
        if (const char* e = getenv("VSTAB_GRAY_THREADS")) best = std::min(1024, std::max(64, (atoi(e) + 63) / 64 * 64));
        return best;
    };
    // output rows per workgroup: the RANGE pass walks two (measured against 1, 4 and 6 at 256 x 1080p, see the kernel)
    constexpr int RANGE_ROWS = 2, PLAIN_ROWS = 1;
#define LAUNCH_GRAY_G(K, RANGE, G, ROWS, OUT)                                                                             \
    hipLaunchKernelGGL((gray_area_int_kernel<K, RANGE, G>), dim3((unsigned)(n * (((ROWS) + G - 1) / G))), dim3(threads), 0, st, frames, OUT, \
                       n, src_h, src_w, (ROWS), src_w / K, body, row_max)
#define LAUNCH_GRAY(K, ROWS, OUT)                                                                                         \
    do {                                                                                                                  \
        if (row_max) LAUNCH_GRAY_G(K, true, RANGE_ROWS, ROWS, OUT);                                                       \
        else LAUNCH_GRAY_G(K, false, PLAIN_ROWS, ROWS, OUT);                                                              \
        VSTAB_HIP(hipGetLastError());                                                                                     \
    } while (0)

    // the fused kernel forms the exact 2 x 2 and 4 x 4 boxes itself; every other working size is a resize of the full-size gray
    const AreaPlan pl = plan_area(src_h, src_w, work_h, work_w);
    const bool same = (work_h == src_h && work_w == src_w);
    const bool fused = !same && pl.mode != AREA_GENERAL && pl.isx == pl.isy && (pl.isx == 2 || pl.isx == 4);
    const int K = fused ? pl.isx : 1;
    const int threads = threads_for(src_w / K * K);   // the one launch of gray_area_int_kernel below, whichever it is
    if (frame_max) {
        // the gray pass covers every source sample exactly when its K x K boxes tile the source; every wavefront of
        // every row group leaves one partial
        const int rows = (same || !fused) ? src_h : work_h;
        const int partials = (rows + RANGE_ROWS - 1) / RANGE_ROWS * (threads / 64);
        if (ctx->d_range.reserve(sizeof(float) * (size_t)n * partials)) return 1;
        row_max = static_cast<float*>(ctx->d_range.ptr);
        range_rows = partials;
    }
    if (same) {
        LAUNCH_GRAY(1, work_h, gray);
    } else if (fused) {
        VSTAB_REQUIRE(work_w * K == src_w && work_h * K == src_h, "vstab_gray_downscale: %dx%d is not %d x %dx%d", src_w, src_h, K, work_w, work_h);
        if (K == 2) LAUNCH_GRAY(2, work_h, gray);
        else LAUNCH_GRAY(4, work_h, gray);
    } else {
        // two passes: full-resolution gray into scratch, then the area resize
        const size_t full = (size_t)n * src_h * src_w;
        if (ctx->d_gray_tmp.reserve(full)) return 1;
        uint8_t* tmp = static_cast<uint8_t*>(ctx->d_gray_tmp.ptr);
        LAUNCH_GRAY(1, src_h, tmp);
        if (int rc = vstab_area_resize_u8(st, tmp, gray, n, src_h, src_w, work_h, work_w)) return rc;
    }
#undef LAUNCH_GRAY
#undef LAUNCH_GRAY_G
    if (frame_max) {
        // the host's copy of the maxima: written by the kernel itself into coherent host memory (no copy, no event on the stream)
        if (ctx->peaks.reserve(sizeof(float) * (size_t)std::max(1024, n), st)) return 1;
        if (!ctx->d_peaks_count.ptr) {   // the device-side count of finished frames (never reset: passes are told their target)
            if (ctx->d_peaks_count.reserve(256)) return 1;
            VSTAB_HIP(hipMemsetAsync(ctx->d_peaks_count.ptr, 0, ctx->d_peaks_count.bytes, st));
        }
        ctx->peaks_target += (unsigned)n;
        ctx->peaks_frames = n;
        hipLaunchKernelGGL(frame_max_kernel, dim3((unsigned)n), dim3(256), 0, st, row_max, frame_max, range_rows, ctx->peaks.dev<float>(),
                           ctx->status.dev<unsigned>() + VSTAB_PEAKS_DONE_WORD, static_cast<unsigned*>(ctx->d_peaks_count.ptr), ctx->peaks_target);
        VSTAB_HIP(hipGetLastError());
    }
    return 0;
}

static int gray_check(const char* who, vstab_ctx* ctx, const float* frames, int n, int src_h, int src_w, int work_h, int work_w,
                      const uint8_t* gray)
{
    VSTAB_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    VSTAB_REQUIRE(frames && gray, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(n > 0 && src_h > 0 && src_w > 0 && work_h > 0 && work_w > 0, "%s: non-positive size", who);
    VSTAB_REQUIRE(work_h <= src_h && work_w <= src_w, "%s: working size %dx%d larger than source %dx%d", who, work_w, work_h, src_w, src_h);
    return 0;
}

extern "C" int vstab_gray_downscale(vstab_ctx* ctx, const float* frames, int n, int src_h, int src_w, int work_h,
                                    int work_w, uint8_t* gray)
{
    if (int rc = gray_check("vstab_gray_downscale", ctx, frames, n, src_h, src_w, work_h, work_w, gray)) return rc;
    return gray_run(ctx, frames, n, src_h, src_w, work_h, work_w, gray, nullptr);
}

extern "C" int vstab_gray_downscale_range(vstab_ctx* ctx, const float* frames, int n, int src_h, int src_w, int work_h,
                                          int work_w, uint8_t* gray, float* frame_max)
{
    if (int rc = gray_check("vstab_gray_downscale_range", ctx, frames, n, src_h, src_w, work_h, work_w, gray)) return rc;
    VSTAB_REQUIRE(frame_max != nullptr, "vstab_gray_downscale_range: frame_max is NULL");
    return gray_run(ctx, frames, n, src_h, src_w, work_h, work_w, gray, frame_max);
}

// The maxima of the latest vstab_gray_downscale_range call, on the host: waits for that call's frame_max_kernel only (a
// word in coherent host memory that the kernel's last workgroup sets to the pass's target), not for anything queued behind it.
extern "C" int vstab_last_frame_peaks(vstab_ctx* ctx, int n, float* out)
{
    VSTAB_REQUIRE(ctx != nullptr && out != nullptr, "vstab_last_frame_peaks: NULL argument");
    VSTAB_REQUIRE(ctx->peaks.bytes != 0 && n == ctx->peaks_frames, "vstab_last_frame_peaks: no range pass over %d frames is pending", n);
    volatile unsigned* done = ctx->status.host<volatile unsigned>() + VSTAB_PEAKS_DONE_WORD;
    const unsigned target = ctx->peaks_target;
    auto reached = [=] { return vstab_seq_reached(*done, target); };
    // the gray pass of a 256 x 1080p clip takes ~1 ms; should the count never arrive (a lost launch), a stream
    // synchronisation after 2 s turns the wait into the runtime's own error report
    if (!vstab_spin_until(reached, std::chrono::seconds(2))) {
        VSTAB_HIP(hipStreamSynchronize(ctx->stream));
        VSTAB_REQUIRE(reached(), "vstab_last_frame_peaks: the range pass finished without reporting its %d frames", n);
    }
    memcpy(out, ctx->peaks.host<float>(), sizeof(float) * (size_t)n);
    return 0;
}

extern "C" int vstab_frame_range(vstab_ctx* ctx, const float* frames, int n, int h, int w, float* frame_max)
{
    VSTAB_REQUIRE(ctx != nullptr, "vstab_frame_range: ctx is NULL");
    VSTAB_REQUIRE(frames && frame_max, "vstab_frame_range: NULL pointer argument");
    VSTAB_REQUIRE(n > 0 && h > 0 && w > 0, "vstab_frame_range: non-positive size");
    VSTAB_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // a frame is h*w*3 contiguous floats: cut it into pieces of a multiple of 4 floats that divides it evenly
    const long long per_frame = (long long)h * w * 3;
    long long piece = (long long)w * 3;   // one source row per workgroup
    bool vec = false;
    for (long long cand : {(long long)w * 3, (long long)w * 3 * 2, (long long)w * 3 * 4})
        if (cand % 4 == 0 && per_frame % cand == 0 && (reinterpret_cast<uintptr_t>(frames) % 16) == 0) { piece = cand; vec = true; break; }
    const long long pieces = per_frame / piece;
    VSTAB_REQUIRE((long long)n * pieces < 0x7fffffffLL && pieces * 4 < 0x7fffffffLL && piece < 0x7fffffffLL, "vstab_frame_range: clip too large");
    if (ctx->d_range.reserve(sizeof(float) * (size_t)n * pieces * 4)) return 1;   // row_max_kernel: 4 wavefronts per piece
    float* row_max = static_cast<float*>(ctx->d_range.ptr);
    KernelTimer timer(ctx, "range");
    if (vec) hipLaunchKernelGGL(row_max_kernel<true>, dim3((unsigned)(n * pieces)), dim3(256), 0, st, frames, row_max, (int)piece);
    else hipLaunchKernelGGL(row_max_kernel<false>, dim3((unsigned)(n * pieces)), dim3(256), 0, st, frames, row_max, (int)piece);
    hipLaunchKernelGGL(frame_max_kernel, dim3((unsigned)n), dim3(256), 0, st, row_max, frame_max, (int)(pieces * 4), (float*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, 0u);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

extern "C" int vstab_apply_value_range(vstab_ctx* ctx, const float* frames, int n, int h, int w, const float* frame_max, float* out)
{
    VSTAB_REQUIRE(ctx != nullptr, "vstab_apply_value_range: ctx is NULL");
    VSTAB_REQUIRE(frames && frame_max && out, "vstab_apply_value_range: NULL pointer argument");
    VSTAB_REQUIRE(n > 0 && h > 0 && w > 0, "vstab_apply_value_range: non-positive size");
    VSTAB_HIP(hipSetDevice(ctx->device));
    const long long per_frame = (long long)h * w * 3, total = per_frame * n;
    hipLaunchKernelGGL(value_range_kernel, dim3(capped_grid(total, 256LL * 16)), dim3(256), 0, ctx->stream, frames, out, frame_max, per_frame, total);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
