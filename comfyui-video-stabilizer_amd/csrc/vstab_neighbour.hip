// vstab_neighbour.hip -- the neighbour passes, which sample OTHER frames of the clip (FillCand records) with the plain warp's
// own arithmetic (vstab_internal.h, VSTAB_WARP_ARITHMETIC): temporal fill, its blended form and gain sums, sharpness transfer.
// Not reference code.  profiles/warp_traffic.json is tied to vstab_warp.hip + vstab_internal.h: an edit here leaves it valid.
#define VSTAB_WARP_ARITHMETIC
#include "vstab_internal.h"
#include <cmath>

namespace {

// One candidate of one frame.  Every kernel receives the record array (like `own`, `gains`, `ratios`, `live`) as a
// `const T* __restrict__` kernel PARAMETER of its own, never through its argument struct: block-uniform scalar loads.
struct FillCand {
    WarpXform xf;
    int frame;     // clip frame the candidate samples, -1: none (out of the clip, cut chain, singular matrix)
    int pad_;
};

// The geometry every neighbour kernel's arguments carry (set_geometry fills it).
struct NeighbourGeom {
    int K;                  // candidates per frame
    int sh, sw, dh, dw;
    int bw0, bw0_pow2;      // column block width of OpenCV's WarpPerspectiveInvoker, 1 if it is a power of two
    int tiles_x, tiles_y;   // 64 x 8 tiles per frame (0 for the gain sums, whose grid is the lattice)
};

// sample_q5's cub_tab: the bicubic table in the kernel's own `s_cub`, nullptr for bilinear.  All threads call it (barrier).
template <int INTERP>
__device__ __forceinline__ const float* stage_cubic_table(float* s_cub)
{
    if (INTERP != VSTAB_INTERP_BICUBIC) return nullptr;
    if (threadIdx.x < 32) cubic_coeffs((int)threadIdx.x, s_cub + threadIdx.x * 4);
    __syncthreads();
    return s_cub;
}

// All taps of the Q5 coordinate (X, Y) inside an sw x sh frame: the interior tests of sample_q5.
template <int INTERP>
__device__ __forceinline__ bool fill_taps_inside(int sh, int sw, int X, int Y)
{
    const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
    if (INTERP == VSTAB_INTERP_BILINEAR) return (unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1);
    const unsigned width1 = (unsigned)(sw - 3 > 0 ? sw - 3 : 0);
    const unsigned height1 = (unsigned)(sh - 3 > 0 ? sh - 3 : 0);
    return (unsigned)(sx - 1) < width1 && (unsigned)(sy - 1) < height1;
}

// The Q5 coordinate of output pixel (x, y) under one record: warp_pixel with samplers that read nothing.
template <int INTERP>
__device__ __forceinline__ void fill_coordinate(const WarpXform* __restrict__ xf, const XformRegs<INTERP, VSTAB_SUBPIX_Q5>& r,
                                                const NeighbourGeom& g, int x, int y, double dy, int& X, int& Y)
{
    float c_unused = 0.f;
    int ox = 0, oy = 0;
    (void)warp_pixel<INTERP, VSTAB_SUBPIX_Q5, false>(
        xf, r, g.sh, g.sw, g.dw, g.bw0, g.bw0_pow2, x, y, dy, [&](int qx, int qy) { ox = qx; oy = qy; return Px{0.f, 0.f, 0.f}; },
        [&](float, float) { return Px{0.f, 0.f, 0.f}; }, NoDisplacement{}, c_unused);
    X = ox; Y = oy;
}

// A candidate's sample at output pixel (x, y), taken only where every tap is inside (`valid`): the samplers' own interior
// branches (sample_q5's tests, sample_exact's four in-range flags), so the border arguments are never read.
template <int INTERP, int SUBPIX>
__device__ __forceinline__ Px fill_candidate_sample(const float* __restrict__ S, const WarpXform* __restrict__ xf,
                                                    const XformRegs<INTERP, SUBPIX>& r, const NeighbourGeom& g, int x, int y,
                                                    double dy, const float* cub_tab, bool& valid)
{
    float c_unused = 0.f;
    bool ok = false;
    const Px v = warp_pixel<INTERP, SUBPIX, false>(
        xf, r, g.sh, g.sw, g.dw, g.bw0, g.bw0_pow2, x, y, dy,
        [&](int X, int Y) {
            ok = fill_taps_inside<INTERP>(g.sh, g.sw, X, Y);
            return ok ? sample_q5<INTERP>(S, g.sh, g.sw, X, Y, 0.f, 0.f, 0.f, cub_tab) : Px{0.f, 0.f, 0.f};
        },
        [&](float fsx, float fsy) {
            const float flx = __builtin_floorf(fsx), fly = __builtin_floorf(fsy);   // NaN / inf compare false
            ok = flx >= 0.f && flx < (float)(g.sw - 1) && fly >= 0.f && fly < (float)(g.sh - 1);
            return ok ? sample_exact(S, g.sh, g.sw, fsx, fsy, 0.f, 0.f, 0.f) : Px{0.f, 0.f, 0.f};
        },
        NoDisplacement{}, c_unused);
    valid = ok;
    return v;
}

// What every neighbour entry checks.  `q5_only`: nullptr, or why the entry refuses VSTAB_SUBPIX_EXACT (the parenthesis of its
// message).  `also_required`: the entry's other pointer that must not be NULL, reported together with cand_frame.
int check_neighbour_call(const char* who, vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                         const float* matrices, const int32_t* cand_frame, const void* also_required, int K, int out_h, int out_w,
                         int interp, int subpix, const float* dst, const char* q5_only)
{
    const float no_border[3] = {0.f, 0.f, 0.f};
    if (int rc = vstab_check_common(who, ctx, src, n, src_h, src_w, matrices, out_h, out_w, interp, no_border, subpix, dst)) return rc;
    VSTAB_REQUIRE(q5_only == nullptr || subpix == VSTAB_SUBPIX_Q5, "%s: VSTAB_SUBPIX_EXACT is not supported (%s)", who, q5_only);
    VSTAB_REQUIRE(cand_frame != nullptr && also_required != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(K >= 1 && K <= 64, "%s: K=%d outside [1,64]", who, K);
    VSTAB_REQUIRE(clip_frames > 0 && first >= 0 && first + n <= clip_frames, "%s: frames [%d, %d) outside a clip of %d frames", who,
                  first, first + n, clip_frames);
    VSTAB_REQUIRE((const void*)src != (const void*)dst, "%s: dst must not alias src (candidates read src while dst is written)", who);
    return 0;
}

// The candidate records of a call: the transform of every float32 forward matrix and the frame it samples, -1 where the
// fill skips it.  cand_frame == nullptr: the records of a frame's OWN matrices (frame 0 where usable, -1 where not).
int fill_cand_records(const char* who, const float* matrices, const int32_t* cand_frame, size_t count, int clip_frames, FillCand* cd)
{
    for (size_t i = 0; i < count; i++) {
        const int f = cand_frame ? cand_frame[i] : 0;
        VSTAB_REQUIRE(f >= -1 && f < clip_frames, "%s: cand_frame[%zu]=%d outside [-1, %d)", who, i, f, clip_frames);
        const float* m32 = matrices + i * 9;
        vstab_fill_xform(m32, &cd[i].xf);
        // a matrix that cv::invert would refuse (zero or non-finite determinant) has no source position: no candidate
        double M[9], inv[9];
        bool finite = true;
        for (int j = 0; j < 9; j++) { M[j] = (double)m32[j]; finite = finite && std::isfinite(M[j]); }
        bool ok = f >= 0 && finite && vstab_invert3x3_hd(M, inv);
        for (int j = 0; ok && j < 9; j++) ok = std::isfinite(inv[j]);
        cd[i].frame = ok ? f : -1;
        cd[i].pad_ = 0;
    }
    return 0;
}

// Sizes, K and OpenCV's column block width; with `blocks`, the grid of 64 x 8 tiles over `frames` frames too.
int set_geometry(const char* who, NeighbourGeom& g, int frames, int K, int sh, int sw, int dh, int dw, unsigned* blocks)
{
    g.K = K; g.sh = sh; g.sw = sw; g.dh = dh; g.dw = dw;
    vstab_set_block_width(dh, dw, &g.bw0, &g.bw0_pow2);
    return blocks ? vstab_tile_grid(who, frames, dh, dw, 32, 256, &g.tiles_x, &g.tiles_y, blocks) : 0;
}

// Several host arrays staged back to back as ONE block of the call's parameters (one copy to the device); every part gets
// its device pointer.  The callers put the widest element type first, so every part is aligned to its own.
struct StagePart { const void* host; size_t bytes; const void* dev; };
int stage_parts(vstab_ctx* ctx, StagePart* parts, int count)
{
    std::vector<unsigned char> blob;
    for (int i = 0; i < count; i++) {
        const unsigned char* h = static_cast<const unsigned char*>(parts[i].host);
        blob.insert(blob.end(), h, h + parts[i].bytes);
    }
    void* dev = nullptr;
    if (vstab_stage_params(ctx, blob.data(), blob.size(), &dev)) return 1;
    size_t at = 0;
    for (int i = 0; i < count; i++) {
        parts[i].dev = static_cast<const unsigned char*>(dev) + at;
        at += parts[i].bytes;
    }
    return 0;
}

// Zeroes the per-frame counters the caller asked for (nullptr: not asked).
int zero_counts(vstab_ctx* ctx, int n, std::initializer_list<uint32_t*> counts)
{
    for (uint32_t* c : counts)
        if (c) VSTAB_HIP(hipMemsetAsync(c, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    return 0;
}

// KERNEL<interp>'s launch over `grid` workgroups of 256 threads; reads `interp`, `grid` and `ctx` of the calling entry.
#define LAUNCH_INTERP(KERNEL, ...)                                                                                          \
    do {                                                                                                                    \
        if (interp == VSTAB_INTERP_BICUBIC) hipLaunchKernelGGL((KERNEL<VSTAB_INTERP_BICUBIC>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__);  \
        else hipLaunchKernelGGL((KERNEL<VSTAB_INTERP_BILINEAR>), grid, dim3(256), 0, ctx->stream, __VA_ARGS__);             \
    } while (0)

// ---- temporal fill: padding pixels taken from neighbouring frames ----------------------------------------------------
//
// After a warp, an output pixel whose mask is 1 saw no source content in its own frame.  For each such pixel the kernel
// walks up to K candidate (frame, matrix) pairs in order and takes the first one whose source position -- warp_pixel's,
// the plain warp's own arithmetic -- has EVERY interpolation tap inside that frame: the value written is then the one
// vstab_warp_batch would have written for that frame and matrix, and no border colour can enter it.
//
// Shape: the warp's 64 x 8 tile and XCD remap.  A tile reads its mask (4 B per pixel); if none of its pixels is padded the
// block returns -- the common case, so the pass over a mostly covered clip is close to a plain read of the mask.  The
// candidate records are block-uniform (scalar loads, see FillCand).  A wavefront leaves the candidate loop as soon as none
// of its pixels is waiting.  Only filled pixels are stored.  dst is read by nobody (candidates sample src): in place is safe.
struct FillArgs : NeighbourGeom {
    const float* src;
    float* dst;
    float* mask;
    signed char* filled_from;
    unsigned* fill_count;
    unsigned* pad_count;
};

template <int INTERP, int SUBPIX>
__global__ __launch_bounds__(256) void temporal_fill_kernel(FillArgs a, const FillCand* __restrict__ cands)
{
    constexpr int TILE_TX = 32;
    __shared__ __attribute__((aligned(16))) float s_cub[32 * 4];
    const TileShell<TILE_TX> t(a.tiles_x, a.tiles_y, a.dh, a.dw);
    const int frame = t.frame, x0 = t.x0, y = t.y, npx = t.npx;

    float* __restrict__ Mk = a.mask + (size_t)frame * a.dh * a.dw;
    const unsigned row = (unsigned)y * (unsigned)a.dw;
    bool need[TILE_PX];
    bool any = false;
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) {
        need[p] = (p < npx) && Mk[row + (unsigned)(x0 + p * TILE_TX)] == 1.0f;
        any = any || need[p];
    }
    if (!__syncthreads_or(any)) return;   // nothing padded in this tile: nothing to fill, nothing to count

    const float* cub_tab = stage_cubic_table<INTERP>(s_cub);

    float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
    signed char* __restrict__ From = a.filled_from ? a.filled_from + (size_t)frame * a.dh * a.dw : nullptr;
    const size_t src_frame = (size_t)a.sh * a.sw * 3;
    const double dy = (double)y;
    unsigned filled = 0;
    typedef float f3 __attribute__((ext_vector_type(3)));

    for (int k = 0; k < a.K; k++) {
        if (!__any(any)) break;                       // wave-uniform: no pixel of this wavefront is waiting
        const FillCand* __restrict__ cd = cands + (size_t)frame * a.K + k;
        if (cd->frame < 0) continue;                  // block-uniform
        const float* __restrict__ S = a.src + (size_t)cd->frame * src_frame;
        const WarpXform* __restrict__ xf = &cd->xf;
        const XformRegs<INTERP, SUBPIX> r(xf);
        any = false;
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (!need[p]) continue;
            const int x = x0 + p * TILE_TX;
            bool valid = false;
            const Px v = fill_candidate_sample(S, xf, r, a, x, y, dy, cub_tab, valid);
            if (valid) {
                const unsigned pix = row + (unsigned)x;
                f3 rgb = {v.r, v.g, v.b};
                __builtin_memcpy(D + pix * 3u, &rgb, 12);
                Mk[pix] = 0.f;
                if (From) From[pix] = (signed char)k;
                need[p] = false;
                filled += 1u;
            }
            any = any || need[p];
        }
    }

    if (a.fill_count != nullptr || a.pad_count != nullptr) {
        unsigned cnt[2] = {filled, 0};   // filled, left
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) cnt[1] += need[p] ? 1u : 0u;
        block_count_add<2>(cnt, {a.fill_count, a.pad_count}, frame);
    }
}

// ---- blended temporal fill: exposure-matched candidates, feathered seam (include/vstab.h states both rules) -------------
//
// Two kernels beside temporal_fill_kernel, which keeps its instances, its FillCand records and its cost:
//   fill_gain_sums_kernel       integer sums of own and candidate values over the lattice x % 8 == 4 && y % 8 == 4 where
//                               both see source content by the interior rule; the host turns them into one gain per
//                               (frame, candidate, channel).  A workgroup = 256 lattice pixels of one (frame, candidate) pair, so
//                               both records are block-uniform (scalar loads); per-thread values -> BlockSums
//                               (vstab_internal.h) -> one 64-bit atomic per sum, skipped where the workgroup counted nothing.
//                               Nothing waits for another workgroup.
//   temporal_fill_blend_kernel  the fill's tile, shell and candidate walk, with (a) the sample scaled by the candidate's gain
//                               and (b) the own pixels within feather_px of the frame's tap-interior border cross-faded
//                               towards the first valid candidate.  Whether an own pixel takes part costs its mask and its
//                               own coordinate (warp_pixel with a sampler that only records X, Y: ALU, no loads); a tile
//                               without padded or feathered pixels returns before anything else is read or stored.

// q of the gain sums: a value in 16 fractional bits, truncated; below 0 and NaN give 0, 1 and above give 65536.
__device__ __forceinline__ unsigned gain_q(float v)
{
    return v > 0.f ? (v < 1.f ? (unsigned)(v * 65536.0f) : 65536u) : 0u;
}

struct GainArgs : NeighbourGeom {
    const float* src;
    const float* dst;
    unsigned long long* sums;   // [n, K, 7]
    int lw;                    // lattice columns: x = 8 * lx + 4 < dw
    unsigned lattice;           // lattice pixels per frame
    unsigned blocks_per_pair;   // workgroups per (frame, candidate) pair
};

template <int INTERP>
__global__ __launch_bounds__(256) void fill_gain_sums_kernel(GainArgs a, const FillCand* __restrict__ cands, const FillCand* __restrict__ own)
{
    constexpr int NS = 7;
    __shared__ __attribute__((aligned(16))) float s_cub[32 * 4];
    __shared__ BlockSums<unsigned, NS, 256> s_sums;
    const unsigned pair = blockIdx.x / a.blocks_per_pair;          // frame * K + k
    const unsigned chunk = blockIdx.x - pair * a.blocks_per_pair;
    const unsigned frame = pair / (unsigned)a.K;
    const FillCand* __restrict__ cd = cands + pair;
    const FillCand* __restrict__ ow = own + frame;
    if (ow->frame < 0 || cd->frame < 0) return;                    // block-uniform: this pair counts nothing

    const float* cub_tab = stage_cubic_table<INTERP>(s_cub);

    // a workgroup's sums fit 32 bits: 256 values of at most 65536
    unsigned v[NS];
#pragma unroll
    for (int c = 0; c < NS; c++) v[c] = 0u;
    const unsigned l = chunk * 256u + threadIdx.x;
    if (l < a.lattice) {
        const unsigned ly = l / (unsigned)a.lw;
        const int x = (int)(l - ly * (unsigned)a.lw) * VSTAB_FILL_GAIN_STRIDE + VSTAB_FILL_GAIN_STRIDE / 2;   // x < dw, y < dh by the
        const int y = (int)ly * VSTAB_FILL_GAIN_STRIDE + VSTAB_FILL_GAIN_STRIDE / 2;                            // lattice's size
        const double dy = (double)y;
        int X, Y;
        {
            const WarpXform* __restrict__ xo = &ow->xf;
            const XformRegs<INTERP, VSTAB_SUBPIX_Q5> ro(xo);
            fill_coordinate(xo, ro, a, x, y, dy, X, Y);
        }
        if (fill_taps_inside<INTERP>(a.sh, a.sw, X, Y)) {
            const float* __restrict__ S = a.src + (size_t)cd->frame * ((size_t)a.sh * a.sw * 3);
            const WarpXform* __restrict__ xf = &cd->xf;
            const XformRegs<INTERP, VSTAB_SUBPIX_Q5> r(xf);
            bool valid = false;
            const Px s = fill_candidate_sample(S, xf, r, a, x, y, dy, cub_tab, valid);
            if (valid) {
                const float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
                const Px o = load_px(D + ((unsigned)y * (unsigned)a.dw + (unsigned)x) * 3u);
                v[0] = 1u;
                v[1] = gain_q(o.r); v[2] = gain_q(o.g); v[3] = gain_q(o.b);
                v[4] = gain_q(s.r); v[5] = gain_q(s.g); v[6] = gain_q(s.b);
            }
        }
    }

    s_sums.put(v);
    __syncthreads();
    if (threadIdx.x == 0 && s_sums.total(0) != 0u) {       // nothing counted: every sum is zero, no atomic
        unsigned long long* out = a.sums + (size_t)pair * NS;
#pragma unroll
        for (int c = 0; c < NS; c++) atomicAdd(out + c, s_sums.total<unsigned long long>(c));
    }
}

struct BlendArgs : FillArgs {
    unsigned* blend_count;
    int Fe;             // 32 * feather_px
    int lo, hi_x, hi_y; // the tap-interior border in 1/32 px: lo <= X <= hi_x, lo <= Y <= hi_y
};

template <int INTERP>
__global__ __launch_bounds__(256) void temporal_fill_blend_kernel(BlendArgs a, const FillCand* __restrict__ cands,
                                                                  const FillCand* __restrict__ own, const float* __restrict__ gains)
{
    constexpr int TILE_TX = 32;
    __shared__ __attribute__((aligned(16))) float s_cub[32 * 4];
    const TileShell<TILE_TX> t(a.tiles_x, a.tiles_y, a.dh, a.dw);
    const int frame = t.frame, x0 = t.x0, y = t.y, npx = t.npx;

    float* __restrict__ Mk = a.mask + (size_t)frame * a.dh * a.dw;
    const unsigned row = (unsigned)y * (unsigned)a.dw;
    const double dy = (double)y;
    const FillCand* __restrict__ ow = own + frame;
    const bool feather = a.Fe > 0 && ow->frame >= 0;      // block-uniform
    bool need[TILE_PX], padded[TILE_PX];
    float wgt[TILE_PX];                                   // own pixels: the weight of the own value
    bool any = false;
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) {
        need[p] = padded[p] = false;
        wgt[p] = 1.0f;
        if (p < npx) {
            const int x = x0 + p * TILE_TX;
            if (Mk[row + (unsigned)x] == 1.0f) need[p] = padded[p] = true;
            else if (feather) {
                const WarpXform* __restrict__ xo = &ow->xf;
                const XformRegs<INTERP, VSTAB_SUBPIX_Q5> ro(xo);
                int X, Y;
                fill_coordinate(xo, ro, a, x, y, dy, X, Y);
                // d32 = min(X - lo, Y - lo, hi_x - X, hi_y - Y), clamped to [0, Fe].  X and Y may be anywhere in int: one
                // step outside the border already gives a negative term, so they are clamped to that first and no
                // difference can overflow.
                const int Xc = min(max(X, a.lo - 1), a.hi_x + 1), Yc = min(max(Y, a.lo - 1), a.hi_y + 1);
                const int d32 = min(min(Xc - a.lo, Yc - a.lo), min(a.hi_x - Xc, a.hi_y - Yc));
                const int d = min(max(d32, 0), a.Fe);
                wgt[p] = (float)d / (float)a.Fe;
                need[p] = d < a.Fe;                       // w < 1 (d == Fe divides to exactly 1.0f)
            }
        }
        any = any || need[p];
    }
    if (!__syncthreads_or(any)) return;   // nothing padded, nothing within the feather: nothing to read, store or count

    const float* cub_tab = stage_cubic_table<INTERP>(s_cub);

    float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
    signed char* __restrict__ From = a.filled_from ? a.filled_from + (size_t)frame * a.dh * a.dw : nullptr;
    const size_t src_frame = (size_t)a.sh * a.sw * 3;
    unsigned filled = 0, blended = 0;
    typedef float f3 __attribute__((ext_vector_type(3)));

    for (int k = 0; k < a.K; k++) {
        if (!__any(any)) break;                       // wave-uniform: no pixel of this wavefront is waiting
        const FillCand* __restrict__ cd = cands + (size_t)frame * a.K + k;
        if (cd->frame < 0) continue;                  // block-uniform
        const float* __restrict__ S = a.src + (size_t)cd->frame * src_frame;
        const float* __restrict__ g = gains + ((size_t)frame * a.K + k) * 3;
        const float g0 = g[0], g1 = g[1], g2 = g[2];
        const WarpXform* __restrict__ xf = &cd->xf;
        const XformRegs<INTERP, VSTAB_SUBPIX_Q5> r(xf);
        any = false;
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (!need[p]) continue;
            const int x = x0 + p * TILE_TX;
            bool valid = false;
            const Px s = fill_candidate_sample(S, xf, r, a, x, y, dy, cub_tab, valid);
            if (valid) {
                const unsigned pix = row + (unsigned)x;
                f3 rgb = {g0 * s.r, g1 * s.g, g2 * s.b};      // one float32 multiply; nothing of the old pixel enters
                if (padded[p]) {
                    Mk[pix] = 0.f;
                    filled += 1u;
                } else {
                    const float w = wgt[p];
                    if (w != 0.f) {                           // w == 0 (the fringe ring and beyond): the candidate alone
                        const Px o = load_px(D + pix * 3u);
                        const float u = 1.0f - w;
                        rgb.x = o.r * w + rgb.x * u;
                        rgb.y = o.g * w + rgb.y * u;
                        rgb.z = o.b * w + rgb.z * u;
                    }
                    blended += 1u;
                }
                __builtin_memcpy(D + pix * 3u, &rgb, 12);
                if (From) From[pix] = (signed char)k;
                need[p] = false;
            }
            any = any || need[p];
        }
    }

    if (a.fill_count != nullptr || a.pad_count != nullptr || a.blend_count != nullptr) {
        unsigned cnt[3] = {filled, 0, blended};   // filled, left, blended
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) cnt[1] += (need[p] && padded[p]) ? 1u : 0u;
        block_count_add<3>(cnt, {a.fill_count, a.pad_count, a.blend_count}, frame);
    }
}

// What the plain and the blended fill do in front of their launch: the arguments they share, the tile grid, filled_from
// preset to -1 (neither filled nor blended), their counters zeroed (blend_count: nullptr for the plain fill).
int prepare_fill(const char* who, vstab_ctx* ctx, FillArgs& a, const float* src, int n, int K, int src_h, int src_w, int out_h,
                 int out_w, float* dst, float* mask, int8_t* filled_from, uint32_t* fill_count, uint32_t* pad_count, uint32_t* blend_count, unsigned* blocks)
{
    a.src = src; a.dst = dst; a.mask = mask; a.filled_from = reinterpret_cast<signed char*>(filled_from);
    a.fill_count = fill_count; a.pad_count = pad_count;
    if (int rc = set_geometry(who, a, n, K, src_h, src_w, out_h, out_w, blocks)) return rc;
    if (filled_from) VSTAB_HIP(hipMemsetAsync(filled_from, 0xff, (size_t)n * out_h * out_w, ctx->stream));
    return zero_counts(ctx, n, {fill_count, pad_count, blend_count});
}

const char* const FILL_BLEND_Q5_ONLY = "the feather distance and the gain lattice are stated on the 1/32-px coordinates of VSTAB_SUBPIX_Q5";

// Candidate records [n * K], the own records [n] and, where given, the gains [n * K * 3], staged as one block: parts[0..2].
int stage_fill_blend_records(const char* who, vstab_ctx* ctx, const float* matrices, const int32_t* cand_frame, int n, int K,
                             int clip_frames, const float* own_matrices, const float* gains, StagePart (&parts)[3])
{
    const size_t pairs = (size_t)n * K;
    std::vector<FillCand> cd(pairs + (size_t)n);
    if (int rc = fill_cand_records(who, matrices, cand_frame, pairs, clip_frames, cd.data())) return rc;
    if (int rc = fill_cand_records(who, own_matrices, nullptr, (size_t)n, clip_frames, cd.data() + pairs)) return rc;
    parts[0] = {cd.data(), pairs * sizeof(FillCand)};
    parts[1] = {cd.data() + pairs, (size_t)n * sizeof(FillCand)};
    parts[2] = {gains, gains ? pairs * 3 * sizeof(float) : 0};
    return stage_parts(ctx, parts, 3);
}
}  // namespace

extern "C" int vstab_temporal_fill_batch(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first,
                                         int n, const float* matrices, const int32_t* cand_frame, int K, int out_h, int out_w,
                                         int interp, int subpix, float* dst, float* mask, int8_t* filled_from,
                                         uint32_t* fill_count, uint32_t* pad_count)
{
    const char* who = "vstab_temporal_fill_batch";
    if (int rc = check_neighbour_call(who, ctx, src, clip_frames, src_h, src_w, first, n, matrices, cand_frame, mask, K, out_h, out_w,
                                      interp, subpix, dst, nullptr)) return rc;
    std::vector<FillCand> cd((size_t)n * K);
    if (int rc = fill_cand_records(who, matrices, cand_frame, cd.size(), clip_frames, cd.data())) return rc;
    VSTAB_HIP(hipSetDevice(ctx->device));
    StagePart staged[1] = {{cd.data(), cd.size() * sizeof(FillCand)}};
    if (stage_parts(ctx, staged, 1)) return 1;
    const FillCand* cands = static_cast<const FillCand*>(staged[0].dev);
    FillArgs a{};
    unsigned blocks = 0;
    if (int rc = prepare_fill(who, ctx, a, src, n, K, src_h, src_w, out_h, out_w, dst, mask, filled_from, fill_count, pad_count, nullptr, &blocks)) return rc;
    KernelTimer timer(ctx, "fill");
    const dim3 grid(blocks);
    if (interp == VSTAB_INTERP_BICUBIC) hipLaunchKernelGGL((temporal_fill_kernel<VSTAB_INTERP_BICUBIC, VSTAB_SUBPIX_Q5>), grid, dim3(256), 0, ctx->stream, a, cands);
    else if (subpix == VSTAB_SUBPIX_EXACT) hipLaunchKernelGGL((temporal_fill_kernel<VSTAB_INTERP_BILINEAR, VSTAB_SUBPIX_EXACT>), grid, dim3(256), 0, ctx->stream, a, cands);
    else hipLaunchKernelGGL((temporal_fill_kernel<VSTAB_INTERP_BILINEAR, VSTAB_SUBPIX_Q5>), grid, dim3(256), 0, ctx->stream, a, cands);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

extern "C" int vstab_fill_gain_sums(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                                    const float* matrices, const int32_t* cand_frame, int K, const float* own_matrices, int out_h,
                                    int out_w, int interp, int subpix, const float* dst, uint64_t* sums)
{
    const char* who = "vstab_fill_gain_sums";
    if (int rc = check_neighbour_call(who, ctx, src, clip_frames, src_h, src_w, first, n, matrices, cand_frame, own_matrices, K, out_h,
                                      out_w, interp, subpix, dst, FILL_BLEND_Q5_ONLY)) return rc;
    VSTAB_REQUIRE(sums != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(((uintptr_t)sums & 7) == 0, "%s: sums is not aligned to its element size", who);
    GainArgs a{};
    a.src = src; a.dst = dst; a.sums = reinterpret_cast<unsigned long long*>(sums);
    if (int rc = set_geometry(who, a, n, K, src_h, src_w, out_h, out_w, nullptr)) return rc;
    constexpr int STRIDE = VSTAB_FILL_GAIN_STRIDE, REST = STRIDE - STRIDE / 2 - 1;
    a.lw = (out_w + REST) / STRIDE;                                    // x = STRIDE * lx + STRIDE / 2 < out_w
    a.lattice = (unsigned)a.lw * (unsigned)((out_h + REST) / STRIDE);
    a.blocks_per_pair = (a.lattice + 255u) / 256u;
    const unsigned long long blocks = (unsigned long long)a.blocks_per_pair * (unsigned long long)n * (unsigned long long)K;
    VSTAB_REQUIRE(blocks < 0x7fffffffULL, "%s: grid of %llu blocks is out of range", who, blocks);
    VSTAB_HIP(hipSetDevice(ctx->device));
    StagePart staged[3];
    if (int rc = stage_fill_blend_records(who, ctx, matrices, cand_frame, n, K, clip_frames, own_matrices, nullptr, staged)) return rc;
    KernelTimer timer(ctx, "fill_gain");
    VSTAB_HIP(hipMemsetAsync(sums, 0, sizeof(uint64_t) * 7 * (size_t)n * K, ctx->stream));
    if (blocks == 0) return 0;                                         // a canvas without a lattice pixel: every sum is zero
    const dim3 grid((unsigned)blocks);
    LAUNCH_INTERP(fill_gain_sums_kernel, a, static_cast<const FillCand*>(staged[0].dev), static_cast<const FillCand*>(staged[1].dev));
    VSTAB_HIP(hipGetLastError());
    return 0;
}

extern "C" int vstab_temporal_fill_blend_batch(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first,
                                               int n, const float* matrices, const int32_t* cand_frame, int K,
                                               const float* own_matrices, const float* gains, int feather_px, int out_h, int out_w,
                                               int interp, int subpix, float* dst, float* mask, int8_t* filled_from,
                                               uint32_t* fill_count, uint32_t* pad_count, uint32_t* blend_count)
{
    const char* who = "vstab_temporal_fill_blend_batch";
    if (int rc = check_neighbour_call(who, ctx, src, clip_frames, src_h, src_w, first, n, matrices, cand_frame, own_matrices, K, out_h,
                                      out_w, interp, subpix, dst, FILL_BLEND_Q5_ONLY)) return rc;
    VSTAB_REQUIRE(mask != nullptr && gains != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(feather_px >= 0 && feather_px <= VSTAB_FILL_FEATHER_MAX, "%s: feather_px=%d outside [0,%d]", who, feather_px,
                  VSTAB_FILL_FEATHER_MAX);
    VSTAB_HIP(hipSetDevice(ctx->device));
    StagePart staged[3];
    if (int rc = stage_fill_blend_records(who, ctx, matrices, cand_frame, n, K, clip_frames, own_matrices, gains, staged)) return rc;

    BlendArgs a{};
    a.blend_count = blend_count;
    a.Fe = 32 * feather_px;
    const int inset = interp == VSTAB_INTERP_BICUBIC ? 1 : 0;          // bicubic: X - 32 and 32 (sw - 2) - X
    a.lo = 32 * inset; a.hi_x = 32 * (src_w - 1 - inset); a.hi_y = 32 * (src_h - 1 - inset);
    unsigned blocks = 0;
    if (int rc = prepare_fill(who, ctx, a, src, n, K, src_h, src_w, out_h, out_w, dst, mask, filled_from, fill_count, pad_count, blend_count, &blocks)) return rc;
    KernelTimer timer(ctx, "fill_blend");
    const dim3 grid(blocks);
    LAUNCH_INTERP(temporal_fill_blend_kernel, a, static_cast<const FillCand*>(staged[0].dev), static_cast<const FillCand*>(staged[1].dev), static_cast<const float*>(staged[2].dev));
    VSTAB_HIP(hipGetLastError());
    return 0;
}

// ---- sharpness transfer: own pixels of a blurred frame pulled towards what sharper neighbours show there -------------------
//
// The rule is stated in include/vstab.h (vstab_sharp_transfer_batch; Matsushita et al., PAMI 2006, section 5).  The fill's
// tile, shell, XCD remap, candidate records and sampler (fill_candidate_sample: warp_pixel with the interior test), but the
// other way round: the fill writes PADDED pixels from the FIRST valid candidate, this writes OWN pixels from EVERY valid
// candidate with a positive ratio, weighted by how well the sample agrees with the pixel.
//
// Shape: only frames with a live candidate (ratio > 0, not skipped) get workgroups at all -- the host lists them
// (`live`), so a clip without a blurred frame launches nothing and a frame that borrows nothing costs nothing: the
// "all ratios zero" exit is taken before the launch instead of per block.  A tile reads its mask and returns if it has
// no own pixel.  Candidates whose ratio is 0 or that are skipped are passed over block-uniformly (scalar loads of the
// record and the ratio); there is no "first wins" exit, so every other candidate is sampled for every own pixel.  Per
// pixel the kernel keeps o (3), num (3) and den (1) in registers, two pixels per thread.
// Resource usage (-Rpass-analysis=kernel-resource-usage, gfx950): bilinear 52 VGPRs, 8 waves per SIMD; bicubic 100 VGPRs, 4
// waves per SIMD; no scratch in either.
// The two divisions are IEEE-correct (-fhip-fp32-correctly-rounded-divide-sqrt, csrc/Makefile) and nothing is fused
// (-ffp-contract=off), so NumPy float32 gives the same bits.
namespace {

struct SharpArgs : NeighbourGeom {
    const float* src;
    float* dst;
    const float* mask;          // nullptr: every pixel is own
    unsigned* transfer_count;
    float alpha;
};

template <int INTERP>
__global__ __launch_bounds__(256) void sharp_transfer_kernel(SharpArgs a, const FillCand* __restrict__ cands,
                                                             const float* __restrict__ ratios, const int* __restrict__ live)
{
    constexpr int TILE_TX = 32;
    __shared__ __attribute__((aligned(16))) float s_cub[32 * 4];
    const TileShell<TILE_TX> t(a.tiles_x, a.tiles_y, a.dh, a.dw);
    const int frame = live[t.frame], x0 = t.x0, y = t.y, npx = t.npx;      // t.frame counts the live frames

    const unsigned row = (unsigned)y * (unsigned)a.dw;
    bool own[TILE_PX];
    bool any = false;
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) {
        own[p] = p < npx;
        if (own[p] && a.mask != nullptr) own[p] = !(a.mask[(size_t)frame * a.dh * a.dw + row + (unsigned)(x0 + p * TILE_TX)] == 1.0f);
        any = any || own[p];
    }
    if (!__syncthreads_or(any)) return;   // a tile of padding: nothing to read, store or count

    const float* cub_tab = stage_cubic_table<INTERP>(s_cub);

    float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
    const size_t src_frame = (size_t)a.sh * a.sw * 3;
    const double dy = (double)y;
    Px o[TILE_PX], num[TILE_PX];
    float den[TILE_PX];
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) {
        num[p] = Px{0.f, 0.f, 0.f};
        den[p] = 0.f;
        o[p] = own[p] ? load_px(D + (row + (unsigned)(x0 + p * TILE_TX)) * 3u) : Px{0.f, 0.f, 0.f};
    }

    for (int k = 0; k < a.K; k++) {
        const FillCand* __restrict__ cd = cands + (size_t)frame * a.K + k;
        const float ratio = ratios[(size_t)frame * a.K + k];
        if (cd->frame < 0 || !(ratio > 0.f)) continue;             // block-uniform
        const float* __restrict__ S = a.src + (size_t)cd->frame * src_frame;
        const WarpXform* __restrict__ xf = &cd->xf;
        const XformRegs<INTERP, VSTAB_SUBPIX_Q5> r(xf);
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (!own[p]) continue;
            bool valid = false;
            const Px s = fill_candidate_sample(S, xf, r, a, x0 + p * TILE_TX, y, dy, cub_tab, valid);
            if (!valid) continue;
            const float Dd = (__builtin_fabsf(s.r - o[p].r) + __builtin_fabsf(s.g - o[p].g)) + __builtin_fabsf(s.b - o[p].b);
            if (Dd < __builtin_inff()) {                           // false for a NaN in the sample or in the pixel
                const float w = ratio / (ratio + a.alpha * Dd);
                num[p].r = num[p].r + w * s.r;
                num[p].g = num[p].g + w * s.g;
                num[p].b = num[p].b + w * s.b;
                den[p] = den[p] + w;
            }
        }
    }

    unsigned cnt[1] = {0u};
    typedef float f3 __attribute__((ext_vector_type(3)));
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) {
        if (own[p] && den[p] > 0.f) {
            const float d1 = 1.0f + den[p];
            const f3 rgb = {(o[p].r + num[p].r) / d1, (o[p].g + num[p].g) / d1, (o[p].b + num[p].b) / d1};
            __builtin_memcpy(D + (row + (unsigned)(x0 + p * TILE_TX)) * 3u, &rgb, 12);
            cnt[0] += 1u;
        }
    }
    if (a.transfer_count != nullptr) block_count_add<1>(cnt, {a.transfer_count}, frame);
}

}  // namespace

extern "C" int vstab_sharp_transfer_batch(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                                          const float* matrices, const int32_t* cand_frame, int K, const float* ratio, float alpha,
                                          int out_h, int out_w, int interp, int subpix, float* dst, const float* mask,
                                          uint32_t* transfer_count)
{
    const char* who = "vstab_sharp_transfer_batch";
    if (int rc = check_neighbour_call(who, ctx, src, clip_frames, src_h, src_w, first, n, matrices, cand_frame, ratio, K, out_h, out_w,
        interp, subpix, dst, "the transfer samples as the blended fill does, on the 1/32-px coordinates of VSTAB_SUBPIX_Q5")) return rc;
    VSTAB_REQUIRE(alpha >= 0.f && std::isfinite(alpha), "%s: alpha=%g is not a finite number >= 0", who, (double)alpha);
    const size_t pairs = (size_t)n * K;
    for (size_t i = 0; i < pairs; i++)
        VSTAB_REQUIRE(ratio[i] >= 0.f && std::isfinite(ratio[i]), "%s: ratio[%zu]=%g is not a finite number >= 0", who, i, (double)ratio[i]);

    std::vector<FillCand> cd(pairs);
    if (int rc = fill_cand_records(who, matrices, cand_frame, pairs, clip_frames, cd.data())) return rc;
    std::vector<int> live;                                         // the frames with a candidate that is not skipped and has ratio > 0
    for (int f = 0; f < n; f++) {
        bool any = false;
        for (int k = 0; k < K && !any; k++) any = cd[(size_t)f * K + k].frame >= 0 && ratio[(size_t)f * K + k] > 0.f;
        if (any) live.push_back(f);
    }

    VSTAB_HIP(hipSetDevice(ctx->device));
    KernelTimer timer(ctx, "sharp_transfer");
    if (int rc = zero_counts(ctx, n, {transfer_count})) return rc;
    if (live.empty()) return 0;                                    // no frame borrows anything: dst keeps every byte
    SharpArgs a{};
    a.src = src; a.dst = dst; a.mask = mask; a.transfer_count = transfer_count; a.alpha = alpha;
    unsigned blocks = 0;
    if (int rc = set_geometry(who, a, (int)live.size(), K, src_h, src_w, out_h, out_w, &blocks)) return rc;
    StagePart staged[3] = {{cd.data(), pairs * sizeof(FillCand)}, {ratio, pairs * sizeof(float)}, {live.data(), live.size() * sizeof(int)}};
    if (stage_parts(ctx, staged, 3)) return 1;
    const dim3 grid(blocks);
    LAUNCH_INTERP(sharp_transfer_kernel, a, static_cast<const FillCand*>(staged[0].dev), static_cast<const float*>(staged[1].dev), static_cast<const int*>(staged[2].dev));
    VSTAB_HIP(hipGetLastError());
    return 0;
}
