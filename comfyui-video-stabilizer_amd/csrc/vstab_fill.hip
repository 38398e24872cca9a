// vstab_fill.hip -- spatial fill: push-pull inpainting of the pixels that stay padding (the rule: include/vstab.h).
//
// One float4 {r, g, b, valid} record per pyramid cell of levels >= 1, per frame, in ctx->d_sfill.  Kernel boundaries are
// the only synchronisation between levels:
//   sfill_pull0_kernel   reads dst and mask once; a 64 x 32 tile gives its cells of levels 1..3 through LDS; counts holes
//   sfill_pull_kernel    one level from the one below, for the levels between 3 and the tail
//   sfill_tail_kernel    one workgroup per frame: the levels that fit its LDS, up to 1 x 1 and back down
//   sfill_push_kernel    one level from the one above, invalid cells only
//   sfill_push0_kernel   level 0: hole pixels only, 12 B each
// Every kernel behind the first returns per workgroup on its frame's word (holes == 0, later: no valid pixel either).
#include "vstab_internal.h"

namespace {

constexpr int SFILL_MAX_LEVELS = 32;     // levels above level 0: ceil(log2(INT_MAX)) = 31
constexpr int SFILL_TILE_W = 64, SFILL_TILE_H = 32;   // level-0 tile of the first pass: 32x16, 16x8, 8x4 cells of levels 1..3
constexpr int SFILL_TAIL_CELLS = 4032;   // records the tail kernel holds: 63 KB of LDS
constexpr size_t SFILL_WORKSPACE_MAX = (size_t)1 << 30;

struct Pyramid {
    int levels;                          // L: number of levels above the frame (0 for a 1 x 1 frame)
    int tail;                            // T: the tail kernel holds levels T..L in LDS
    int h[SFILL_MAX_LEVELS + 1];         // [0] is the frame; 0 behind level L
    int w[SFILL_MAX_LEVELS + 1];
    unsigned off[SFILL_MAX_LEVELS + 1];  // first record of level l >= 1 within a frame's records
    unsigned cells;                      // records per frame
};

__device__ __forceinline__ bool is_hole(float m) { return !(m <= 0.5f); }

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// a record as a tap: an invalid cell enters as +0.0f
__device__ __forceinline__ float4 as_tap(float4 r) { return r.w != 0.f ? r : zero4(); }

// one pull cell from its four taps (already +0.0f where invalid or outside)
__device__ __forceinline__ float4 pull_cell(float4 t00, float4 t01, float4 t10, float4 t11)
{
    const int n = (t00.w != 0.f) + (t01.w != 0.f) + (t10.w != 0.f) + (t11.w != 0.f);
    if (n == 0) return zero4();
    const float fn = (float)n;
    return make_float4(((t00.x + t01.x) + (t10.x + t11.x)) / fn, ((t00.y + t01.y) + (t10.y + t11.y)) / fn,
                       ((t00.z + t01.z) + (t10.z + t11.z)) / fn, 1.f);
}

// up(F)(y, x) from a coarse level of hc x wc records at F; .w of the result is 0 (the cell stays invalid)
__device__ __forceinline__ float4 upsample(const float4* F, int hc, int wc, int y, int x)
{
    const int yn = y >> 1, xn = x >> 1;
    int yf = (y & 1) ? yn + 1 : yn - 1;
    int xf = (x & 1) ? xn + 1 : xn - 1;
    yf = yf < 0 ? 0 : (yf > hc - 1 ? hc - 1 : yf);
    xf = xf < 0 ? 0 : (xf > wc - 1 ? wc - 1 : xf);
    const float4 a = F[(size_t)yn * wc + xn], b = F[(size_t)yn * wc + xf];
    const float4 c = F[(size_t)yf * wc + xn], d = F[(size_t)yf * wc + xf];
    const float nx = a.x * 0.75f + b.x * 0.25f, ny = a.y * 0.75f + b.y * 0.25f, nz = a.z * 0.75f + b.z * 0.25f;
    const float fx = c.x * 0.75f + d.x * 0.25f, fy = c.y * 0.75f + d.y * 0.25f, fz = c.z * 0.75f + d.z * 0.25f;
    return make_float4(nx * 0.75f + fx * 0.25f, ny * 0.75f + fy * 0.25f, nz * 0.75f + fz * 0.25f, 0.f);
}

__device__ __forceinline__ float4 level0_tap(const float* frame, const float* mask, int h, int w, int y, int x, unsigned& holes)
{
    if (y >= h || x >= w) return zero4();
    const size_t i = (size_t)y * w + x;
    if (is_hole(mask[i])) {
        holes++;
        return zero4();
    }
    const float* p = frame + i * 3;
    return make_float4(p[0], p[1], p[2], 1.f);
}

// grid (tiles_x, tiles_y, frames), 256 threads
__global__ __launch_bounds__(256) void sfill_pull0_kernel(const float* __restrict__ dst, const float* __restrict__ mask,
                                                          float4* __restrict__ rec, unsigned* __restrict__ holes_out, Pyramid p)
{
    __shared__ float4 l1[SFILL_TILE_H / 2][SFILL_TILE_W / 2];
    __shared__ float4 l2[SFILL_TILE_H / 4][SFILL_TILE_W / 4];
    __shared__ BlockSums<unsigned, 1, 256> s_holes;
    const int t = threadIdx.x, f = blockIdx.z;
    const int h = p.h[0], w = p.w[0];
    const size_t px = (size_t)h * w;
    const float* frame = dst + (size_t)f * px * 3;
    const float* m = mask + (size_t)f * px;
    float4* r = rec + (size_t)f * p.cells;

    unsigned holes = 0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int idx = t + k * 256, ly = idx >> 5, lx = idx & 31;
        const int Y = blockIdx.y * (SFILL_TILE_H / 2) + ly, X = blockIdx.x * (SFILL_TILE_W / 2) + lx;
        float4 c = zero4();
        if (2 * (long long)Y < h && 2 * (long long)X < w) {
            const float4 t00 = level0_tap(frame, m, h, w, 2 * Y, 2 * X, holes);
            const float4 t01 = level0_tap(frame, m, h, w, 2 * Y, 2 * X + 1, holes);
            const float4 t10 = level0_tap(frame, m, h, w, 2 * Y + 1, 2 * X, holes);
            const float4 t11 = level0_tap(frame, m, h, w, 2 * Y + 1, 2 * X + 1, holes);
            c = pull_cell(t00, t01, t10, t11);
            if (p.levels >= 1) r[p.off[1] + (size_t)Y * p.w[1] + X] = c;   // (a 1 x 1 frame has no level 1: holes are counted only)
        }
        l1[ly][lx] = c;   // cells outside the level are invalid taps of the level above
    }
    // holes of the tile: BlockSums (vstab_internal.h), one atomic per workgroup
    s_holes.put({holes});
    __syncthreads();
    if (t == 0) {
        const unsigned total = s_holes.total(0);
        if (total) atomicAdd(&holes_out[f], total);
    }
    if (t < 128) {
        const int ly = t >> 4, lx = t & 15;
        const float4 c = pull_cell(as_tap(l1[2 * ly][2 * lx]), as_tap(l1[2 * ly][2 * lx + 1]), as_tap(l1[2 * ly + 1][2 * lx]),
                                   as_tap(l1[2 * ly + 1][2 * lx + 1]));
        const int Y = blockIdx.y * (SFILL_TILE_H / 4) + ly, X = blockIdx.x * (SFILL_TILE_W / 4) + lx;
        if (Y < p.h[2] && X < p.w[2]) r[p.off[2] + (size_t)Y * p.w[2] + X] = c;
        l2[ly][lx] = c;
    }
    __syncthreads();
    if (t < 32) {
        const int ly = t >> 3, lx = t & 7;
        const float4 c = pull_cell(as_tap(l2[2 * ly][2 * lx]), as_tap(l2[2 * ly][2 * lx + 1]), as_tap(l2[2 * ly + 1][2 * lx]),
                                   as_tap(l2[2 * ly + 1][2 * lx + 1]));
        const int Y = blockIdx.y * (SFILL_TILE_H / 8) + ly, X = blockIdx.x * (SFILL_TILE_W / 8) + lx;
        if (Y < p.h[3] && X < p.w[3]) r[p.off[3] + (size_t)Y * p.w[3] + X] = c;
    }
}

// level l (>= 2) from level l - 1; grid (ceil(w_l / 64), ceil(h_l / 4), frames), block (64, 4)
__global__ __launch_bounds__(256) void sfill_pull_kernel(float4* __restrict__ rec, const unsigned* __restrict__ holes, Pyramid p, int l)
{
    const int f = blockIdx.z;
    if (holes[f] == 0) return;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int hl = p.h[l], wl = p.w[l], hs = p.h[l - 1], ws = p.w[l - 1];
    if (x >= wl || y >= hl) return;
    float4* r = rec + (size_t)f * p.cells;
    const float4* src = r + p.off[l - 1];
    const bool x1 = 2 * x + 1 < ws, y1 = 2 * y + 1 < hs;   // (2y, 2x) is always inside
    const float4 t00 = as_tap(src[(size_t)(2 * y) * ws + 2 * x]);
    const float4 t01 = x1 ? as_tap(src[(size_t)(2 * y) * ws + 2 * x + 1]) : zero4();
    const float4 t10 = y1 ? as_tap(src[(size_t)(2 * y + 1) * ws + 2 * x]) : zero4();
    const float4 t11 = (x1 && y1) ? as_tap(src[(size_t)(2 * y + 1) * ws + 2 * x + 1]) : zero4();
    r[p.off[l] + (size_t)y * wl + x] = pull_cell(t00, t01, t10, t11);
}

// levels T..L of one frame in LDS: pull to 1 x 1, push back down to T, store T's invalid cells; grid (frames), 256 threads.
// Writes the frame's word for the push kernels and its counts.
__global__ __launch_bounds__(256) void sfill_tail_kernel(float4* __restrict__ rec, const unsigned* __restrict__ holes,
                                                         unsigned* __restrict__ active, unsigned* __restrict__ hole_count,
                                                         unsigned* __restrict__ fill_count, Pyramid p)
{
    __shared__ float4 s[SFILL_TAIL_CELLS];
    const int t = threadIdx.x, f = blockIdx.x;
    const unsigned nh = holes[f];
    const int T = p.tail, L = p.levels;
    if (nh == 0 || L == 0) {   // nothing to fill (a 1 x 1 frame is either valid or all hole)
        if (t == 0) {
            active[f] = 0;
            if (hole_count) hole_count[f] = nh;
            if (fill_count) fill_count[f] = 0;
        }
        return;
    }
    float4* r = rec + (size_t)f * p.cells;
    const unsigned base = p.off[T];
    const int cells_t = p.h[T] * p.w[T];
    for (int i = t; i < cells_t; i += 256) s[i] = as_tap(r[base + i]);
    __syncthreads();
    for (int l = T + 1; l <= L; l++) {
        const float4* src = s + (p.off[l - 1] - base);
        float4* out = s + (p.off[l] - base);
        const int hl = p.h[l], wl = p.w[l], hs = p.h[l - 1], ws = p.w[l - 1];
        for (int i = t; i < hl * wl; i += 256) {
            const int y = i / wl, x = i - y * wl;
            const bool x1 = 2 * x + 1 < ws, y1 = 2 * y + 1 < hs;
            const float4 t00 = as_tap(src[(2 * y) * ws + 2 * x]);
            const float4 t01 = x1 ? as_tap(src[(2 * y) * ws + 2 * x + 1]) : zero4();
            const float4 t10 = y1 ? as_tap(src[(2 * y + 1) * ws + 2 * x]) : zero4();
            const float4 t11 = (x1 && y1) ? as_tap(src[(2 * y + 1) * ws + 2 * x + 1]) : zero4();
            out[i] = pull_cell(t00, t01, t10, t11);
        }
        __syncthreads();
    }
    const bool any_valid = s[p.off[L] - base].w != 0.f;   // the 1 x 1 top
    if (t == 0) {
        active[f] = any_valid ? 1u : 0u;
        if (hole_count) hole_count[f] = nh;
        if (fill_count) fill_count[f] = any_valid ? nh : 0u;
    }
    if (!any_valid) return;   // the whole frame is hole: left untouched
    for (int l = L - 1; l >= T; l--) {
        float4* cur = s + (p.off[l] - base);
        const float4* up = s + (p.off[l + 1] - base);
        const int hl = p.h[l], wl = p.w[l], hc = p.h[l + 1], wc = p.w[l + 1];
        for (int i = t; i < hl * wl; i += 256) {
            if (cur[i].w != 0.f) continue;
            const int y = i / wl, x = i - y * wl;
            cur[i] = upsample(up, hc, wc, y, x);
        }
        __syncthreads();
    }
    for (int i = t; i < cells_t; i += 256)
        if (s[i].w == 0.f) r[base + i] = s[i];
}

// level l (1 <= l < T) from level l + 1: invalid cells take up(F); grid (ceil(w_l / 64), ceil(h_l / 4), frames), block (64, 4)
__global__ __launch_bounds__(256) void sfill_push_kernel(float4* __restrict__ rec, const unsigned* __restrict__ active, Pyramid p, int l)
{
    const int f = blockIdx.z;
    if (active[f] == 0) return;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int hl = p.h[l], wl = p.w[l];
    if (x >= wl || y >= hl) return;
    float4* r = rec + (size_t)f * p.cells;
    float4* cell = r + p.off[l] + (size_t)y * wl + x;
    if (cell->w != 0.f) return;
    *cell = upsample(r + p.off[l + 1], p.h[l + 1], p.w[l + 1], y, x);
}

// level 0: hole pixels take up(F_1); grid (ceil(w / 64), ceil(h / 4), frames), block (64, 4)
__global__ __launch_bounds__(256) void sfill_push0_kernel(float* __restrict__ dst, const float* __restrict__ mask,
                                                          const float4* __restrict__ rec, const unsigned* __restrict__ active, Pyramid p)
{
    const int f = blockIdx.z;
    if (active[f] == 0) return;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int h = p.h[0], w = p.w[0];
    if (x >= w || y >= h) return;
    const size_t i = (size_t)f * h * w + (size_t)y * w + x;
    if (!is_hole(mask[i])) return;
    const float4 v = upsample(rec + (size_t)f * p.cells + p.off[1], p.h[1], p.w[1], y, x);
    float* o = dst + i * 3;
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
}

inline unsigned ceil_div(int a, int b) { return (unsigned)((a + b - 1) / b); }

}  // namespace

extern "C" int vstab_spatial_fill_batch(vstab_ctx* ctx, float* dst, const float* mask, int n, int h, int w, int chunk_frames,
                                        uint32_t* hole_count, uint32_t* fill_count)
{
    const char* who = "vstab_spatial_fill_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(dst != nullptr && mask != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(chunk_frames >= 0, "%s: chunk_frames=%d is negative", who, chunk_frames);
    // grid.y carries 4 rows per workgroup in the push kernels
    VSTAB_REQUIRE(h <= 4 * 65535, "%s: h=%d above %d rows", who, h, 4 * 65535);

    Pyramid p{};
    p.h[0] = h;
    p.w[0] = w;
    size_t cells = 0;
    int L = 0;
    while (p.h[L] > 1 || p.w[L] > 1) {
        p.h[L + 1] = (p.h[L] + 1) >> 1;
        p.w[L + 1] = (p.w[L] + 1) >> 1;
        L++;
        p.off[L] = (unsigned)cells;
        cells += (size_t)p.h[L] * p.w[L];
        VSTAB_REQUIRE(cells * sizeof(float4) + 8 <= SFILL_WORKSPACE_MAX, "%s: the pyramid of one %d x %d frame exceeds the 1 GiB workspace", who, w, h);
    }
    p.levels = L;
    p.cells = (unsigned)cells;
    const int first_pass_levels = L < 3 ? L : 3;
    // the tail starts at the lowest level from which the rest of the pyramid fits its LDS: level 1 for a small frame (it
    // forms the levels above again from the first pass's level 1, in the same arithmetic), above level 3 for a large one
    int T = L < 1 ? L : 1;
    while (T < L && cells - p.off[T] > (size_t)SFILL_TAIL_CELLS) T++;   // (level L alone is one cell)
    p.tail = T;

    // frames per pass: the workspace stays at or below 1 GiB, grid.z at or below 65535
    const size_t per_frame = (cells ? cells : 1) * sizeof(float4) + 2 * sizeof(unsigned);
    size_t chunk = SFILL_WORKSPACE_MAX / per_frame;
    if (chunk > 65535) chunk = 65535;
    if (chunk_frames > 0 && (size_t)chunk_frames < chunk) chunk = (size_t)chunk_frames;
    if (chunk > (size_t)n) chunk = (size_t)n;

    VSTAB_HIP(hipSetDevice(ctx->device));
    if (ctx->d_sfill.reserve(chunk * per_frame)) return 1;
    float4* rec = static_cast<float4*>(ctx->d_sfill.ptr);
    unsigned* holes = reinterpret_cast<unsigned*>(rec + chunk * (cells ? cells : 1));
    unsigned* active = holes + chunk;

    KernelTimer timer(ctx, "sfill");
    const dim3 block2d(64, 4);
    const size_t px = (size_t)h * w;
    for (size_t first = 0; first < (size_t)n; first += chunk) {
        const unsigned frames = (unsigned)((size_t)n - first < chunk ? (size_t)n - first : chunk);
        float* d = dst + first * px * 3;
        const float* m = mask + first * px;
        VSTAB_HIP(hipMemsetAsync(holes, 0, sizeof(unsigned) * frames, ctx->stream));
        hipLaunchKernelGGL(sfill_pull0_kernel, dim3(ceil_div(w, SFILL_TILE_W), ceil_div(h, SFILL_TILE_H), frames), dim3(256), 0,
                           ctx->stream, d, m, rec, holes, p);
        for (int l = first_pass_levels + 1; l <= T; l++)
            hipLaunchKernelGGL(sfill_pull_kernel, dim3(ceil_div(p.w[l], 64), ceil_div(p.h[l], 4), frames), block2d, 0, ctx->stream,
                               rec, holes, p, l);
        hipLaunchKernelGGL(sfill_tail_kernel, dim3(frames), dim3(256), 0, ctx->stream, rec, holes, active,
                           hole_count ? hole_count + first : nullptr, fill_count ? fill_count + first : nullptr, p);
        if (L >= 1) {
            for (int l = T - 1; l >= 1; l--)
                hipLaunchKernelGGL(sfill_push_kernel, dim3(ceil_div(p.w[l], 64), ceil_div(p.h[l], 4), frames), block2d, 0, ctx->stream,
                                   rec, active, p, l);
            hipLaunchKernelGGL(sfill_push0_kernel, dim3(ceil_div(w, 64), ceil_div(h, 4), frames), block2d, 0, ctx->stream, d, m, rec,
                               active, p);
        }
        VSTAB_HIP(hipGetLastError());
    }
    return 0;
}
