// vstab_handoff.hip -- mask hand-off: hold, grow and feather a padding mask for a generative outpainter (the rules:
// include/vstab.h, vstab_mask_hold_batch and vstab_mask_grow_batch).  Every operation is a maximum, taken on integers: a float
// is compared through its order key (mh_key: sign-magnitude bits turned into a two's-complement integer, so -0.0 < +0.0 and
// the order is total once a NaN has been read as 1.0f), the feather on 16-bit fixed-point levels.  An integer maximum is the
// same in any order, so the result equals the NumPy restatement in bits whatever the decomposition below.
//
//   mask_hold_kernel<VEC>  streaming: one float4 (VEC, h * w a multiple of 4 and both pointers 16-byte aligned) or one float
//                          per lane, the maximum over the frame's window [lo, hi] of the same pixel.  The window table comes
//                          from the host (shots and clip ends are cut there).  The 2T + 1 reads are whole-frame re-reads.
//   mask_relax_kernel      one pass of up to 16 one-step relaxations.  A workgroup of 256 threads owns a 64 x 32 core tile and
//                          stages it with a halo of H = the pass's steps into LDS as 32-bit integers, rows packed densely
//                          (pitch = 64 + 2H words): the lanes of a wavefront own consecutive words, and so are the words of
//                          each of their 4 or 8 neighbour reads -- no two lanes of a ds_read_b32 group share a bank.  Two
//                          buffers ping-pong; step s writes the cells at least s away from the region's edge (the valid
//                          region shrinks by one per step and ends as the core).  Cells outside the frame hold the identity
//                          and are never relaxed: the ball stays clipped to the frame.  Flat steps (grow: max of the keys;
//                          an erosion runs on the complemented keys, ~k reverses the order) come first, then the cells are
//                          quantised in place (gain_q of vstab_neighbour.hip) and the integer steps (feather: max of
//                          neighbour - step) follow.  The core is stored once, counted where asked (block_count_add).
//                          The first form of this kernel walked its cells with run-time indices and tested every cell's
//                          range in every step: about 40 VALU instructions per cell and step, and it ran at exactly the rate
//                          that count predicts (5.3 ms for grow 5 on 256 x 1080p).  This form keeps a cell's MARGIN (the
//                          steps it takes part in) in 5-bit register fields formed while staging and unrolls the cell
//                          loops, so offsets and fields are instruction constants; LDS is sized per launch.
// A radius above 16 is split into passes -- balls and cones of one norm compose, D_a (+) D_b = D_(a+b), also clipped to a
// rectangle, where a shortest lattice path between two pixels stays inside their bounding box -- that alternate between
// `out` and the context's grow-only workspace (d_sfill, which the spatial fill uses inside its own calls only; calls on one
// context are ordered on its stream), a chunk of frames at a time, at most 1 GiB, the last pass landing in `out`.
// Between two feather passes the levels travel as float Q / 65536, whose quantisation gives Q back exactly.
#include "vstab_internal.h"

#include <algorithm>

namespace {

typedef float mh_f4 __attribute__((ext_vector_type(4)));

constexpr int MH_THREADS = 256;
constexpr int MH_TW = 64, MH_TH = 32;                    // the core tile: 2048 pixels, 8 per thread
constexpr int MH_MAX_STEPS = 16;                         // per pass = the widest halo
constexpr int MH_FLAT_IDENT = (int)0x80000000;           // below every key (it is the key of a NaN pattern, which is never formed)
constexpr int MH_CONE_IDENT = -(1 << 30);                // 16 decrements of at most 32768 stay far from wrapping, and below 0

// a NaN reads as 1.0f; then the order key: for v >= +0 its bits, for v <= -0 the bits with the low 31 inverted
__device__ __forceinline__ int mh_key_of_bits(int b) { return b ^ ((b >> 31) & 0x7fffffff); }
__device__ __forceinline__ int mh_key(float v) { return mh_key_of_bits(__float_as_int(v != v ? 1.0f : v)); }
__device__ __forceinline__ float mh_unkey(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

// the blended fill's 16-bit quantiser (vstab_neighbour.hip: gain_q)
__device__ __forceinline__ int mh_q16(float v) { return v > 0.f ? (v < 1.f ? (int)(unsigned)(v * 65536.0f) : 65536) : 0; }

// ---- hold -----------------------------------------------------------------------------------------------------------------
// grid: ceil(n * per_frame / 256) blocks; per_frame = px / 4 (VEC) or px items of a frame; window host-formed {lo, hi} per frame
template <bool VEC>
__global__ __launch_bounds__(MH_THREADS) void mask_hold_kernel(const float* __restrict__ mask, unsigned per_frame, unsigned long long items,
                                                               const int2* __restrict__ window, float* __restrict__ out)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * MH_THREADS + threadIdx.x;
    if (i >= items) return;
    const unsigned frame = (unsigned)(i / per_frame);
    const unsigned long long at = i - (unsigned long long)frame * per_frame;
    const int2 win = window[frame];                       // 0 <= lo <= frame <= hi < n
    if (VEC) {
        const mh_f4* src = reinterpret_cast<const mh_f4*>(mask);
        int k0 = MH_FLAT_IDENT, k1 = MH_FLAT_IDENT, k2 = MH_FLAT_IDENT, k3 = MH_FLAT_IDENT;
        for (int j = win.x; j <= win.y; j++) {
            const mh_f4 v = src[(unsigned long long)j * per_frame + at];
            k0 = max(k0, mh_key(v.x)); k1 = max(k1, mh_key(v.y)); k2 = max(k2, mh_key(v.z)); k3 = max(k3, mh_key(v.w));
        }
        reinterpret_cast<mh_f4*>(out)[i] = mh_f4{mh_unkey(k0), mh_unkey(k1), mh_unkey(k2), mh_unkey(k3)};
    } else {
        int k = MH_FLAT_IDENT;
        for (int j = win.x; j <= win.y; j++) k = max(k, mh_key(mask[(unsigned long long)j * per_frame + at]));
        out[i] = mh_unkey(k);
    }
}

// ---- grow and feather: one pass -------------------------------------------------------------------------------------------
struct RelaxPass {
    int flat;         // one-step flat relaxations of this pass (grow)
    int cone;         // one-step integer relaxations with the decrement behind them (feather); flat + cone <= 16
    int step;         // the feather's decrement per pixel of distance, 65536 / (f + 1)
    int erode;        // the flat steps take minima: they run on the complemented keys
    int square;       // 8 neighbours (L-infinity ball) instead of 4 (L1 ball)
    int nan_one;      // a NaN loaded from `src` reads as 1.0f (any pass of a call that grows or feathers)
};

template <bool SQUARE>
__device__ __forceinline__ int relax_neighbours(const int* __restrict__ cur, int i, int rw)
{
    int m = max(max(cur[i - 1], cur[i + 1]), max(cur[i - rw], cur[i + rw]));
    if (SQUARE) m = max(m, max(max(cur[i - rw - 1], cur[i - rw + 1]), max(cur[i + rw - 1], cur[i + rw + 1])));
    return m;
}

// A thread's cells: word t of the staged region, then every 256th -- at most 24.  Everything a step needs to know of a cell
// is its MARGIN, the distance to the nearest edge of the region (0 for a cell outside the frame or outside the region): step s
// writes the cells with margin >= s.  The margins are formed once, while staging, and kept as 5-bit fields of four registers;
// the loops over the cells are unrolled, so a cell's field, its LDS offset (256 k words) and those of its neighbours are
// constants of the instruction and a cell-step costs about ten VALU instructions.
constexpr int MH_CELLS = 24;                 // per thread: 96 x 64 / 256
constexpr int MH_BATCH = 4;                  // LDS reads of a relaxation step in flight: 4 cells x 5 or 9
constexpr int MH_STAGE_BATCH = 8;            // global loads of the staging in flight
constexpr int MH_MARGIN_BITS = 5, MH_MARGINS_PER_WORD = 6, MH_MARGIN_WORDS = MH_CELLS / MH_MARGINS_PER_WORD;
constexpr int MH_PAD = MH_BATCH * MH_THREADS;   // a buffer is padded to whole batches, so that a batch reads unconditionally

struct CellWalk {                            // (column, row) of a thread's cells, stepped with one wrap test and no division
    int i, lx, ly;
    __device__ __forceinline__ void next(int dx, int dy, int rw)
    {
        i += MH_THREADS; lx += dx; ly += dy;
        if (lx >= rw) { lx -= rw; ly++; }
    }
};

__device__ __forceinline__ int cell_margin(const unsigned (&margins)[MH_MARGIN_WORDS], int k)
{
    return (int)((margins[k / MH_MARGINS_PER_WORD] >> (MH_MARGIN_BITS * (k % MH_MARGINS_PER_WORD))) & ((1u << MH_MARGIN_BITS) - 1u));
}

// One relaxation step: the cells with margin >= s take max(own, best neighbour - dec).  cur / nxt point at the thread's first
// cell.  Every read of a batch is unconditional: the buffers are padded to whole batches and have a guard of a row and a word
// on both sides, so the neighbours of any word of the padded buffer lie in the allocation; what a cell without margin reads
// is discarded.  A cell outside the frame is never written: it keeps the identity it was staged with, in both buffers.
template <bool SQUARE>
__device__ __forceinline__ void relax_step(const int* __restrict__ cur, int* __restrict__ nxt, const unsigned (&margins)[MH_MARGIN_WORDS],
                                           int cells, int rw, int s, int dec)
{
#pragma unroll
    for (int b = 0; b < MH_CELLS / MH_BATCH; b++) {
        if (b * MH_PAD < cells) {                                        // (uniform)
            int own[MH_BATCH], best[MH_BATCH];
#pragma unroll
            for (int u = 0; u < MH_BATCH; u++) {
                const int o = (b * MH_BATCH + u) * MH_THREADS;
                own[u] = cur[o];
                best[u] = relax_neighbours<SQUARE>(cur, o, rw);
            }
#pragma unroll
            for (int u = 0; u < MH_BATCH; u++)
                if (cell_margin(margins, b * MH_BATCH + u) >= s) nxt[(b * MH_BATCH + u) * MH_THREADS] = max(own[u], best[u] - dec);
        }
    }
}

// grid (tiles_x * tiles_y * n), 256 threads, dynamic LDS relax_lds_bytes(halo); h * w < 2^31
template <bool SQUARE>
__global__ __launch_bounds__(MH_THREADS) void mask_relax_kernel(const float* __restrict__ src, int h, int w, unsigned tiles_x,
                                                                unsigned tiles_per_frame, RelaxPass ps, float* __restrict__ dst,
                                                                unsigned* __restrict__ count)
{
    extern __shared__ int s_cells[];                                     // [guard][padded][guard], twice: the launch sizes it
    const int t = (int)threadIdx.x;
    const unsigned frame = blockIdx.x / tiles_per_frame, tile = blockIdx.x - frame * tiles_per_frame;
    const unsigned tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int halo = ps.flat + ps.cone;                                  // 0..16
    const int rw = MH_TW + 2 * halo, rh = MH_TH + 2 * halo, cells = rw * rh;   // the staged region, at most 96 x 64
    const int padded = (cells + MH_PAD - 1) / MH_PAD * MH_PAD, guard = rw + 1;
    const int gx0 = (int)tile_x * MH_TW - halo, gy0 = (int)tile_y * MH_TH - halo;   // the frame position of region cell (0, 0)
    const size_t px = (size_t)h * (size_t)w;
    const float* __restrict__ f = src + (size_t)frame * px;
    const int dx = MH_THREADS % rw, dy = MH_THREADS / rw;                // a thread's next cell: 256 words on, as (column, row)
    int* const s_a = s_cells + guard;
    int* const s_b = s_a + padded + 2 * guard;

    // stage the region into BOTH buffers: the key (complemented for an erosion) of every in-frame cell, the identity outside
    // the frame; and form the margins
    unsigned margins[MH_MARGIN_WORDS] = {0u, 0u, 0u, 0u};
    {
        CellWalk c = {t, t % rw, t / rw};
#pragma unroll
        for (int b = 0; b < MH_CELLS / MH_STAGE_BATCH; b++) {
            if (b * MH_STAGE_BATCH * MH_THREADS < cells) {               // (uniform)
                float v[MH_STAGE_BATCH];
                bool inside[MH_STAGE_BATCH];
#pragma unroll
                for (int u = 0; u < MH_STAGE_BATCH; u++) {               // the batch's loads first
                    const int k = b * MH_STAGE_BATCH + u;
                    const int x = gx0 + c.lx, y = gy0 + c.ly;
                    inside[u] = c.i < cells && x >= 0 && x < w && y >= 0 && y < h;
                    v[u] = inside[u] ? f[(size_t)y * (size_t)w + (size_t)x] : 0.f;
                    const int margin = inside[u] ? min(min(c.lx, rw - 1 - c.lx), min(c.ly, rh - 1 - c.ly)) : 0;   // <= 31: rh <= 64
                    margins[k / MH_MARGINS_PER_WORD] |= (unsigned)margin << (MH_MARGIN_BITS * (k % MH_MARGINS_PER_WORD));
                    c.next(dx, dy, rw);
                }
#pragma unroll
                for (int u = 0; u < MH_STAGE_BATCH; u++) {
                    const int i = t + (b * MH_STAGE_BATCH + u) * MH_THREADS;
                    if (i < cells) {
                        int k = ps.nan_one ? mh_key(v[u]) : mh_key_of_bits(__float_as_int(v[u]));   // (a call without steps keeps a NaN's bits)
                        if (ps.erode) k = ~k;
                        k = inside[u] ? k : MH_FLAT_IDENT;
                        s_a[i] = k;
                        s_b[i] = k;
                    }
                }
            }
        }
    }
    __syncthreads();

    int* cur = s_a;
    int* nxt = s_b;
    // flat steps: step s (1-based, counted over the whole pass) writes the cells at least s from the region's edge
    for (int s = 1; s <= ps.flat; s++) {
        relax_step<SQUARE>(cur + t, nxt + t, margins, cells, rw, s, 0);
        __syncthreads();
        int* sw = cur; cur = nxt; nxt = sw;
    }

    if (ps.cone > 0) {
        // the valid cells become 16-bit levels in place; a cell outside the frame takes the levels' identity in both buffers
        const int s0 = ps.flat;
#pragma unroll
        for (int k = 0; k < MH_CELLS; k++) {
            const int i = t + k * MH_THREADS;
            if (i < cells) {
                const int c = cur[i];
                if (c == MH_FLAT_IDENT) {
                    cur[i] = MH_CONE_IDENT;
                    nxt[i] = MH_CONE_IDENT;
                } else if (cell_margin(margins, k) >= s0) {
                    cur[i] = mh_q16(mh_unkey(ps.erode ? ~c : c));
                }
            }
        }
        __syncthreads();
        for (int s = s0 + 1; s <= halo; s++) {
            relax_step<SQUARE>(cur + t, nxt + t, margins, cells, rw, s, ps.step);
            __syncthreads();
            int* sw = cur; cur = nxt; nxt = sw;
        }
    }

    // the core, stored once: rows of 64 consecutive floats
    unsigned above[1] = {0u};
    const int lx = t & (MH_TW - 1);
    const int x = (int)tile_x * MH_TW + lx;
#pragma unroll
    for (int r = 0; r < MH_TH / (MH_THREADS / MH_TW); r++) {
        const int ly = (t >> 6) + r * (MH_THREADS / MH_TW);
        const int y = (int)tile_y * MH_TH + ly;
        if (x < w && y < h) {
            const int c = cur[(ly + halo) * rw + lx + halo];
            float v;
            if (ps.cone > 0) v = (float)max(c, 0) * (1.0f / 65536.0f);    // exact: an integer <= 65536 times a power of two
            else v = mh_unkey(ps.erode ? ~c : c);
            dst[(size_t)frame * px + (size_t)y * (size_t)w + (size_t)x] = v;
            above[0] += v > 0.5f ? 1u : 0u;
        }
    }
    if (count != nullptr) {                                               // (uniform over the grid)
        unsigned* const outs[1] = {count};
        block_count_add<1, MH_THREADS>(above, outs, (int)frame);
    }
}

// the kernel's dynamic LDS for a pass of `halo` steps: two buffers of the staged region, each padded to whole batches of
// 1024 words and with a guard of a row and a word in front of and behind it
size_t relax_lds_bytes(int halo)
{
    const size_t rw = MH_TW + 2 * (size_t)halo, rh = MH_TH + 2 * (size_t)halo;
    const size_t padded = (rw * rh + MH_PAD - 1) / MH_PAD * MH_PAD;
    return 2 * sizeof(int) * (padded + 2 * (rw + 1));
}

bool ranges_overlap(const void* a, const void* b, size_t bytes)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace

extern "C" int vstab_mask_hold_batch(vstab_ctx* ctx, const float* mask, int n, int h, int w, int hold, const int32_t* shot, float* out)
{
    const char* who = "vstab_mask_hold_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(mask != nullptr && out != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(hold >= 0 && hold <= VSTAB_MASK_HOLD_MAX, "%s: hold=%d outside 0..%d", who, hold, VSTAB_MASK_HOLD_MAX);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE(((uintptr_t)mask & 3) == 0 && ((uintptr_t)out & 3) == 0, "%s: a pointer argument is not aligned to its element size", who);
    const size_t px = (size_t)h * (size_t)w, bytes = px * (size_t)n * sizeof(float);
    VSTAB_REQUIRE(!ranges_overlap(mask, out, bytes), "%s: out overlaps mask (a pixel's window reads frames that would already be written)", who);
    if (shot != nullptr)
        for (int i = 1; i < n; i++) VSTAB_REQUIRE(shot[i] >= shot[i - 1], "%s: shot[%d]=%d < shot[%d]=%d: not non-decreasing", who, i, shot[i], i - 1, shot[i - 1]);
    const bool vec = (px & 3) == 0 && (((uintptr_t)mask | (uintptr_t)out) & 15) == 0;
    const unsigned long long per_frame = vec ? px >> 2 : px, items = per_frame * (unsigned long long)n;
    const unsigned long long blocks = (items + MH_THREADS - 1) / MH_THREADS;
    VSTAB_REQUIRE(blocks <= 0x7fffffffull, "%s: n=%d frames of %d x %d exceed the grid", who, n, w, h);

    VSTAB_HIP(hipSetDevice(ctx->device));
    KernelTimer timer(ctx, "mask_hold");
    if (hold == 0) {                                       // the input's bits, its NaNs included
        VSTAB_HIP(hipMemcpyAsync(out, mask, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    }
    std::vector<int32_t> window((size_t)n * 2);
    for (int i = 0; i < n; i++) {
        int lo = std::max(i - hold, 0), hi = std::min(i + hold, n - 1);
        if (shot != nullptr) {
            while (shot[lo] != shot[i]) lo++;
            while (shot[hi] != shot[i]) hi--;
        }
        window[(size_t)i * 2] = lo;
        window[(size_t)i * 2 + 1] = hi;
    }
    void* d_window = nullptr;
    if (vstab_stage_params(ctx, window.data(), window.size() * sizeof(int32_t), &d_window)) return 1;
    if (vec)
        hipLaunchKernelGGL(mask_hold_kernel<true>, dim3((unsigned)blocks), dim3(MH_THREADS), 0, ctx->stream, mask, (unsigned)per_frame, items,
                           static_cast<const int2*>(d_window), out);
    else
        hipLaunchKernelGGL(mask_hold_kernel<false>, dim3((unsigned)blocks), dim3(MH_THREADS), 0, ctx->stream, mask, (unsigned)per_frame, items,
                           static_cast<const int2*>(d_window), out);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

extern "C" int vstab_mask_grow_batch(vstab_ctx* ctx, const float* mask, int n, int h, int w, int grow, int footprint, int feather,
                                     float* out, uint32_t* count_out)
{
    const char* who = "vstab_mask_grow_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(mask != nullptr && out != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(grow >= -VSTAB_MASK_GROW_MAX && grow <= VSTAB_MASK_GROW_MAX, "%s: grow=%d outside -%d..%d", who, grow,
                  VSTAB_MASK_GROW_MAX, VSTAB_MASK_GROW_MAX);
    VSTAB_REQUIRE(feather >= 0 && feather <= VSTAB_MASK_FEATHER_MAX, "%s: feather=%d outside 0..%d", who, feather, VSTAB_MASK_FEATHER_MAX);
    VSTAB_REQUIRE(footprint == VSTAB_GROW_TAPERED || footprint == VSTAB_GROW_SQUARE, "%s: unknown footprint %d", who, footprint);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE(((uintptr_t)mask & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)count_out & 3) == 0,
                  "%s: a pointer argument is not aligned to its element size", who);
    const size_t px = (size_t)h * (size_t)w;
    VSTAB_REQUIRE(!ranges_overlap(mask, out, px * (size_t)n * sizeof(float)), "%s: out overlaps mask (a tile's halo reads pixels another "
                  "workgroup would already have written)", who);
    const unsigned tiles_x = ((unsigned)w + MH_TW - 1) / MH_TW, tiles_y = ((unsigned)h + MH_TH - 1) / MH_TH;
    const unsigned long long tiles = (unsigned long long)tiles_x * tiles_y;
    VSTAB_REQUIRE(tiles <= 0x7fffffffull, "%s: %d x %d exceeds the grid", who, w, h);

    // the call's steps, |grow| flat ones then `feather` integer ones, in passes of at most 16
    const int flat_total = grow < 0 ? -grow : grow, total = flat_total + feather;
    const int passes = std::max(1, (total + MH_MAX_STEPS - 1) / MH_MAX_STEPS);
    // frames per chunk: every pass of a chunk before the next chunk, so that the scratch buffer stays at or below 1 GiB
    size_t chunk = (size_t)n;
    if (passes > 1) {
        chunk = std::max<size_t>(1, ((size_t)1 << 30) / (px * sizeof(float)));
        chunk = std::min(chunk, (size_t)n);
    }
    chunk = std::min<size_t>(chunk, (size_t)(0x7fffffffull / tiles));
    VSTAB_REQUIRE(chunk >= 1, "%s: %d x %d exceeds the grid", who, w, h);

    VSTAB_HIP(hipSetDevice(ctx->device));
    KernelTimer timer(ctx, "mask_grow");
    float* scratch = nullptr;
    if (passes > 1) {
        if (ctx->d_sfill.reserve(chunk * px * sizeof(float))) return 1;
        scratch = static_cast<float*>(ctx->d_sfill.ptr);
    }
    if (count_out != nullptr) VSTAB_HIP(hipMemsetAsync(count_out, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    for (size_t first = 0; first < (size_t)n; first += chunk) {
        const size_t frames = std::min(chunk, (size_t)n - first);
        const float* from = mask + first * px;
        float* const final_dst = out + first * px;
        int done = 0;
        for (int p = 0; p < passes; p++) {
            const int steps = std::min(MH_MAX_STEPS, total - done);
            RelaxPass ps;
            ps.flat = std::max(0, std::min(steps, flat_total - done));
            ps.cone = steps - ps.flat;
            ps.step = 65536 / (feather + 1);
            ps.erode = grow < 0 ? 1 : 0;
            ps.square = footprint == VSTAB_GROW_SQUARE ? 1 : 0;
            ps.nan_one = total > 0 ? 1 : 0;
            const bool last = p == passes - 1;
            float* to = ((passes - 1 - p) & 1) ? scratch : final_dst;    // the passes alternate and the last one lands in out
            unsigned* cnt = last && count_out != nullptr ? reinterpret_cast<unsigned*>(count_out) + first : nullptr;
            const dim3 grid((unsigned)(tiles * frames));
            const size_t lds = relax_lds_bytes(ps.flat + ps.cone);       // a small radius leaves room for more workgroups (at most 49.5 KiB)
            if (ps.square)
                hipLaunchKernelGGL(mask_relax_kernel<true>, grid, dim3(MH_THREADS), lds, ctx->stream, from, h, w, tiles_x, (unsigned)tiles, ps, to, cnt);
            else
                hipLaunchKernelGGL(mask_relax_kernel<false>, grid, dim3(MH_THREADS), lds, ctx->stream, from, h, w, tiles_x, (unsigned)tiles, ps, to, cnt);
            from = to;
            done += steps;
        }
    }
    VSTAB_HIP(hipGetLastError());
    return 0;
}
