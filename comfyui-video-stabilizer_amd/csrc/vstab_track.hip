// vstab_track.hip -- template track: one box followed through a clip by a fixed-template search, exact integers
// (the rule: include/vstab_track.h, vstab_track_template_batch).
//
//   track_template_kernel  frame `key`: the template's samples into the scratch, (n_s, sum T, sum T^2), and the key frame's
//                          own outputs (pos = the box, best 0, near / surface 0 at the centre and the sentinel elsewhere)
//   track_search_kernel    one launch per searched frame, one workgroup per dy row of the window.  Every workgroup first
//                          reduces the previous frame's 2R+1 row minima to the previous pick (the start of this frame is the
//                          previous start plus that pick), workgroup 0 writes pos / best / near of the previous frame; then
//                          the workgroup stages the template and, chunk of rows by chunk of rows, the frame rows its
//                          candidates read through LDS, forms sum d and sum d^2 of every dx of its row, writes the costs
//                          and its row minimum.  frame < 0: the resolving half alone (the last frame of a direction).
// The chain is sequential: frame k starts where frame k -+ 1 ended.  The launches are queued back to back on one stream, so the
// order of the stream is the only synchronisation; the row minima and (where the caller wants no surface) the cost surface
// alternate between two slots of the scratch, a launch reading the slot its predecessor wrote.
// A thread is (candidate dx, part): the 256 threads hold 256 / (2R+1) parts per candidate, which share the chunk's rows;
// sum d fits an int (4096 * 255) and sum d^2 an unsigned (4096 * 255^2), J is formed in 64 bits once per candidate.
#include "vstab_internal.h"
#include "../../include/vstab_track.h"

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_TILE_BYTES = 2 * VSTAB_TRACK_MAX_SPAN;     // the staged frame rows of one chunk: at least two rows
constexpr unsigned long long TK_SENTINEL = VSTAB_TRACK_SENTINEL;

// one candidate under the pick's order: (J, dx^2 + dy^2, dy, dx), lexicographic
struct Cand {
    unsigned long long J;
    unsigned d2;
    int dy, dx;
};

__device__ __forceinline__ bool cand_less(const Cand& a, const Cand& b)
{
    if (a.J != b.J) return a.J < b.J;
    if (a.d2 != b.d2) return a.d2 < b.d2;
    if (a.dy != b.dy) return a.dy < b.dy;
    return a.dx < b.dx;
}

// behind every real candidate, the sentinel ones included (their d2 is a real distance)
__device__ __forceinline__ Cand cand_none() { return Cand{TK_SENTINEL, 0xFFFFFFFFu, 0x7fffffff, 0x7fffffff}; }

__device__ __forceinline__ Cand cand_at(unsigned long long J, int dx, int dy) { return Cand{J, (unsigned)(dx * dx + dy * dy), dy, dx}; }

// The minimum over the workgroup, in every thread: wave shuffles, then the four waves through LDS.  All threads call it.
__device__ __forceinline__ Cand block_min(Cand c, Cand* s_wave)
{
    for (int off = 32; off > 0; off >>= 1) {
        Cand o;
        o.J = __shfl_down(c.J, off, 64);
        o.d2 = __shfl_down(c.d2, off, 64);
        o.dy = __shfl_down(c.dy, off, 64);
        o.dx = __shfl_down(c.dx, off, 64);
        if (cand_less(o, c)) c = o;
    }
    __syncthreads();   // (a previous call's readers are done with s_wave)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    Cand r = s_wave[0];
#pragma unroll
    for (int k = 1; k < TK_THREADS / 64; k++)
        if (cand_less(s_wave[k], r)) r = s_wave[k];
    return r;
}

__global__ __launch_bounds__(TK_THREADS) void track_template_kernel(const uint8_t* __restrict__ key_frame, int w, int bx, int by,
                                                                    int nx, int ny, int s, int R, int key, uint8_t* __restrict__ tmpl,
                                                                    unsigned long long* __restrict__ tsums, int* __restrict__ pos,
                                                                    unsigned long long* __restrict__ best,
                                                                    unsigned long long* __restrict__ near,
                                                                    unsigned long long* __restrict__ key_surface)
{
    __shared__ BlockSums<unsigned long long, 2, TK_THREADS> s_sums;
    const int t = threadIdx.x, ns = nx * ny, D = 2 * R + 1;
    unsigned long long v[2] = {0ull, 0ull};
    for (int i = t; i < ns; i += TK_THREADS) {
        const int j = i / nx, ii = i - j * nx;
        const unsigned g = key_frame[(by + j * s) * w + (bx + ii * s)];
        tmpl[i] = (uint8_t)g;
        v[0] += g;
        v[1] += g * g;
    }
    s_sums.put(v);
    __syncthreads();
    if (t == 0) {
        tsums[0] = (unsigned long long)ns;
        tsums[1] = s_sums.total(0);
        tsums[2] = s_sums.total(1);
        pos[2 * key] = bx;
        pos[2 * key + 1] = by;
        best[key] = 0ull;
    }
    if (t < 9) near[(size_t)key * 9 + t] = t == 4 ? 0ull : TK_SENTINEL;
    if (key_surface != nullptr)
        for (int i = t; i < D * D; i += TK_THREADS) key_surface[i] = i == R * D + R ? 0ull : TK_SENTINEL;
}

struct TrackArgs {
    const uint8_t* gray;            // [n,h,w]
    const uint8_t* tmpl;            // n_s samples
    int h, w, nx, ny, s, R;
    int* pos;
    unsigned long long* best;
    unsigned long long* near;
    // the resolving half: frame `prev` was searched by the launch before this one (prev < 0: nothing to resolve, the start is
    // pos[base] as it stands); its start was pos[base]
    int prev, base;
    const unsigned long long* prev_surface;   // [D,D]
    const unsigned long long* prev_rows;      // [D,2] = (cost, dx)
    // the searching half: frame < 0 for none
    int frame;
    unsigned long long* surface;
    unsigned long long* rows;
};

// grid 2R+1 (frame >= 0) or 1 (frame < 0)
__global__ __launch_bounds__(TK_THREADS) void track_search_kernel(TrackArgs a)
{
    __shared__ uint8_t s_tile[TK_TILE_BYTES];
    __shared__ uint8_t s_tmpl[VSTAB_TRACK_MAX_SAMPLES];
    __shared__ int s_sd[TK_THREADS];
    __shared__ unsigned s_sd2[TK_THREADS];
    __shared__ Cand s_wave[TK_THREADS / 64];
    const int t = threadIdx.x, R = a.R, D = 2 * R + 1;

    int px = a.pos[2 * a.base], py = a.pos[2 * a.base + 1];
    if (a.prev >= 0) {
        Cand c = cand_none();
        if (t < D) c = cand_at(a.prev_rows[2 * t], (int)(long long)a.prev_rows[2 * t + 1], t - R);
        c = block_min(c, s_wave);
        px += c.dx;       // (an all-sentinel frame picks (0, 0): the position is carried)
        py += c.dy;
        if (blockIdx.x == 0) {
            if (t == 0) {
                a.pos[2 * a.prev] = px;
                a.pos[2 * a.prev + 1] = py;
                a.best[a.prev] = c.J;
            }
            if (t < 9) {
                const int cx = c.dx + (t % 3 - 1), cy = c.dy + (t / 3 - 1);
                const bool inside = cx >= -R && cx <= R && cy >= -R && cy <= R;
                a.near[(size_t)a.prev * 9 + t] = inside ? a.prev_surface[(cy + R) * D + (cx + R)] : TK_SENTINEL;
            }
        }
    }
    if (a.frame < 0) return;

    const int dy = (int)blockIdx.x - R, qy = py + dy;
    const int reach_x = (a.nx - 1) * a.s, reach_y = (a.ny - 1) * a.s;
    const bool row_inside = qy >= 0 && qy + reach_y <= a.h - 1;       // uniform over the workgroup
    unsigned long long* __restrict__ out_row = a.surface + (size_t)blockIdx.x * D;
    Cand mine = cand_none();
    if (!row_inside) {
        if (t < D) {
            out_row[t] = TK_SENTINEL;
            mine = cand_at(TK_SENTINEL, t - R, dy);
        }
    } else {
        const int ns = a.nx * a.ny;
        for (int i = t; i < ns; i += TK_THREADS) s_tmpl[i] = a.tmpl[i];
        const uint8_t* __restrict__ F = a.gray + (size_t)a.frame * a.h * a.w;
        const int x0 = px - R, span = 2 * R + reach_x + 1;            // span <= VSTAB_TRACK_MAX_SPAN (host-checked)
        const int rows_per_chunk = TK_TILE_BYTES / span;              // >= 2
        const int parts = TK_THREADS / D, cand = t % D, part = t / D;
        const int wave = t >> 6, lane = t & 63;
        int sd = 0;
        unsigned sd2 = 0;
        for (int j0 = 0; j0 < a.ny; j0 += rows_per_chunk) {
            const int rows = min(rows_per_chunk, a.ny - j0);
            __syncthreads();   // the tile is free (first chunk: nothing to wait for but the template's stores, below)
            for (int jj = wave; jj < rows; jj += TK_THREADS / 64) {
                const uint8_t* __restrict__ src = F + (qy + (j0 + jj) * a.s) * a.w;   // a row inside the frame
                uint8_t* __restrict__ dst = s_tile + jj * span;
                for (int xx = lane; xx < span; xx += 64) {
                    const int x = x0 + xx;
                    dst[xx] = (x >= 0 && x < a.w) ? src[x] : (uint8_t)0;   // (a column outside: only sentinel candidates read it)
                }
            }
            __syncthreads();
            if (part < parts) {
                for (int jj = part; jj < rows; jj += parts) {
                    const uint8_t* __restrict__ c_row = s_tile + jj * span + cand;
                    const uint8_t* __restrict__ t_row = s_tmpl + (j0 + jj) * a.nx;
#pragma unroll 4   // (one wave per SIMD: several loads in flight, or every sample pays the whole LDS latency)
                    for (int i = 0; i < a.nx; i++) {
                        const int d = (int)c_row[i * a.s] - (int)t_row[i];
                        sd += d;
                        sd2 += (unsigned)(d * d);
                    }
                }
            }
        }
        s_sd[t] = sd;
        s_sd2[t] = sd2;
        __syncthreads();
        if (t < D) {
            long long S = 0;
            unsigned long long S2 = 0ull;
            for (int p = 0; p < parts; p++) {
                S += s_sd[t + p * D];
                S2 += s_sd2[t + p * D];
            }
            const int qx = px + (t - R);
            const bool inside = qx >= 0 && qx + reach_x <= a.w - 1;
            const unsigned long long J = inside ? (unsigned long long)ns * S2 - (unsigned long long)(S * S) : TK_SENTINEL;
            out_row[t] = J;
            mine = cand_at(J, t - R, dy);
        }
    }
    const Cand m = block_min(mine, s_wave);
    if (t == 0) {
        a.rows[2 * blockIdx.x] = m.J;
        a.rows[2 * blockIdx.x + 1] = (unsigned long long)(long long)m.dx;
    }
}

}  // namespace

extern "C" int vstab_track_template_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, int bx, int by, int bw, int bh,
                                          int stride, int radius, int key, uint64_t* tsums, int32_t* pos, uint64_t* best,
                                          uint64_t* near, uint64_t* surface, uint64_t* work)
{
    const char* who = "vstab_track_template_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(gray != nullptr && tsums != nullptr && pos != nullptr && best != nullptr && near != nullptr && work != nullptr,
                  "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE(key >= 0 && key < n, "%s: key=%d outside a clip of %d frames", who, key, n);
    VSTAB_REQUIRE(radius >= 1 && radius <= VSTAB_TRACK_RADIUS_MAX, "%s: radius=%d outside 1..%d", who, radius, VSTAB_TRACK_RADIUS_MAX);
    VSTAB_REQUIRE(bw >= VSTAB_TRACK_MIN_BOX && bh >= VSTAB_TRACK_MIN_BOX, "%s: a box of %d x %d pixels, the minimum is %d per axis", who,
                  bw, bh, VSTAB_TRACK_MIN_BOX);
    VSTAB_REQUIRE(bx >= 0 && by >= 0 && bw <= w - bx && bh <= h - by, "%s: the box (%d, %d, %d, %d) leaves the %d x %d frame", who, bx, by,
                  bw, bh, w, h);
    const int longest = bw > bh ? bw : bh;
    VSTAB_REQUIRE(stride == (longest + 63) / 64, "%s: stride=%d, the rule gives ceil(max(%d, %d) / 64) = %d", who, stride, bw, bh,
                  (longest + 63) / 64);
    const int nx = bw / stride, ny = bh / stride, D = 2 * radius + 1;
    VSTAB_REQUIRE(nx >= 1 && ny >= 1 && nx * ny <= VSTAB_TRACK_MAX_SAMPLES, "%s: %d x %d samples", who, nx, ny);
    VSTAB_REQUIRE(2 * radius + (nx - 1) * stride + 1 <= VSTAB_TRACK_MAX_SPAN, "%s: a box %d pixels wide, the limit is %d", who, bw,
                  VSTAB_TRACK_MAX_SPAN - 2 * radius);
    VSTAB_REQUIRE(((uintptr_t)tsums & 7) == 0 && ((uintptr_t)pos & 3) == 0 && ((uintptr_t)best & 7) == 0 && ((uintptr_t)near & 7) == 0 &&
                      ((uintptr_t)surface & 7) == 0 && ((uintptr_t)work & 7) == 0,
                  "%s: a pointer argument is not aligned to its element size", who);

    VSTAB_HIP(hipSetDevice(ctx->device));
    KernelTimer timer(ctx, "track_template");
    typedef unsigned long long u64;
    const size_t cells = (size_t)D * D, slot_words = cells + 2 * (size_t)D;
    uint8_t* tmpl = reinterpret_cast<uint8_t*>(work);
    u64* slots = reinterpret_cast<u64*>(work) + VSTAB_TRACK_MAX_SAMPLES / 8;
    u64* user_surface = reinterpret_cast<u64*>(surface);
    // where frame f's costs go (the caller's surface, or the scratch slot) and where its row minima go
    auto surface_of = [&](int f, int slot) { return user_surface ? user_surface + (size_t)f * cells : slots + (size_t)slot * slot_words; };
    auto rows_of = [&](int slot) { return slots + (size_t)slot * slot_words + cells; };

    hipLaunchKernelGGL(track_template_kernel, dim3(1), dim3(TK_THREADS), 0, ctx->stream, gray + (size_t)key * h * w, w, bx, by, nx, ny,
                       stride, radius, key, tmpl, reinterpret_cast<u64*>(tsums), pos, reinterpret_cast<u64*>(best),
                       reinterpret_cast<u64*>(near), user_surface ? user_surface + (size_t)key * cells : nullptr);

    TrackArgs a;
    a.gray = gray; a.tmpl = tmpl; a.h = h; a.w = w; a.nx = nx; a.ny = ny; a.s = stride; a.R = radius;
    a.pos = pos; a.best = reinterpret_cast<u64*>(best); a.near = reinterpret_cast<u64*>(near);
    int slot = 0;
    for (int dir = 1; dir >= -1; dir -= 2) {
        int last = -1, last_slot = 0;
        for (int f = key + dir; f >= 0 && f < n; f += dir) {
            if (last < 0) {                     // the direction's first frame starts from the box itself
                a.prev = -1; a.base = key; a.prev_surface = nullptr; a.prev_rows = nullptr;
            } else {
                a.prev = last; a.base = last - dir; a.prev_surface = surface_of(last, last_slot); a.prev_rows = rows_of(last_slot);
            }
            a.frame = f; a.surface = surface_of(f, slot); a.rows = rows_of(slot);
            hipLaunchKernelGGL(track_search_kernel, dim3((unsigned)D), dim3(TK_THREADS), 0, ctx->stream, a);
            last = f; last_slot = slot; slot ^= 1;
        }
        if (last >= 0) {                        // the direction's last frame: the resolving half alone
            a.prev = last; a.base = last - dir; a.prev_surface = surface_of(last, last_slot); a.prev_rows = rows_of(last_slot);
            a.frame = -1; a.surface = nullptr; a.rows = nullptr;
            hipLaunchKernelGGL(track_search_kernel, dim3(1), dim3(TK_THREADS), 0, ctx->stream, a);
        }
    }
    VSTAB_HIP(hipGetLastError());
    return 0;
}
