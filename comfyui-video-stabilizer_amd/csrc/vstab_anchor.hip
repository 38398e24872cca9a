// vstab_anchor.hip -- drift correction: the normal equations of aligning every frame to its keyframe, as exact integer sums.
// The rule has two forms, both stated in include/vstab.h: the plain one (vstab_anchor_sums_batch: 4 regression columns, 17
// sums) and the exposure-matched, masked one (vstab_anchor_sums_ex_batch: a gain and an offset per frame, the columns T and 1
// beside the four, the estimation mask's block grid; 31 sums).  The plain form is the second at G = 1024, O = 0 without a
// grid, and that is how it is built here: one kernel template, anchor_sums_kernel<COLS, VEC, MASK>.  Not a reference feature.
//
// The kernel is shaped after pair_residual_kernel (vstab_cut.hip).  A workgroup owns ANCHOR_ROWS template rows of one frame;
// a lane takes 16 template pixels with one 16-byte load per row (the row itself and its two neighbours for the vertical
// gradient; the two pixels beside the piece come as byte loads), maps each through the frame's matrix in fp64 (the rule's
// association, nothing fused: -ffp-contract=off), rounds to Q5 half-to-even and reads the four taps of the frame's image
// with byte loads.  A shake-sized matrix keeps those taps within a few rows of the pixel, so template and image cross HBM
// about once: ~2 * h * w bytes per frame.  Everything that is summed is an integer: 17 / 31 lane sums (i64) -> BlockSums
// (vstab_internal.h) -> thread k finishes slot k with one 64-bit atomic per workgroup, only where the workgroup counted,
// capped or masked a pixel.
//
// Bounds (max(h, w) <= 1024, required by the entry points): |gx|, |gy| <= 255; |u|, |q| <= 1023; so |J2|, |J3| <=
// 2 * 255 * 1023 = 521730 < 2^19 (int32), |r| <= 261120 < 2^18, a product J_j J_k < 2^38 and J_k r < 2^37 (formed in 64
// bits), and at most 1022^2 < 2^20 pixels take part: |sum J_j J_k| < 2^58, |sum J_k r| < 2^57, sum |r| < 2^38.  Nothing
// reaches 2^59, for a lane, a workgroup or a frame.  With a gain and an offset: |G T + O| <= 4096 * 255 + 2^20 < 2^21 and
// v < 2^18, so r fits an int; a counted pixel has |r| <= 1024 * 255 < 2^18 by the cap test itself, and the columns J4 = T <=
// 255 and J5 = 1 are smaller than the other four, so every product and every sum stays below the bounds above.
#include "vstab_internal.h"

namespace {

constexpr int ANCHOR_ROWS = 16;     // template rows per workgroup (960x540: 34 workgroups per frame)
constexpr int ANCHOR_THREADS = 256;

// The slots of a form with COLS regression columns, in the order of the rule's output: the counters (count, capped and, with
// six columns, masked), sum |r|, b_0.., then J_j J_k for j <= k row-major.
constexpr int anchor_head(int cols) { return cols == 6 ? 4 : 3; }
constexpr int anchor_slots(int cols) { return anchor_head(cols) + cols + cols * (cols + 1) / 2; }
static_assert(anchor_slots(4) == VSTAB_ANCHOR_SLOTS && anchor_slots(6) == VSTAB_ANCHOR_EX_SLOTS, "the two forms of include/vstab.h");

struct AnchorMatrix {
    double r0, r1, r2, r3, r4, r5;
};

// the frame's gain and offset, and the two frames' block grids
struct AnchorFrame {
    int gain, offset;                       // G in 1/1024, O in 1/1024 grey level
    const uint8_t* __restrict__ blocked_t;  // the anchor's [gh,gw] grid and the frame's (MASK only)
    const uint8_t* __restrict__ blocked_i;
    int step, gh, gw;
};

// steps 1-5 of the rule for one template pixel: the sample position in Q5 and the bilinear integer v of the frame's image;
// false where the pixel does not take part (outside the frame, or a position that is not finite)
__device__ __forceinline__ bool anchor_tap(const AnchorMatrix& R, const uint8_t* __restrict__ img, int x, int y, int h, int w, int& ix,
                                           int& iy, int& v)
{
    const double dx = (double)x, dy = (double)y;
    const double X = (R.r0 * dx + R.r1 * dy) + R.r2;
    const double Y = (R.r3 * dx + R.r4 * dy) + R.r5;
    const double fix = rint(32.0 * X), fiy = rint(32.0 * Y);    // half-to-even; NaN / inf fail the comparisons below
    if (!(fix >= 0.0 && fix <= (double)(32 * (w - 1)) && fiy >= 0.0 && fiy <= (double)(32 * (h - 1)))) return false;
    ix = (int)fix, iy = (int)fiy;
    const int x0 = ix >> 5, fx = ix & 31, x1 = min(x0 + 1, w - 1);
    const int y0 = iy >> 5, fy = iy & 31, y1 = min(y0 + 1, h - 1);
    const uint8_t* __restrict__ r0 = img + (size_t)y0 * w;
    const uint8_t* __restrict__ r1 = img + (size_t)y1 * w;
    v = (32 - fx) * (32 - fy) * (int)r0[x0] + fx * (32 - fy) * (int)r0[x1] + (32 - fx) * fy * (int)r1[x0] + fx * fy * (int)r1[x1];
    return true;
}

// one template pixel of the rule into the lane's sums a: t = T[y,x], l / r / up / dn its four neighbours, img = the frame's
// image.  With four columns f.gain and f.offset are the constants 1024 and 0 (the kernel sets them) and nothing is hidden.
template <int COLS, bool MASK>
__device__ __forceinline__ void anchor_pixel(long long (&a)[anchor_slots(COLS)], const AnchorMatrix& R, const AnchorFrame& f,
                                             const uint8_t* __restrict__ img, int x, int y, int h, int w, int cap1024, int t, int l,
                                             int r, int up, int dn)
{
    static_assert(COLS == 6 || !MASK, "the block grid belongs to the second form");
    constexpr int HEAD = anchor_head(COLS);
    int ix, iy, v;
    if (!anchor_tap(R, img, x, y, h, w, ix, iy, v)) return;
    int hidden = 0;
    if (MASK) {
        const int half = f.step >> 1;
        const int ty = min((y + half) / f.step, f.gh - 1), tx = min((x + half) / f.step, f.gw - 1);
        const int xn = min((ix + 16) >> 5, w - 1), yn = min((iy + 16) >> 5, h - 1);
        const int sy = min((yn + half) / f.step, f.gh - 1), sx = min((xn + half) / f.step, f.gw - 1);
        hidden = (f.blocked_t[ty * f.gw + tx] | f.blocked_i[sy * f.gw + sx]) != 0 ? 1 : 0;
    }
    const int res = v - (f.gain * t + f.offset);        // |G T + O| < 2^21
    // (the counters are added to without a branch: behind `if (over) capped += 1; else count += 1` the compiler selects
    // between the addresses of the two and puts them into scratch memory)
    const int over = (1 - hidden) & (abs(res) > cap1024 ? 1 : 0);
    if (HEAD == 4) a[2] += hidden;
    a[1] += over;
    a[0] += 1 - hidden - over;
    if (hidden | over) return;
    const int gx = r - l, gy = dn - up, u = 2 * x - (w - 1), q = 2 * y - (h - 1);
    const int j[6] = {gx, gy, gx * u + gy * q, gy * u - gx * q, t, 1};
    a[HEAD - 1] += abs(res);
    int slot = HEAD + COLS;
#pragma unroll
    for (int m = 0; m < COLS; m++) {
        a[HEAD + m] += (long long)j[m] * res;
#pragma unroll
        for (int k = m; k < COLS; k++) {
            // (four columns: the products of the first two rows are < 2^27 and formed in 32 bits, as they were timed; with six
            // columns the same choice makes the kernel ~100 instructions longer, profiles/r32_anchor_one_kernel.md)
            if (COLS == 4 && m < 2) a[slot++] += j[m] * j[k];
            else a[slot++] += (long long)j[m] * j[k];
        }
    }
}

__device__ __forceinline__ int byte_of(const uint4& v, int k)
{
    const unsigned word = (k < 4) ? v.x : (k < 8) ? v.y : (k < 12) ? v.z : v.w;
    return (int)((word >> ((k & 3) * 8)) & 0xffu);
}

// A workgroup's template pixels: `rows` rows from y_first, in 16-pixel pieces, one piece per lane and step.
// pixel(x, y, t, l, r, up, dn) gets every pixel with 1 <= x <= w-2 and its four neighbours.
// VEC: w % 16 == 0 and the base 16-byte aligned (every row of every frame then is)
template <bool VEC, class Pixel>
__device__ __forceinline__ void anchor_walk(const uint8_t* __restrict__ tmpl, int y_first, int rows, int w, Pixel pixel)
{
    const int chunks = (w + 15) >> 4;                   // 16-pixel pieces of a row
    for (int item = threadIdx.x; item < rows * chunks; item += ANCHOR_THREADS) {
        const int r = item / chunks, c = item - r * chunks;
        const int y = y_first + r, xa = c << 4;
        const uint8_t* __restrict__ row = tmpl + (size_t)y * w;
        const int xs = max(xa, 1), xe = min(xa + 16, w - 1);   // the piece's pixels with 1 <= x <= w-2
        if (VEC) {
            const uint4 mid = *reinterpret_cast<const uint4*>(row + xa);
            const uint4 upv = *reinterpret_cast<const uint4*>(row - w + xa);
            const uint4 dnv = *reinterpret_cast<const uint4*>(row + w + xa);
            const int before = xa > 0 ? (int)row[xa - 1] : 0, after = xa + 16 < w ? (int)row[xa + 16] : 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int x = xa + k;
                if (x >= xs && x < xe)
                    pixel(x, y, byte_of(mid, k), k == 0 ? before : byte_of(mid, k - 1), k == 15 ? after : byte_of(mid, k + 1),
                          byte_of(upv, k), byte_of(dnv, k));
            }
        } else {
            for (int x = xs; x < xe; x++)
                pixel(x, y, (int)row[x], (int)row[x - 1], (int)row[x + 1], (int)row[x - w], (int)row[x + w]);
        }
    }
}

// COLS: 4, the plain form (G = 1024 and O = 0 are constants: `params` holds the anchors alone, and n, blocked, step, gh and
// gw are not read), or 6, the second form (`params` holds the anchors, the gains and the offsets of all frames, n each).
// VEC: see anchor_walk.  MASK: the two block-grid bytes are read (a kernel-uniform choice, made at the launch).
template <int COLS, bool VEC, bool MASK>
__global__ __launch_bounds__(ANCHOR_THREADS) void anchor_sums_kernel(const uint8_t* __restrict__ gray, const double* __restrict__ mats,
                                                                      const int* __restrict__ params, int n, int h, int w, int tiles,
                                                                      int cap1024, const uint8_t* __restrict__ blocked, int step,
                                                                      int gh, int gw, long long* __restrict__ out)
{
    constexpr int SLOTS = anchor_slots(COLS), COUNTERS = anchor_head(COLS) - 1;
    __shared__ BlockSums<long long, SLOTS, ANCHOR_THREADS> s_sums;
    const int frame = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - frame * tiles;
    const int anchor = params[frame];
    if (anchor < 0) return;                             // the whole workgroup: no barrier has been reached
    const int y_first = 1 + tile * ANCHOR_ROWS, rows = min(ANCHOR_ROWS, (h - 1) - y_first);   // template rows 1..h-2
    const double* __restrict__ mat = mats + (size_t)frame * 6;
    const AnchorMatrix R = {mat[0], mat[1], mat[2], mat[3], mat[4], mat[5]};
    const uint8_t* __restrict__ tmpl = gray + (size_t)anchor * h * w;
    const uint8_t* __restrict__ img = gray + (size_t)frame * h * w;
    const AnchorFrame f = {COLS == 6 ? params[n + frame] : 1024, COLS == 6 ? params[2 * n + frame] : 0,
                           MASK ? blocked + (size_t)anchor * gh * gw : nullptr, MASK ? blocked + (size_t)frame * gh * gw : nullptr,
                           step, gh, gw};
    long long acc[SLOTS] = {};
    anchor_walk<VEC>(tmpl, y_first, rows, w, [&](int x, int y, int t, int l, int r, int up, int dn) {
        anchor_pixel<COLS, MASK>(acc, R, f, img, x, y, h, w, cap1024, t, l, r, up, dn);
    });
    s_sums.put(acc);
    __syncthreads();
    if (threadIdx.x < SLOTS) {
        long long touched = 0;
#pragma unroll
        for (int c = 0; c < COUNTERS; c++) touched += s_sums.total(c);
        const long long total = s_sums.total(threadIdx.x);
        if (touched) atomicAdd(reinterpret_cast<unsigned long long*>(out + (size_t)frame * SLOTS + threadIdx.x), (unsigned long long)total);
    }
}

// Both entry points.  ex: the second form (gain and offset are required; blocked may be NULL).  The plain form passes no
// gain, offset or grid and step 1.
int anchor_sums(const char* name, const char* kind, bool ex, vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w,
                const int32_t* anchor, const double* R, const int32_t* gain, const int32_t* offset, int cap, const uint8_t* blocked,
                int step, int gh, int gw, int64_t* out)
{
    VSTAB_REQUIRE(ctx != nullptr, "%s: ctx is NULL", name);
    VSTAB_REQUIRE(gray && anchor && R && out && (!ex || (gain && offset)), "%s: NULL pointer argument", name);
    VSTAB_REQUIRE(n >= 1 && h > 0 && w > 0, "%s: needs at least one frame of a positive size (n=%d, %dx%d)", name, n, w, h);
    VSTAB_REQUIRE(h <= 1024 && w <= 1024, "%s: %dx%d image larger than 1024 on a side (the sums are exact up to there)", name, w, h);
    VSTAB_REQUIRE(cap >= 0 && cap <= 255, "%s: cap %d outside [0, 255]", name, cap);
    VSTAB_REQUIRE(step >= 1, "%s: step %d is not positive", name, step);
    if (blocked)
        VSTAB_REQUIRE(gh == (h + step - 1) / step && gw == (w + step - 1) / step,
                      "%s: a %dx%d block grid for a %dx%d image at step %d (expected %dx%d)", name, gw, gh, w, h, step,
                      (w + step - 1) / step, (h + step - 1) / step);
    for (int i = 0; i < n; i++) {
        VSTAB_REQUIRE(anchor[i] >= -1 && anchor[i] < n, "%s: anchor[%d] = %d outside [-1, %d)", name, i, (int)anchor[i], n);
        if (!ex) continue;
        VSTAB_REQUIRE(gain[i] >= 256 && gain[i] <= 4096, "%s: gain[%d] = %d outside [256, 4096]", name, i, (int)gain[i]);
        VSTAB_REQUIRE(offset[i] >= -(1 << 20) && offset[i] <= (1 << 20), "%s: offset[%d] = %d outside [-2^20, 2^20]", name, i, (int)offset[i]);
    }
    VSTAB_HIP(hipSetDevice(ctx->device));
    VSTAB_HIP(hipMemsetAsync(out, 0, (size_t)n * anchor_slots(ex ? 6 : 4) * sizeof(int64_t), ctx->stream));
    if (h < 3 || w < 3) return 0;                       // no template pixel has all four neighbours
    const int tiles = (h - 2 + ANCHOR_ROWS - 1) / ANCHOR_ROWS;
    VSTAB_REQUIRE((long long)n * tiles < 0x7fffffffLL, "%s: clip too large", name);
    // one staged blob: the matrices (fp64, so they come first), then the anchors and, in the second form, the gains and the offsets
    const size_t mat_bytes = (size_t)n * 6 * sizeof(double), int_bytes = (size_t)n * sizeof(int32_t);
    std::vector<unsigned char> blob(mat_bytes + (ex ? 3 : 1) * int_bytes);
    memcpy(blob.data(), R, mat_bytes);
    memcpy(blob.data() + mat_bytes, anchor, int_bytes);
    if (ex) {
        memcpy(blob.data() + mat_bytes + int_bytes, gain, int_bytes);
        memcpy(blob.data() + mat_bytes + 2 * int_bytes, offset, int_bytes);
    }
    void* d_blob = nullptr;
    if (int rc = vstab_stage_params(ctx, blob.data(), blob.size(), &d_blob)) return rc;
    const double* d_mats = static_cast<const double*>(d_blob);
    const int* d_params = reinterpret_cast<const int*>(static_cast<const unsigned char*>(d_blob) + mat_bytes);
    KernelTimer timer(ctx, kind);
    const bool vec = (w % 16 == 0) && (reinterpret_cast<uintptr_t>(gray) % 16 == 0);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(n * tiles)), dim3(ANCHOR_THREADS), 0, ctx->stream, gray, d_mats, d_params, n, h, w, tiles,
                           1024 * cap, blocked, step, gh, gw, reinterpret_cast<long long*>(out));
    };
    if (!ex) vec ? launch(anchor_sums_kernel<4, true, false>) : launch(anchor_sums_kernel<4, false, false>);
    else if (blocked) vec ? launch(anchor_sums_kernel<6, true, true>) : launch(anchor_sums_kernel<6, false, true>);
    else vec ? launch(anchor_sums_kernel<6, true, false>) : launch(anchor_sums_kernel<6, false, false>);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int vstab_anchor_sums_ex_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const int32_t* anchor,
                                          const double* R, const int32_t* gain, const int32_t* offset, int cap, const uint8_t* blocked,
                                          int step, int gh, int gw, int64_t* out)
{
    return anchor_sums("vstab_anchor_sums_ex_batch", "anchor_ex", true, ctx, gray, n, h, w, anchor, R, gain, offset, cap, blocked, step, gh, gw, out);
}

extern "C" int vstab_anchor_sums_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const int32_t* anchor,
                                       const double* R, int cap, int64_t* out)
{
    return anchor_sums("vstab_anchor_sums_batch", "anchor", false, ctx, gray, n, h, w, anchor, R, nullptr, nullptr, cap, nullptr, 1, 0, 0, out);
}
