// vstab_rolling.hip -- rolling shutter: the per-row readout correction of the final warp (vstab_rolling_warp_batch), its
// closed-form inverse (vstab_rolling_unwarp_batch) and the per-row median of the global fit's residual that the readout
// estimate is made from (vstab_row_residual_batch).  Not a reference feature; the rules are stated in include/vstab.h.
// profiles/warp_traffic.json is tied to vstab_warp.hip + vstab_internal.h: an edit here leaves it valid.
//
// rolling_warp_kernel: the plain warp's 64 x 8 tile (TileShell, XCD remap, block_count_add) around warp_pixel with a
// displacement of the source position that is a closed form of the frame's six velocity coefficients and the readout -- seven
// uniform doubles, so there is no table and no LDS beyond the count reduction's; what it adds to the plain warp is ~20 fp64
// operations per pixel (two of them divisions) under the same HBM stream.  Its inverse is the same kernel template with
// RowInverseDisplacement, warp_pixel's OUTPUT kind: a 2x2 solve at the output pixel whose row terms (tau, the matrix, its
// determinant) are the same for a thread's two pixels: one division per thread for the row, two per pixel by the determinant.
// row_residual_kernel: one workgroup per (pair, grid row); the row's admitted residuals are compacted into LDS (order does
// not matter to a median) and ranked by counting, as vstab_mesh.hip does per vertex.  A row of a 960-px estimation image has
// 120 samples: microseconds per clip.
// Built with -ffp-contract=off like the rest of the library.
#define VSTAB_WARP_ARITHMETIC
#include "vstab_internal.h"
#include <cmath>

namespace {

constexpr int ROLL_TILE_TX = 32;            // the plain warp's default tile: 64 x 8 output pixels per 256 threads
constexpr int ROW_THREADS = 256;
constexpr int ROW_MAX_SAMPLES = 4096;       // grid positions of one row: 2 x 16 KB of LDS

__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN
__device__ __forceinline__ bool finite_d(double v) { return __builtin_fabs(v) <= 1.7976931348623157e308; }  // false for NaN

// The rolling-shutter displacement (the rule: vstab_rolling_warp_batch in include/vstab.h): every operation fp64 and
// rounded on its own.
struct RowDisplacement {
    static constexpr bool ACTIVE = true;
    static constexpr bool OUTPUT = false;
    double v0, v1, v2, v3, v4, v5;   // the frame's velocity V, px per frame interval
    double rho, hm1;                 // readout; src_h - 1
    __device__ __forceinline__ void operator()(double qx, double qy, double& cx, double& cy) const
    {
        double yc = (qy > 0.0) ? qy : 0.0;          // NaN -> 0
        yc = (yc < hm1) ? yc : hm1;
        const double vx = (v0 * qx + v1 * qy) + v2;
        const double vy = (v3 * qx + v4 * qy) + v5;
        double D = 1.0 - rho * vy / hm1;
        if (!(D >= 0.5)) D = 0.5;                   // also a NaN
        const double tau = rho * (yc / hm1 - 0.5) / D;
        cx = -(tau * vx);
        cy = -(tau * vy);
        if (!(finite_d(cx) && finite_d(cy))) { cx = 0.0; cy = 0.0; }
    }
};

// The inverse (the rule: vstab_rolling_unwarp_batch in include/vstab.h): the forward warp sampled its source at
// s = q + tau(s_y) v(q); restoring, the output pixel IS s, so tau is known from the output row and q solves
// (I + tau L) q = s - tau t.  e = q - s moves the output pixel in front of the matrix (warp_pixel's OUTPUT kind).  tau, a..d
// and det depend on the row only: a thread's pixels share them.
struct RowInverseDisplacement {
    static constexpr bool ACTIVE = true;
    static constexpr bool OUTPUT = true;
    double v0, v1, v2, v3, v4, v5;   // the frame's velocity V, px per frame interval
    double rho, hm1;                 // readout; out_h - 1
    // -> solved; (ex, ey) = q - s, (0, 0) if not solved
    __device__ __forceinline__ bool solve(int x, int y, double& ex, double& ey) const
    {
        const double xd = (double)x, yd = (double)y;
        const double tau = rho * (yd / hm1 - 0.5);
        const double a = 1.0 + tau * v0, b = tau * v1, c = tau * v3, d = 1.0 + tau * v4;
        const double det = a * d - b * c;
        const double vx = (v0 * xd + v1 * yd) + v2;
        const double vy = (v3 * xd + v4 * yd) + v5;
        const double rx = tau * vx, ry = tau * vy;
        ex = -((d * rx - b * ry) / det);
        ey = -((a * ry - c * rx) / det);
        if (!(det >= VSTAB_ROLLING_UNWARP_MIN_DET) || !(finite_d(ex) && finite_d(ey))) { ex = 0.0; ey = 0.0; return false; }   // also a NaN
        return true;
    }
};

struct RollingWarpArgs {
    const float* src;
    float* dst;
    float* mask;
    unsigned* pad_count;
    unsigned* unsolved;       // [n] or nullptr; the inverse only
    const WarpXform* xf;
    const double* velocity;   // [n, 6]
    double readout;
    int n, sh, sw, dh, dw;
    int bw0, bw0_pow2;        // column block width of OpenCV's WarpPerspectiveInvoker, 1 if it is a power of two
    int tiles_x, tiles_y;
    float b0, b1, b2;         // border colour
};

// One 64 x 8 tile: the plain warp's kernel body (vstab_warp.hip: warp_kernel) with Disp = RowDisplacement (the forward warp;
// its row lever is the SOURCE's height) or RowInverseDisplacement (the inverse; the OUTPUT's height, which is the forward
// warp's source).
template <int SUBPIX, bool WITH_MASK, class Disp>
__global__ __launch_bounds__(256) void rolling_warp_kernel(RollingWarpArgs a)
{
    constexpr int INTERP = VSTAB_INTERP_BILINEAR;
    const TileShell<ROLL_TILE_TX> t(a.tiles_x, a.tiles_y, a.dh, a.dw);
    const int frame = t.frame, x0 = t.x0, y = t.y, npx = t.npx;
    const double* __restrict__ V = a.velocity + (size_t)frame * 6;      // block-uniform
    const Disp disp{V[0], V[1], V[2], V[3], V[4], V[5], a.readout, (double)((Disp::OUTPUT ? a.dh : a.sh) - 1)};
    const float* __restrict__ S = a.src + (size_t)frame * a.sh * a.sw * 3;

    float acc[TILE_PX][3];
    float cov[TILE_PX];
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) { acc[p][0] = acc[p][1] = acc[p][2] = 0.f; cov[p] = 0.f; }
    unsigned unsolved = 0;    // the inverse only: this thread's pixels whose solve was refused

    if (t.active) {
        const double dy = (double)y;
        const WarpXform* __restrict__ xf = a.xf + frame;
        const XformRegs<INTERP, SUBPIX> r(xf);
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (p >= npx) continue;
            const int x = x0 + p * ROLL_TILE_TX;
            float c = 0.f;
            const Px v = warp_pixel<INTERP, SUBPIX, WITH_MASK>(
                xf, r, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x, y, dy,
                [&](int X, int Y) { return sample_q5<INTERP>(S, a.sh, a.sw, X, Y, a.b0, a.b1, a.b2, nullptr); },
                [&](float fsx, float fsy) { return sample_exact(S, a.sh, a.sw, fsx, fsy, a.b0, a.b1, a.b2); }, disp, c, &unsolved);
            acc[p][0] = v.r; acc[p][1] = v.g; acc[p][2] = v.b;
            if (WITH_MASK) cov[p] = c;
        }
    }

    float mk[TILE_PX];
    unsigned padded[1] = {0};
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) {
        float m = 1.0f - cov[p];
        mk[p] = (m < 1e-3f) ? 0.f : m;
        if (WITH_MASK && p < npx) padded[0] += (mk[p] > 0.5f) ? 1u : 0u;
    }

    if (t.active) {
        // inside a frame 32-bit element offsets suffice (the host checks that a frame has fewer than 2^30 pixels)
        float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
        float* __restrict__ Mk = WITH_MASK ? a.mask + (size_t)frame * a.dh * a.dw : nullptr;
        const unsigned row = (unsigned)y * (unsigned)a.dw;
        typedef float f3 __attribute__((ext_vector_type(3)));
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (p >= npx) continue;
            const unsigned pix = row + (unsigned)(x0 + p * ROLL_TILE_TX);
            f3 rgb = {acc[p][0], acc[p][1], acc[p][2]};
            __builtin_memcpy(D + pix * 3u, &rgb, 12);
            if (WITH_MASK) Mk[pix] = mk[p];
        }
    }

    if constexpr (Disp::OUTPUT) {
        // two counters through one reduction (the conditions are kernel arguments: uniform)
        if ((WITH_MASK && a.pad_count != nullptr) || a.unsolved != nullptr) {
            unsigned counts[2] = {padded[0], unsolved};
            block_count_add<2>(counts, {WITH_MASK ? a.pad_count : nullptr, a.unsolved}, frame);
        }
    } else {
        if (WITH_MASK && a.pad_count != nullptr) block_count_add<1>(padded, {a.pad_count}, frame);
    }
}

struct RowResidualArgs {
    const float* grid;
    const float* mats;       // [pairs, 9] f32
    const uint8_t* blocked;  // [pairs + 1, gh, gw] or nullptr
    float* residual;         // [pairs, gh, 2]
    int* count;              // [pairs, gh]
    int gh, gw, step;
};

__global__ __launch_bounds__(ROW_THREADS) void row_residual_kernel(RowResidualArgs a)
{
    extern __shared__ float s_val[];       // [2][gw]: x residuals, y residuals
    __shared__ int s_n;
    __shared__ float s_mid[2][2];          // [axis][lo, hi]
    float* s_rx = s_val;
    float* s_ry = s_val + a.gw;
    const int pair = (int)blockIdx.x / a.gh, gy = (int)blockIdx.x - pair * a.gh;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();

    double A[9];
    for (int k = 0; k < 9; k++) A[k] = (double)a.mats[(size_t)pair * 9 + k];
    const size_t cells = (size_t)a.gh * a.gw;
    const float* __restrict__ G = a.grid + (size_t)pair * cells * 2;
    const uint8_t* __restrict__ B0 = a.blocked ? a.blocked + (size_t)pair * cells : nullptr;
    const uint8_t* __restrict__ B1 = a.blocked ? B0 + cells : nullptr;
    const double y = (double)(gy * a.step);

    for (int gx = threadIdx.x; gx < a.gw; gx += ROW_THREADS) {
        const double x = (double)(gx * a.step);
        const size_t g = (size_t)gy * a.gw + gx;
        if (B0 != nullptr && (B0[g] | B1[g])) continue;
        const float u = G[g * 2], v = G[g * 2 + 1];
        const double X = (A[0] * x + A[1] * y) + A[2];
        const double Y = (A[3] * x + A[4] * y) + A[5];
        const double W = (A[6] * x + A[7] * y) + A[8];
        const float rx = (float)((x + (double)u) - X / W);
        const float ry = (float)((y + (double)v) - Y / W);
        if (!(finite_f(u) && finite_f(v) && finite_f(rx) && finite_f(ry))) continue;
        const int slot = atomicAdd(&s_n, 1);     // slot < gw: every grid position of the row is visited once
        s_rx[slot] = rx; s_ry[slot] = ry;
    }
    __syncthreads();
    const int n = s_n;
    const size_t cell = (size_t)pair * a.gh + gy;
    float* out = a.residual + cell * 2;
    if (n < VSTAB_ROW_MIN_SAMPLES) {
        if (threadIdx.x == 0) { out[0] = 0.f; out[1] = 0.f; a.count[cell] = n; }
        return;
    }
    // rank of element i: values below it, and equal values in front of it -- a permutation of 0..n-1
    const int klo = (n - 1) >> 1, khi = n >> 1;
    for (int i = threadIdx.x; i < n; i += ROW_THREADS) {
#pragma unroll
        for (int axis = 0; axis < 2; axis++) {
            const float* __restrict__ s = axis ? s_ry : s_rx;
            const float vi = s[i];
            int rank = 0;
            for (int j = 0; j < n; j++) {
                const float vj = s[j];
                rank += (vj < vi || (vj == vi && j < i)) ? 1 : 0;
            }
            if (rank == klo) s_mid[axis][0] = vi;
            if (rank == khi) s_mid[axis][1] = vi;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = (n & 1) ? s_mid[0][0] : (s_mid[0][0] + s_mid[0][1]) / 2.0f;
        out[1] = (n & 1) ? s_mid[1][0] : (s_mid[1][0] + s_mid[1][1]) / 2.0f;
        a.count[cell] = n;
    }
}

template <class Disp>
void launch_rolling(const RollingWarpArgs& a, unsigned blocks, int subpix, hipStream_t stream)
{
    const dim3 grid(blocks), block(256);
    if (subpix == VSTAB_SUBPIX_EXACT) {
        if (a.mask) hipLaunchKernelGGL((rolling_warp_kernel<VSTAB_SUBPIX_EXACT, true, Disp>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((rolling_warp_kernel<VSTAB_SUBPIX_EXACT, false, Disp>), grid, block, 0, stream, a);
    } else {
        if (a.mask) hipLaunchKernelGGL((rolling_warp_kernel<VSTAB_SUBPIX_Q5, true, Disp>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((rolling_warp_kernel<VSTAB_SUBPIX_Q5, false, Disp>), grid, block, 0, stream, a);
    }
}

// Both directions: the checks, the staged table and the launch.  inverse: the row lever is the output's height, `unsolved` is
// zeroed and counted.
int rolling_batch(const char* who, bool inverse, vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                  int out_h, int out_w, const float* border_rgb, int subpix, const double* velocity, double readout, float* dst,
                  float* mask, uint32_t* pad_count, uint32_t* unsolved)
{
    if (int rc = vstab_check_common(who, ctx, src, n, src_h, src_w, matrices, out_h, out_w, VSTAB_INTERP_BILINEAR, border_rgb, subpix, dst)) return rc;
    VSTAB_REQUIRE(velocity != nullptr, "%s: NULL pointer argument", who);
    if (inverse) VSTAB_REQUIRE(out_h >= 2, "%s: bad size (n=%d src=%dx%d out=%dx%d; the output must have at least 2 rows)", who, n, src_w, src_h, out_w, out_h);
    else VSTAB_REQUIRE(src_h >= 2, "%s: bad size (n=%d src=%dx%d out=%dx%d; the source must have at least 2 rows)", who, n, src_w, src_h, out_w, out_h);
    VSTAB_REQUIRE(readout >= -1.0 && readout <= 1.0, "%s: readout=%g outside [-1, 1] (a fraction of the frame interval)", who, readout);
    VSTAB_HIP(hipSetDevice(ctx->device));
    // one staged table (the staging buffer holds one table per call): n transform records, then n x 6 velocity coefficients
    static_assert(sizeof(WarpXform) % sizeof(double) == 0, "the velocity table behind the records stays 8-byte aligned");
    const size_t xf_bytes = (size_t)n * sizeof(WarpXform), vel_bytes = (size_t)n * 6 * sizeof(double);
    std::vector<unsigned char> table(xf_bytes + vel_bytes);
    for (int i = 0; i < n; i++) vstab_fill_xform(matrices + (size_t)i * 9, reinterpret_cast<WarpXform*>(table.data()) + i);
    memcpy(table.data() + xf_bytes, velocity, vel_bytes);
    void* d_table = nullptr;
    if (int rc = vstab_stage_params(ctx, table.data(), table.size(), &d_table)) return rc;
    RollingWarpArgs a{};
    a.src = src; a.dst = dst; a.mask = mask; a.pad_count = pad_count; a.unsolved = unsolved;
    a.xf = static_cast<const WarpXform*>(d_table);
    a.velocity = reinterpret_cast<const double*>(static_cast<const unsigned char*>(d_table) + xf_bytes);
    a.readout = readout;
    a.n = n; a.sh = src_h; a.sw = src_w; a.dh = out_h; a.dw = out_w;
    vstab_set_block_width(out_h, out_w, &a.bw0, &a.bw0_pow2);
    a.b0 = border_rgb[0]; a.b1 = border_rgb[1]; a.b2 = border_rgb[2];
    unsigned blocks = 0;
    if (int rc = vstab_tile_grid(who, n, out_h, out_w, ROLL_TILE_TX, 256, &a.tiles_x, &a.tiles_y, &blocks)) return rc;
    if (pad_count) VSTAB_HIP(hipMemsetAsync(pad_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    if (unsolved) VSTAB_HIP(hipMemsetAsync(unsolved, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    KernelTimer timer(ctx, inverse ? "rolling_unwarp" : "rolling_warp");
    if (inverse) launch_rolling<RowInverseDisplacement>(a, blocks, subpix, ctx->stream);
    else launch_rolling<RowDisplacement>(a, blocks, subpix, ctx->stream);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int vstab_rolling_warp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                                        int out_h, int out_w, const float* border_rgb, int subpix, const double* velocity,
                                        double readout, float* dst, float* mask, uint32_t* pad_count)
{
    return rolling_batch("vstab_rolling_warp_batch", false, ctx, src, n, src_h, src_w, matrices, out_h, out_w, border_rgb, subpix,
                         velocity, readout, dst, mask, pad_count, nullptr);
}

extern "C" int vstab_rolling_unwarp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                                          int out_h, int out_w, const float* border_rgb, int subpix, const double* velocity,
                                          double readout, float* dst, float* mask, uint32_t* pad_count, uint32_t* unsolved)
{
    return rolling_batch("vstab_rolling_unwarp_batch", true, ctx, src, n, src_h, src_w, matrices, out_h, out_w, border_rgb, subpix,
                         velocity, readout, dst, mask, pad_count, unsolved);
}

extern "C" int vstab_row_residual_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h,
                                        int work_w, const float* transitions, const uint8_t* blocked, float* residual,
                                        int32_t* count)
{
    const char* who = "vstab_row_residual_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    VSTAB_REQUIRE(grid_flow && transitions && residual && count, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(pairs > 0 && step > 0 && work_h >= 2 && work_w >= 2, "%s: needs pairs > 0, step > 0 and an image of at least 2x2 (pairs=%d step=%d %dx%d)", who, pairs, step, work_w, work_h);
    VSTAB_REQUIRE(gh == (work_h + step - 1) / step && gw == (work_w + step - 1) / step, "%s: grid %dx%d is not ceil(%dx%d / %d)", who, gw, gh, work_w, work_h, step);
    VSTAB_REQUIRE(gw <= ROW_MAX_SAMPLES, "%s: a row of %d grid positions exceeds %d", who, gw, ROW_MAX_SAMPLES);
    const long long blocks = (long long)pairs * gh;
    VSTAB_REQUIRE(blocks < 0x7fffffffLL, "%s: clip too large", who);
    VSTAB_HIP(hipSetDevice(ctx->device));
    void* d_mats = nullptr;
    if (int rc = vstab_stage_params(ctx, transitions, (size_t)pairs * 9 * sizeof(float), &d_mats)) return rc;
    RowResidualArgs a{};
    a.grid = grid_flow; a.mats = static_cast<const float*>(d_mats); a.blocked = blocked; a.residual = residual; a.count = count;
    a.gh = gh; a.gw = gw; a.step = step;
    const size_t lds = (size_t)gw * 2 * sizeof(float);     // <= 32 KB
    KernelTimer timer(ctx, "row_residual");
    hipLaunchKernelGGL(row_residual_kernel, dim3((unsigned)blocks), dim3(ROW_THREADS), lds, ctx->stream, a);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
