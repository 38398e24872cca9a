// vstab_rolling.hip -- rolling shutter: the per-row readout correction of the final warp (vstab_rolling_warp_batch), its
// closed-form inverse (vstab_rolling_unwarp_batch), the per-row median of the global fit's residual that the readout
// estimate is made from (vstab_row_residual_batch), and the rectifier of the flow samples that the refit of the transitions
// reads (vstab_rectify_samples_batch).  Not a reference feature; the rules are stated in include/vstab.h.
// profiles/warp_traffic.json is tied to vstab_warp.hip + vstab_internal.h: an edit here leaves it valid.
//
// The warps: the plain warp's kernel body (warp_kernel, vstab_internal.h) with Args = RollingWarpArgs, whose displacement of
// the source position is a closed form of the frame's six velocity coefficients and the readout -- seven
// uniform doubles, so there is no table and no LDS beyond the count reduction's; what it adds to the plain warp is ~20 fp64
// operations per pixel (two of them divisions) under the same HBM stream.  Its inverse is the same body with
// RollingUnwarpArgs: RowInverseDisplacement, warp_pixel's OUTPUT kind: a 2x2 solve at the output pixel whose row terms (tau,
// the matrix, its determinant) are the same for a thread's two pixels: one division per thread for the row, two per pixel by
// the determinant.  Launch and host preparation are the displaced warps' (vstab_launch_displaced, vstab_prepare_displaced).
// row_residual_kernel: one workgroup per (pair, grid row); the row's admitted residuals (vstab_fit_residual) are compacted
// into LDS (order does not matter to a median) and ranked by counting (vstab_median_pair), as vstab_mesh.hip does per vertex.
// A row of a 960-px estimation image has 120 samples: microseconds per clip.
// rectify_kernel (vstab_rectify_samples_batch): the flow grid's samples as point pairs whose two ends are moved by the
// inverse's e at a point (RowInverseDisplacement::solve_at), for the refit of the pair transitions; one workgroup per pair,
// an ordered block compaction of the admitted samples, 24 bytes per sample: 0.05 ms for the 255 pairs of a 960 x 540 grid.
// Built with -ffp-contract=off like the rest of the library.
#define VSTAB_WARP_ARITHMETIC
#include "vstab_internal.h"
#include <cmath>

namespace {

constexpr int ROW_THREADS = 256;
constexpr int ROW_MAX_SAMPLES = 4096;       // grid positions of one row: 2 x 16 KB of LDS
constexpr int RECTIFY_THREADS = 512;        // the fit kernel's block: one workgroup per pair
constexpr int RECTIFY_WAVES = RECTIFY_THREADS / 64;
constexpr int RECTIFY_MAX_SAMPLES = 16384;  // what vstab_points_fit_batch takes per pair (MAX_SORT in vstab_fit.hip)

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
        return solve_at(rho * (yd / hm1 - 0.5), xd, yd, ex, ey);
    }
    // the same for a point (xd, yd) that is no pixel, at the row time tau (the sample rectifier's: its row is clamped)
    __device__ __forceinline__ bool solve_at(double tau, double xd, double yd, double& ex, double& ey) const
    {
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

// The rolling warp's arguments: the plain warp's plus the per-frame velocity coefficients and the readout.
struct RollingWarpArgs : WarpArgs {
    const double* velocity;   // [n, 6]
    double readout;
};

// The inverse's: the forward warp's plus the count of pixels whose solve was refused (the shared body's second counter).
struct RollingUnwarpArgs : RollingWarpArgs {
    unsigned* unconverged;    // [n] or nullptr
};

// The displacement these arguments ask for (make_displacement, vstab_internal.h): a closed form of the frame's six
// coefficients (block-uniform).  The row lever is the SOURCE's height for the forward warp and the OUTPUT's for the inverse,
// which is the forward warp's source.
__device__ __forceinline__ RowDisplacement make_displacement(const RollingWarpArgs& a, int frame)
{
    const double* __restrict__ V = a.velocity + (size_t)frame * 6;
    return RowDisplacement{V[0], V[1], V[2], V[3], V[4], V[5], a.readout, (double)(a.sh - 1)};
}
__device__ __forceinline__ RowInverseDisplacement make_displacement(const RollingUnwarpArgs& a, int frame)
{
    const double* __restrict__ V = a.velocity + (size_t)frame * 6;
    return RowInverseDisplacement{V[0], V[1], V[2], V[3], V[4], V[5], a.readout, (double)(a.dh - 1)};
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
        float rx, ry;
        if (!vstab_fit_residual(A, x, y, G[g * 2], G[g * 2 + 1], rx, ry)) continue;
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
    vstab_median_pair(s_rx, s_ry, n, out);
    if (threadIdx.x == 0) a.count[cell] = n;
}

struct RectifyArgs {
    const float* grid;        // [pairs][gh*gw][2]
    const double* velocity;   // [pairs + 1][6], working px per frame interval
    const uint8_t* blocked;   // [pairs + 1][gh*gw] or nullptr
    float* out;               // [pairs][gh*gw][4]
    int* counts;              // [pairs]
    unsigned* unsolved;       // [pairs]
    int gw, cells, step;
    double rho, hm1;
};

// s + e of the rule (vstab_rectify_samples_batch in include/vstab.h), each coordinate rounded once to float32 -> solved
__device__ __forceinline__ bool rectify_point(const RowInverseDisplacement& f, float sx, float sy, float& qx, float& qy)
{
    const double x = (double)sx, y = (double)sy;
    double yr = (y < 0.0) ? 0.0 : y;            // a NaN stays a NaN
    yr = (yr > f.hm1) ? f.hm1 : yr;
    double ex, ey;
    const bool solved = f.solve_at(f.rho * (yr / f.hm1 - 0.5), x, y, ex, ey);
    qx = (float)(x + ex);
    qy = (float)(y + ey);
    return solved;
}

// One workgroup per pair.  Thread t owns the grid samples [t*per, (t+1)*per): it counts its admitted ones, the block scans
// the counts (the fit kernel's wavefront scan) and the thread writes its pairs from its offset on, so the grid order is kept.
__global__ __launch_bounds__(RECTIFY_THREADS) void rectify_kernel(RectifyArgs a)
{
    __shared__ int s_wave[RECTIFY_WAVES];
    __shared__ BlockSums<unsigned, 1, RECTIFY_THREADS> s_bad;
    const int pair = (int)blockIdx.x, tid = (int)threadIdx.x;
    const float* __restrict__ G = a.grid + (size_t)pair * a.cells * 2;
    const uint8_t* __restrict__ B0 = a.blocked ? a.blocked + (size_t)pair * a.cells : nullptr;
    const uint8_t* __restrict__ B1 = a.blocked ? B0 + a.cells : nullptr;
    float* __restrict__ out = a.out + (size_t)pair * a.cells * 4;
    const double* __restrict__ V = a.velocity + (size_t)pair * 6;
    const RowInverseDisplacement prev{V[0], V[1], V[2], V[3], V[4], V[5], a.rho, a.hm1};
    const RowInverseDisplacement next{V[6], V[7], V[8], V[9], V[10], V[11], a.rho, a.hm1};

    const int per = (a.cells + RECTIFY_THREADS - 1) / RECTIFY_THREADS;
    const int g0 = min(tid * per, a.cells), g1 = min(g0 + per, a.cells);
    int local = g1 - g0;
    if (B0 != nullptr) {
        local = 0;
        for (int g = g0; g < g1; g++) local += ((B0[g] | B1[g]) == 0) ? 1 : 0;
    }
    int incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d);
        if ((tid & 63) >= d) incl += o;
    }
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < RECTIFY_WAVES; i++) {
        if (i < (tid >> 6)) before += s_wave[i];
        total += s_wave[i];
    }

    const float nan = __uint_as_float(0x7fc00000u);
    int o = before + incl - local;               // < total <= cells
    unsigned bad = 0;
    for (int g = g0; g < g1; g++) {
        if (B0 != nullptr && (B0[g] | B1[g])) continue;
        const int gy = g / a.gw, gx = g - gy * a.gw;
        const float px = (float)(gx * a.step), py = (float)(gy * a.step);
        const float cx = px + G[(size_t)g * 2], cy = py + G[(size_t)g * 2 + 1];
        float4 q;
        bad += rectify_point(prev, px, py, q.x, q.y) ? 0u : 1u;
        if (isfinite(cx) && isfinite(cy)) bad += rectify_point(next, cx, cy, q.z, q.w) ? 0u : 1u;
        else { q.z = nan; q.w = nan; }
        *reinterpret_cast<float4*>(out + (size_t)o * 4) = q;
        o++;
    }
    for (int k = total + tid; k < a.cells; k += RECTIFY_THREADS)
        *reinterpret_cast<float4*>(out + (size_t)k * 4) = make_float4(nan, nan, nan, nan);
    s_bad.put({bad});
    __syncthreads();
    if (tid == 0) { a.counts[pair] = total; a.unsolved[pair] = s_bad.total(0); }
}

// Both directions: the checks, the preparation and the launch.  inverse: the row lever is the output's height, `unsolved` is
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
    RollingUnwarpArgs a{};
    unsigned blocks = 0;
    const void* d_velocity = nullptr;      // the n x 6 coefficients ride behind the transform records of the staged table
    if (int rc = vstab_prepare_displaced(who, ctx, a, src, n, src_h, src_w, matrices, out_h, out_w, border_rgb, dst, mask, pad_count,
                                         unsolved, velocity, (size_t)n * 6 * sizeof(double), &d_velocity, &blocks)) return rc;
    a.velocity = static_cast<const double*>(d_velocity); a.readout = readout; a.unconverged = unsolved;
    KernelTimer timer(ctx, inverse ? "rolling_unwarp" : "rolling_warp");
    if (inverse) vstab_launch_displaced<RollingUnwarpArgs>(a, blocks, subpix, mask != nullptr, 0, ctx->stream);
    else vstab_launch_displaced<RollingWarpArgs>(a, blocks, subpix, mask != nullptr, 0, ctx->stream);
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
    unsigned blocks = 0;
    if (int rc = vstab_check_residual(who, ctx, grid_flow, transitions, residual, count, pairs, gh, gw, step, work_h, work_w, gh, &blocks)) return rc;
    VSTAB_REQUIRE(gw <= ROW_MAX_SAMPLES, "%s: a row of %d grid positions exceeds %d", who, gw, ROW_MAX_SAMPLES);
    VSTAB_HIP(hipSetDevice(ctx->device));
    void* d_mats = nullptr;
    if (int rc = vstab_stage_params(ctx, transitions, (size_t)pairs * 9 * sizeof(float), &d_mats)) return rc;
    RowResidualArgs a{};
    a.grid = grid_flow; a.mats = static_cast<const float*>(d_mats); a.blocked = blocked; a.residual = residual; a.count = count;
    a.gh = gh; a.gw = gw; a.step = step;
    const size_t lds = (size_t)gw * 2 * sizeof(float);     // <= 32 KB
    KernelTimer timer(ctx, "row_residual");
    hipLaunchKernelGGL(row_residual_kernel, dim3(blocks), dim3(ROW_THREADS), lds, ctx->stream, a);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

extern "C" int vstab_rectify_samples_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h,
                                           const double* velocity, double readout, const uint8_t* blocked, float* point_pairs,
                                           int32_t* counts, uint32_t* unsolved)
{
    const char* who = "vstab_rectify_samples_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    VSTAB_REQUIRE(grid_flow && velocity && point_pairs && counts && unsolved, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(pairs > 0 && gh > 0 && gw > 0 && step > 0 && work_h >= 2, "%s: needs pairs > 0, a grid, step > 0 and an image of at least 2 rows (pairs=%d grid=%dx%d step=%d work_h=%d)", who, pairs, gw, gh, step, work_h);
    VSTAB_REQUIRE(gh == (work_h + step - 1) / step, "%s: %d grid rows are not ceil(%d / %d)", who, gh, work_h, step);
    VSTAB_REQUIRE((long long)gh * gw <= RECTIFY_MAX_SAMPLES, "%s: %lld sample points exceed the supported %d", who, (long long)gh * gw, RECTIFY_MAX_SAMPLES);
    VSTAB_REQUIRE((long long)(gw - 1) * step < (1LL << 24), "%s: a grid of %d columns at step %d leaves the exact float32 range", who, gw, step);
    VSTAB_REQUIRE(readout >= -1.0 && readout <= 1.0, "%s: readout=%g outside [-1, 1] (a fraction of the frame interval)", who, readout);
    VSTAB_HIP(hipSetDevice(ctx->device));
    void* d_velocity = nullptr;
    if (int rc = vstab_stage_params(ctx, velocity, (size_t)(pairs + 1) * 6 * sizeof(double), &d_velocity)) return rc;
    RectifyArgs a{};
    a.grid = grid_flow; a.velocity = static_cast<const double*>(d_velocity); a.blocked = blocked; a.out = point_pairs;
    a.counts = counts; a.unsolved = unsolved; a.gw = gw; a.cells = gh * gw; a.step = step; a.rho = readout; a.hm1 = (double)(work_h - 1);
    KernelTimer timer(ctx, "rectify");
    hipLaunchKernelGGL(rectify_kernel, dim3((unsigned)pairs), dim3(RECTIFY_THREADS), 0, ctx->stream, a);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
