// vstab_mesh.hip -- mesh warp: the per-vertex residual of a global fit (vstab_mesh_residual_batch).  The warp that takes it
// out (vstab_mesh_warp_batch) is warp_pixel (vstab_internal.h) with a displacement hook and lives in vstab_warp.hip.  Not a reference
// feature; both rules are stated in include/vstab.h.
//
// mesh_residual_kernel: one workgroup per (pair, vertex).  The grid samples of the four cells around the vertex are
// tested, their residuals (vstab_fit_residual) compacted into LDS (order does not matter to a median) and ranked by
// counting (vstab_median_pair); both pieces and the entry point's common checks (vstab_check_residual, defined here) are
// vstab_internal.h's, shared with the per-row form in vstab_rolling.hip.  8 k samples per pair at 960x540 -- microseconds;
// it is not where the time goes.
// Built with -ffp-contract=off like the rest of the library.
#include "vstab_internal.h"
#include <cmath>

namespace {

constexpr int MESH_THREADS = 256;
constexpr int MESH_MAX_NEIGHBOURHOOD = 16384;   // grid positions of one vertex: 2 x 64 KB of the CU's 160 KB of LDS

struct MeshResidualArgs {
    const float* grid;
    const float* mats;       // [pairs, 9] f32
    const uint8_t* blocked;  // [pairs + 1, gh, gw] or nullptr
    float* residual;
    int* count;
    int gh, gw, step, work_h, work_w, mw, mh, cap;
};

__global__ __launch_bounds__(MESH_THREADS) void mesh_residual_kernel(MeshResidualArgs a)
{
    extern __shared__ float s_val[];       // [2][cap]: x residuals, y residuals
    __shared__ int s_n;
    float* s_rx = s_val;
    float* s_ry = s_val + a.cap;
    const int verts = a.mw * a.mh;
    const int pair = (int)blockIdx.x / verts, vert = (int)blockIdx.x - pair * verts;
    const int vb = vert / a.mw, va = vert - vb * a.mw;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();

    const double cw = (double)(a.work_w - 1) / (double)(a.mw - 1), ch = (double)(a.work_h - 1) / (double)(a.mh - 1);
    const double vx = (double)va * (double)(a.work_w - 1) / (double)(a.mw - 1);
    const double vy = (double)vb * (double)(a.work_h - 1) / (double)(a.mh - 1);
    // a rectangle of grid positions that holds every admitted one (the test below decides); at most `cap` positions
    const double dstep = (double)a.step;
    int gx0 = (int)floor((vx - cw) / dstep), gx1 = (int)ceil((vx + cw) / dstep);
    int gy0 = (int)floor((vy - ch) / dstep), gy1 = (int)ceil((vy + ch) / dstep);
    gx0 = max(gx0, 0); gy0 = max(gy0, 0); gx1 = min(gx1, a.gw - 1); gy1 = min(gy1, a.gh - 1);
    const int rw = gx1 - gx0 + 1, rh = gy1 - gy0 + 1;

    double A[9];
    for (int k = 0; k < 9; k++) A[k] = (double)a.mats[(size_t)pair * 9 + k];
    const size_t cells = (size_t)a.gh * a.gw;
    const float* __restrict__ G = a.grid + (size_t)pair * cells * 2;
    const uint8_t* __restrict__ B0 = a.blocked ? a.blocked + (size_t)pair * cells : nullptr;
    const uint8_t* __restrict__ B1 = a.blocked ? B0 + cells : nullptr;

    for (int item = threadIdx.x; item < rw * rh; item += MESH_THREADS) {
        const int ry_ = item / rw, gx = gx0 + item - ry_ * rw, gy = gy0 + ry_;
        const double x = (double)(gx * a.step), y = (double)(gy * a.step);
        if (!(fabs(x - vx) < cw && fabs(y - vy) < ch)) continue;
        const size_t g = (size_t)gy * a.gw + gx;
        if (B0 != nullptr && (B0[g] | B1[g])) continue;
        float rx, ry;
        if (!vstab_fit_residual(A, x, y, G[g * 2], G[g * 2 + 1], rx, ry)) continue;
        const int slot = atomicAdd(&s_n, 1);
        if (slot < a.cap) { s_rx[slot] = rx; s_ry[slot] = ry; }     // (slot < cap always: rw * rh <= cap, checked on the host)
    }
    __syncthreads();
    const int n = min(s_n, a.cap);
    float* out = a.residual + ((size_t)pair * verts + vert) * 2;
    if (n < VSTAB_MESH_MIN_SAMPLES) {
        if (threadIdx.x == 0) { out[0] = 0.f; out[1] = 0.f; a.count[(size_t)pair * verts + vert] = n; }
        return;
    }
    vstab_median_pair(s_rx, s_ry, n, out);
    if (threadIdx.x == 0) a.count[(size_t)pair * verts + vert] = n;
}

}  // namespace

int vstab_check_residual(const char* who, vstab_ctx* ctx, const void* grid_flow, const void* transitions, const void* residual,
                         const void* count, int pairs, int gh, int gw, int step, int work_h, int work_w, long long per_pair,
                         unsigned* blocks)
{
    VSTAB_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    VSTAB_REQUIRE(grid_flow && transitions && residual && count, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(pairs > 0 && step > 0 && work_h >= 2 && work_w >= 2, "%s: needs pairs > 0, step > 0 and an image of at least 2x2 (pairs=%d step=%d %dx%d)", who, pairs, step, work_w, work_h);
    VSTAB_REQUIRE(gh == (work_h + step - 1) / step && gw == (work_w + step - 1) / step, "%s: grid %dx%d is not ceil(%dx%d / %d)", who, gw, gh, work_w, work_h, step);
    VSTAB_REQUIRE(pairs * per_pair < 0x7fffffffLL, "%s: clip too large", who);
    *blocks = (unsigned)(pairs * per_pair);
    return 0;
}

extern "C" int vstab_mesh_residual_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h,
                                         int work_w, const float* transitions, const uint8_t* blocked, int mw, int mh,
                                         float* residual, int32_t* count)
{
    const char* who = "vstab_mesh_residual_batch";
    unsigned blocks = 0;
    if (int rc = vstab_check_residual(who, ctx, grid_flow, transitions, residual, count, pairs, gh, gw, step, work_h, work_w, (long long)mw * mh, &blocks)) return rc;
    VSTAB_REQUIRE(mw >= 2 && mh >= 2 && mw <= MESH_MAX_VERTS && mh <= MESH_MAX_VERTS, "vstab_mesh_residual_batch: %dx%d vertices outside 2..%d", mw, mh, MESH_MAX_VERTS);
    // the kernel's rectangle spans floor((v - c) / step) .. ceil((v + c) / step): at most 2c / step + 3 positions per axis
    const double cw = (double)(work_w - 1) / (double)(mw - 1), ch = (double)(work_h - 1) / (double)(mh - 1);
    const long long span_x = std::min<long long>(gw, (long long)std::floor(2.0 * cw / step) + 3);
    const long long span_y = std::min<long long>(gh, (long long)std::floor(2.0 * ch / step) + 3);
    const long long cap = span_x * span_y;
    VSTAB_REQUIRE(cap <= MESH_MAX_NEIGHBOURHOOD, "vstab_mesh_residual_batch: a vertex neighbourhood of %lld grid positions exceeds %d (use a finer mesh)", cap, MESH_MAX_NEIGHBOURHOOD);
    VSTAB_HIP(hipSetDevice(ctx->device));
    void* d_mats = nullptr;
    if (int rc = vstab_stage_params(ctx, transitions, (size_t)pairs * 9 * sizeof(float), &d_mats)) return rc;
    MeshResidualArgs a{};
    a.grid = grid_flow; a.mats = static_cast<const float*>(d_mats); a.blocked = blocked; a.residual = residual; a.count = count;
    a.gh = gh; a.gw = gw; a.step = step; a.work_h = work_h; a.work_w = work_w; a.mw = mw; a.mh = mh; a.cap = (int)cap;
    const size_t lds = (size_t)cap * 2 * sizeof(float);
    if (lds > 48 * 1024)
        VSTAB_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mesh_residual_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    KernelTimer timer(ctx, "mesh_residual");
    hipLaunchKernelGGL(mesh_residual_kernel, dim3(blocks), dim3(MESH_THREADS), lds, ctx->stream, a);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
