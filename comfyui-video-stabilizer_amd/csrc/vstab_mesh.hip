// vstab_mesh.hip -- mesh warp: the per-vertex residual of a global fit (vstab_mesh_residual_batch) and the warp that takes
// it out (vstab_mesh_warp_batch).  Not a reference feature; both rules are stated in include/vstab.h.
//
// mesh_residual_kernel: one workgroup per (pair, vertex).  The grid samples of the four cells around the vertex are
// tested, their residuals compacted into LDS (order does not matter to a median), and every thread counts the rank of its
// elements against all others: the element of rank (n-1)/2 and the one of rank n/2 are the middle(s).  8 k samples per
// pair at 960x540 -- microseconds; it is not where the time goes.
//
// mesh_warp_kernel: vstab_warp.hip's warp_kernel (64 x 8 output tile, 2 pixels per thread strided by 32, XCD remap, count
// reduction) with the displacement lookup between the coordinate terms and the roundings.  The frame's vertex table
// (mw * mh * 8 bytes: 1.4 KB by default) is staged in LDS once per workgroup.  The samplers below are the bilinear halves
// of vstab_warp.hip's sample_q5 / sample_exact, operation for operation; tests/test_mesh_warp_gpu.py holds the two kernels
// to each other in bits (all-zero offsets) over both sub-pixel models, affine and perspective matrices and border tiles.
// Built with -ffp-contract=off like the rest of the library.
#include "vstab_internal.h"
#include <cmath>

namespace {

// ---- residual ---------------------------------------------------------------------------------------------------------
constexpr int MESH_THREADS = 256;
constexpr int MESH_MAX_VERTS = 65;          // per axis (64 cells)
constexpr int MESH_MAX_NEIGHBOURHOOD = 16384;   // grid positions of one vertex: 2 x 64 KB of the CU's 160 KB of LDS

struct MeshResidualArgs {
    const float* grid;
    const float* mats;       // [pairs, 9] f32
    const uint8_t* blocked;  // [pairs + 1, gh, gw] or nullptr
    float* residual;
    int* count;
    int gh, gw, step, work_h, work_w, mw, mh, cap;
};

__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN

__global__ __launch_bounds__(MESH_THREADS) void mesh_residual_kernel(MeshResidualArgs a)
{
    extern __shared__ float s_val[];       // [2][cap]: x residuals, y residuals
    __shared__ int s_n;
    __shared__ float s_mid[2][2];          // [axis][lo, hi]
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
        const float u = G[g * 2], v = G[g * 2 + 1];
        const double X = (A[0] * x + A[1] * y) + A[2];
        const double Y = (A[3] * x + A[4] * y) + A[5];
        const double W = (A[6] * x + A[7] * y) + A[8];
        const float rx = (float)((x + (double)u) - X / W);
        const float ry = (float)((y + (double)v) - Y / W);
        if (!(finite_f(u) && finite_f(v) && finite_f(rx) && finite_f(ry))) continue;
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
    // rank of element i: values below it, and equal values in front of it -- a permutation of 0..n-1
    const int klo = (n - 1) >> 1, khi = n >> 1;
    for (int i = threadIdx.x; i < n; i += MESH_THREADS) {
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
        a.count[(size_t)pair * verts + vert] = n;
    }
}

// ---- warp --------------------------------------------------------------------------------------------------------------
constexpr int TILE_PX = 2, TILE_TX = 32, TILE_W = TILE_TX * TILE_PX, TILE_H = 256 / TILE_TX;   // vstab_warp.hip's default tile

struct MeshWarpArgs {
    const float* src;
    float* dst;
    float* mask;
    unsigned* pad_count;
    const WarpXform* xf;
    const float* offsets;   // [n, mh, mw, 2]
    int n, sh, sw, dh, dw, mw, mh;
    int bw0, bw0_pow2;      // column block width of OpenCV's WarpPerspectiveInvoker
    int tiles_x, tiles_y;
    float b0, b1, b2;
};

__device__ __forceinline__ int clamp_round_i32(double v)
{
    // std::max((double)INT_MIN, std::min((double)INT_MAX, v)) followed by cvRound
    const double hi = 2147483647.0, lo = -2147483648.0;
    double m = (v < hi) ? v : hi;
    double r = (lo < m) ? m : lo;
    return (int)__builtin_rint(r);
}

__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

struct Px { float r, g, b; };

__device__ __forceinline__ Px load_px(const float* p)
{
    Px v;
    __builtin_memcpy(&v, p, 12);
    return v;
}

// vstab_warp.hip: sample_q5<VSTAB_INTERP_BILINEAR>
__device__ __forceinline__ Px sample_q5_bilinear(const float* __restrict__ S, int sh, int sw, int X, int Y, float b0, float b1, float b2)
{
    const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
    const int fx = X & 31, fy = Y & 31;
    Px o;
    const float wx1 = fx * (1.f / 32), wx0 = 1.f - wx1;
    const float wy1 = fy * (1.f / 32), wy0 = 1.f - wy1;
    const float w0 = wy0 * wx0, w1 = wy0 * wx1, w2 = wy1 * wx0, w3 = wy1 * wx1;
    if ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1)) {
        const float* p = S + ((unsigned)sy * (unsigned)sw + (unsigned)sx) * 3u;
        float r0[6], r1[6];
        __builtin_memcpy(r0, p, 24);
        __builtin_memcpy(r1, p + (unsigned)sw * 3u, 24);
        o.r = r0[0] * w0 + r0[3] * w1 + r1[0] * w2 + r1[3] * w3;
        o.g = r0[1] * w0 + r0[4] * w1 + r1[1] * w2 + r1[4] * w3;
        o.b = r0[2] * w0 + r0[5] * w1 + r1[2] * w2 + r1[5] * w3;
        return o;
    }
    if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
        o.r = b0; o.g = b1; o.b = b2;
        return o;
    }
    const bool x0ok = sx >= 0 && sx < sw, x1ok = sx + 1 >= 0 && sx + 1 < sw;
    const bool y0ok = sy >= 0 && sy < sh, y1ok = sy + 1 >= 0 && sy + 1 < sh;
    const Px bd = {b0, b1, b2};
    const Px v0 = (x0ok && y0ok) ? load_px(S + ((unsigned)sy * (unsigned)sw + (unsigned)sx) * 3u) : bd;
    const Px v1 = (x1ok && y0ok) ? load_px(S + ((unsigned)sy * (unsigned)sw + (unsigned)(sx + 1)) * 3u) : bd;
    const Px v2 = (x0ok && y1ok) ? load_px(S + ((unsigned)(sy + 1) * (unsigned)sw + (unsigned)sx) * 3u) : bd;
    const Px v3 = (x1ok && y1ok) ? load_px(S + ((unsigned)(sy + 1) * (unsigned)sw + (unsigned)(sx + 1)) * 3u) : bd;
    o.r = v0.r * w0 + v1.r * w1 + v2.r * w2 + v3.r * w3;
    o.g = v0.g * w0 + v1.g * w1 + v2.g * w2 + v3.g * w3;
    o.b = v0.b * w0 + v1.b * w1 + v2.b * w2 + v3.b * w3;
    return o;
}

// vstab_warp.hip: sample_exact
__device__ __forceinline__ Px sample_exact(const float* __restrict__ S, int sh, int sw, float fsx, float fsy, float b0, float b1, float b2)
{
    Px o;
    const float flx = __builtin_floorf(fsx), fly = __builtin_floorf(fsy);
    const bool bad = !(fsx == fsx) || !(fsy == fsy) || flx >= 2.0e9f || flx <= -2.0e9f || fly >= 2.0e9f || fly <= -2.0e9f;
    const int ix = bad ? 0 : (int)flx, iy = bad ? 0 : (int)fly;
    const float ax = fsx - ix, ay = fsy - iy;
    if (bad || ix >= sw || ix + 1 < 0 || iy >= sh || iy + 1 < 0) {
        o.r = b0; o.g = b1; o.b = b2;
        return o;
    }
    const bool x0ok = ix >= 0 && ix < sw, x1ok = ix + 1 >= 0 && ix + 1 < sw;
    const bool y0ok = iy >= 0 && iy < sh, y1ok = iy + 1 >= 0 && iy + 1 < sh;
    const Px bd = {b0, b1, b2};
    const Px p00 = (x0ok && y0ok) ? load_px(S + ((unsigned)iy * (unsigned)sw + (unsigned)ix) * 3u) : bd;
    const Px p01 = (x1ok && y0ok) ? load_px(S + ((unsigned)iy * (unsigned)sw + (unsigned)(ix + 1)) * 3u) : bd;
    const Px p10 = (x0ok && y1ok) ? load_px(S + ((unsigned)(iy + 1) * (unsigned)sw + (unsigned)ix) * 3u) : bd;
    const Px p11 = (x1ok && y1ok) ? load_px(S + ((unsigned)(iy + 1) * (unsigned)sw + (unsigned)(ix + 1)) * 3u) : bd;
    float v0, v1;
    v0 = p00.r + ax * (p01.r - p00.r); v1 = p10.r + ax * (p11.r - p10.r); o.r = v0 + ay * (v1 - v0);
    v0 = p00.g + ax * (p01.g - p00.g); v1 = p10.g + ax * (p11.g - p10.g); o.g = v0 + ay * (v1 - v0);
    v0 = p00.b + ax * (p01.b - p00.b); v1 = p10.b + ax * (p11.b - p10.b); o.b = v0 + ay * (v1 - v0);
    return o;
}

// vstab_warp.hip: xcd_remap (8 XCDs, round-robin dispatch: the blocks of one XCD get a contiguous run of tiles)
__device__ __forceinline__ unsigned xcd_remap(unsigned b, unsigned nblk)
{
    const unsigned q = nblk >> 3, r = nblk & 7, x = b & 7, i = b >> 3;
    const unsigned base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + i;
}

// one axis of the lookup: clamped coordinate -> cell index and fraction (the rule's operation order)
__device__ __forceinline__ void mesh_cell(double q, int size, int verts, int* cell, double* frac)
{
    double t = (q > 0.0) ? q : 0.0;                 // NaN -> 0
    const double top = (double)(size - 1);
    t = (t < top) ? t : top;
    const double g = t * (double)(verts - 1) / top;
    int i = (int)g;
    i = i < verts - 2 ? i : verts - 2;
    *cell = i;
    *frac = g - (double)i;
}

template <int SUBPIX, bool WITH_MASK>
__global__ __launch_bounds__(256) void mesh_warp_kernel(MeshWarpArgs a)
{
    constexpr bool EXACT = SUBPIX == VSTAB_SUBPIX_EXACT;
    extern __shared__ float s_off[];      // this frame's vertex table [mh][mw][2]
    __shared__ unsigned s_cnt[4];
    const unsigned t = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned tiles_per_frame = (unsigned)a.tiles_x * a.tiles_y;
    const int frame = t / tiles_per_frame;
    const unsigned tr = t - frame * tiles_per_frame;
    const int tile_y = tr / a.tiles_x, tile_x = tr - tile_y * a.tiles_x;
    const int tx = threadIdx.x % TILE_TX, ty = threadIdx.x / TILE_TX;
    const int x0 = tile_x * TILE_W + tx;
    const int y = tile_y * TILE_H + ty;
    const bool active = (y < a.dh) && (x0 < a.dw);
    const int npx = active ? (a.dw - x0 + TILE_TX - 1) / TILE_TX : 0;

    const int table = a.mw * a.mh * 2;
    const float* __restrict__ O = a.offsets + (size_t)frame * table;
    for (int i = threadIdx.x; i < table; i += 256) s_off[i] = O[i];
    __syncthreads();

    const float* __restrict__ S = a.src + (size_t)frame * a.sh * a.sw * 3;
    float acc[TILE_PX][3];
    float cov[TILE_PX];
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) { acc[p][0] = acc[p][1] = acc[p][2] = 0.f; cov[p] = 0.f; }

    if (active) {
        const WarpXform* __restrict__ xf = a.xf + frame;
        const double m0 = xf->m[0], m1 = xf->m[1], m2 = xf->m[2], m3 = xf->m[3], m4 = xf->m[4], m5 = xf->m[5];
        const double m6 = xf->m[6], m7 = xf->m[7], m8 = xf->m[8];
        const bool affine = xf->affine != 0;
        float mf[9];
        if (EXACT) {
#pragma unroll
            for (int i = 0; i < 9; i++) mf[i] = (float)xf->m[i];
        }
        const double dy = (double)y;
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (p >= npx) continue;
            const int x = x0 + p * TILE_TX;
            int xb;
            if (a.bw0 >= a.dw) xb = 0;
            else if (a.bw0_pow2) xb = x & ~(a.bw0 - 1);
            else xb = (x / a.bw0) * a.bw0;
            const double dxb = (double)xb;
            const double X0 = m0 * dxb + m1 * dy + m2;
            const double Y0 = m3 * dxb + m4 * dy + m5;
            const double W0 = m6 * dxb + m7 * dy + m8;
            const double dx1 = (double)(x - xb);
            const double Xn = X0 + m0 * dx1, Yn = Y0 + m3 * dx1;
            double Wq, Wn;
            if (affine) { Wq = xf->wq; Wn = xf->wn; }
            else {
                const double W = W0 + m6 * dx1;
                Wn = (W != 0.0) ? 1.0 / W : 0.0;
                Wq = 32.0 * Wn;
            }
            // ---- the displacement at q
            const double qx = Xn * Wn, qy = Yn * Wn;
            int ia, ib;
            double fa, fb;
            mesh_cell(qx, a.sw, a.mw, &ia, &fa);
            mesh_cell(qy, a.sh, a.mh, &ib, &fb);
            const float* __restrict__ c0 = s_off + (ib * a.mw + ia) * 2;
            const float* __restrict__ c1 = c0 + a.mw * 2;
            const double ga = 1.0 - fa, gb = 1.0 - fb;
            const double cx = ((double)c0[0] * ga + (double)c0[2] * fa) * gb + ((double)c1[0] * ga + (double)c1[2] * fa) * fb;
            const double cy = ((double)c0[1] * ga + (double)c0[3] * fa) * gb + ((double)c1[1] * ga + (double)c1[3] * fa) * fb;
            // ---- the plain warp's roundings, at s = q - c
            Px v;
            if (EXACT) {
                const float w = x * mf[6] + y * mf[7] + mf[8];
                const float fsx = (x * mf[0] + y * mf[1] + mf[2]) / w;
                const float fsy = (x * mf[3] + y * mf[4] + mf[5]) / w;
                v = sample_exact(S, a.sh, a.sw, (float)((double)fsx - cx), (float)((double)fsy - cy), a.b0, a.b1, a.b2);
            } else {
                const int X = clamp_round_i32(Xn * Wq - 32.0 * cx);
                const int Y = clamp_round_i32(Yn * Wq - 32.0 * cy);
                v = sample_q5_bilinear(S, a.sh, a.sw, X, Y, a.b0, a.b1, a.b2);
            }
            acc[p][0] = v.r; acc[p][1] = v.g; acc[p][2] = v.b;
            if (WITH_MASK) {
                const int nx = sat_short(clamp_round_i32(qx - cx));
                const int ny = sat_short(clamp_round_i32(qy - cy));
                cov[p] = ((unsigned)nx < (unsigned)a.sw && (unsigned)ny < (unsigned)a.sh) ? 1.f : 0.f;
            }
        }
    }

    float mk[TILE_PX];
    unsigned padded = 0;
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) {
        float m = 1.0f - cov[p];
        mk[p] = (m < 1e-3f) ? 0.f : m;
        if (WITH_MASK && p < npx) padded += (mk[p] > 0.5f) ? 1u : 0u;
    }

    if (active) {
        float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
        float* __restrict__ Mk = WITH_MASK ? a.mask + (size_t)frame * a.dh * a.dw : nullptr;
        const unsigned row = (unsigned)y * (unsigned)a.dw;
        typedef float f3 __attribute__((ext_vector_type(3)));
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (p >= npx) continue;
            const unsigned pix = row + (unsigned)(x0 + p * TILE_TX);
            f3 rgb = {acc[p][0], acc[p][1], acc[p][2]};
            __builtin_memcpy(D + pix * 3u, &rgb, 12);
            if (WITH_MASK) Mk[pix] = mk[p];
        }
    }

    if (WITH_MASK && a.pad_count != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) padded += __shfl_down(padded, off);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = padded;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            if (total) atomicAdd(a.pad_count + frame, total);
        }
    }
}

}  // namespace

extern "C" int vstab_mesh_residual_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h,
                                         int work_w, const float* transitions, const uint8_t* blocked, int mw, int mh,
                                         float* residual, int32_t* count)
{
    VSTAB_REQUIRE(ctx != nullptr, "vstab_mesh_residual_batch: ctx is NULL");
    VSTAB_REQUIRE(grid_flow && transitions && residual && count, "vstab_mesh_residual_batch: NULL pointer argument");
    VSTAB_REQUIRE(pairs > 0 && step > 0 && work_h >= 2 && work_w >= 2, "vstab_mesh_residual_batch: needs pairs > 0, step > 0 and an image of at least 2x2 (pairs=%d step=%d %dx%d)", pairs, step, work_w, work_h);
    VSTAB_REQUIRE(gh == (work_h + step - 1) / step && gw == (work_w + step - 1) / step, "vstab_mesh_residual_batch: grid %dx%d is not ceil(%dx%d / %d)", gw, gh, work_w, work_h, step);
    VSTAB_REQUIRE(mw >= 2 && mh >= 2 && mw <= MESH_MAX_VERTS && mh <= MESH_MAX_VERTS, "vstab_mesh_residual_batch: %dx%d vertices outside 2..%d", mw, mh, MESH_MAX_VERTS);
    // the kernel's rectangle spans floor((v - c) / step) .. ceil((v + c) / step): at most 2c / step + 3 positions per axis
    const double cw = (double)(work_w - 1) / (double)(mw - 1), ch = (double)(work_h - 1) / (double)(mh - 1);
    const long long span_x = std::min<long long>(gw, (long long)std::floor(2.0 * cw / step) + 3);
    const long long span_y = std::min<long long>(gh, (long long)std::floor(2.0 * ch / step) + 3);
    const long long cap = span_x * span_y;
    VSTAB_REQUIRE(cap <= MESH_MAX_NEIGHBOURHOOD, "vstab_mesh_residual_batch: a vertex neighbourhood of %lld grid positions exceeds %d (use a finer mesh)", cap, MESH_MAX_NEIGHBOURHOOD);
    const long long blocks = (long long)pairs * mw * mh;
    VSTAB_REQUIRE(blocks < 0x7fffffffLL, "vstab_mesh_residual_batch: clip too large");
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
    hipLaunchKernelGGL(mesh_residual_kernel, dim3((unsigned)blocks), dim3(MESH_THREADS), lds, ctx->stream, a);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

extern "C" int vstab_mesh_warp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                                     int out_h, int out_w, const float* border_rgb, int subpix, const float* offsets, int mw, int mh,
                                     float* dst, float* mask, uint32_t* pad_count)
{
    const char* who = "vstab_mesh_warp_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    VSTAB_REQUIRE(src && matrices && border_rgb && offsets && dst, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(n > 0 && src_h >= 2 && src_w >= 2 && out_h > 0 && out_w > 0, "%s: bad size (n=%d src=%dx%d out=%dx%d; the source must be at least 2x2)", who, n, src_w, src_h, out_w, out_h);
    VSTAB_REQUIRE(src_h <= 32767 && src_w <= 32767, "%s: source larger than 32767 px is not representable in OpenCV's short maps", who);
    VSTAB_REQUIRE((long long)src_h * src_w < (1LL << 30) && (long long)out_h * out_w < (1LL << 30), "%s: frames of 2^30 pixels or more are not supported (32-bit in-frame offsets)", who);
    VSTAB_REQUIRE(subpix == VSTAB_SUBPIX_Q5 || subpix == VSTAB_SUBPIX_EXACT, "%s: unknown subpix mode %d", who, subpix);
    VSTAB_REQUIRE(mw >= 2 && mh >= 2 && mw <= MESH_MAX_VERTS && mh <= MESH_MAX_VERTS, "%s: %dx%d vertices outside 2..%d", who, mw, mh, MESH_MAX_VERTS);
    VSTAB_HIP(hipSetDevice(ctx->device));
    std::vector<WarpXform> xf((size_t)n);
    for (int i = 0; i < n; i++) vstab_fill_xform(matrices + (size_t)i * 9, &xf[i]);
    void* d_xf = nullptr;
    if (int rc = vstab_stage_params(ctx, xf.data(), xf.size() * sizeof(WarpXform), &d_xf)) return rc;

    MeshWarpArgs a{};
    a.src = src; a.dst = dst; a.mask = mask; a.pad_count = pad_count; a.offsets = offsets;
    a.xf = static_cast<const WarpXform*>(d_xf);
    a.n = n; a.sh = src_h; a.sw = src_w; a.dh = out_h; a.dw = out_w; a.mw = mw; a.mh = mh;
    // OpenCV's WarpPerspectiveInvoker: blocks of bw0 columns (as vstab_warp.hip's fill_geometry)
    const int BLOCK_SZ = 32;
    const int bh0 = BLOCK_SZ / 2 < out_h ? BLOCK_SZ / 2 : out_h;
    a.bw0 = BLOCK_SZ * BLOCK_SZ / bh0 < out_w ? BLOCK_SZ * BLOCK_SZ / bh0 : out_w;
    a.bw0_pow2 = (a.bw0 & (a.bw0 - 1)) == 0;
    a.b0 = border_rgb[0]; a.b1 = border_rgb[1]; a.b2 = border_rgb[2];
    a.tiles_x = (out_w + TILE_W - 1) / TILE_W;
    a.tiles_y = (out_h + TILE_H - 1) / TILE_H;
    const unsigned long long blocks = (unsigned long long)a.tiles_x * a.tiles_y * n;
    VSTAB_REQUIRE(blocks > 0 && blocks < 0x7fffffffULL, "%s: grid of %llu blocks is out of range", who, blocks);
    if (pad_count) VSTAB_HIP(hipMemsetAsync(pad_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    const size_t lds = (size_t)mw * mh * 2 * sizeof(float);    // <= 33.8 KB
    const dim3 grid((unsigned)blocks), block(256);
    KernelTimer timer(ctx, "mesh_warp");
    if (subpix == VSTAB_SUBPIX_EXACT) {
        if (mask) hipLaunchKernelGGL((mesh_warp_kernel<VSTAB_SUBPIX_EXACT, true>), grid, block, lds, ctx->stream, a);
        else hipLaunchKernelGGL((mesh_warp_kernel<VSTAB_SUBPIX_EXACT, false>), grid, block, lds, ctx->stream, a);
    } else {
        if (mask) hipLaunchKernelGGL((mesh_warp_kernel<VSTAB_SUBPIX_Q5, true>), grid, block, lds, ctx->stream, a);
        else hipLaunchKernelGGL((mesh_warp_kernel<VSTAB_SUBPIX_Q5, false>), grid, block, lds, ctx->stream, a);
    }
    VSTAB_HIP(hipGetLastError());
    return 0;
}
