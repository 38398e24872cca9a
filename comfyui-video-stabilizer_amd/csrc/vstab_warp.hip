// vstab_warp.hip -- perspective/similarity warp with padding mask, its mesh-displaced forms (mesh_warp_kernel and its
// inverse, mesh_unwarp_kernel), the multi-sample motion blur, the temporal fill (plain, and blended: fill_gain_sums_kernel,
// temporal_fill_blend_kernel), the sharpness transfer (sharp_transfer_kernel) and the coverage extent of the dynamic zoom
// (cover_extent_kernel: warp_pixel's coverage bit alone, nothing sampled).
// All of them take their coordinates from ONE definition, warp_pixel, and
// share one tile shell (TileShell, warp_kernel's body, block_count_add); the scalar pieces that vstab_crop / vstab_dis / vstab_tvl1
// use too are in vstab_internal.h.  profiles/warp_traffic.json is tied to the hash of these two files: the warp's arithmetic
// stays in them.
//
// Replaces the OpenCV calls of nodes/video_stabilizer_flow.py:560-588 (F13) and
// nodes/motion_apply.py:75-202 (A3, A5) of the reference.  Arithmetic follows OpenCV's
// legacy warpPerspective/remap kernels (f64 coordinate math evaluated per 64-wide block,
// 1/32-px quantised fractions, f32 weights, left-to-right f32 sums) so that the result is
// bit-identical to oracle/vo_warp.c.  Built with -ffp-contract=off: no FMA may be formed.
//
// Kernel shape (HBM-bound, 28 B of algorithmic traffic per output pixel):
//   * one 256-thread block = 64 x 8 output tile (32 threads along x, 2 pixels per thread strided by 32, so the
//     lanes of a wavefront cover consecutive pixels: tap loads and stores touch whole cache lines); the bilinear
//     source footprint of the tile stays in the CU's L1, vertically adjacent tiles share a source row through L2
//   * blockIdx is remapped so that the 8 XCDs (private L2 each) own contiguous runs of tiles
//   * padding-pixel count: wave shuffle reduction -> LDS -> one atomic per block, only if non-zero
#include "vstab_internal.h"
#include "vstab_wait.h"
#include <type_traits>
#include <cstdlib>
#include <cmath>

namespace {

constexpr int TILE_PX = 2;        // pixels per thread along x, strided by the tile width (profiles/r01_warp_tile_sweep.md)
constexpr int MAX_BLUR_SAMPLES = 33;

// WarpXform (per frame / sample transform record): vstab_internal.h

struct WarpArgs {
    const float* src;
    float* dst;
    float* mask;
    unsigned* pad_count;
    const WarpXform* xf;
    int n, sh, sw, dh, dw;
    int bw0;          // column block width of OpenCV's WarpPerspectiveInvoker
    int bw0_pow2;     // 1 if bw0 is a power of two
    int tiles_x, tiles_y;
    int samples;      // 1 for the plain warp
    int nxf_per_frame;  // sample matrices stored per frame (1 for a single-frame blur clip)
    int blur_fast;      // blur: the interior fast path may be used (host-checked preconditions, see warp_blur_kernel)
    float b0, b1, b2;   // border colour
};

// clamp_round_i32, sat_short, vstab_nn_covered (used by other translation units too): vstab_internal.h

// Round-half-even of an fp64 value known to satisfy |v| < 2^31: adding 1.5*2^52 leaves the integer in the
// low 32 bits of the sum's bit pattern (one fp64 add instead of clamp + rint + convert).  Exactly what
// cvRound gives for such values.
__device__ __forceinline__ int round_small(double v)
{
    return (int)(unsigned)__double_as_longlong(v + 6755399441055744.0);
}

// initInterTab1D(INTER_CUBIC): A = -0.75, x = i/32, same operation order as OpenCV's interpolateCubic
__device__ __forceinline__ void cubic_coeffs(int i, float* c)
{
    const float A = -0.75f;
    const float x = i * (1.f / 32);
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

struct Px { float r, g, b; };

__device__ __forceinline__ Px load_px(const float* p)
{
    Px v;
    __builtin_memcpy(&v, p, 12);
    return v;
}

template <int INTERP>
__device__ __forceinline__ Px sample_q5(const float* __restrict__ S, int sh, int sw, int X, int Y,
                                        float b0, float b1, float b2, const float* cub_tab /* LDS [32][4] or nullptr */)
{
    const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
    const int fx = X & 31, fy = Y & 31;
    Px o;
    if (INTERP == VSTAB_INTERP_BILINEAR) {
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
    } else {
        float cx[4], cy[4];
        if (cub_tab != nullptr) {   // OpenCV reads these from its own 32-entry table too (initInterTab1D): same values
            typedef float f4_t __attribute__((ext_vector_type(4)));
            const f4_t tx = reinterpret_cast<const f4_t*>(cub_tab)[fx], ty = reinterpret_cast<const f4_t*>(cub_tab)[fy];
            cx[0] = tx.x; cx[1] = tx.y; cx[2] = tx.z; cx[3] = tx.w;
            cy[0] = ty.x; cy[1] = ty.y; cy[2] = ty.z; cy[3] = ty.w;
        } else {
            cubic_coeffs(fx, cx);
            cubic_coeffs(fy, cy);
        }
        const int x0 = sx - 1, y0 = sy - 1;
        const unsigned width1 = (unsigned)(sw - 3 > 0 ? sw - 3 : 0);
        const unsigned height1 = (unsigned)(sh - 3 > 0 ? sh - 3 : 0);
        if ((unsigned)x0 < width1 && (unsigned)y0 < height1) {
            const float* p = S + ((unsigned)y0 * (unsigned)sw + (unsigned)x0) * 3u;
            float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float row[12];
                __builtin_memcpy(row, p + (unsigned)i * (unsigned)sw * 3u, 48);
                const float w0 = cy[i] * cx[0], w1 = cy[i] * cx[1], w2 = cy[i] * cx[2], w3 = cy[i] * cx[3];
                const float tr = row[0] * w0 + row[3] * w1 + row[6] * w2 + row[9] * w3;
                const float tg = row[1] * w0 + row[4] * w1 + row[7] * w2 + row[10] * w3;
                const float tb = row[2] * w0 + row[5] * w1 + row[8] * w2 + row[11] * w3;
                if (i == 0) { sr = tr; sg = tg; sb = tb; }
                else { sr += tr; sg += tg; sb += tb; }
            }
            o.r = sr; o.g = sg; o.b = sb;
            return o;
        }
        if (x0 >= sw || x0 + 4 <= 0 || y0 >= sh || y0 + 4 <= 0) {
            o.r = b0; o.g = b1; o.b = b2;
            return o;
        }
        float sr = b0, sg = b1, sb = b2;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int yy = y0 + i;
            if (yy < 0 || yy >= sh) continue;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int xx = x0 + j;
                if (xx < 0 || xx >= sw) continue;
                const Px v = load_px(S + ((unsigned)yy * (unsigned)sw + (unsigned)xx) * 3u);
                const float w = cy[i] * cx[j];
                sr += (v.r - b0) * w;
                sg += (v.g - b1) * w;
                sb += (v.b - b2) * w;
            }
        }
        o.r = sr; o.g = sg; o.b = sb;
        return o;
    }
}

__device__ __forceinline__ Px sample_exact(const float* __restrict__ S, int sh, int sw, float fsx, float fsy,
                                           float b0, float b1, float b2)
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

// XCD-aware bijective remap of the linear block id (8 XCDs, round-robin dispatch):
// blocks that share an XCD get a contiguous run of logical tile ids.
__device__ __forceinline__ unsigned xcd_remap(unsigned b, unsigned nblk)
{
    const unsigned q = nblk >> 3, r = nblk & 7, x = b & 7, i = b >> 3;
    const unsigned base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + i;
}

// Column-block origin of output column x (OpenCV evaluates the row-start terms once per block of bw0 columns).
__device__ __forceinline__ int block_origin(int x, int dw, int bw0, int bw0_pow2)
{
    if (bw0 >= dw) return 0;
    if (bw0_pow2) return x & ~(bw0 - 1);
    return (x / bw0) * bw0;
}

// The tile shell of every warp kernel: block -> (frame, tile) through the XCD remap, thread -> row y and first pixel x0 of
// its npx pixels.  Pixel p of a thread is x0 + p * TILE_TX: the lanes of a wavefront cover CONSECUTIVE output pixels, so
// one load instruction of the bilinear taps touches ~13 cache lines (24 B per lane at a 12-B lane stride) instead of 48 (at
// the 48-B stride of 4 consecutive pixels per thread) -- the texture addresser was 83 % busy that way (PMC TA_BUSY) and
// limited the read side to 2.8 TB/s -- and the stores are whole lines (12 B per lane, contiguous).
template <int TILE_TX, int NT = 256>
struct TileShell {
    static constexpr int TILE_W = TILE_TX * TILE_PX, TILE_H = NT / TILE_TX;
    int frame, tile_x, tile_y, x0, y, npx;
    bool active;
    __device__ __forceinline__ TileShell(int tiles_x, int tiles_y, int dh, int dw)
    {
        const unsigned t = xcd_remap(blockIdx.x, gridDim.x);
        const unsigned tiles_per_frame = (unsigned)tiles_x * tiles_y;
        frame = t / tiles_per_frame;
        const unsigned tr = t - frame * tiles_per_frame;
        tile_y = tr / tiles_x;
        tile_x = tr - tile_y * tiles_x;
        const int tx = threadIdx.x % TILE_TX, ty = threadIdx.x / TILE_TX;
        x0 = tile_x * TILE_W + tx;
        y = tile_y * TILE_H + ty;
        active = (y < dh) && (x0 < dw);
        npx = active ? (int)((unsigned)(dw - x0 + TILE_TX - 1) / TILE_TX) : 0;   // pixels x0 + p*TILE_TX < dw (callers cap it at TILE_PX); active: dw > x0
    }
};

// Per-thread counts of an NT-thread block -> wave shuffle -> LDS -> one atomic per counter and block, only if non-zero
// and asked for (out[c] != nullptr); out[c] is a per-frame array.
template <int NC, int NT = 256>
__device__ __forceinline__ void block_count_add(unsigned (&v)[NC], unsigned* const (&out)[NC], int frame)
{
    static_assert(NT % 64 == 0, "whole wavefronts");
    constexpr int WAVES = NT / 64;
    __shared__ unsigned s_cnt[NC][WAVES];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < NC; c++) v[c] += __shfl_down(v[c], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) s_cnt[c][threadIdx.x >> 6] = v[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            unsigned total = s_cnt[c][0];
#pragma unroll
            for (int w = 1; w < WAVES; w++) total += s_cnt[c][w];
            if (total && out[c]) atomicAdd(out[c] + frame, total);
        }
    }
}

// warp_pixel's displacement hook, of two kinds.  OUTPUT == false: a functor evaluated at the source position
// q = (Xn * Wn, Yn * Wn) that gives the offset (cx, cy) taken off it before the roundings.  OUTPUT == true: `solve`, evaluated
// on the output pixel in front of the matrix (MeshInverseDisplacement).  NoDisplacement is the plain warp: nothing of the
// hook is compiled.
struct NoDisplacement {
    static constexpr bool ACTIVE = false;
    static constexpr bool OUTPUT = false;
};

// one axis of the mesh lookup: clamped coordinate -> cell index and fraction (the rule's operation order, include/vstab.h)
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

// The mesh warp's displacement: bilinear in the frame's mw x mh vertex table (staged in LDS, [mh][mw][2]).
struct MeshDisplacement {
    static constexpr bool ACTIVE = true;
    static constexpr bool OUTPUT = false;
    const float* off;
    int sh, sw, mw, mh;
    __device__ __forceinline__ void operator()(double qx, double qy, double& cx, double& cy) const
    {
        int ia, ib;
        double fa, fb;
        mesh_cell(qx, sw, mw, &ia, &fa);
        mesh_cell(qy, sh, mh, &ib, &fb);
        const float* __restrict__ c0 = off + (ib * mw + ia) * 2;
        const float* __restrict__ c1 = c0 + mw * 2;
        const double ga = 1.0 - fa, gb = 1.0 - fb;
        cx = ((double)c0[0] * ga + (double)c0[2] * fa) * gb + ((double)c1[0] * ga + (double)c1[2] * fa) * fb;
        cy = ((double)c0[1] * ga + (double)c0[3] * fa) * gb + ((double)c1[1] * ga + (double)c1[3] * fa) * fb;
    }
};

// The mesh unwarp's displacement: the inverse of q -> q - c(q) at the output pixel, by the bounded fixed-point iteration of
// vstab_mesh_unwarp_batch's rule (include/vstab.h); `mesh` is the lookup over the OUTPUT canvas.  The trip count differs per
// lane: a plain loop, the wavefront runs as long as its slowest pixel (3 steps on a smooth field).
struct MeshInverseDisplacement {
    static constexpr bool ACTIVE = true;
    static constexpr bool OUTPUT = true;
    MeshDisplacement mesh;
    // -> converged; (ex, ey) = c of the last step taken
    __device__ __forceinline__ bool solve(int x, int y, double& ex, double& ey) const
    {
        const double px = (double)x, py = (double)y;
        double qx = px, qy = py;
        bool done = false;
        for (int k = 0; k < VSTAB_MESH_UNWARP_MAX_STEPS && !done; k++) {
            mesh(qx, qy, ex, ey);
            const double nx = px + ex, ny = py + ey;
            done = __builtin_fabs(nx - qx) <= VSTAB_MESH_UNWARP_TOL && __builtin_fabs(ny - qy) <= VSTAB_MESH_UNWARP_TOL;   // NaN: not met
            qx = nx; qy = ny;
        }
        return done;
    }
};

// One transform record in registers, as warp_kernel and temporal_fill_kernel use it for all pixels of a thread.
template <int INTERP, int SUBPIX>
struct XformRegs {
    static constexpr bool EXACT = SUBPIX == VSTAB_SUBPIX_EXACT && INTERP == VSTAB_INTERP_BILINEAR;
    double m0, m1, m2, m3, m4, m5, m6, m7, m8;
    float mf[9];      // EXACT only
    bool affine, fast_ok;
    __device__ __forceinline__ explicit XformRegs(const WarpXform* __restrict__ xf)
        : m0(xf->m[0]), m1(xf->m[1]), m2(xf->m[2]), m3(xf->m[3]), m4(xf->m[4]), m5(xf->m[5]), m6(xf->m[6]), m7(xf->m[7]),
          m8(xf->m[8]), affine(xf->affine != 0)
    {
        if (EXACT) {
#pragma unroll
            for (int i = 0; i < 9; i++) mf[i] = (float)xf->m[i];
        }
        fast_ok = affine && !EXACT;
    }
};

// The warp's source position of output pixel (x, y) under one transform, and what is sampled there: THE definition of the
// coordinate arithmetic (f64 row-start terms per OpenCV column block, Q5 rounding or the float32 `exact` chain), shared by
// warp_kernel, mesh_warp_kernel and temporal_fill_kernel.  `q5(X, Y)` samples at the 1/32-px coordinates, `exact(fsx, fsy)`
// at the float32 ones; `c` receives the nearest-neighbour coverage (WITH_MASK only).  `disp` (see NoDisplacement) moves
// the source position: s = q - disp(q), applied to the unrounded value in front of each of the three roundings.  A `disp` of
// the OUTPUT kind moves the output pixel by e = disp.solve(x, y) in front of the matrix instead: m * e is added to the
// unrounded terms Xn, Yn, W (and, float32-rounded, to the `exact` chain's), and *unconverged counts the pixels whose solve
// hit its step limit.  e == 0 adds nothing at all (not even a signed zero): the plain warp's bits.
template <int INTERP, int SUBPIX, bool WITH_MASK, class SampleQ5, class SampleExact, class Disp>
__device__ __forceinline__ Px warp_pixel(const WarpXform* __restrict__ xf, const XformRegs<INTERP, SUBPIX>& r, int sh, int sw,
                                         int dw, int bw0, int bw0_pow2, int x, int y, double dy, SampleQ5&& q5,
                                         SampleExact&& exact, const Disp& disp, float& c, unsigned* unconverged = nullptr)
{
    // OpenCV evaluates the row-start terms X0, Y0, W0 once per 64-wide column block (xb) and adds m * (x - xb)
    // per pixel; a thread's pixels lie in up to TILE_PX different blocks, so the terms are formed per pixel.
    const int xb = block_origin(x, dw, bw0, bw0_pow2);
    const double dxb = (double)xb;
    const double X0 = r.m0 * dxb + r.m1 * dy + r.m2;
    const double Y0 = r.m3 * dxb + r.m4 * dy + r.m5;
    const double W0 = r.m6 * dxb + r.m7 * dy + r.m8;
    const double dx1 = (double)(x - xb);
    const double Xn = X0 + r.m0 * dx1, Yn = Y0 + r.m3 * dx1;
    Px v;
    // Fast path (the common case): affine map whose 1/32-px coordinates stay far inside the range where
    // OpenCV's INT clamp and short saturation are no-ops.  A displaced pixel takes the general branch.
    bool small = false;
    if constexpr (!Disp::ACTIVE) small = r.fast_ok && __builtin_fabs(Xn * xf->wq) < 1.0e6 && __builtin_fabs(Yn * xf->wq) < 1.0e6;
    if (small) {
        const int X = round_small(Xn * xf->wq), Y = round_small(Yn * xf->wq);
        v = q5(X, Y);
        if (WITH_MASK) {
            const int nx = round_small(Xn * xf->wn), ny = round_small(Yn * xf->wn);
            c = ((unsigned)nx < (unsigned)sw && (unsigned)ny < (unsigned)sh) ? 1.f : 0.f;
        }
    } else {
        // OUTPUT kind: the displaced terms (Xd, Yd) and what m * e adds to W and to the float32 chain
        double Xd = Xn, Yd = Yn, dX = 0.0, dY = 0.0, dW = 0.0;
        bool moved = false;
        if constexpr (Disp::OUTPUT) {
            double ex, ey;
            if (!disp.solve(x, y, ex, ey)) *unconverged += 1u;
            moved = !(ex == 0.0 && ey == 0.0);
            if (moved) {
                dX = r.m0 * ex + r.m1 * ey; dY = r.m3 * ex + r.m4 * ey; dW = r.m6 * ex + r.m7 * ey;
                Xd = Xn + dX; Yd = Yn + dY;
            }
        }
        double Wq, Wn;
        if (r.affine) { Wq = xf->wq; Wn = xf->wn; }
        else {
            // one fp64 division serves both: 32/W == 32 * (1/W) bit for bit (scaling a correctly rounded
            // quotient by a power of two is exact)
            double W = W0 + r.m6 * dx1;
            if constexpr (Disp::OUTPUT) { if (moved) W = W + dW; }
            Wn = (W != 0.0) ? 1.0 / W : 0.0;
            Wq = 32.0 * Wn;
        }
        double cx = 0.0, cy = 0.0;
        if constexpr (Disp::ACTIVE && !Disp::OUTPUT) disp(Xn * Wn, Yn * Wn, cx, cy);
        if (XformRegs<INTERP, SUBPIX>::EXACT) {
            float fsx, fsy;
            if constexpr (Disp::OUTPUT) {
                float w = x * r.mf[6] + y * r.mf[7] + r.mf[8];
                float numx = x * r.mf[0] + y * r.mf[1] + r.mf[2], numy = x * r.mf[3] + y * r.mf[4] + r.mf[5];
                if (moved) { numx = numx + (float)dX; numy = numy + (float)dY; w = w + (float)dW; }
                fsx = numx / w; fsy = numy / w;
            } else {
                const float w = x * r.mf[6] + y * r.mf[7] + r.mf[8];
                fsx = (x * r.mf[0] + y * r.mf[1] + r.mf[2]) / w;
                fsy = (x * r.mf[3] + y * r.mf[4] + r.mf[5]) / w;
                if constexpr (Disp::ACTIVE) { fsx = (float)((double)fsx - cx); fsy = (float)((double)fsy - cy); }
            }
            v = exact(fsx, fsy);
        } else {
            double Xq = Xd * Wq, Yq = Yd * Wq;
            if constexpr (Disp::ACTIVE && !Disp::OUTPUT) { Xq = Xq - 32.0 * cx; Yq = Yq - 32.0 * cy; }
            v = q5(clamp_round_i32(Xq), clamp_round_i32(Yq));
        }
        if (WITH_MASK) {
            double qx = Xd * Wn, qy = Yd * Wn;
            if constexpr (Disp::ACTIVE && !Disp::OUTPUT) { qx = qx - cx; qy = qy - cy; }
            c = vstab_nn_covered(qx, qy, sh, sw) ? 1.f : 0.f;
        }
    }
    return v;
}

// The mesh warp's arguments: the plain warp's plus the per-frame vertex tables.
struct MeshWarpArgs : WarpArgs {
    const float* offsets;   // [n, mh, mw, 2]
    int mw, mh;
};

// The mesh unwarp's: the mesh warp's plus the count of pixels whose fixed point hit the step limit.
struct MeshUnwarpArgs : MeshWarpArgs {
    unsigned* unconverged;  // [n] or nullptr
};

// The displacement a kernel's arguments ask for.  Plain warp: none.  Mesh warp: the frame's vertex table (mw * mh * 8 bytes:
// 1.4 KB by default) is staged in LDS once per workgroup.
__device__ __forceinline__ NoDisplacement make_displacement(const WarpArgs&, int) { return {}; }
__device__ __forceinline__ const float* stage_vertex_table(const MeshWarpArgs& a, int frame)
{
    extern __shared__ float s_off[];      // this frame's vertex table [mh][mw][2]
    const int table = a.mw * a.mh * 2;
    const float* __restrict__ O = a.offsets + (size_t)frame * table;
    for (int i = threadIdx.x; i < table; i += 256) s_off[i] = O[i];
    __syncthreads();
    return s_off;
}
__device__ __forceinline__ MeshDisplacement make_displacement(const MeshWarpArgs& a, int frame)
{
    return MeshDisplacement{stage_vertex_table(a, frame), a.sh, a.sw, a.mw, a.mh};
}
// (the unwarp's mesh lies over the OUTPUT canvas: the source canvas of the forward mesh warp being undone)
__device__ __forceinline__ MeshInverseDisplacement make_displacement(const MeshUnwarpArgs& a, int frame)
{
    return MeshInverseDisplacement{MeshDisplacement{stage_vertex_table(a, frame), a.dh, a.dw, a.mw, a.mh}};
}

// One 64 x 8 (TILE_TX = 32) tile of the warp: every pixel through warp_pixel, RGB + mask stored, padded pixels counted.
// Args = WarpArgs is the plain warp, Args = MeshWarpArgs the mesh warp, Args = MeshUnwarpArgs its inverse (the rules are in
// include/vstab.h): the same body with the displacement its arguments ask for.
// The body stays in the kernel: inlined from a device function that receives the
// arguments by reference, the compiler issued the two epilogue stores in another order and the plain warp ran 0.3-1 %
// slower (profiles/r11_one_warp_arithmetic.md).
template <int INTERP, int SUBPIX, bool WITH_MASK, int TILE_TX, class Args>
__global__ __launch_bounds__(256) void warp_kernel(Args a)
{
    __shared__ __attribute__((aligned(16))) float s_cub[32 * 4];
    const float* cub_tab = nullptr;
    if (INTERP == VSTAB_INTERP_BICUBIC) {
        if (threadIdx.x < 32) cubic_coeffs((int)threadIdx.x, s_cub + threadIdx.x * 4);
        __syncthreads();
        cub_tab = s_cub;
    }
    const TileShell<TILE_TX> t(a.tiles_x, a.tiles_y, a.dh, a.dw);
    const int frame = t.frame, x0 = t.x0, y = t.y, npx = t.npx;
    const auto disp = make_displacement(a, frame);
    using Disp = std::remove_const_t<decltype(disp)>;
    const float* __restrict__ S = a.src + (size_t)frame * a.sh * a.sw * 3;

    float acc[TILE_PX][3];
    float cov[TILE_PX];
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) { acc[p][0] = acc[p][1] = acc[p][2] = 0.f; cov[p] = 0.f; }
    unsigned unconv = 0;      // mesh unwarp only: this thread's pixels whose fixed point hit the step limit

    if (t.active) {
        const double dy = (double)y;
        const WarpXform* __restrict__ xf = a.xf + frame;   // one matrix per frame (the S-sample blur is warp_blur_kernel)
        const XformRegs<INTERP, SUBPIX> r(xf);
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (p >= npx) continue;
            const int x = x0 + p * TILE_TX;
            float c = 0.f;
            const Px v = warp_pixel<INTERP, SUBPIX, WITH_MASK>(
                xf, r, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x, y, dy,
                [&](int X, int Y) { return sample_q5<INTERP>(S, a.sh, a.sw, X, Y, a.b0, a.b1, a.b2, cub_tab); },
                [&](float fsx, float fsy) { return sample_exact(S, a.sh, a.sw, fsx, fsy, a.b0, a.b1, a.b2); }, disp, c, &unconv);
            acc[p][0] = v.r; acc[p][1] = v.g; acc[p][2] = v.b;
            if (WITH_MASK) cov[p] = c;
        }
    }

    // ---- epilogue ----
    float mk[TILE_PX];
    unsigned padded[1] = {0};
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) {
        float m = 1.0f - cov[p];
        mk[p] = (m < 1e-3f) ? 0.f : m;
        if (WITH_MASK && p < npx) padded[0] += (mk[p] > 0.5f) ? 1u : 0u;
    }

    if (t.active) {
        // per-frame bases are uniform (scalar registers); inside a frame 32-bit element offsets suffice (the host checks
        // that a frame has fewer than 2^30 pixels), which keeps the address arithmetic out of 64-bit VALU multiplies
        float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
        float* __restrict__ Mk = WITH_MASK ? a.mask + (size_t)frame * a.dh * a.dw : nullptr;
        const unsigned row = (unsigned)y * (unsigned)a.dw;
        typedef float f3 __attribute__((ext_vector_type(3)));
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (p >= npx) continue;
            const unsigned pix = row + (unsigned)(x0 + p * TILE_TX);
            // 12 B per lane, consecutive lanes -> consecutive pixels: every store instruction writes whole lines
            f3 rgb = {acc[p][0], acc[p][1], acc[p][2]};
            __builtin_memcpy(D + pix * 3u, &rgb, 12);
            if (WITH_MASK) Mk[pix] = mk[p];
        }
    }

    if constexpr (Disp::OUTPUT) {
        // two counters through one reduction (the conditions are kernel arguments: uniform)
        if ((WITH_MASK && a.pad_count != nullptr) || a.unconverged != nullptr) {
            unsigned counts[2] = {padded[0], unconv};
            block_count_add<2>(counts, {WITH_MASK ? a.pad_count : nullptr, a.unconverged}, frame);
        }
    } else {
        if (WITH_MASK && a.pad_count != nullptr) block_count_add<1>(padded, {a.pad_count}, frame);
    }
}

template <int SUBPIX, bool WITH_MASK>
constexpr auto mesh_warp_kernel = warp_kernel<VSTAB_INTERP_BILINEAR, SUBPIX, WITH_MASK, 32, MeshWarpArgs>;
template <int SUBPIX, bool WITH_MASK>
constexpr auto mesh_unwarp_kernel = warp_kernel<VSTAB_INTERP_BILINEAR, SUBPIX, WITH_MASK, 32, MeshUnwarpArgs>;

// ---- coverage extent (dynamic zoom; the rule: vstab_cover_extent_batch in include/vstab.h) ------------------------------
// How far the warp's own nearest-neighbour coverage reaches around the canvas centre: the minimum over a frame's uncovered
// pixels of their scaled Chebyshev distance e from the centre.  The coverage bit is warp_pixel's `c`, taken with samplers
// that load nothing: the compiler drops the Q5 / float32 sampling chains, what stays is the fp64 coordinate arithmetic and,
// under a mesh, the LDS vertex lookups.  No image memory is read or written, so the pass is bound by fp64 VALU.
// Args = WarpArgs: the plain warp's coverage; Args = MeshWarpArgs: the mesh warp's (src, dst, mask, pad_count unused).
__global__ void extent_preset_kernel(unsigned* __restrict__ extent, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) extent[i] = 0xFFFFFFFFu;
}

template <int SUBPIX, class Args>
__global__ __launch_bounds__(256) void cover_extent_kernel(Args a, unsigned* __restrict__ extent)
{
    constexpr int TILE_TX = 32;
    __shared__ unsigned s_min[256 / 64];
    const TileShell<TILE_TX> t(a.tiles_x, a.tiles_y, a.dh, a.dw);
    const int frame = t.frame, x0 = t.x0, y = t.y, npx = t.npx;
    const auto disp = make_displacement(a, frame);

    unsigned best = 0xFFFFFFFFu;
    if (t.active) {
        const double dy = (double)y;
        const WarpXform* __restrict__ xf = a.xf + frame;
        const XformRegs<VSTAB_INTERP_BILINEAR, SUBPIX> r(xf);
        // |2y - (dh-1)| * (dw-1) and |2x - (dw-1)| * (dh-1): below 2^31 each (the host checks (dw-1) * (dh-1) < 2^31)
        const unsigned wm = (unsigned)(a.dw - 1), hm = (unsigned)(a.dh - 1);
        const unsigned y2 = 2u * (unsigned)y;
        const unsigned ey = (y2 > hm ? y2 - hm : hm - y2) * wm;
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (p >= npx) continue;
            const int x = x0 + p * TILE_TX;
            float c = 0.f;
            (void)warp_pixel<VSTAB_INTERP_BILINEAR, SUBPIX, true>(
                xf, r, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x, y, dy,
                [](int, int) { return Px{0.f, 0.f, 0.f}; }, [](float, float) { return Px{0.f, 0.f, 0.f}; }, disp, c);
            const unsigned x2 = 2u * (unsigned)x;
            const unsigned ex = (x2 > wm ? x2 - wm : wm - x2) * hm;
            const unsigned e = ex > ey ? ex : ey;
            if (c == 0.f) best = e < best ? e : best;     // mask = 1 - c == 1.0f: uncovered
        }
    }

    // per thread -> wave shuffle -> LDS -> one atomic minimum per workgroup, none if it saw no uncovered pixel
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_down(best, off);
        best = o < best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total = s_min[0];
#pragma unroll
        for (int w = 1; w < 256 / 64; w++) total = s_min[w] < total ? s_min[w] : total;
        if (total != 0xFFFFFFFFu) atomicMin(extent + frame, total);
    }
}

// ---- motion blur: S samples per output pixel (motion_apply.py:137-202) ---------------------------------------------
//
// What bounds the S-sample loop (profiles/r03_blur_kernel.md): a bicubic sample reads 16 taps x 12 B = 192 B per output
// pixel; served by the CU's vector L1 at 64 B per clock that is 3 clocks per pixel-sample -- 12.6 ms for 64 x 1080p x 17
// samples at 2.2 GHz, which is what round 2's kernel took (12.6 ms) and what every rearrangement of its arithmetic took
// too (fewer bounds tests, shared block-origin terms, product table, scalar-base addressing: 12.85-12.88 ms each).  The
// VALU work (176 instructions per pixel-sample, 84 % issue) was only just hidden behind it.  The loop is therefore fed
// from LDS (256 B per clock) instead:
//
//   * A block owns a 64 x TILE_H output tile for ALL samples.  Once per block, the source coordinates of the tile's four
//     corners are evaluated for every sample with the kernel's own arithmetic (4 x S threads).  For affine samples the
//     per-pixel evaluation is monotone in x and in y (a chain of correctly rounded operations, same column-block origin
//     for the whole tile), so the corner values bound every pixel's: their bounding box + the tap footprint is the
//     source window the tile can touch.  If all samples are affine, the window lies inside the source and fits the LDS
//     budget, the block stages it (each texel read from memory once, padded to a float4) and runs the STAGED loop;
//     otherwise (border tiles, perspective samples, very fast motion) it runs the general loop (sample_q5), which is
//     the arithmetic definition.  Both give the oracle's bits (tests/test_warp_gpu.py, tests/test_configs_gpu.py).
//   * The staged loop has no bounds tests, no short saturation (no-ops in the interior) and no coverage arithmetic
//     (all S samples covered: mask = 1 - S/S = 0, the float the general loop produces); the f64 block-origin terms
//     X0, Y0 are formed once per thread and sample, not per pixel; taps are 16-byte LDS reads at a 16-byte lane stride.
//   * bilinear: the four tap weights are formed in registers by the expressions of OpenCV's 32 x 32 product table
//     (initInterTab2D; bilinear_weights above -- round 3 read an LDS copy of the table: 35 % bank conflicts); bicubic keeps
//     the 1-D table in LDS + 16 products per sample: its 64 KB product table would halve the blocks per CU for 16 of ~140
//     instructions.
// The four bilinear tap weights of a 1/32-px fraction pair, formed in registers by the expressions that fill OpenCV's 32 x 32
// table of products (initInterTab2D) -- the same float32 products.  Round 3 read them from a copy of that table in LDS: its
// random 16-B reads were 35 % bank conflicts of a loop that keeps the LDS array 73 % busy; ten VALU instructions instead:
// 16 x 4K x 33 samples 5.87 -> 5.55 ms (profiles/r04_blur_kernel.md).
typedef float blur_f4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ blur_f4_t bilinear_weights(int fx, int fy)
{
    const float wx1 = fx * (1.f / 32), wx0 = 1.f - wx1;
    const float wy1 = fy * (1.f / 32), wy0 = 1.f - wy1;
    return blur_f4_t{wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1};
}

template <int INTERP, int SUBPIX>
struct BlurGeom {
    // the staged loops exist for every sampler; `exact` (the OpenCV >= 4.11 bilinear form: float32 coordinates, lerp
    // arithmetic) runs the border-capable one for all of its staged tiles
    static constexpr bool FAST = true;
    static constexpr bool EXACT = SUBPIX == VSTAB_SUBPIX_EXACT;
    static constexpr bool BICUBIC = INTERP == VSTAB_INTERP_BICUBIC;
    static constexpr int NT = 512;                                    // 64 x 16 output pixels
    static constexpr int FOOT_TEXELS = !FAST ? 0 : (BICUBIC ? 4864 : 2304);   // staged source window (float4 per texel)
    static constexpr int TAPS = BICUBIC ? 4 : 2, LEAD = BICUBIC ? 1 : 0;      // taps per axis, taps left of / above (sx, sy)
    // LDS per block: bicubic 76 KB + 0.5 KB (two blocks per CU), bilinear 36 + 0.5 KB (four)
    static constexpr size_t LDS_BYTES = sizeof(float) * (32 * 4 + (size_t)FOOT_TEXELS * 4);
};

// amdgpu_waves_per_eu(4): at most 128 VGPRs, so that two 512-thread bicubic blocks share a CU.
// `xfs` is a kernel argument of its own (not the WarpArgs member): a `const T* __restrict__` PARAMETER is what lets the
// compiler read the per-sample matrices with scalar loads (s_load into SGPRs) -- through the by-value struct it used
// per-lane vector loads, a full memory round trip at the head of every sample's dependent chain.
template <int INTERP, int SUBPIX, bool WITH_MASK>
__global__ __launch_bounds__((BlurGeom<INTERP, SUBPIX>::NT)) __attribute__((amdgpu_waves_per_eu(4))) void warp_blur_kernel(WarpArgs a, const WarpXform* __restrict__ xfs)
{
    using G = BlurGeom<INTERP, SUBPIX>;
    constexpr int NT = G::NT, TILE_TX = 32, TILE_W = TILE_TX * TILE_PX, TILE_H = NT / TILE_TX;
    typedef float f4_t __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) float s_mem[];   // [1-D cubic table][staged window]
    float* s_cub = s_mem;
    f4_t* s_foot = reinterpret_cast<f4_t*>(s_mem + 32 * 4);
    __shared__ int s_box[4];   // min sx, min sy, max sx, max sy over corners x samples
    const float* cub_tab = nullptr;
    if (INTERP == VSTAB_INTERP_BICUBIC) {
        if (threadIdx.x < 32) cubic_coeffs((int)threadIdx.x, s_cub + threadIdx.x * 4);
        cub_tab = s_cub;
    }
    if (threadIdx.x == 0) { s_box[0] = s_box[1] = 0x7fffffff; s_box[2] = s_box[3] = (int)0x80000000; }
    __syncthreads();

    const TileShell<TILE_TX, NT> t(a.tiles_x, a.tiles_y, a.dh, a.dw);
    const int frame = t.frame, tile_x = t.tile_x, tile_y = t.tile_y, x0 = t.x0, y = t.y, npx = t.npx;
    const bool active = t.active;
    const float* __restrict__ S = a.src + (size_t)frame * a.sh * a.sw * 3;
    const int nxf = a.nxf_per_frame;
    const WarpXform* __restrict__ xf0 = xfs + (size_t)frame * nxf;

    // ---- the source window this tile can touch, over all samples
    bool fast = G::FAST && a.blur_fast != 0;
    bool inside = false;   // the staged window lies inside the source: no tap of the tile meets the border
    bool inside_persp = false;   // ... and some sample of the frame has a perspective row (its own copy of the interior loop)
    int ox = 0, oy = 0, fw = 0;
    if (fast) {
        bool ok = true, any_persp = false;
        int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = (int)0x80000000, by1 = (int)0x80000000;
        if ((int)threadIdx.x < 4 * nxf) {
            const int k = threadIdx.x >> 2, c = threadIdx.x & 3;
            const WarpXform* __restrict__ xf = xf0 + k;
            const int cx_ = (c & 1) ? min(tile_x * TILE_W + TILE_W, a.dw) - 1 : tile_x * TILE_W;
            const int cy_ = (c & 2) ? min(tile_y * TILE_H + TILE_H, a.dh) - 1 : tile_y * TILE_H;
            const int xb = block_origin(cx_, a.dw, a.bw0, a.bw0_pow2);
            const double dxb = (double)xb, dyc = (double)cy_, dx1 = (double)(cx_ - xb);
            const double Xn = (xf->m[0] * dxb + xf->m[1] * dyc + xf->m[2]) + xf->m[0] * dx1;
            const double Yn = (xf->m[3] * dxb + xf->m[4] * dyc + xf->m[5]) + xf->m[3] * dx1;
            // A sample with a perspective row (Flow in perspective mode -> Motion Apply: BASELINE C3) maps the tile onto a
            // convex quadrilateral as long as its denominator W = m6 x + m7 y + m8 keeps one sign over the tile -- W is
            // affine in (x, y), so that is a test of the four corners -- and a convex quadrilateral lies inside the
            // bounding box of its corners.  The kernel's rounded coordinates can leave that box by one 1/32-px unit at
            // most (fp64 evaluation error ~1e-10 of a unit), which the window's one-texel margin absorbs.
            double wq_c = xf->wq;
            bool w_ok = true;
            if (!xf->affine) {
                const double W = (xf->m[6] * dxb + xf->m[7] * dyc + xf->m[8]) + xf->m[6] * dx1;
                const bool pos = W > 0.0;
                w_ok = !G::EXACT && W != 0.0 && W == W && (__shfl_xor((int)pos, 1) == (int)pos) && (__shfl_xor((int)pos, 2) == (int)pos);
                wq_c = 32.0 * ((W != 0.0) ? 1.0 / W : 0.0);
                any_persp = true;
            }
            const double Xq = Xn * wq_c, Yq = Yn * wq_c;
            ok = w_ok && __builtin_fabs(Xq) < 9.0e5 && __builtin_fabs(Yq) < 9.0e5;   // NaN compares false
            if (ok) { bx0 = bx1 = round_small(Xq) >> 5; by0 = by1 = round_small(Yq) >> 5; }
            if (G::EXACT && ok) {
                // the exact sampler's own source position of this corner (float32 chain, monotone in x and in y for an
                // affine sample: every operation is correctly rounded and the divisor is the constant m8)
                float mf[9];
#pragma unroll
                for (int i = 0; i < 9; i++) mf[i] = (float)xf->m[i];
                const float w = cx_ * mf[6] + cy_ * mf[7] + mf[8];
                const float fsx = (cx_ * mf[0] + cy_ * mf[1] + mf[2]) / w, fsy = (cx_ * mf[3] + cy_ * mf[4] + mf[5]) / w;
                ok = __builtin_fabsf(fsx) < 28000.f && __builtin_fabsf(fsy) < 28000.f;
                if (ok) { bx0 = bx1 = (int)__builtin_floorf(fsx); by0 = by1 = (int)__builtin_floorf(fsy); }
                else { bx0 = by0 = 0x7fffffff; bx1 = by1 = (int)0x80000000; }
            }
        }
        // bounding box: butterfly over the wavefront (idle lanes hold the neutral elements), one LDS atomic set per wavefront
        if ((int)(threadIdx.x & ~63u) < 4 * nxf) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                bx0 = min(bx0, __shfl_xor(bx0, off)); by0 = min(by0, __shfl_xor(by0, off));
                bx1 = max(bx1, __shfl_xor(bx1, off)); by1 = max(by1, __shfl_xor(by1, off));
            }
            if ((threadIdx.x & 63) == 0) {
                atomicMin(&s_box[0], bx0); atomicMin(&s_box[1], by0);
                atomicMax(&s_box[2], bx1); atomicMax(&s_box[3], by1);
            }
        }
        fast = __syncthreads_and(ok) != 0;
        const bool persp = __syncthreads_or(any_persp) != 0;   // uniform: some sample of this frame has a perspective row
        if (fast) {
            // taps of (sx, sy): columns sx - LEAD .. sx - LEAD + TAPS - 1; one texel of margin on every side
            ox = s_box[0] - G::LEAD - 1;
            oy = s_box[1] - G::LEAD - 1;
            fw = s_box[2] - s_box[0] + G::TAPS + 2;
            const int fh = s_box[3] - s_box[1] + G::TAPS + 2;
            fast = fw * fh <= G::FOOT_TEXELS;   // uniform
            // (the exact sampler takes the border-capable loop, which carries its coordinate form; a window that lies inside
            // the source serves perspective samples through the interior loop too since round 5: the window bounds every
            // tap of every pixel-sample, so no tap meets the border and the nearest-neighbour coverage pixel -- one of the
            // two bilinear columns / rows around the sample -- lies inside as well)
            inside = !G::EXACT && ox >= 0 && oy >= 0 && ox + fw <= a.sw && oy + fh <= a.sh;
            inside_persp = inside && persp;
            if (fast) {
                // stage the window: one texel (12 contiguous bytes) per lane and step -> whole cache lines per row.  A
                // window that leaves the source (the ring of tiles along the content's edge) is filled with the border
                // colour there: BORDER_CONSTANT replaces a tap outside the source by the border value, tap by tap.
                typedef float f3_t __attribute__((ext_vector_type(3), aligned(4)));
                for (int i = threadIdx.x; i < fw * fh; i += NT) {
                    const int r = i / fw, c = i - r * fw;
                    const int gy = oy + r, gx = ox + c;
                    f4_t e = f4_t{a.b0, a.b1, a.b2, 0.f};
                    if ((unsigned)gx < (unsigned)a.sw && (unsigned)gy < (unsigned)a.sh) {
                        const f3_t v = *reinterpret_cast<const f3_t*>(S + ((unsigned)gy * (unsigned)a.sw + (unsigned)gx) * 3u);
                        e = f4_t{v.x, v.y, v.z, 0.f};
                    }
                    s_foot[i] = e;
                }
            }
            __syncthreads();
        }
    }

    float acc[TILE_PX][3];
    float cov[TILE_PX];
#pragma unroll
    for (int p = 0; p < TILE_PX; p++) { acc[p][0] = acc[p][1] = acc[p][2] = 0.f; cov[p] = 0.f; }

    if (active && fast && !inside) {
        // ---- the STAGED loop for a tile whose window leaves the source: the taps still come from LDS (border-filled),
        // and what the interior loop may leave out is put back per pixel-sample -- the three cases of cv::remap with
        // BORDER_CONSTANT (all taps inside: the plain sums; no tap inside: the border value itself, not a weighted sum of
        // sixteen copies of it; otherwise bilinear: the same sums over the border-filled taps, bicubic: OpenCV's separate
        // formula border + sum over the VALID taps of (tap - border) * weight), and the nearest-neighbour coverage test.
        // Round 3 ran these tiles (the ring along the content's edge: ~10 % of a crop_and_pad clip's tiles) through the
        // general loop, at the L1-bound rate of round 2.
        const int xb = block_origin(x0, a.dw, a.bw0, a.bw0_pow2);
        const double dy = (double)y, dxb = (double)xb;
        double dx1[TILE_PX];
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) dx1[p] = (double)((p < npx ? x0 + p * TILE_TX : x0) - xb);
        for (int k = 0; k < nxf; k++) {
            const WarpXform* __restrict__ xf = xf0 + k;
            const double m0 = xf->m[0], m3 = xf->m[3], m6 = xf->m[6];
            const bool aff = xf->affine != 0;
            const double X0 = m0 * dxb + xf->m[1] * dy + xf->m[2];
            const double Y0 = m3 * dxb + xf->m[4] * dy + xf->m[5];
            const double W0 = m6 * dxb + xf->m[7] * dy + xf->m[8];
            float mf[9];
            if (G::EXACT) {
#pragma unroll
                for (int i = 0; i < 9; i++) mf[i] = (float)xf->m[i];
            }
#pragma unroll
            for (int p = 0; p < TILE_PX; p++) {
                const double Xn = X0 + m0 * dx1[p], Yn = Y0 + m3 * dx1[p];
                double wq = xf->wq, wn = xf->wn;
                if (!aff) {   // the general loop's per-pixel denominator (uniform branch: a property of the sample)
                    const double W = W0 + m6 * dx1[p];
                    wn = (W != 0.0) ? 1.0 / W : 0.0;
                    wq = 32.0 * wn;
                }
                const int X = round_small(Xn * wq), Y = round_small(Yn * wq);
                int sx = X >> 5, sy = Y >> 5;           // |sx|, |sy| < 2^15 (corner test): sat_short is the identity
                const int fx = X & 31, fy = Y & 31;
                float ax = 0.f, ay = 0.f;
                if (G::EXACT) {   // sample_exact's coordinates: float32, no 1/32-px quantisation
                    const int x = p < npx ? x0 + p * TILE_TX : x0;
                    const float w = x * mf[6] + y * mf[7] + mf[8];
                    const float fsx = (x * mf[0] + y * mf[1] + mf[2]) / w, fsy = (x * mf[3] + y * mf[4] + mf[5]) / w;
                    sx = (int)__builtin_floorf(fsx); sy = (int)__builtin_floorf(fsy);
                    ax = fsx - sx; ay = fsy - sy;
                }
                const f4_t* __restrict__ T = s_foot + ((int)__umul24((unsigned)(sy - oy - G::LEAD), (unsigned)fw) + (sx - ox - G::LEAD));
                float vr, vg, vb;
                if (G::EXACT) {
                    const f4_t p00 = T[0], p01 = T[1], p10 = T[fw], p11 = T[fw + 1];
                    const bool none = sx >= a.sw || sx + 1 < 0 || sy >= a.sh || sy + 1 < 0;
                    float v0, v1;
                    v0 = p00.x + ax * (p01.x - p00.x); v1 = p10.x + ax * (p11.x - p10.x); vr = v0 + ay * (v1 - v0);
                    v0 = p00.y + ax * (p01.y - p00.y); v1 = p10.y + ax * (p11.y - p10.y); vg = v0 + ay * (v1 - v0);
                    v0 = p00.z + ax * (p01.z - p00.z); v1 = p10.z + ax * (p11.z - p10.z); vb = v0 + ay * (v1 - v0);
                    if (none) { vr = a.b0; vg = a.b1; vb = a.b2; }
                } else if (INTERP == VSTAB_INTERP_BICUBIC) {
                    const f4_t cxv = reinterpret_cast<const f4_t*>(s_cub)[fx], cyv = reinterpret_cast<const f4_t*>(s_cub)[fy];
                    const float cx[4] = {cxv.x, cxv.y, cxv.z, cxv.w}, cy[4] = {cyv.x, cyv.y, cyv.z, cyv.w};
                    const int bx0 = sx - 1, by0 = sy - 1;
                    const unsigned width1 = (unsigned)(a.sw - 3 > 0 ? a.sw - 3 : 0), height1 = (unsigned)(a.sh - 3 > 0 ? a.sh - 3 : 0);
                    if ((unsigned)bx0 < width1 && (unsigned)by0 < height1) {
                        float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const f4_t t0 = T[i * fw], t1 = T[i * fw + 1], t2 = T[i * fw + 2], t3 = T[i * fw + 3];
                            const float w0 = cy[i] * cx[0], w1 = cy[i] * cx[1], w2 = cy[i] * cx[2], w3 = cy[i] * cx[3];
                            const float tr_ = t0.x * w0 + t1.x * w1 + t2.x * w2 + t3.x * w3;
                            const float tg_ = t0.y * w0 + t1.y * w1 + t2.y * w2 + t3.y * w3;
                            const float tb_ = t0.z * w0 + t1.z * w1 + t2.z * w2 + t3.z * w3;
                            if (i == 0) { sr = tr_; sg = tg_; sb = tb_; }
                            else { sr += tr_; sg += tg_; sb += tb_; }
                        }
                        vr = sr; vg = sg; vb = sb;
                    } else if (bx0 >= a.sw || bx0 + 4 <= 0 || by0 >= a.sh || by0 + 4 <= 0) {
                        vr = a.b0; vg = a.b1; vb = a.b2;
                    } else {
                        float sr = a.b0, sg = a.b1, sb = a.b2;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const int yy = by0 + i;
                            if (yy < 0 || yy >= a.sh) continue;
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                const int xx = bx0 + j;
                                if (xx < 0 || xx >= a.sw) continue;
                                const f4_t v = T[i * fw + j];
                                const float w = cy[i] * cx[j];
                                sr += (v.x - a.b0) * w;
                                sg += (v.y - a.b1) * w;
                                sb += (v.z - a.b2) * w;
                            }
                        }
                        vr = sr; vg = sg; vb = sb;
                    }
                } else {
                    const f4_t t00 = T[0], t01 = T[1], t10 = T[fw], t11 = T[fw + 1];
                    const f4_t w = bilinear_weights(fx, fy);
                    const bool none = sx >= a.sw || sx + 1 < 0 || sy >= a.sh || sy + 1 < 0;
                    vr = t00.x * w.x + t01.x * w.y + t10.x * w.z + t11.x * w.w;
                    vg = t00.y * w.x + t01.y * w.y + t10.y * w.z + t11.y * w.w;
                    vb = t00.z * w.x + t01.z * w.y + t10.z * w.z + t11.z * w.w;
                    if (none) { vr = a.b0; vg = a.b1; vb = a.b2; }
                }
                acc[p][0] += vr; acc[p][1] += vg; acc[p][2] += vb;
                if (WITH_MASK) {
                    const int nx = round_small(Xn * wn), ny = round_small(Yn * wn);
                    cov[p] += ((unsigned)nx < (unsigned)a.sw && (unsigned)ny < (unsigned)a.sh) ? 1.f : 0.f;
                }
                if (INTERP == VSTAB_INTERP_BICUBIC) __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else if (active && fast) {
        // ---- the INTERIOR loop.  Two copies, chosen per block: frames whose samples are all affine keep the loop of rounds
        // 3-4 untouched (it sits at the 128-VGPR limit); a frame with a perspective sample (Flow in perspective mode ->
        // Motion Apply: BASELINE C3) takes the copy that forms the general loop's per-pixel denominator -- 1 / W in fp64 per
        // pixel-sample is the contract, W's tile-uniform part W0 is formed once per thread and sample like X0 / Y0 -- and
        // nothing else of the border-capable loop: no bounds tests, no per-tap validity, no coverage arithmetic
        // (C3's blur warp: see profiles/r05_c3_chain.md).
        const int xb = block_origin(x0, a.dw, a.bw0, a.bw0_pow2);                 // == block_origin(x0 + TILE_TX): blur_fast
        const double dy = (double)y, dxb = (double)xb;
        // a pixel of this thread beyond the right edge (ragged last tile) re-evaluates pixel 0 instead of being skipped:
        // no divergent branch inside the sample loop, its sum is never stored
        double dx1[TILE_PX];
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) dx1[p] = (double)((p < npx ? x0 + p * TILE_TX : x0) - xb);
        const int tap0 = (oy + G::LEAD) * fw + ox + G::LEAD;   // window index of tap (0,0) = (sy * fw + sx) - tap0
        auto interior = [&](auto persp_tag) {
            constexpr bool PERSP = decltype(persp_tag)::value;
            for (int k = 0; k < nxf; k++) {
                const WarpXform* __restrict__ xf = xf0 + k;
                const double m0 = xf->m[0], m3 = xf->m[3];
                const double X0 = m0 * dxb + xf->m[1] * dy + xf->m[2];
                const double Y0 = m3 * dxb + xf->m[4] * dy + xf->m[5];
                const bool aff = !PERSP || xf->affine != 0;            // uniform: a property of the sample
                const double m6 = PERSP ? xf->m[6] : 0.0;
                const double W0 = PERSP ? m6 * dxb + xf->m[7] * dy + xf->m[8] : 0.0;
#pragma unroll
                for (int p = 0; p < TILE_PX; p++) {
                    const double Xn = X0 + m0 * dx1[p], Yn = Y0 + m3 * dx1[p];
                    double wq = xf->wq;
                    if (PERSP && !aff) {
                        const double W = W0 + m6 * dx1[p];
                        wq = 32.0 * ((W != 0.0) ? 1.0 / W : 0.0);
                    }
                    const int X = round_small(Xn * wq), Y = round_small(Yn * wq);
                    const int sx = X >> 5, sy = Y >> 5;
                    const int fx = X & 31, fy = Y & 31;
                    const f4_t* __restrict__ T = s_foot + ((int)__umul24((unsigned)sy, (unsigned)fw) + sx - tap0);
                    if (INTERP == VSTAB_INTERP_BICUBIC) {
                        const f4_t cxv = reinterpret_cast<const f4_t*>(s_cub)[fx], cyv = reinterpret_cast<const f4_t*>(s_cub)[fy];
                        const float cx[4] = {cxv.x, cxv.y, cxv.z, cxv.w}, cy[4] = {cyv.x, cyv.y, cyv.z, cyv.w};
                        float sr = 0.f, sg = 0.f, sb = 0.f;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const f4_t t0 = T[i * fw], t1 = T[i * fw + 1], t2 = T[i * fw + 2], t3 = T[i * fw + 3];
                            const float w0 = cy[i] * cx[0], w1 = cy[i] * cx[1], w2 = cy[i] * cx[2], w3 = cy[i] * cx[3];
                            const float tr_ = t0.x * w0 + t1.x * w1 + t2.x * w2 + t3.x * w3;
                            const float tg_ = t0.y * w0 + t1.y * w1 + t2.y * w2 + t3.y * w3;
                            const float tb_ = t0.z * w0 + t1.z * w1 + t2.z * w2 + t3.z * w3;
                            if (i == 0) { sr = tr_; sg = tg_; sb = tb_; }
                            else { sr += tr_; sg += tg_; sb += tb_; }
                        }
                        acc[p][0] += sr; acc[p][1] += sg; acc[p][2] += sb;
                        __builtin_amdgcn_sched_barrier(0);   // one pixel's 16 taps at a time: both in flight need > 128 VGPRs (spills)
                    } else {
                        const f4_t t00 = T[0], t01 = T[1], t10 = T[fw], t11 = T[fw + 1];
                        const f4_t w = bilinear_weights(fx, fy);
                        acc[p][0] += t00.x * w.x + t01.x * w.y + t10.x * w.z + t11.x * w.w;
                        acc[p][1] += t00.y * w.x + t01.y * w.y + t10.y * w.z + t11.y * w.w;
                        acc[p][2] += t00.z * w.x + t01.z * w.y + t10.z * w.z + t11.z * w.w;
                    }
                }
            }
        };
        if (inside_persp) interior(std::true_type{});
        else interior(std::false_type{});
        if (WITH_MASK) {
#pragma unroll
            for (int p = 0; p < TILE_PX; p++) cov[p] = (float)nxf;   // every sample covered: 1.f added nxf times
        }
    } else if (active) {
        const double dy = (double)y;
        for (int k = 0; k < nxf; k++) {
            const WarpXform* __restrict__ xf = xf0 + k;
            const double m0 = xf->m[0], m1 = xf->m[1], m2 = xf->m[2];
            const double m3 = xf->m[3], m4 = xf->m[4], m5 = xf->m[5];
            const double m6 = xf->m[6], m7 = xf->m[7], m8 = xf->m[8];
            const bool affine = xf->affine != 0;
            float mf[9];
            if (SUBPIX == VSTAB_SUBPIX_EXACT && INTERP == VSTAB_INTERP_BILINEAR) {
#pragma unroll
                for (int i = 0; i < 9; i++) mf[i] = (float)xf->m[i];
            }
#pragma unroll
            for (int p = 0; p < TILE_PX; p++) {
                if (p >= npx) continue;
                const int x = x0 + p * TILE_TX;
                const int xb = block_origin(x, a.dw, a.bw0, a.bw0_pow2);
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
                Px v;
                if (SUBPIX == VSTAB_SUBPIX_EXACT && INTERP == VSTAB_INTERP_BILINEAR) {
                    const float w = x * mf[6] + y * mf[7] + mf[8];
                    const float fsx = (x * mf[0] + y * mf[1] + mf[2]) / w;
                    const float fsy = (x * mf[3] + y * mf[4] + mf[5]) / w;
                    v = sample_exact(S, a.sh, a.sw, fsx, fsy, a.b0, a.b1, a.b2);
                } else {
                    const int X = clamp_round_i32(Xn * Wq);
                    const int Y = clamp_round_i32(Yn * Wq);
                    v = sample_q5<INTERP>(S, a.sh, a.sw, X, Y, a.b0, a.b1, a.b2, cub_tab);
                }
                acc[p][0] += v.r; acc[p][1] += v.g; acc[p][2] += v.b;
                if (WITH_MASK) cov[p] += vstab_nn_covered(Xn * Wn, Yn * Wn, a.sh, a.sw) ? 1.f : 0.f;
            }
        }
    }

    if (active) {
        const float fs = (float)a.samples;   // the reference divides by the sample count even when a 1-frame clip yields one sample
        float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
        float* __restrict__ Mk = WITH_MASK ? a.mask + (size_t)frame * a.dh * a.dw : nullptr;
        const unsigned row = (unsigned)y * (unsigned)a.dw;
        typedef float f3 __attribute__((ext_vector_type(3)));
#pragma unroll
        for (int p = 0; p < TILE_PX; p++) {
            if (p >= npx) continue;
            const unsigned pix = row + (unsigned)(x0 + p * TILE_TX);
            f3 rgb = {acc[p][0] / fs, acc[p][1] / fs, acc[p][2] / fs};
            __builtin_memcpy(D + pix * 3u, &rgb, 12);
            if (WITH_MASK) {
                const float m = 1.0f - cov[p] / fs;
                Mk[pix] = (m < 1e-3f) ? 0.f : m;
            }
        }
    }
}

// Tiles of tx * TILE_PX x nt / tx output pixels over n frames of dw x dh: the tile counts and the launch grid.
int tile_grid(const char* who, int n, int dh, int dw, int tx, int nt, int* tiles_x, int* tiles_y, unsigned* grid)
{
    *tiles_x = (dw + tx * TILE_PX - 1) / (tx * TILE_PX);
    *tiles_y = (dh + nt / tx - 1) / (nt / tx);
    const unsigned long long blocks = (unsigned long long)*tiles_x * *tiles_y * n;
    VSTAB_REQUIRE(blocks > 0 && blocks < 0x7fffffffULL, "%s: grid of %llu blocks is out of range", who, blocks);
    *grid = (unsigned)blocks;
    return 0;
}

template <int INTERP, int SUBPIX>
int launch_blur(WarpArgs a, bool with_mask, hipStream_t st)
{
    using G = BlurGeom<INTERP, SUBPIX>;
    constexpr int TILE_W = 32 * TILE_PX;
    unsigned blocks = 0;
    if (int rc = tile_grid("warp", a.n, a.dh, a.dw, 32, G::NT, &a.tiles_x, &a.tiles_y, &blocks)) return rc;
    // staged-path precondition that does not depend on the block: a thread's two pixels share OpenCV's column block (the
    // u24 multiply of the window index is exact: check_common has sh, sw <= 32767 and the window is at most 4864 texels)
    a.blur_fast = ((a.bw0 >= a.dw) || (a.bw0 % TILE_W == 0)) ? 1 : 0;
    // the prologue (corner classification, staging, two barriers) is amortised over the samples: measured break-even
    // S = 4 for bilinear (S = 3: 2.00 vs 1.86 ms per 64 x 1080p; S = 5: 2.38 vs 2.50), below 3 for bicubic
    if (INTERP == VSTAB_INTERP_BILINEAR && a.nxf_per_frame < 4) a.blur_fast = 0;
    // 0: general loop everywhere (tests toggle it inside one process, so it is read per launch: ~0.1 us against a kernel
    // of milliseconds)
    if (const char* e = getenv("VSTAB_BLUR_FAST")) a.blur_fast = a.blur_fast && atoi(e) != 0;
    // The staged window needs more than the default 64 KB of dynamic LDS for bicubic (76.5 KB): asked for ONCE per kernel
    // instance AND DEVICE (hipFuncSetAttribute applies to the current device's function object, and one process may hold a
    // context per GPU); a device (or runtime) that refuses it gets the general loop everywhere with the small allocation
    // instead of an error -- the staged path is an optimisation, the general loop is the definition.
    constexpr int MAX_DEV = 64;
    static signed char opt_in[2][MAX_DEV] = {};   // [with_mask][device]: 0 not asked yet, 1 granted, -1 refused
    int dev = 0;
    VSTAB_HIP(hipGetDevice(&dev));
    bool big_lds = G::LDS_BYTES <= 64 * 1024;
    if (!big_lds) {
        signed char* slot = (dev >= 0 && dev < MAX_DEV) ? &opt_in[with_mask ? 1 : 0][dev] : nullptr;
        signed char state = slot ? __atomic_load_n(slot, __ATOMIC_RELAXED) : 0;
        if (state == 0) {
            const void* fn = with_mask ? reinterpret_cast<const void*>(warp_blur_kernel<INTERP, SUBPIX, true>)
                                       : reinterpret_cast<const void*>(warp_blur_kernel<INTERP, SUBPIX, false>);
            state = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS_BYTES) == hipSuccess ? 1 : -1;
            if (slot) __atomic_store_n(slot, state, __ATOMIC_RELAXED);
        }
        big_lds = state > 0;
    }
    size_t lds = G::LDS_BYTES;
    if (!big_lds) {
        (void)hipGetLastError();
        a.blur_fast = 0;
        lds = sizeof(float) * 32 * 4;
    }
    if (with_mask) hipLaunchKernelGGL((warp_blur_kernel<INTERP, SUBPIX, true>), dim3(blocks), dim3(G::NT), lds, st, a, a.xf);
    else hipLaunchKernelGGL((warp_blur_kernel<INTERP, SUBPIX, false>), dim3(blocks), dim3(G::NT), lds, st, a, a.xf);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

template <int INTERP, int SUBPIX>
void launch_mask(const WarpArgs& a, bool with_mask, unsigned grid, hipStream_t st, int tx)
{
#define LAUNCH_TX(TX)                                                                                              \
    do {                                                                                                           \
        if (with_mask) hipLaunchKernelGGL((warp_kernel<INTERP, SUBPIX, true, TX, WarpArgs>), dim3(grid), dim3(256), 0, st, a);  \
        else hipLaunchKernelGGL((warp_kernel<INTERP, SUBPIX, false, TX, WarpArgs>), dim3(grid), dim3(256), 0, st, a);  \
    } while (0)
    if (tx == 16) LAUNCH_TX(16);
    else if (tx == 64) LAUNCH_TX(64);
    else if (tx == 8) LAUNCH_TX(8);
    else LAUNCH_TX(32);
#undef LAUNCH_TX
}

int launch_warp(WarpArgs a, int interp, int subpix, bool with_mask, hipStream_t st)
{
    // threads along x of the 256-thread tile: 32 (64 x 8 px) by default; VSTAB_WARP_TX = 8|16|64 for sweeps
    // (profiles/r01_warp_tile_sweep.md)
    int tx = 32;
    if (const char* e = getenv("VSTAB_WARP_TX")) { const int v = atoi(e); if (v == 8 || v == 16 || v == 64) tx = v; }
    unsigned grid = 0;
    if (int rc = tile_grid("warp", a.n, a.dh, a.dw, tx, 256, &a.tiles_x, &a.tiles_y, &grid)) return rc;
    if (interp == VSTAB_INTERP_BICUBIC) launch_mask<VSTAB_INTERP_BICUBIC, VSTAB_SUBPIX_Q5>(a, with_mask, grid, st, tx);
    else if (subpix == VSTAB_SUBPIX_EXACT) launch_mask<VSTAB_INTERP_BILINEAR, VSTAB_SUBPIX_EXACT>(a, with_mask, grid, st, tx);
    else launch_mask<VSTAB_INTERP_BILINEAR, VSTAB_SUBPIX_Q5>(a, with_mask, grid, st, tx);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

int launch_warp_blur(const WarpArgs& a, int interp, int subpix, bool with_mask, hipStream_t st)
{
    if (interp == VSTAB_INTERP_BICUBIC) return launch_blur<VSTAB_INTERP_BICUBIC, VSTAB_SUBPIX_Q5>(a, with_mask, st);
    if (subpix == VSTAB_SUBPIX_EXACT) return launch_blur<VSTAB_INTERP_BILINEAR, VSTAB_SUBPIX_EXACT>(a, with_mask, st);
    return launch_blur<VSTAB_INTERP_BILINEAR, VSTAB_SUBPIX_Q5>(a, with_mask, st);
}

// The limits every entry point of this file puts on frame count and sizes, and on the sub-pixel mode: one definition each, so
// that an entry point "checked as vstab_warp_batch checks it" (the mesh forms, the coverage extent) stays so.
int check_sizes(const char* who, int n, int sh, int sw, int dh, int dw)
{
    VSTAB_REQUIRE(n > 0 && sh > 0 && sw > 0 && dh > 0 && dw > 0, "%s: non-positive size (n=%d src=%dx%d out=%dx%d)", who, n, sw, sh, dw, dh);
    VSTAB_REQUIRE(sh <= 32767 && sw <= 32767, "%s: source larger than 32767 px is not representable in OpenCV's short maps", who);
    VSTAB_REQUIRE((long long)sh * sw < (1LL << 30) && (long long)dh * dw < (1LL << 30), "%s: frames of 2^30 pixels or more are not supported (32-bit in-frame offsets)", who);
    return 0;
}

int check_subpix(const char* who, int subpix)
{
    VSTAB_REQUIRE(subpix == VSTAB_SUBPIX_Q5 || subpix == VSTAB_SUBPIX_EXACT, "%s: unknown subpix mode %d", who, subpix);
    return 0;
}

// A mesh of mw x mh vertices over a domain_w x domain_h canvas (`domain`: which canvas that is, for the message).
int check_mesh(const char* who, int n, int sh, int sw, int dh, int dw, int domain_h, int domain_w, const char* domain, int mw, int mh)
{
    VSTAB_REQUIRE(domain_h >= 2 && domain_w >= 2, "%s: bad size (n=%d src=%dx%d out=%dx%d; the %s must be at least 2x2)", who, n, sw, sh, dw, dh, domain);
    VSTAB_REQUIRE(mw >= 2 && mh >= 2 && mw <= MESH_MAX_VERTS && mh <= MESH_MAX_VERTS, "%s: %dx%d vertices outside 2..%d", who, mw, mh, MESH_MAX_VERTS);
    return 0;
}

int check_common(const char* who, vstab_ctx* ctx, const void* src, int n, int sh, int sw, const void* mats,
                 int dh, int dw, int interp, const float* border, int subpix, const void* dst)
{
    VSTAB_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    VSTAB_REQUIRE(src && mats && border && dst, "%s: NULL pointer argument", who);
    if (int rc = check_sizes(who, n, sh, sw, dh, dw)) return rc;
    VSTAB_REQUIRE(interp == VSTAB_INTERP_BILINEAR || interp == VSTAB_INTERP_BICUBIC, "%s: unknown interpolation %d", who, interp);
    if (int rc = check_subpix(who, subpix)) return rc;
    VSTAB_REQUIRE(!(subpix == VSTAB_SUBPIX_EXACT && interp == VSTAB_INTERP_BICUBIC), "%s: exact sub-pixel mode exists for bilinear only", who);
    return 0;
}

// OpenCV's column block width for a dw x dh output and whether it is a power of two (block_origin's cheap form).
void set_block_width(int dh, int dw, int* bw0, int* bw0_pow2)
{
    *bw0 = vstab_warp_block_width(dh, dw);
    *bw0_pow2 = (*bw0 & (*bw0 - 1)) == 0;
}

// What every warp launch shares: pointers, sizes, OpenCV's column block width, the border colour.
void fill_geometry(WarpArgs& a, const float* src, const WarpXform* xf, int n, int sh, int sw, int dh, int dw, const float* border,
                   float* dst, float* mask, unsigned* pad_count)
{
    a.src = src; a.dst = dst; a.mask = mask; a.pad_count = pad_count; a.xf = xf;
    a.samples = 1; a.nxf_per_frame = 1;
    a.n = n; a.sh = sh; a.sw = sw; a.dh = dh; a.dw = dw;
    set_block_width(dh, dw, &a.bw0, &a.bw0_pow2);
    a.b0 = border[0]; a.b1 = border[1]; a.b2 = border[2];
}

}  // namespace

int vstab_stage_xforms(vstab_ctx* ctx, const float* m32, size_t count, const WarpXform** dev_out)
{
    std::vector<WarpXform> xf(count);
    for (size_t i = 0; i < count; i++) vstab_fill_xform(m32 + i * 9, &xf[i]);
    void* d_xf = nullptr;
    if (vstab_stage_params(ctx, xf.data(), xf.size() * sizeof(WarpXform), &d_xf)) return 1;
    *dev_out = static_cast<const WarpXform*>(d_xf);
    return 0;
}

// ---- the counts' way to the host (see vstab_internal.h) ----
namespace {
__global__ __launch_bounds__(256) void mirror_counts_kernel(const uint32_t* __restrict__ counts, unsigned* host, int n, unsigned* flag, unsigned gen)
{
    for (int i = threadIdx.x; i < n; i += 256) host[i] = counts[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int mirror_counts(vstab_ctx* ctx, const uint32_t* pad_count, int n)
{
    if (ctx->counts.reserve(sizeof(unsigned) * (size_t)(n > 4096 ? n : 4096), ctx->stream)) return 1;
    ctx->counts_gen += 1;
    ctx->counts_n = n;
    hipLaunchKernelGGL(mirror_counts_kernel, dim3(1), dim3(256), 0, ctx->stream, pad_count, ctx->counts.dev<unsigned>(), n,
                       ctx->status.dev<unsigned>() + VSTAB_COUNTS_DONE_WORD, ctx->counts_gen);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
}  // namespace

// The padded-pixel counts of the latest vstab_warp_batch / vstab_warp_batch_planned call that asked for them, on the host:
// waits for that call's kernels only (a word in coherent host memory), nothing is copied by the caller.
extern "C" int vstab_last_pad_counts(vstab_ctx* ctx, int n, uint32_t* out)
{
    VSTAB_REQUIRE(ctx != nullptr && out != nullptr, "vstab_last_pad_counts: NULL argument");
    VSTAB_REQUIRE(ctx->counts.bytes != 0 && n == ctx->counts_n, "vstab_last_pad_counts: no warp with counts over %d frames is pending", n);
    volatile unsigned* done = ctx->status.host<volatile unsigned>() + VSTAB_COUNTS_DONE_WORD;
    const unsigned gen = ctx->counts_gen;
    auto reached = [=] { return *done == gen; };
    // 10 s: a warp of a long 4K clip takes tens of milliseconds; then the runtime's own report
    if (!vstab_spin_until(reached, std::chrono::seconds(10))) {
        VSTAB_HIP(hipStreamSynchronize(ctx->stream));
        VSTAB_REQUIRE(reached(), "vstab_last_pad_counts: the warp finished without reporting its counts");
    }
    memcpy(out, ctx->counts.host<uint32_t>(), sizeof(uint32_t) * (size_t)n);
    return 0;
}

extern "C" int vstab_warp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                                int out_h, int out_w, int interp, const float* border_rgb, int subpix, float* dst,
                                float* mask, uint32_t* pad_count)
{
    if (int rc = check_common("vstab_warp_batch", ctx, src, n, src_h, src_w, matrices, out_h, out_w, interp, border_rgb, subpix, dst)) return rc;
    VSTAB_HIP(hipSetDevice(ctx->device));
    const WarpXform* xf = nullptr;
    if (vstab_stage_xforms(ctx, matrices, (size_t)n, &xf)) return 1;
    WarpArgs a{};
    fill_geometry(a, src, xf, n, src_h, src_w, out_h, out_w, border_rgb, dst, mask, pad_count);
    if (pad_count) VSTAB_HIP(hipMemsetAsync(pad_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    {
        KernelTimer timer(ctx, "warp");
        if (int rc = launch_warp(a, interp, subpix, mask != nullptr, ctx->stream)) return rc;
    }
    return pad_count ? mirror_counts(ctx, pad_count, n) : 0;
}

const WarpXform* vstab_plan_xforms(vstab_ctx* ctx, int first, int n);   // vstab_traj.hip

// vstab_warp_batch for frames [first, first + n) of the clip whose plan vstab_flow_plan_device left on the device: the
// transform table is read where the plan kernel wrote it, nothing crosses the host.
extern "C" int vstab_warp_batch_planned(vstab_ctx* ctx, const float* src, int first, int n, int src_h, int src_w, int out_h,
                                        int out_w, int interp, const float* border_rgb, int subpix, float* dst, float* mask,
                                        uint32_t* pad_count)
{
    if (int rc = check_common("vstab_warp_batch_planned", ctx, src, n, src_h, src_w, border_rgb, out_h, out_w, interp, border_rgb, subpix, dst)) return rc;
    const WarpXform* xf = vstab_plan_xforms(ctx, first, n);
    VSTAB_REQUIRE(xf != nullptr, "vstab_warp_batch_planned: frames [%d, %d) are outside the pending device plan", first, first + n);
    VSTAB_HIP(hipSetDevice(ctx->device));
    WarpArgs a{};
    fill_geometry(a, src, xf, n, src_h, src_w, out_h, out_w, border_rgb, dst, mask, pad_count);
    if (pad_count && pad_count != ctx->plan_zeroed_ptr) VSTAB_HIP(hipMemsetAsync(pad_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    ctx->plan_zeroed_ptr = nullptr;   // (the plan kernel zeroed a registered array once: a second warp into it fills it itself)
    {
        KernelTimer timer(ctx, "warp");
        if (int rc = launch_warp(a, interp, subpix, mask != nullptr, ctx->stream)) return rc;
    }
    return pad_count ? mirror_counts(ctx, pad_count, n) : 0;
}

// motion_apply.py:125-134 (_blurred_matrix_samples) + the f32 cast of motion_apply.py:172, for frames
// [first, first+count) of a clip of `total` matrices.  Host arithmetic only.
extern "C" int vstab_blur_sample_matrices(const double* matrices, int total, int first, int count, const double* ts,
                                          int samples, float* out)
{
    VSTAB_REQUIRE(matrices && ts && out, "vstab_blur_sample_matrices: NULL pointer argument");
    VSTAB_REQUIRE(total >= 1 && first >= 0 && count >= 1 && first + count <= total,
                  "vstab_blur_sample_matrices: frames [%d, %d) outside a clip of %d matrices", first, first + count, total);
    VSTAB_REQUIRE(samples >= 1 && samples <= MAX_BLUR_SAMPLES, "vstab_blur_sample_matrices: samples=%d outside [1,%d]", samples, MAX_BLUR_SAMPLES);
    // a single-frame clip yields one sample matrix per frame (the caller still divides by `samples`)
    const int per_frame = (total <= 1) ? 1 : samples;
    for (int c = 0; c < count; c++) {
        const int i = first + c;
        const double* base = matrices + (size_t)i * 9;
        double delta[9];
        if (total > 1) {
            if (i < total - 1) for (int j = 0; j < 9; j++) delta[j] = matrices[(size_t)(i + 1) * 9 + j] - base[j];
            else for (int j = 0; j < 9; j++) delta[j] = base[j] - matrices[(size_t)(i - 1) * 9 + j];
        }
        for (int k = 0; k < per_frame; k++) {
            float* m32 = out + ((size_t)c * per_frame + k) * 9;
            for (int j = 0; j < 9; j++) m32[j] = (total > 1) ? (float)(base[j] + delta[j] * ts[k]) : (float)base[j];
        }
    }
    return 0;
}

extern "C" int vstab_warp_blur_clip_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w,
                                          const double* clip_matrices, int clip_total, int clip_first, const double* ts,
                                          int samples, int out_h, int out_w, int interp, const float* border_rgb, int subpix,
                                          float* dst, float* mask)
{
    if (int rc = check_common("vstab_warp_blur_clip_batch", ctx, src, n, src_h, src_w, clip_matrices, out_h, out_w, interp, border_rgb, subpix, dst)) return rc;
    VSTAB_REQUIRE(ts != nullptr, "vstab_warp_blur_clip_batch: ts is NULL");
    VSTAB_REQUIRE(samples >= 1 && samples <= MAX_BLUR_SAMPLES, "vstab_warp_blur_clip_batch: samples=%d outside [1,%d]", samples, MAX_BLUR_SAMPLES);
    VSTAB_REQUIRE(clip_first >= 0 && clip_first + n <= clip_total,
                  "vstab_warp_blur_clip_batch: frames [%d, %d) outside a clip of %d matrices", clip_first, clip_first + n, clip_total);
    VSTAB_HIP(hipSetDevice(ctx->device));
    const int per_frame = (clip_total <= 1) ? 1 : samples;
    std::vector<float> m32((size_t)n * per_frame * 9);
    if (int rc = vstab_blur_sample_matrices(clip_matrices, clip_total, clip_first, n, ts, samples, m32.data())) return rc;
    const WarpXform* xf = nullptr;
    if (vstab_stage_xforms(ctx, m32.data(), (size_t)n * per_frame, &xf)) return 1;
    WarpArgs a{};
    fill_geometry(a, src, xf, n, src_h, src_w, out_h, out_w, border_rgb, dst, mask, nullptr);
    a.samples = samples; a.nxf_per_frame = per_frame;
    KernelTimer timer(ctx, "warp_blur");
    return launch_warp_blur(a, interp, subpix, mask != nullptr, ctx->stream);
}

extern "C" int vstab_warp_blur_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w,
                                     const double* matrices, const double* ts, int samples, int out_h, int out_w,
                                     int interp, const float* border_rgb, int subpix, float* dst, float* mask)
{
    return vstab_warp_blur_clip_batch(ctx, src, n, src_h, src_w, matrices, n, 0, ts, samples, out_h, out_w, interp, border_rgb,
                                      subpix, dst, mask);
}

namespace {
// vstab_mesh_warp_batch and vstab_mesh_unwarp_batch: the same checks, staging, grid and LDS; the kernel differs.
// domain_h x domain_w is the canvas the mesh lies over: the source (warp) or the output (unwarp).
int mesh_launch(const char* who, const char* kind, bool inverse, vstab_ctx* ctx, const float* src, int n, int src_h, int src_w,
                const float* matrices, int out_h, int out_w, const float* border_rgb, int subpix, const float* offsets, int mw,
                int mh, float* dst, float* mask, uint32_t* pad_count, uint32_t* unconverged)
{
    if (int rc = check_common(who, ctx, src, n, src_h, src_w, matrices, out_h, out_w, VSTAB_INTERP_BILINEAR, border_rgb, subpix, dst)) return rc;
    VSTAB_REQUIRE(offsets != nullptr, "%s: NULL pointer argument", who);
    const int domain_h = inverse ? out_h : src_h, domain_w = inverse ? out_w : src_w;
    if (int rc = check_mesh(who, n, src_h, src_w, out_h, out_w, domain_h, domain_w, inverse ? "output" : "source", mw, mh)) return rc;
    VSTAB_HIP(hipSetDevice(ctx->device));
    const WarpXform* xf = nullptr;
    if (vstab_stage_xforms(ctx, matrices, (size_t)n, &xf)) return 1;
    MeshUnwarpArgs a{};
    fill_geometry(a, src, xf, n, src_h, src_w, out_h, out_w, border_rgb, dst, mask, pad_count);
    a.offsets = offsets; a.mw = mw; a.mh = mh; a.unconverged = unconverged;
    unsigned blocks = 0;
    if (int rc = tile_grid(who, n, out_h, out_w, 32, 256, &a.tiles_x, &a.tiles_y, &blocks)) return rc;
    if (pad_count) VSTAB_HIP(hipMemsetAsync(pad_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    if (unconverged) VSTAB_HIP(hipMemsetAsync(unconverged, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    const size_t lds = (size_t)mw * mh * 2 * sizeof(float);    // <= 33.8 KB
    const dim3 grid(blocks), block(256);
    KernelTimer timer(ctx, kind);
#define LAUNCH_MESH(KERNEL, ARGS)                                                                                          \
    do {                                                                                                                   \
        if (subpix == VSTAB_SUBPIX_EXACT) {                                                                                \
            if (mask) hipLaunchKernelGGL((KERNEL<VSTAB_SUBPIX_EXACT, true>), grid, block, lds, ctx->stream, ARGS);         \
            else hipLaunchKernelGGL((KERNEL<VSTAB_SUBPIX_EXACT, false>), grid, block, lds, ctx->stream, ARGS);             \
        } else {                                                                                                           \
            if (mask) hipLaunchKernelGGL((KERNEL<VSTAB_SUBPIX_Q5, true>), grid, block, lds, ctx->stream, ARGS);            \
            else hipLaunchKernelGGL((KERNEL<VSTAB_SUBPIX_Q5, false>), grid, block, lds, ctx->stream, ARGS);                \
        }                                                                                                                  \
    } while (0)
    if (inverse) LAUNCH_MESH(mesh_unwarp_kernel, a);
    else LAUNCH_MESH(mesh_warp_kernel, static_cast<const MeshWarpArgs&>(a));
#undef LAUNCH_MESH
    VSTAB_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int vstab_mesh_warp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                                     int out_h, int out_w, const float* border_rgb, int subpix, const float* offsets, int mw, int mh,
                                     float* dst, float* mask, uint32_t* pad_count)
{
    return mesh_launch("vstab_mesh_warp_batch", "mesh_warp", false, ctx, src, n, src_h, src_w, matrices, out_h, out_w, border_rgb,
                       subpix, offsets, mw, mh, dst, mask, pad_count, nullptr);
}

extern "C" int vstab_mesh_unwarp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                                       int out_h, int out_w, const float* border_rgb, int subpix, const float* offsets, int mw, int mh,
                                       float* dst, float* mask, uint32_t* pad_count, uint32_t* unconverged)
{
    return mesh_launch("vstab_mesh_unwarp_batch", "mesh_unwarp", true, ctx, src, n, src_h, src_w, matrices, out_h, out_w, border_rgb,
                       subpix, offsets, mw, mh, dst, mask, pad_count, unconverged);
}

extern "C" int vstab_cover_extent_batch(vstab_ctx* ctx, const float* matrices, int n, int src_h, int src_w, int out_h, int out_w,
                                        int subpix, const float* offsets, int mw, int mh, uint32_t* extent)
{
    const char* who = "vstab_cover_extent_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    VSTAB_REQUIRE(matrices != nullptr && extent != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(out_w >= 2 && out_h >= 2, "%s: a %dx%d canvas has no centred extent (both sides must be at least 2 px)", who, out_w, out_h);
    VSTAB_REQUIRE((long long)(out_w - 1) * (out_h - 1) < (1LL << 31), "%s: (out_w-1)*(out_h-1) of a %dx%d canvas does not fit the 32-bit extent", who, out_w, out_h);
    // the rest as vstab_warp_batch / vstab_mesh_warp_batch check it: the same routines
    if (int rc = check_sizes(who, n, src_h, src_w, out_h, out_w)) return rc;
    if (int rc = check_subpix(who, subpix)) return rc;
    VSTAB_REQUIRE(((uintptr_t)extent & 3) == 0, "%s: extent is not aligned to its element size", who);
    if (offsets != nullptr) {
        if (int rc = check_mesh(who, n, src_h, src_w, out_h, out_w, src_h, src_w, "source", mw, mh)) return rc;
    }
    VSTAB_HIP(hipSetDevice(ctx->device));
    const WarpXform* xf = nullptr;
    if (vstab_stage_xforms(ctx, matrices, (size_t)n, &xf)) return 1;
    const float no_border[3] = {0.f, 0.f, 0.f};
    MeshWarpArgs a{};
    fill_geometry(a, nullptr, xf, n, src_h, src_w, out_h, out_w, no_border, nullptr, nullptr, nullptr);
    a.offsets = offsets; a.mw = mw; a.mh = mh;
    unsigned blocks = 0;
    if (int rc = tile_grid(who, n, out_h, out_w, 32, 256, &a.tiles_x, &a.tiles_y, &blocks)) return rc;
    const dim3 grid(blocks), block(256);
    KernelTimer timer(ctx, "cover_extent");
    hipLaunchKernelGGL(extent_preset_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, extent, n);
    if (offsets != nullptr) {
        const size_t lds = (size_t)mw * mh * 2 * sizeof(float);    // <= 33.8 KB
        if (subpix == VSTAB_SUBPIX_EXACT) hipLaunchKernelGGL((cover_extent_kernel<VSTAB_SUBPIX_EXACT, MeshWarpArgs>), grid, block, lds, ctx->stream, a, extent);
        else hipLaunchKernelGGL((cover_extent_kernel<VSTAB_SUBPIX_Q5, MeshWarpArgs>), grid, block, lds, ctx->stream, a, extent);
    } else {
        const WarpArgs& plain = a;
        if (subpix == VSTAB_SUBPIX_EXACT) hipLaunchKernelGGL((cover_extent_kernel<VSTAB_SUBPIX_EXACT, WarpArgs>), grid, block, 0, ctx->stream, plain, extent);
        else hipLaunchKernelGGL((cover_extent_kernel<VSTAB_SUBPIX_Q5, WarpArgs>), grid, block, 0, ctx->stream, plain, extent);
    }
    VSTAB_HIP(hipGetLastError());
    return 0;
}

// ---- temporal fill: padding pixels taken from neighbouring frames ----------------------------------------------------
//
// After a warp, an output pixel whose mask is 1 saw no source content in its own frame.  For each such pixel the kernel
// walks up to K candidate (frame, matrix) pairs in order and takes the first one whose source position -- warp_pixel's,
// the plain warp's own arithmetic -- has EVERY interpolation tap inside that frame: the value written is then the one
// vstab_warp_batch would have written for that frame and matrix, and no border colour can enter it.
//
// Shape: the warp's 64 x 8 tile and XCD remap.  A tile reads its mask (4 B per pixel); if none of its pixels is padded the
// block returns -- the common case, so the pass over a mostly covered clip is close to a plain read of the mask.  The
// candidate records are block-uniform (a `const T* __restrict__` kernel parameter: scalar loads).  A wavefront leaves the
// candidate loop as soon as none of its pixels is waiting.  Only filled pixels are stored.  dst is read by nobody
// (candidates sample src), so working in place is free of races.
namespace {

struct FillCand {
    WarpXform xf;
    int frame;     // clip frame the candidate samples, -1: none (out of the clip, cut chain, singular matrix)
    int pad_;
};

struct FillArgs {
    const float* src;
    float* dst;
    float* mask;
    signed char* filled_from;
    unsigned* fill_count;
    unsigned* pad_count;
    int n, K, sh, sw, dh, dw;
    int bw0, bw0_pow2;
    int tiles_x, tiles_y;
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

    const float* cub_tab = nullptr;
    if (INTERP == VSTAB_INTERP_BICUBIC) {
        if (threadIdx.x < 32) cubic_coeffs((int)threadIdx.x, s_cub + threadIdx.x * 4);
        __syncthreads();
        cub_tab = s_cub;
    }

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
            float c_unused = 0.f;
            // validity = the samplers' own "all taps inside" branches (sample_q5's interior tests, sample_exact's four
            // in-range flags): the sample is taken only then, so the border arguments are never read
            const Px v = warp_pixel<INTERP, SUBPIX, false>(
                xf, r, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x, y, dy,
                [&](int X, int Y) {
                    const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
                    if (INTERP == VSTAB_INTERP_BILINEAR) {
                        valid = (unsigned)sx < (unsigned)(a.sw - 1) && (unsigned)sy < (unsigned)(a.sh - 1);
                    } else {
                        const unsigned width1 = (unsigned)(a.sw - 3 > 0 ? a.sw - 3 : 0);
                        const unsigned height1 = (unsigned)(a.sh - 3 > 0 ? a.sh - 3 : 0);
                        valid = (unsigned)(sx - 1) < width1 && (unsigned)(sy - 1) < height1;
                    }
                    return valid ? sample_q5<INTERP>(S, a.sh, a.sw, X, Y, 0.f, 0.f, 0.f, cub_tab) : Px{0.f, 0.f, 0.f};
                },
                [&](float fsx, float fsy) {
                    const float flx = __builtin_floorf(fsx), fly = __builtin_floorf(fsy);   // NaN / inf compare false
                    valid = flx >= 0.f && flx < (float)(a.sw - 1) && fly >= 0.f && fly < (float)(a.sh - 1);
                    return valid ? sample_exact(S, a.sh, a.sw, fsx, fsy, 0.f, 0.f, 0.f) : Px{0.f, 0.f, 0.f};
                },
                NoDisplacement{}, c_unused);
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

// ---- blended temporal fill: exposure-matched candidates, feathered seam (include/vstab.h states both rules) -------------
//
// Two kernels beside temporal_fill_kernel, which stays as it is (its instances, its FillCand records, its cost):
//   fill_gain_sums_kernel       integer sums of own and candidate values over the lattice x % 8 == 4 && y % 8 == 4 where
//                               both see source content by the interior rule; the host turns them into one gain per
//                               (frame, candidate, channel).  A workgroup = 256 lattice pixels of one (frame, candidate) pair, so
//                               both records are block-uniform (scalar loads); per-thread values -> wave shuffle -> LDS -> one
//                               64-bit atomic per sum, skipped where the workgroup counted nothing.  Nothing waits for
//                               another workgroup, and integer sums do not depend on the order of the atomics.
//   temporal_fill_blend_kernel  the fill's tile, shell and candidate walk, with (a) the sample scaled by the candidate's gain
//                               and (b) the own pixels within feather_px of the frame's tap-interior border cross-faded
//                               towards the first valid candidate.  Whether an own pixel takes part costs its mask and its
//                               own coordinate (warp_pixel with a sampler that only records X, Y: ALU, no loads); a tile
//                               without padded or feathered pixels returns before anything else is read or stored.

// All taps of the Q5 coordinate (X, Y) inside an sw x sh frame: the interior tests of sample_q5, as temporal_fill_kernel
// states them in its sampler.
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
__device__ __forceinline__ void fill_coordinate(const WarpXform* __restrict__ xf, const XformRegs<INTERP, VSTAB_SUBPIX_Q5>& r, int sh,
                                                int sw, int dw, int bw0, int bw0_pow2, int x, int y, double dy, int& X, int& Y)
{
    float c_unused = 0.f;
    int ox = 0, oy = 0;
    (void)warp_pixel<INTERP, VSTAB_SUBPIX_Q5, false>(
        xf, r, sh, sw, dw, bw0, bw0_pow2, x, y, dy, [&](int qx, int qy) { ox = qx; oy = qy; return Px{0.f, 0.f, 0.f}; },
        [&](float, float) { return Px{0.f, 0.f, 0.f}; }, NoDisplacement{}, c_unused);
    X = ox; Y = oy;
}

// The fill's sample of one candidate at (x, y), taken only where every tap is inside (`valid`).
template <int INTERP>
__device__ __forceinline__ Px fill_candidate_sample(const float* __restrict__ S, const WarpXform* __restrict__ xf,
                                                    const XformRegs<INTERP, VSTAB_SUBPIX_Q5>& r, int sh, int sw, int dw, int bw0,
                                                    int bw0_pow2, int x, int y, double dy, const float* cub_tab, bool& valid)
{
    float c_unused = 0.f;
    bool ok = false;
    const Px v = warp_pixel<INTERP, VSTAB_SUBPIX_Q5, false>(
        xf, r, sh, sw, dw, bw0, bw0_pow2, x, y, dy,
        [&](int X, int Y) {
            ok = fill_taps_inside<INTERP>(sh, sw, X, Y);
            return ok ? sample_q5<INTERP>(S, sh, sw, X, Y, 0.f, 0.f, 0.f, cub_tab) : Px{0.f, 0.f, 0.f};
        },
        [&](float, float) { return Px{0.f, 0.f, 0.f}; }, NoDisplacement{}, c_unused);
    valid = ok;
    return v;
}

// q of the gain sums: a value in 16 fractional bits, truncated; below 0 and NaN give 0, 1 and above give 65536.
__device__ __forceinline__ unsigned gain_q(float v)
{
    return v > 0.f ? (v < 1.f ? (unsigned)(v * 65536.0f) : 65536u) : 0u;
}

struct GainArgs {
    const float* src;
    const float* dst;
    unsigned long long* sums;   // [n, K, 7]
    int K, sh, sw, dh, dw;
    int bw0, bw0_pow2;
    int lw;                     // lattice columns: x = 8 * lx + 4 < dw
    unsigned lattice;           // lattice pixels per frame
    unsigned blocks_per_pair;   // workgroups per (frame, candidate) pair
};

template <int INTERP>
__global__ __launch_bounds__(256) void fill_gain_sums_kernel(GainArgs a, const FillCand* __restrict__ cands, const FillCand* __restrict__ own)
{
    constexpr int NS = 7, WAVES = 4;
    __shared__ __attribute__((aligned(16))) float s_cub[32 * 4];
    __shared__ unsigned s_sum[NS][WAVES];
    const unsigned pair = blockIdx.x / a.blocks_per_pair;          // frame * K + k
    const unsigned chunk = blockIdx.x - pair * a.blocks_per_pair;
    const unsigned frame = pair / (unsigned)a.K;
    const FillCand* __restrict__ cd = cands + pair;
    const FillCand* __restrict__ ow = own + frame;
    if (ow->frame < 0 || cd->frame < 0) return;                    // block-uniform: this pair counts nothing

    const float* cub_tab = nullptr;
    if (INTERP == VSTAB_INTERP_BICUBIC) {
        if (threadIdx.x < 32) cubic_coeffs((int)threadIdx.x, s_cub + threadIdx.x * 4);
        __syncthreads();
        cub_tab = s_cub;
    }

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
            fill_coordinate<INTERP>(xo, ro, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x, y, dy, X, Y);
        }
        if (fill_taps_inside<INTERP>(a.sh, a.sw, X, Y)) {
            const float* __restrict__ S = a.src + (size_t)cd->frame * ((size_t)a.sh * a.sw * 3);
            const WarpXform* __restrict__ xf = &cd->xf;
            const XformRegs<INTERP, VSTAB_SUBPIX_Q5> r(xf);
            bool valid = false;
            const Px s = fill_candidate_sample<INTERP>(S, xf, r, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x, y, dy, cub_tab, valid);
            if (valid) {
                const float* __restrict__ D = a.dst + (size_t)frame * a.dh * a.dw * 3;
                const Px o = load_px(D + ((unsigned)y * (unsigned)a.dw + (unsigned)x) * 3u);
                v[0] = 1u;
                v[1] = gain_q(o.r); v[2] = gain_q(o.g); v[3] = gain_q(o.b);
                v[4] = gain_q(s.r); v[5] = gain_q(s.g); v[6] = gain_q(s.b);
            }
        }
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < NS; c++) v[c] += __shfl_down(v[c], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NS; c++) s_sum[c][threadIdx.x >> 6] = v[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned total[NS];
#pragma unroll
        for (int c = 0; c < NS; c++) total[c] = s_sum[c][0] + s_sum[c][1] + s_sum[c][2] + s_sum[c][3];
        if (total[0] != 0u) {       // nothing counted: every sum is zero, no atomic
            unsigned long long* out = a.sums + (size_t)pair * NS;
#pragma unroll
            for (int c = 0; c < NS; c++) atomicAdd(out + c, (unsigned long long)total[c]);
        }
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
                fill_coordinate<INTERP>(xo, ro, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x, y, dy, X, Y);
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

    const float* cub_tab = nullptr;
    if (INTERP == VSTAB_INTERP_BICUBIC) {
        if (threadIdx.x < 32) cubic_coeffs((int)threadIdx.x, s_cub + threadIdx.x * 4);
        __syncthreads();
        cub_tab = s_cub;
    }

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
            const Px s = fill_candidate_sample<INTERP>(S, xf, r, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x, y, dy, cub_tab, valid);
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

}  // namespace

extern "C" int vstab_temporal_fill_batch(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first,
                                         int n, const float* matrices, const int32_t* cand_frame, int K, int out_h, int out_w,
                                         int interp, int subpix, float* dst, float* mask, int8_t* filled_from,
                                         uint32_t* fill_count, uint32_t* pad_count)
{
    const char* who = "vstab_temporal_fill_batch";
    const float no_border[3] = {0.f, 0.f, 0.f};
    if (int rc = check_common(who, ctx, src, n, src_h, src_w, matrices, out_h, out_w, interp, no_border, subpix, dst)) return rc;
    VSTAB_REQUIRE(mask != nullptr && cand_frame != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(K >= 1 && K <= 64, "%s: K=%d outside [1,64]", who, K);
    VSTAB_REQUIRE(clip_frames > 0 && first >= 0 && first + n <= clip_frames, "%s: frames [%d, %d) outside a clip of %d frames", who,
                  first, first + n, clip_frames);
    VSTAB_REQUIRE((const void*)src != (const void*)dst, "%s: dst must not alias src (candidates read src while dst is written)", who);
    std::vector<FillCand> cd((size_t)n * K);
    if (int rc = fill_cand_records(who, matrices, cand_frame, cd.size(), clip_frames, cd.data())) return rc;
    VSTAB_HIP(hipSetDevice(ctx->device));
    void* d_cd = nullptr;
    if (vstab_stage_params(ctx, cd.data(), cd.size() * sizeof(FillCand), &d_cd)) return 1;

    FillArgs a{};
    a.src = src; a.dst = dst; a.mask = mask; a.filled_from = reinterpret_cast<signed char*>(filled_from);
    a.fill_count = fill_count; a.pad_count = pad_count;
    a.n = n; a.K = K; a.sh = src_h; a.sw = src_w; a.dh = out_h; a.dw = out_w;
    set_block_width(out_h, out_w, &a.bw0, &a.bw0_pow2);
    unsigned blocks = 0;
    if (int rc = tile_grid(who, n, out_h, out_w, 32, 256, &a.tiles_x, &a.tiles_y, &blocks)) return rc;
    const size_t px = (size_t)n * out_h * out_w;
    if (filled_from) VSTAB_HIP(hipMemsetAsync(filled_from, 0xff, px, ctx->stream));   // -1: not filled
    if (fill_count) VSTAB_HIP(hipMemsetAsync(fill_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    if (pad_count) VSTAB_HIP(hipMemsetAsync(pad_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    const FillCand* cands = static_cast<const FillCand*>(d_cd);
    KernelTimer timer(ctx, "fill");
    const dim3 grid(blocks), block(256);
    if (interp == VSTAB_INTERP_BICUBIC) hipLaunchKernelGGL((temporal_fill_kernel<VSTAB_INTERP_BICUBIC, VSTAB_SUBPIX_Q5>), grid, block, 0, ctx->stream, a, cands);
    else if (subpix == VSTAB_SUBPIX_EXACT) hipLaunchKernelGGL((temporal_fill_kernel<VSTAB_INTERP_BILINEAR, VSTAB_SUBPIX_EXACT>), grid, block, 0, ctx->stream, a, cands);
    else hipLaunchKernelGGL((temporal_fill_kernel<VSTAB_INTERP_BILINEAR, VSTAB_SUBPIX_Q5>), grid, block, 0, ctx->stream, a, cands);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

namespace {
// What the two blended entries share with vstab_temporal_fill_batch: its checks, plus Q5 and the own matrices.
int check_fill_blend(const char* who, vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                     const float* matrices, const int32_t* cand_frame, int K, const float* own_matrices, int out_h, int out_w,
                     int interp, int subpix, const float* dst)
{
    const float no_border[3] = {0.f, 0.f, 0.f};
    if (int rc = check_common(who, ctx, src, n, src_h, src_w, matrices, out_h, out_w, interp, no_border, subpix, dst)) return rc;
    VSTAB_REQUIRE(subpix == VSTAB_SUBPIX_Q5, "%s: VSTAB_SUBPIX_EXACT is not supported (the feather distance and the gain lattice "
                  "are stated on the 1/32-px coordinates of VSTAB_SUBPIX_Q5)", who);
    VSTAB_REQUIRE(cand_frame != nullptr && own_matrices != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(K >= 1 && K <= 64, "%s: K=%d outside [1,64]", who, K);
    VSTAB_REQUIRE(clip_frames > 0 && first >= 0 && first + n <= clip_frames, "%s: frames [%d, %d) outside a clip of %d frames", who,
                  first, first + n, clip_frames);
    VSTAB_REQUIRE((const void*)src != (const void*)dst, "%s: dst must not alias src (candidates read src while dst is written)", who);
    return 0;
}

// Candidate records [n * K] followed by the own records [n], staged as one block.
int stage_fill_blend_records(const char* who, vstab_ctx* ctx, const float* matrices, const int32_t* cand_frame, int n, int K,
                             int clip_frames, const float* own_matrices, const float* gains, const FillCand** cands,
                             const FillCand** own, const float** gains_dev)
{
    const size_t pairs = (size_t)n * K;
    const size_t rec_bytes = (pairs + (size_t)n) * sizeof(FillCand);
    std::vector<unsigned char> blob(rec_bytes + (gains ? pairs * 3 * sizeof(float) : 0));
    FillCand* cd = reinterpret_cast<FillCand*>(blob.data());
    if (int rc = fill_cand_records(who, matrices, cand_frame, pairs, clip_frames, cd)) return rc;
    if (int rc = fill_cand_records(who, own_matrices, nullptr, (size_t)n, clip_frames, cd + pairs)) return rc;
    if (gains) memcpy(blob.data() + rec_bytes, gains, pairs * 3 * sizeof(float));
    void* dev = nullptr;
    if (vstab_stage_params(ctx, blob.data(), blob.size(), &dev)) return 1;
    *cands = static_cast<const FillCand*>(dev);
    *own = *cands + pairs;
    if (gains_dev) *gains_dev = reinterpret_cast<const float*>(static_cast<const unsigned char*>(dev) + rec_bytes);
    return 0;
}
}  // namespace

extern "C" int vstab_fill_gain_sums(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                                    const float* matrices, const int32_t* cand_frame, int K, const float* own_matrices, int out_h,
                                    int out_w, int interp, int subpix, const float* dst, uint64_t* sums)
{
    const char* who = "vstab_fill_gain_sums";
    if (int rc = check_fill_blend(who, ctx, src, clip_frames, src_h, src_w, first, n, matrices, cand_frame, K, own_matrices, out_h,
                                  out_w, interp, subpix, dst)) return rc;
    VSTAB_REQUIRE(sums != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(((uintptr_t)sums & 7) == 0, "%s: sums is not aligned to its element size", who);
    GainArgs a{};
    a.src = src; a.dst = dst; a.sums = reinterpret_cast<unsigned long long*>(sums);
    a.K = K; a.sh = src_h; a.sw = src_w; a.dh = out_h; a.dw = out_w;
    set_block_width(out_h, out_w, &a.bw0, &a.bw0_pow2);
    constexpr int STRIDE = VSTAB_FILL_GAIN_STRIDE, REST = STRIDE - STRIDE / 2 - 1;
    a.lw = (out_w + REST) / STRIDE;                                    // x = STRIDE * lx + STRIDE / 2 < out_w
    a.lattice = (unsigned)a.lw * (unsigned)((out_h + REST) / STRIDE);
    a.blocks_per_pair = (a.lattice + 255u) / 256u;
    const unsigned long long blocks = (unsigned long long)a.blocks_per_pair * (unsigned long long)n * (unsigned long long)K;
    VSTAB_REQUIRE(blocks < 0x7fffffffULL, "%s: grid of %llu blocks is out of range", who, blocks);
    VSTAB_HIP(hipSetDevice(ctx->device));
    const FillCand *cands = nullptr, *own = nullptr;
    if (int rc = stage_fill_blend_records(who, ctx, matrices, cand_frame, n, K, clip_frames, own_matrices, nullptr, &cands, &own, nullptr)) return rc;
    KernelTimer timer(ctx, "fill_gain");
    VSTAB_HIP(hipMemsetAsync(sums, 0, sizeof(uint64_t) * 7 * (size_t)n * K, ctx->stream));
    if (blocks == 0) return 0;                                         // a canvas without a lattice pixel: every sum is zero
    const dim3 grid((unsigned)blocks), block(256);
    if (interp == VSTAB_INTERP_BICUBIC) hipLaunchKernelGGL((fill_gain_sums_kernel<VSTAB_INTERP_BICUBIC>), grid, block, 0, ctx->stream, a, cands, own);
    else hipLaunchKernelGGL((fill_gain_sums_kernel<VSTAB_INTERP_BILINEAR>), grid, block, 0, ctx->stream, a, cands, own);
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
    if (int rc = check_fill_blend(who, ctx, src, clip_frames, src_h, src_w, first, n, matrices, cand_frame, K, own_matrices, out_h,
                                  out_w, interp, subpix, dst)) return rc;
    VSTAB_REQUIRE(mask != nullptr && gains != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(feather_px >= 0 && feather_px <= VSTAB_FILL_FEATHER_MAX, "%s: feather_px=%d outside [0,%d]", who, feather_px,
                  VSTAB_FILL_FEATHER_MAX);
    VSTAB_HIP(hipSetDevice(ctx->device));
    const FillCand *cands = nullptr, *own = nullptr;
    const float* gains_dev = nullptr;
    if (int rc = stage_fill_blend_records(who, ctx, matrices, cand_frame, n, K, clip_frames, own_matrices, gains, &cands, &own, &gains_dev)) return rc;

    BlendArgs a{};
    a.src = src; a.dst = dst; a.mask = mask; a.filled_from = reinterpret_cast<signed char*>(filled_from);
    a.fill_count = fill_count; a.pad_count = pad_count; a.blend_count = blend_count;
    a.n = n; a.K = K; a.sh = src_h; a.sw = src_w; a.dh = out_h; a.dw = out_w;
    a.Fe = 32 * feather_px;
    const int inset = interp == VSTAB_INTERP_BICUBIC ? 1 : 0;          // bicubic: X - 32 and 32 (sw - 2) - X
    a.lo = 32 * inset; a.hi_x = 32 * (src_w - 1 - inset); a.hi_y = 32 * (src_h - 1 - inset);
    set_block_width(out_h, out_w, &a.bw0, &a.bw0_pow2);
    unsigned blocks = 0;
    if (int rc = tile_grid(who, n, out_h, out_w, 32, 256, &a.tiles_x, &a.tiles_y, &blocks)) return rc;
    const size_t px = (size_t)n * out_h * out_w;
    if (filled_from) VSTAB_HIP(hipMemsetAsync(filled_from, 0xff, px, ctx->stream));   // -1: neither filled nor blended
    if (fill_count) VSTAB_HIP(hipMemsetAsync(fill_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    if (pad_count) VSTAB_HIP(hipMemsetAsync(pad_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    if (blend_count) VSTAB_HIP(hipMemsetAsync(blend_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    KernelTimer timer(ctx, "fill_blend");
    const dim3 grid(blocks), block(256);
    if (interp == VSTAB_INTERP_BICUBIC) hipLaunchKernelGGL((temporal_fill_blend_kernel<VSTAB_INTERP_BICUBIC>), grid, block, 0, ctx->stream, a, cands, own, gains_dev);
    else hipLaunchKernelGGL((temporal_fill_blend_kernel<VSTAB_INTERP_BILINEAR>), grid, block, 0, ctx->stream, a, cands, own, gains_dev);
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

struct SharpArgs {
    const float* src;
    float* dst;
    const float* mask;          // nullptr: every pixel is own
    unsigned* transfer_count;
    float alpha;
    int K, sh, sw, dh, dw;
    int bw0, bw0_pow2;
    int tiles_x, tiles_y;
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

    const float* cub_tab = nullptr;
    if (INTERP == VSTAB_INTERP_BICUBIC) {
        if (threadIdx.x < 32) cubic_coeffs((int)threadIdx.x, s_cub + threadIdx.x * 4);
        __syncthreads();
        cub_tab = s_cub;
    }

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
            const Px s = fill_candidate_sample<INTERP>(S, xf, r, a.sh, a.sw, a.dw, a.bw0, a.bw0_pow2, x0 + p * TILE_TX, y, dy, cub_tab, valid);
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
    const float no_border[3] = {0.f, 0.f, 0.f};
    if (int rc = check_common(who, ctx, src, n, src_h, src_w, matrices, out_h, out_w, interp, no_border, subpix, dst)) return rc;
    VSTAB_REQUIRE(subpix == VSTAB_SUBPIX_Q5, "%s: VSTAB_SUBPIX_EXACT is not supported (the transfer samples as the blended fill "
                  "does, on the 1/32-px coordinates of VSTAB_SUBPIX_Q5)", who);
    VSTAB_REQUIRE(cand_frame != nullptr && ratio != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(K >= 1 && K <= 64, "%s: K=%d outside [1,64]", who, K);
    VSTAB_REQUIRE(clip_frames > 0 && first >= 0 && first + n <= clip_frames, "%s: frames [%d, %d) outside a clip of %d frames", who,
                  first, first + n, clip_frames);
    VSTAB_REQUIRE((const void*)src != (const void*)dst, "%s: dst must not alias src (candidates read src while dst is written)", who);
    VSTAB_REQUIRE(alpha >= 0.f && std::isfinite(alpha), "%s: alpha=%g is not a finite number >= 0", who, (double)alpha);
    const size_t pairs = (size_t)n * K;
    for (size_t i = 0; i < pairs; i++)
        VSTAB_REQUIRE(ratio[i] >= 0.f && std::isfinite(ratio[i]), "%s: ratio[%zu]=%g is not a finite number >= 0", who, i, (double)ratio[i]);

    // one staged block: candidate records [n * K], ratios [n * K], the list of live frames [n_live]
    const size_t rec_bytes = pairs * sizeof(FillCand), ratio_bytes = pairs * sizeof(float);
    std::vector<unsigned char> blob(rec_bytes + ratio_bytes + (size_t)n * sizeof(int));
    FillCand* cd = reinterpret_cast<FillCand*>(blob.data());
    if (int rc = fill_cand_records(who, matrices, cand_frame, pairs, clip_frames, cd)) return rc;
    memcpy(blob.data() + rec_bytes, ratio, ratio_bytes);
    int* live = reinterpret_cast<int*>(blob.data() + rec_bytes + ratio_bytes);
    int n_live = 0;
    for (int f = 0; f < n; f++) {
        bool any = false;
        for (int k = 0; k < K && !any; k++) any = cd[(size_t)f * K + k].frame >= 0 && ratio[(size_t)f * K + k] > 0.f;
        if (any) live[n_live++] = f;
    }

    VSTAB_HIP(hipSetDevice(ctx->device));
    KernelTimer timer(ctx, "sharp_transfer");
    if (transfer_count) VSTAB_HIP(hipMemsetAsync(transfer_count, 0, sizeof(uint32_t) * (size_t)n, ctx->stream));
    if (n_live == 0) return 0;                                     // no frame borrows anything: dst keeps every byte
    SharpArgs a{};
    a.src = src; a.dst = dst; a.mask = mask; a.transfer_count = transfer_count; a.alpha = alpha;
    a.K = K; a.sh = src_h; a.sw = src_w; a.dh = out_h; a.dw = out_w;
    set_block_width(out_h, out_w, &a.bw0, &a.bw0_pow2);
    unsigned blocks = 0;
    if (int rc = tile_grid(who, n_live, out_h, out_w, 32, 256, &a.tiles_x, &a.tiles_y, &blocks)) return rc;
    void* dev = nullptr;
    if (vstab_stage_params(ctx, blob.data(), rec_bytes + ratio_bytes + (size_t)n_live * sizeof(int), &dev)) return 1;
    const FillCand* cands = static_cast<const FillCand*>(dev);
    const float* ratios_dev = reinterpret_cast<const float*>(static_cast<const unsigned char*>(dev) + rec_bytes);
    const int* live_dev = reinterpret_cast<const int*>(static_cast<const unsigned char*>(dev) + rec_bytes + ratio_bytes);
    const dim3 grid(blocks), block(256);
    if (interp == VSTAB_INTERP_BICUBIC) hipLaunchKernelGGL((sharp_transfer_kernel<VSTAB_INTERP_BICUBIC>), grid, block, 0, ctx->stream, a, cands, ratios_dev, live_dev);
    else hipLaunchKernelGGL((sharp_transfer_kernel<VSTAB_INTERP_BILINEAR>), grid, block, 0, ctx->stream, a, cands, ratios_dev, live_dev);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
