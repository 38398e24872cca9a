// vstab_tvl1.hip -- Dual TV-L1 optical flow over the consecutive pairs of a clip (include/vstab.h,
// vstab_tvl1_flow_batch): cv::optflow::DualTVL1OpticalFlow::calc(prev, curr, None) with useInitialFlow false and
// gamma 0, the Flow node's second dense estimator (nodes/video_stabilizer_flow.py:76-107).
//
// The arithmetic follows the float32 restatement tests/tvl1_restatement.py association for association (it names the
// OpenCV version it restates; unpinned against a real OpenCV).  -ffp-contract=off keeps every product and sum rounded
// on its own.  The one stated deviation is the order of the error sum (a pairwise tree in double per row, then over the
// rows), which OpenCV forms in its own thread-dependent order.
//
// GPU form.  Pairs are independent (no initial flow), so every launch covers all pairs of a chunk:
//   per chunk    u8 -> f32, INTER_LINEAR pyramid of every frame (scale_step), centred gradients of every level
//   per scale    p := 0; u := 0 (coarsest) or the bilinear upsample of the coarser u times 1/scale_step
//   per warp     tvl1_warp_kernel: bicubic remap of I1, I1x, I1y at (x+u1, y+u2), grad, rho_c; every pair active
//   per outer    tvl1_median_kernel: 5x5 median of u1, u2 (active pairs) into a scratch copy
//   per inner    tvl1_inner_kernel: thresholding, divergence, u update, error terms, forward gradient, dual update --
//                one launch.  u and p are double-buffered (a workgroup reads its neighbours' old values in a one-pixel
//                halo), the buffer index is a per-pair word flipped by the pair's last workgroup, which also sums the
//                row totals, counts the iteration and clears the pair's active flag once error <= scaledEpsilon.
// Workgroups of inactive pairs return at once.  The launch's last workgroup mirrors (launch number, active pairs) into
// coherent host memory; the host reads that word every few launches and stops launching for the (scale, warp) once it
// reports no active pair.  No workgroup ever waits for another one.
//
// Algorithmic traffic of one inner iteration: read u1 u2 (8 B), p11 p12 p21 p22 (16 B), I1wx I1wy grad rho_c (16 B),
// write u1 u2 p11 p12 p21 p22 (24 B): 64 B per pixel.
#include "vstab_internal.h"
#include "vstab_wait.h"

#include <algorithm>
#include <cmath>
#include <memory>

namespace {

// initInterTab1D(INTER_CUBIC): A = -0.75, x = i/32, same operation order as OpenCV's interpolateCubic (the same
// table as cubic_coeffs of vstab_internal.h)
__device__ __forceinline__ void tvl1_cubic_coeffs(int i, float* c)
{
    const float A = -0.75f;
    const float x = i * (1.f / 32);
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

constexpr int TVL1_MAX_SCALES = 10;
constexpr int TVL1_NT = 256;
constexpr int TVL1_MAX_W = 2048, TVL1_MAX_H = 2048;

struct TLevel { int h, w; };

inline int pow2_at_least(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

dim3 tvl1_grid(long long per_item, int items)
{
    long long b = (per_item + TVL1_NT - 1) / TVL1_NT;
    const long long cap = std::max(1LL, (256LL * 32) / std::max(items, 1));
    b = std::min(std::max(b, 1LL), cap);
    return dim3((unsigned)b, (unsigned)items);
}

#define TVL1_STRIDE(t, per_item) \
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < (unsigned)(per_item); t += gridDim.x * blockDim.x)

__device__ __forceinline__ int t_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- resize INTER_LINEAR (cv::resize generic path: horizontal pass into float rows, then vertical) ----
__device__ __forceinline__ void lin_tap(int d, double scale, int& s, float& f)
{
    const float fx = (float)((d + 0.5) * scale - 0.5);
    s = (int)__builtin_floorf(fx);
    f = fx - (float)s;
}

__device__ __forceinline__ float resize_px(const float* __restrict__ S, int sh, int sw, int dx, int dy, double scx, double scy)
{
    int sx, sy;
    float fx, fy;
    lin_tap(dx, scx, sx, fx);
    if (sx < 0) { sx = 0; fx = 0.f; }
    bool tail = false;
    if (sx + 1 >= sw) { sx = sw - 1; fx = 0.f; tail = true; }
    lin_tap(dy, scy, sy, fy);
    const int r0 = t_clamp(sy, 0, sh - 1), r1 = t_clamp(sy + 1, 0, sh - 1);
    const float* S0 = S + (size_t)r0 * sw;
    const float* S1 = S + (size_t)r1 * sw;
    float h0, h1;
    if (tail) {
        h0 = S0[sx];
        h1 = S1[sx];
    } else {
        const float a0 = 1.f - fx, a1 = fx;
        h0 = S0[sx] * a0 + S0[sx + 1] * a1;
        h1 = S1[sx] * a0 + S1[sx + 1] * a1;
    }
    const float b0 = 1.f - fy, b1 = fy;
    return h0 * b0 + h1 * b1;
}

__global__ __launch_bounds__(TVL1_NT) void tvl1_convert_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int per_frame)
{
    const size_t f = blockIdx.y;
    TVL1_STRIDE(t, per_frame) dst[f * per_frame + t] = (float)src[f * per_frame + t];
}

// one pyramid level of every frame: resize(prev, Size(), step, step, INTER_LINEAR)
__global__ __launch_bounds__(TVL1_NT) void tvl1_pyr_kernel(const float* __restrict__ src, int sh, int sw, float* __restrict__ dst, int dh,
                                                          int dw, double scx, double scy)
{
    const size_t f = blockIdx.y;
    src += f * sh * sw;
    dst += f * dh * dw;
    TVL1_STRIDE(t, dh * dw) {
        const int y = (int)(t / (unsigned)dw), x = (int)(t - (unsigned)y * (unsigned)dw);
        dst[t] = resize_px(src, sh, sw, x, y, scx, scy);
    }
}

// centredGradient: 0.5 * (I[x+1] - I[x-1]) with the index clamped (OpenCV's one-sided rows, columns and corners)
__global__ __launch_bounds__(TVL1_NT) void tvl1_grad_kernel(const float* __restrict__ I, float* __restrict__ Ix, float* __restrict__ Iy, int h, int w)
{
    const size_t off = (size_t)blockIdx.y * h * w;
    I += off;
    TVL1_STRIDE(t, h * w) {
        const int y = (int)(t / (unsigned)w), x = (int)(t - (unsigned)y * (unsigned)w);
        const int xm = x > 0 ? x - 1 : 0, xp = x + 1 < w ? x + 1 : w - 1;
        const int ym = y > 0 ? y - 1 : 0, yp = y + 1 < h ? y + 1 : h - 1;
        Ix[off + t] = 0.5f * (I[y * w + xp] - I[y * w + xm]);
        Iy[off + t] = 0.5f * (I[yp * w + x] - I[ym * w + x]);
    }
}

// the coarser scale's u (buffer cur[p]) -> this scale's u (same buffer index), resize to the finer size then * mul
__global__ __launch_bounds__(TVL1_NT) void tvl1_upsample_kernel(const float* __restrict__ Uc, int ch, int cw, float* __restrict__ Uf, int fh, int fw,
                                                               double scx, double scy, float mul, const int* __restrict__ cur)
{
    const int p = blockIdx.y;
    const int b = cur[p];
    const size_t cpx = (size_t)ch * cw, fpx = (size_t)fh * fw;
    TVL1_STRIDE(t, fh * fw) {
        const int y = (int)(t / (unsigned)fw), x = (int)(t - (unsigned)y * (unsigned)fw);
        for (int c = 0; c < 2; c++) {
            const float* S = Uc + (((size_t)p * 2 + b) * 2 + c) * cpx;
            Uf[(((size_t)p * 2 + b) * 2 + c) * fpx + t] = resize_px(S, ch, cw, x, y, scx, scy) * mul;
        }
    }
}

// ---- remap INTER_CUBIC, BORDER_CONSTANT 0, float maps rounded to 1/32 px ----
__device__ __forceinline__ float cubic_sample(const float* __restrict__ S, int sh, int sw, int X, int Y, const float* cub)
{
    const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
    const float* cx = cub + (X & 31) * 4;
    const float* cy = cub + (Y & 31) * 4;
    const int x0 = sx - 1, y0 = sy - 1;
    const unsigned width1 = (unsigned)(sw - 3 > 0 ? sw - 3 : 0), height1 = (unsigned)(sh - 3 > 0 ? sh - 3 : 0);
    if ((unsigned)x0 < width1 && (unsigned)y0 < height1) {
        const float* r = S + (size_t)y0 * sw + x0;
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float* q = r + (size_t)i * sw;
            const float t = q[0] * (cy[i] * cx[0]) + q[1] * (cy[i] * cx[1]) + q[2] * (cy[i] * cx[2]) + q[3] * (cy[i] * cx[3]);
            sum = i == 0 ? t : sum + t;
        }
        return sum;
    }
    if (x0 >= sw || x0 + 4 <= 0 || y0 >= sh || y0 + 4 <= 0) return 0.f;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int yy = y0 + i;
        if (yy < 0 || yy >= sh) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int xx = x0 + j;
            if (xx < 0 || xx >= sw) continue;
            sum += (S[(size_t)yy * sw + xx] - 0.f) * (cy[i] * cx[j]);
        }
    }
    return sum;
}

struct WarpArgs {
    const float *I0, *I1, *I1x, *I1y;   // level images of the chunk's frames [frames][npx]
    const float* U;                     // [P][2][2][npx]
    float* W;                           // [P][4][npx]: I1wx, I1wy, grad, rho_c
    const int* cur;
    int* active;
    int h, w;
};

__global__ __launch_bounds__(TVL1_NT) void tvl1_warp_kernel(WarpArgs a)
{
    __shared__ float s_cub[32 * 4];
    if (threadIdx.x < 32) tvl1_cubic_coeffs((int)threadIdx.x, s_cub + threadIdx.x * 4);
    __syncthreads();
    const int p = blockIdx.y;
    const size_t npx = (size_t)a.h * a.w;
    const int b = a.cur[p];
    const float* u1 = a.U + (((size_t)p * 2 + b) * 2 + 0) * npx;
    const float* u2 = a.U + (((size_t)p * 2 + b) * 2 + 1) * npx;
    const float* I0 = a.I0 + (size_t)p * npx;
    const float* I1 = a.I1 + (size_t)(p + 1) * npx;
    const float* I1x = a.I1x + (size_t)(p + 1) * npx;
    const float* I1y = a.I1y + (size_t)(p + 1) * npx;
    float* Wp = a.W + (size_t)p * 4 * npx;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.active[p] = 1;
    TVL1_STRIDE(t, npx) {
        const int y = (int)(t / (unsigned)a.w), x = (int)(t - (unsigned)y * (unsigned)a.w);
        const float U1 = u1[t], U2 = u2[t];
        const float mx = (float)x + U1, my = (float)y + U2;
        const int X = (int)__builtin_rintf(mx * 32.f), Y = (int)__builtin_rintf(my * 32.f);
        const float w0 = cubic_sample(I1, a.h, a.w, X, Y, s_cub);
        const float wx = cubic_sample(I1x, a.h, a.w, X, Y, s_cub);
        const float wy = cubic_sample(I1y, a.h, a.w, X, Y, s_cub);
        Wp[t] = wx;
        Wp[npx + t] = wy;
        Wp[2 * npx + t] = wx * wx + wy * wy;
        Wp[3 * npx + t] = ((w0 - wx * U1) - wy * U2) - I0[t];
    }
}

// ---- medianBlur 5x5 (replicated border) of u1, u2 into the scratch copy the next inner launch reads ----
__device__ __forceinline__ float median25(float (&v)[25])
{
    // Batcher's odd-even merge sort for 25 inputs (140 compare-exchanges); the exact 13th smallest
#pragma unroll
    for (int p = 1; p < 25; p <<= 1)
#pragma unroll
        for (int k = p; k >= 1; k >>= 1)
#pragma unroll
            for (int j = k % p; j + k < 25; j += 2 * k)
#pragma unroll
                for (int i = 0; i < k; i++)
                    if (i + j + k < 25 && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        const float lo = __builtin_fminf(v[i + j], v[i + j + k]), hi = __builtin_fmaxf(v[i + j], v[i + j + k]);
                        v[i + j] = lo;
                        v[i + j + k] = hi;
                    }
    return v[12];
}

__global__ __launch_bounds__(TVL1_NT) void tvl1_median_kernel(const float* __restrict__ U, float* __restrict__ M, const int* __restrict__ cur,
                                                             const int* __restrict__ active, int h, int w)
{
    const int p = blockIdx.z;
    if (!active[p]) return;
    const int c = blockIdx.y;
    const size_t npx = (size_t)h * w;
    const float* S = U + (((size_t)p * 2 + cur[p]) * 2 + c) * npx;
    float* D = M + ((size_t)p * 2 + c) * npx;
    TVL1_STRIDE(t, npx) {
        const int y = (int)(t / (unsigned)w), x = (int)(t - (unsigned)y * (unsigned)w);
        float v[25];
#pragma unroll
        for (int dy = 0; dy < 5; dy++) {
            const float* row = S + (size_t)t_clamp(y + dy - 2, 0, h - 1) * w;
#pragma unroll
            for (int dx = 0; dx < 5; dx++) v[dy * 5 + dx] = row[t_clamp(x + dx - 2, 0, w - 1)];
        }
        D[t] = median25(v);
    }
}

// ---- one inner iteration, fused ----
struct InnerArgs {
    float* U;            // [P][2][2][npx]
    float* Pd;           // [P][2][4][npx]: p11, p12, p21, p22
    const float* W;      // [P][4][npx]
    const float* M;      // [P][2][npx]: the median copy (from_median)
    double* rowsum;      // [P][h]
    int* active;
    int* cur;
    unsigned* ticket;    // [P] + 1 (the launch's)
    int* iterations;     // this (scale, warp)'s counter of pair 0, or nullptr
    int iter_stride;     // ints between two pairs' counters
    unsigned long long* mirror;
    unsigned gen;
    int P, h, w, R, L, HL;
    int from_median;
    float l_t, taut, theta, eps;
};

__device__ __forceinline__ float div_at(const float* __restrict__ q1, const float* __restrict__ q2, int x, int y, int w)
{
    const size_t i = (size_t)y * w + x;
    if (x > 0 && y > 0) return (q1[i] - q1[i - 1]) + (q2[i] - q2[i - w]);
    if (y == 0 && x > 0) return (q1[i] - q1[i - 1]) + q2[i];
    if (x == 0 && y > 0) return (q1[i] + q2[i]) - q2[i - w];
    return q1[i] + q2[i];
}

// the launch's last workgroup to report: mirrors (launch number, active pairs) into coherent host memory
__device__ void tvl1_report(const InnerArgs& a)
{
    __threadfence();
    const unsigned prev = __hip_atomic_fetch_add(a.ticket + a.P, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev + 1u != (unsigned)a.P) return;
    unsigned n_active = 0;
    for (int q = 0; q < a.P; q++) n_active += __hip_atomic_load(a.active + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
    a.ticket[a.P] = 0u;
    __threadfence_system();
    __hip_atomic_store(a.mirror, ((unsigned long long)a.gen << 32) | n_active, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(TVL1_NT) void tvl1_inner_kernel(InnerArgs a)
{
    const int p = blockIdx.y;
    if (!a.active[p]) {
        if (blockIdx.x == 0 && threadIdx.x == 0) tvl1_report(a);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    const int w = a.w, h = a.h, R = a.R, L = a.L;
    double* s_term = s_dyn;                                   // [R][L]
    double* s_rows = s_term + (size_t)R * L;                  // [HL] (the pair's last workgroup)
    float* s_u1 = reinterpret_cast<float*>(s_rows + a.HL);    // [R+1][w]
    float* s_u2 = s_u1 + (size_t)(R + 1) * w;
    __shared__ int s_last;

    const size_t npx = (size_t)h * w;
    const int b = a.cur[p];
    const float* uo1 = a.from_median ? a.M + (size_t)p * 2 * npx : a.U + (((size_t)p * 2 + b) * 2 + 0) * npx;
    const float* uo2 = a.from_median ? a.M + ((size_t)p * 2 + 1) * npx : a.U + (((size_t)p * 2 + b) * 2 + 1) * npx;
    float* un1 = a.U + (((size_t)p * 2 + (b ^ 1)) * 2 + 0) * npx;
    float* un2 = a.U + (((size_t)p * 2 + (b ^ 1)) * 2 + 1) * npx;
    const float* po = a.Pd + ((size_t)p * 2 + b) * 4 * npx;
    float* pn = a.Pd + ((size_t)p * 2 + (b ^ 1)) * 4 * npx;
    const float* Wp = a.W + (size_t)p * 4 * npx;

    const int y0 = blockIdx.x * R;
    const int own = min(R, h - y0);
    const int rows = min(R + 1, h - y0);   // own rows + the next one (its new u feeds the forward gradient)
    // 1. thresholding, divergence, u update (own rows + one), error terms (own rows)
    for (int idx = threadIdx.x; idx < rows * w; idx += TVL1_NT) {
        const int r = idx / w, x = idx - r * w, y = y0 + r;
        const size_t i = (size_t)y * w + x;
        const float u1 = uo1[i], u2 = uo2[i];
        const float gx = Wp[i], gy = Wp[npx + i], grad = Wp[2 * npx + i], rho_c = Wp[3 * npx + i];
        const float rho = rho_c + (gx * u1 + gy * u2);
        float d1 = 0.f, d2 = 0.f;
        if (rho < -a.l_t * grad) {
            d1 = a.l_t * gx;
            d2 = a.l_t * gy;
        } else if (rho > a.l_t * grad) {
            d1 = -a.l_t * gx;
            d2 = -a.l_t * gy;
        } else if (grad > __FLT_EPSILON__) {
            const float fi = -rho / grad;
            d1 = fi * gx;
            d2 = fi * gy;
        }
        const float v1 = u1 + d1, v2 = u2 + d2;
        const float n1 = v1 + a.theta * div_at(po, po + npx, x, y, w);
        const float n2 = v2 + a.theta * div_at(po + 2 * npx, po + 3 * npx, x, y, w);
        s_u1[r * w + x] = n1;
        s_u2[r * w + x] = n2;
        if (r < own) {
            const float e1 = n1 - u1, e2 = n2 - u2;
            s_term[(size_t)r * L + x] = (double)(e1 * e1 + e2 * e2);
            un1[i] = n1;
            un2[i] = n2;
        }
    }
    for (int idx = threadIdx.x; idx < own * (L - w); idx += TVL1_NT) {
        const int r = idx / (L - w);
        s_term[(size_t)r * L + w + (idx - r * (L - w))] = 0.0;
    }
    __syncthreads();
    // 2. forward gradient of the new u, dual update
    for (int idx = threadIdx.x; idx < own * w; idx += TVL1_NT) {
        const int r = idx / w, x = idx - r * w, y = y0 + r;
        const size_t i = (size_t)y * w + x;
        const float n1 = s_u1[r * w + x], n2 = s_u2[r * w + x];
        const float u1x = x + 1 < w ? s_u1[r * w + x + 1] - n1 : 0.f;
        const float u1y = y + 1 < h ? s_u1[(r + 1) * w + x] - n1 : 0.f;
        const float u2x = x + 1 < w ? s_u2[r * w + x + 1] - n2 : 0.f;
        const float u2y = y + 1 < h ? s_u2[(r + 1) * w + x] - n2 : 0.f;
        const float g1 = (float)__builtin_sqrt((double)u1x * (double)u1x + (double)u1y * (double)u1y);
        const float g2 = (float)__builtin_sqrt((double)u2x * (double)u2x + (double)u2y * (double)u2y);
        const float ng1 = 1.f + a.taut * g1, ng2 = 1.f + a.taut * g2;
        pn[i] = (po[i] + a.taut * u1x) / ng1;
        pn[npx + i] = (po[npx + i] + a.taut * u1y) / ng1;
        pn[2 * npx + i] = (po[2 * npx + i] + a.taut * u2x) / ng2;
        pn[3 * npx + i] = (po[3 * npx + i] + a.taut * u2y) / ng2;
    }
    // 3. row sums: pairwise tree over each own row (zero-padded to L), in double
    for (int st = 1; st < L; st <<= 1) {
        const int per_row = L / (2 * st);
        for (int idx = threadIdx.x; idx < own * per_row; idx += TVL1_NT) {
            const int r = idx / per_row, k = (idx - r * per_row) * 2 * st;
            s_term[(size_t)r * L + k] = s_term[(size_t)r * L + k] + s_term[(size_t)r * L + k + st];
        }
        __syncthreads();
    }
    if (threadIdx.x < own) a.rowsum[(size_t)p * h + y0 + threadIdx.x] = s_term[(size_t)threadIdx.x * L];
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned prev = __hip_atomic_fetch_add(a.ticket + p, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev + 1u == gridDim.x;
    }
    __syncthreads();
    if (!s_last) return;
    // 4. the pair's last workgroup: error = the rows' pairwise tree, rounded to float; the iteration's bookkeeping
    __threadfence();
    for (int i = threadIdx.x; i < a.HL; i += TVL1_NT)
        s_rows[i] = i < h ? __hip_atomic_load(a.rowsum + (size_t)p * h + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    __syncthreads();
    for (int st = 1; st < a.HL; st <<= 1) {
        for (int k = threadIdx.x * 2 * st; k < a.HL; k += TVL1_NT * 2 * st) s_rows[k] = s_rows[k] + s_rows[k + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float error = (float)s_rows[0];
        if (a.iterations) a.iterations[(size_t)p * a.iter_stride] += 1;
        a.cur[p] = b ^ 1;
        if (!(error > a.eps)) a.active[p] = 0;
        a.ticket[p] = 0u;
        tvl1_report(a);
    }
}

// ---- outputs: the finest u as [P][h][w][2], and sampled at the stride-`step` grid ----
__global__ __launch_bounds__(TVL1_NT) void tvl1_output_kernel(const float* __restrict__ U, const int* __restrict__ cur, float* __restrict__ out,
                                                             int h, int w, int gh, int gw, int step)
{
    const int p = blockIdx.y;
    const size_t npx = (size_t)h * w;
    const float* u1 = U + (((size_t)p * 2 + cur[p]) * 2 + 0) * npx;
    const float* u2 = u1 + npx;
    out += (size_t)p * gh * gw * 2;
    TVL1_STRIDE(t, gh * gw) {
        const int gy = (int)(t / (unsigned)gw), gx = (int)(t - (unsigned)gy * (unsigned)gw);
        const size_t i = (size_t)gy * step * w + (size_t)gx * step;
        out[2 * (size_t)t] = u1[i];
        out[2 * (size_t)t + 1] = u2[i];
    }
}

struct TCarver {
    char* base;
    size_t off = 0;
    explicit TCarver(void* p) : base(static_cast<char*>(p)) {}
    template <typename T> T* take(size_t count)
    {
        off = (off + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

struct TvWork {
    float *I[TVL1_MAX_SCALES], *Ix[TVL1_MAX_SCALES], *Iy[TVL1_MAX_SCALES], *U[TVL1_MAX_SCALES];
    float *Pd, *W, *M;
    double* rowsum;
    int *active, *cur;
    unsigned* ticket;
};

void tvl1_layout(TCarver& c, TvWork& k, const TLevel* L, int ns, int P)
{
    const size_t frames = (size_t)P + 1, npx0 = (size_t)L[0].h * L[0].w;
    for (int s = 0; s < ns; s++) {
        const size_t npx = (size_t)L[s].h * L[s].w;
        k.I[s] = c.take<float>(frames * npx);
        k.Ix[s] = c.take<float>(frames * npx);
        k.Iy[s] = c.take<float>(frames * npx);
        k.U[s] = c.take<float>((size_t)P * 4 * npx);
    }
    k.Pd = c.take<float>((size_t)P * 8 * npx0);
    k.W = c.take<float>((size_t)P * 4 * npx0);
    k.M = c.take<float>((size_t)P * 2 * npx0);
    k.rowsum = c.take<double>((size_t)P * L[0].h);
    k.active = c.take<int>((size_t)P);
    k.cur = c.take<int>((size_t)P);
    k.ticket = c.take<unsigned>((size_t)P + 1);
}

// Waits (bounded) until the inner launch numbered `target` has mirrored its count; returns the count it reports.
int tvl1_poll(vstab_ctx* ctx, TvState& tv, unsigned target, unsigned* n_active)
{
    volatile unsigned long long* word = tv.word.host<volatile unsigned long long>();
    unsigned long long v = 0;
    auto reached = [&] { v = *word; return vstab_seq_reached((unsigned)(v >> 32), target); };
    // an inner launch of a 960x540 chunk takes a few ms; should the word never arrive (a lost launch), a stream
    // synchronisation after 2 s turns the wait into the runtime's own error report
    if (!vstab_spin_until(reached, std::chrono::seconds(2))) {
        VSTAB_HIP(hipStreamSynchronize(ctx->stream));
        VSTAB_REQUIRE(reached(), "vstab_tvl1_flow_batch: inner launch %u never reported", target);
    }
    *n_active = (unsigned)(v & 0xffffffffu);
    return 0;
}

int tvl1_chunk(vstab_ctx* ctx, TvState& tv, const uint8_t* gray, int P, const TLevel* L, int ns, const vstab_tvl1_params& prm, float* flow,
               float* grid_flow, int sample_step, int32_t* iterations)
{
    hipStream_t st = ctx->stream;
    TvWork k{};
    {
        TCarver sizer(nullptr);
        tvl1_layout(sizer, k, L, ns, P);
        if (tv.work.reserve(sizer.off + 256)) return 1;
    }
    TCarver carver(tv.work.ptr);
    tvl1_layout(carver, k, L, ns, P);
    const int frames = P + 1;
    const int h0 = L[0].h, w0 = L[0].w;
    hipLaunchKernelGGL(tvl1_convert_kernel, tvl1_grid((long long)h0 * w0, frames), dim3(TVL1_NT), 0, st, gray, k.I[0], h0 * w0);
    const double sc = 1.0 / prm.scale_step;
    for (int s = 1; s < ns; s++)
        hipLaunchKernelGGL(tvl1_pyr_kernel, tvl1_grid((long long)L[s].h * L[s].w, frames), dim3(TVL1_NT), 0, st, k.I[s - 1], L[s - 1].h,
                           L[s - 1].w, k.I[s], L[s].h, L[s].w, sc, sc);
    for (int s = 0; s < ns; s++)
        hipLaunchKernelGGL(tvl1_grad_kernel, tvl1_grid((long long)L[s].h * L[s].w, frames), dim3(TVL1_NT), 0, st, k.I[s], k.Ix[s], k.Iy[s],
                           L[s].h, L[s].w);
    VSTAB_HIP(hipMemsetAsync(k.cur, 0, sizeof(int) * P, st));
    VSTAB_HIP(hipMemsetAsync(k.ticket, 0, sizeof(unsigned) * (P + 1), st));
    VSTAB_HIP(hipMemsetAsync(k.U[ns - 1], 0, sizeof(float) * (size_t)P * 4 * L[ns - 1].h * L[ns - 1].w, st));
    VSTAB_HIP(hipGetLastError());

    const float l_t = (float)(prm.lambda * prm.theta), taut = (float)(prm.tau / prm.theta), theta = (float)prm.theta;
    const float mul = (float)(1.0 / prm.scale_step);
    const int K = prm.poll_interval > 0 ? prm.poll_interval : 8;
    for (int s = ns - 1; s >= 0; s--) {
        const int h = L[s].h, w = L[s].w;
        const size_t npx = (size_t)h * w;
        if (s < ns - 1)
            hipLaunchKernelGGL(tvl1_upsample_kernel, tvl1_grid((long long)npx, P), dim3(TVL1_NT), 0, st, k.U[s + 1], L[s + 1].h, L[s + 1].w,
                               k.U[s], h, w, 1.0 / ((double)w / L[s + 1].w), 1.0 / ((double)h / L[s + 1].h), mul, k.cur);
        VSTAB_HIP(hipMemsetAsync(k.Pd, 0, sizeof(float) * (size_t)P * 8 * npx, st));
        InnerArgs ia{};
        ia.U = k.U[s]; ia.Pd = k.Pd; ia.W = k.W; ia.M = k.M; ia.rowsum = k.rowsum; ia.active = k.active; ia.cur = k.cur;
        ia.ticket = k.ticket;
        ia.mirror = tv.word.dev<unsigned long long>();
        ia.P = P; ia.h = h; ia.w = w; ia.L = pow2_at_least(w); ia.HL = pow2_at_least(h);
        ia.l_t = l_t; ia.taut = taut; ia.theta = theta;
        ia.eps = (float)(prm.epsilon * prm.epsilon * (double)((long long)h * w));
        ia.iter_stride = prm.nscales * prm.warps;
        // rows per workgroup: the most that keep the workgroup's LDS within 64 KB
        auto lds_for = [&](int R) { return sizeof(double) * ((size_t)R * ia.L + ia.HL) + sizeof(float) * 2 * (size_t)(R + 1) * w; };
        int R = 8;
        while (R > 1 && lds_for(R) > 64 * 1024) R >>= 1;
        ia.R = R;
        const size_t lds = lds_for(R);
        VSTAB_REQUIRE(lds <= 64 * 1024, "vstab_tvl1_flow_batch: a %dx%d level needs %zu B of LDS per row", w, h, lds);
        const dim3 inner_grid((unsigned)((h + R - 1) / R), (unsigned)P);
        for (int wp = 0; wp < prm.warps; wp++) {
            WarpArgs wa{};
            wa.I0 = k.I[s]; wa.I1 = k.I[s]; wa.I1x = k.Ix[s]; wa.I1y = k.Iy[s]; wa.U = k.U[s]; wa.W = k.W; wa.cur = k.cur;
            wa.active = k.active; wa.h = h; wa.w = w;
            hipLaunchKernelGGL(tvl1_warp_kernel, tvl1_grid((long long)npx, P), dim3(TVL1_NT), 0, st, wa);
            ia.iterations = iterations ? iterations + (size_t)s * prm.warps + wp : nullptr;
            const unsigned first_gen = tv.gen + 1;
            int launched = 0;
            bool done = false;
            for (int o = 0; o < prm.outer_iterations && !done; o++) {
                const bool median = prm.median_filtering > 1;
                if (median)
                    hipLaunchKernelGGL(tvl1_median_kernel, dim3(tvl1_grid((long long)npx, 1).x, 2, (unsigned)P), dim3(TVL1_NT), 0, st, k.U[s],
                                       k.M, k.cur, k.active, h, w);
                for (int it = 0; it < prm.inner_iterations; it++) {
                    ia.from_median = median && it == 0;
                    ia.gen = ++tv.gen;
                    hipLaunchKernelGGL(tvl1_inner_kernel, inner_grid, dim3(TVL1_NT), lds, st, ia);
                    launched++;
                    if (launched % K == 0) {
                        // the word of a launch K back: the queue still holds K launches while the host looks
                        const unsigned target = std::max(first_gen, ia.gen - (unsigned)K);
                        VSTAB_HIP(hipGetLastError());
                        unsigned n_active = 0;
                        if (int rc = tvl1_poll(ctx, tv, target, &n_active)) return rc;
                        if (n_active == 0) { done = true; break; }
                    }
                }
            }
            VSTAB_HIP(hipGetLastError());
        }
    }
    const int h = L[0].h, w = L[0].w;
    if (grid_flow) {
        const int gh = (h + sample_step - 1) / sample_step, gw = (w + sample_step - 1) / sample_step;
        hipLaunchKernelGGL(tvl1_output_kernel, tvl1_grid((long long)gh * gw, P), dim3(TVL1_NT), 0, st, k.U[0], k.cur, grid_flow, h, w, gh, gw,
                           sample_step);
    }
    if (flow)
        hipLaunchKernelGGL(tvl1_output_kernel, tvl1_grid((long long)h * w, P), dim3(TVL1_NT), 0, st, k.U[0], k.cur, flow, h, w, h, w, 1);
    VSTAB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" void vstab_tvl1_default_params(vstab_tvl1_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->tau = 0.25;
    p->lambda = 0.15;
    p->theta = 0.3;
    p->epsilon = 0.01;
    p->scale_step = 0.8;
    p->gamma = 0.0;
    p->nscales = 5;
    p->warps = 5;
    p->inner_iterations = 30;
    p->outer_iterations = 10;
    p->median_filtering = 5;
    p->use_initial_flow = 0;
    p->chunk_pairs = 0;
    p->poll_interval = 0;
}

extern "C" int vstab_tvl1_flow_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const vstab_tvl1_params* params,
                                     float* flow, float* grid_flow, int sample_step, int32_t* iterations)
{
    VSTAB_REQUIRE(ctx != nullptr, "vstab_tvl1_flow_batch: ctx is NULL");
    VSTAB_REQUIRE(gray != nullptr, "vstab_tvl1_flow_batch: gray is NULL");
    VSTAB_REQUIRE(n >= 2, "vstab_tvl1_flow_batch: need at least 2 frames, got %d", n);
    VSTAB_REQUIRE(flow != nullptr || grid_flow != nullptr || iterations != nullptr, "vstab_tvl1_flow_batch: no output requested");
    VSTAB_REQUIRE(sample_step >= 1, "vstab_tvl1_flow_batch: sample_step must be >= 1");
    vstab_tvl1_params prm;
    vstab_tvl1_default_params(&prm);
    if (params) prm = *params;
    VSTAB_REQUIRE(prm.gamma == 0.0, "vstab_tvl1_flow_batch: gamma = %g is not supported (only gamma = 0, the reference's default)", prm.gamma);
    VSTAB_REQUIRE(prm.use_initial_flow == 0, "vstab_tvl1_flow_batch: an initial flow is not supported (useInitialFlow must be false)");
    VSTAB_REQUIRE(prm.nscales >= 1 && prm.nscales <= TVL1_MAX_SCALES, "vstab_tvl1_flow_batch: nscales must be in [1, %d], got %d", TVL1_MAX_SCALES,
                  prm.nscales);
    VSTAB_REQUIRE(prm.warps >= 1 && prm.inner_iterations >= 1 && prm.outer_iterations >= 1,
                  "vstab_tvl1_flow_batch: warps, innerIterations and outerIterations must be >= 1");
    VSTAB_REQUIRE(prm.median_filtering <= 1 || prm.median_filtering == 5, "vstab_tvl1_flow_batch: medianFiltering must be 1 (off) or 5, got %d",
                  prm.median_filtering);
    VSTAB_REQUIRE(prm.scale_step > 0.0 && prm.scale_step < 1.0, "vstab_tvl1_flow_batch: scaleStep must be in (0, 1), got %g", prm.scale_step);
    VSTAB_REQUIRE(prm.tau > 0.0 && prm.theta > 0.0 && prm.lambda >= 0.0 && prm.epsilon >= 0.0, "vstab_tvl1_flow_batch: tau, theta must be > 0, lambda, epsilon >= 0");
    VSTAB_REQUIRE(h >= 16 && w >= 16, "vstab_tvl1_flow_batch: %dx%d: the finest level must be at least 16x16", w, h);
    VSTAB_REQUIRE(h <= TVL1_MAX_H && w <= TVL1_MAX_W, "vstab_tvl1_flow_batch: %dx%d: at most %dx%d", w, h, TVL1_MAX_W, TVL1_MAX_H);
    // calc(): the pyramid ends before a level narrower or shorter than 16
    TLevel L[TVL1_MAX_SCALES];
    L[0] = {h, w};
    int ns = 1;
    for (int s = 1; s < prm.nscales; s++) {
        const int nh = (int)std::rint(L[s - 1].h * prm.scale_step), nw = (int)std::rint(L[s - 1].w * prm.scale_step);
        if (nw < 16 || nh < 16) break;
        L[ns++] = {nh, nw};
    }
    VSTAB_HIP(hipSetDevice(ctx->device));
    TvState& tv = ctx->tvl1;
    if (tv.word.reserve(64, ctx->stream)) return 1;
    KernelTimer timer(ctx, "tvl1");
    const int pairs = n - 1;
    if (iterations) VSTAB_HIP(hipMemsetAsync(iterations, 0, sizeof(int32_t) * (size_t)pairs * prm.nscales * prm.warps, ctx->stream));
    // chunk: the workspace of one pair is ~31 finest-level fields (a 960x540 pair ~64 MB); at most ~4 GB per chunk
    int chunk = prm.chunk_pairs;
    if (chunk <= 0) {
        TvWork k{};
        TCarver one(nullptr), two(nullptr);
        tvl1_layout(one, k, L, ns, 1);
        tvl1_layout(two, k, L, ns, 2);
        const size_t per_pair = std::max<size_t>(two.off - one.off, 1);
        chunk = (int)std::max<size_t>(1, (size_t(4) << 30) / per_pair);
    }
    chunk = std::min(chunk, std::min(pairs, 65535));
    const size_t npx = (size_t)h * w;
    const int gh = (h + sample_step - 1) / sample_step, gw = (w + sample_step - 1) / sample_step;
    for (int p0 = 0; p0 < pairs; p0 += chunk) {
        const int P = std::min(chunk, pairs - p0);
        if (int rc = tvl1_chunk(ctx, tv, gray + (size_t)p0 * npx, P, L, ns, prm, flow ? flow + (size_t)p0 * npx * 2 : nullptr,
                                grid_flow ? grid_flow + (size_t)p0 * gh * gw * 2 : nullptr, sample_step,
                                iterations ? iterations + (size_t)p0 * prm.nscales * prm.warps : nullptr))
            return rc;
    }
    return 0;
}
