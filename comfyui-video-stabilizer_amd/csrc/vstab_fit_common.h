// vstab_fit_common.h -- what fit_kernel (vstab_fit.hip) and homography_kernel (vstab_homography.hip) share: the replay of
// OpenCV's RNG stream and adaptive iteration count, the walk over a pair's valid samples, the block sum, the batch scoring
// and the single-lane "best so far / update niters" loop of their RANSAC, and the float32 inlier tests.  Included by those
// two translation units only.  Everything is inlined into the kernels: the order of the floating-point operations is the
// source's (-ffp-contract=off), so a change here moves both models alike.
#pragma once
#include "vstab_internal.h"
#include <cmath>

namespace {

// cv::RNG (multiply-with-carry), seeded with 2^64-1 by both RANSACs
struct Rng { unsigned long long state; };
__device__ __forceinline__ unsigned rng_next(Rng& r)
{
    r.state = (unsigned long long)(unsigned)r.state * 4164903690ULL + (unsigned)(r.state >> 32);
    return (unsigned)r.state;
}
__device__ __forceinline__ int rng_uniform(Rng& r, int a, int b) { return a == b ? a : (int)(rng_next(r) % (unsigned)(b - a) + a); }

// cv::RANSACUpdateNumIters
__device__ int ransac_update_num_iters(double p, double ep, int modelPoints, int maxIters)
{
    p = p > 0. ? p : 0.; p = p < 1. ? p : 1.;
    ep = ep > 0. ? ep : 0.; ep = ep < 1. ? ep : 1.;
    double num = 1. - p > 2.2250738585072014e-308 ? 1. - p : 2.2250738585072014e-308;
    double denom = 1. - pow(1. - ep, (double)modelPoints);
    if (denom < 2.2250738585072014e-308) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= maxIters * (-denom) ? maxIters : (int)__builtin_rint(num / denom);
}

// The samples of one frame pair.  vmap[0 .. nv) lists, in ascending order, the entries of F that are valid.
struct Samples {
    const float* F;
    const int* vmap;
    int gw, step;

    // gw > 0: stride-`step` grid over a flow field (F = [gh][gw][2] displacements, flow.py:141-147);
    // gw == 0: explicit point pairs (F = [cap][4]: prev.x, prev.y, next.x, next.y; untracked points carry NaN)
    __device__ __forceinline__ void load(int g, float& px, float& py, float& cx, float& cy) const
    {
        if (gw == 0) {
            const float4 v = *reinterpret_cast<const float4*>(F + (size_t)g * 4);
            px = v.x; py = v.y; cx = v.z; cy = v.w;
            return;
        }
        const int gy = g / gw, gx = g - gy * gw;
        px = (float)(gx * step);
        py = (float)(gy * step);
        cx = px + F[(size_t)g * 2];
        cy = py + F[(size_t)g * 2 + 1];
    }

    // body(k, px, py, cx, cy) for the valid samples k = tid, tid + NT, ... of a block of NT threads
    template <int NT, typename Body>
    __device__ __forceinline__ void for_each_valid(int nv, Body&& body) const
    {
        for (int k = threadIdx.x; k < nv; k += NT) {
            float px, py, cx, cy;
            load(vmap[k], px, py, cx, cy);
            body(k, px, py, cx, cy);
        }
    }
};

// Sum of v over a block of WAVES wavefronts: shuffle tree per wavefront, then the wavefronts' partials left to right.
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* scratch /* >= WAVES */)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    T total = scratch[0];
#pragma unroll
    for (int i = 1; i < WAVES; i++) total += scratch[i];
    __syncthreads();
    return total;
}

// float32 squared transfer error of a sample under the affine model M[6] / the homography H[8] (H[8] = 1), as
// OpenCV's computeError forms it
__device__ __forceinline__ float affine_err2(const float* M, float px, float py, float cx, float cy)
{
    const float ea = M[0] * px + M[1] * py + M[2] - cx;
    const float eb = M[3] * px + M[4] * py + M[5] - cy;
    return ea * ea + eb * eb;
}
__device__ __forceinline__ float reproj_err2(const float* H, float px, float py, float cx, float cy)
{
    const float ww = 1.f / (H[6] * px + H[7] * py + 1.f);
    const float ex = (H[0] * px + H[1] * py + H[2]) * ww - cx;
    const float ey = (H[3] * px + H[4] * py + H[5]) * ww - cy;
    return ex * ex + ey * ey;
}

// Inlier counts of the BATCH models of one RANSAC round in one pass over the samples: err(c, px, py, cx, cy) is model c's
// float32 squared error, a sample is an inlier if it is <= thr (a NaN is none).  Integer counts, so the order of the
// additions into s_cnt (zeroed by the caller, read after the next barrier) does not matter.
template <int BATCH, int NT, typename Err>
__device__ __forceinline__ void ransac_score_batch(const Samples& samples, int nv, float thr, int* s_cnt, Err&& err)
{
    int cnt[BATCH];
#pragma unroll
    for (int c = 0; c < BATCH; c++) cnt[c] = 0;
    samples.for_each_valid<NT>(nv, [&](int, float px, float py, float cx, float cy) {
#pragma unroll
        for (int c = 0; c < BATCH; c++) cnt[c] += (err(c, px, py, cx, cy) <= thr) ? 1 : 0;
    });
#pragma unroll
    for (int c = 0; c < BATCH; c++) {
        int v = cnt[c];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[c], v);
    }
}

// What became of model c of a batch: RANSAC_FAILED -- getSubset found no sample, OpenCV's loop ends there; RANSAC_NONE --
// runKernel returned no model, the iteration counts and nothing else happens.
enum { RANSAC_SOLVED, RANSAC_NONE, RANSAC_FAILED };

// One lane replays OpenCV's sequential loop (RANSACPointSetRegistrator::run) over a scored batch: a model of LEN doubles
// with more inliers than the best so far (and than MIN_GOOD) becomes s_best and shortens niters.
// s_ctl: 0 done flag, 1 niters, 2 iter, 3 maxGood.
template <int BATCH, int LEN, int POINTS, int MIN_GOOD, typename State>
__device__ __forceinline__ void ransac_replay(int* s_ctl, const int* s_cnt, const double (*s_model)[LEN], double* s_best, int nv, State&& state)
{
    int niters = s_ctl[1], iter = s_ctl[2], maxGood = s_ctl[3];
    bool stop = false;
    for (int c = 0; c < BATCH && iter < niters; c++, iter++) {
        const int st = state(c);
        if (st == RANSAC_FAILED) { stop = true; break; }   // iter == 0 -> no model, else the best so far stands
        if (st == RANSAC_NONE) continue;
        const int good = s_cnt[c];
        if (good > (maxGood > MIN_GOOD ? maxGood : MIN_GOOD)) {
            for (int k = 0; k < LEN; k++) s_best[k] = s_model[c][k];
            maxGood = good;
            niters = ransac_update_num_iters(0.992, (double)(nv - good) / nv, POINTS, niters);
        }
    }
    s_ctl[1] = niters; s_ctl[2] = iter; s_ctl[3] = maxGood;
    s_ctl[0] = (stop || iter >= niters) ? 1 : 0;
}

}  // namespace
