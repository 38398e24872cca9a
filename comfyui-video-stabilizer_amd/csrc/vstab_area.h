// vstab_area.h -- cv2.resize(..., INTER_AREA) on 8-bit gray, stated once: which path a resize takes, the taps of an output
// sample (OpenCV's computeResizeAreaTab) and the sum that forms it (the 2 x 2 and k x k box paths, the general path in f32
// in OpenCV's order).  The gray pass's working-size resize and every DIS pyramid level are this rule; the kernels of
// vstab_area.hip and the LDS loop of pyramid_tail_kernel (vstab_dis.hip) call it, and so does the host: nothing from HIP in
// here, tests/test_area_rule_cpu.py compiles it on its own against oracle/vo_gray.c.
#pragma once
#include <cfloat>
#include <cmath>

#ifdef __HIP__
#define VSTAB_HD __host__ __device__ __forceinline__
#else
#define VSTAB_HD inline
#endif

VSTAB_HD int sat_u8_round(float v)
{
    int i = (int)__builtin_rintf(v);
    return i < 0 ? 0 : (i > 255 ? 255 : i);
}
VSTAB_HD int ceil_d(double v) { int i = (int)v; return i + (i < v); }
VSTAB_HD int floor_d(double v) { int i = (int)v; return i - (i > v); }

// blocks of `block` threads that cover `items` elements, at most `cap` of them: the kernels stride over the rest
inline unsigned capped_grid(long long items, long long cap, int block = 256)
{
    long long b = (items + block - 1) / block;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// cv::resize picks its path from the ratios: exact 2 x 2, exact integer boxes (both ratios integers within DBL_EPSILON),
// or the general taps.  isx / isy are the box sides on the box paths.
enum { AREA_BOX2 = 0, AREA_BOX = 1, AREA_GENERAL = 2 };
struct AreaPlan { double scale_x, scale_y; int isx, isy, mode; };
inline AreaPlan plan_area(int sh, int sw, int dh, int dw)
{
    AreaPlan pl;
    pl.scale_x = 1. / ((double)dw / sw); pl.scale_y = 1. / ((double)dh / sh);
    pl.isx = (int)std::lrint(pl.scale_x); pl.isy = (int)std::lrint(pl.scale_y);
    const bool fast = std::fabs(pl.scale_x - pl.isx) < DBL_EPSILON && std::fabs(pl.scale_y - pl.isy) < DBL_EPSILON;
    pl.mode = fast ? ((pl.isx == 2 && pl.isy == 2) ? AREA_BOX2 : AREA_BOX) : AREA_GENERAL;
    return pl;
}

// The taps of output sample d along one axis are consecutive source samples from `first` on: `lead` (0 or 1) leading
// partial ones, full ones up to tap k_end, a trailing partial one if `tail` -- computeResizeAreaTab's fp64 expressions and
// its > 1e-3 tests.  Any ratio >= 1.
struct AreaRun {
    int first, n, lead, k_end;
    bool tail;
    float a_lead, a_full, a_tail;
    VSTAB_HD float w(int k) const { return (k < lead) ? a_lead : (k < k_end) ? a_full : a_tail; }
};

VSTAB_HD AreaRun area_run(int d, int ssize, double scale)
{
    const double fsx1 = d * scale, fsx2 = fsx1 + scale;
    const double cell = scale < ssize - fsx1 ? scale : ssize - fsx1;
    int sx1 = ceil_d(fsx1), sx2 = floor_d(fsx2);
    sx2 = sx2 < ssize - 1 ? sx2 : ssize - 1;
    sx1 = sx1 < sx2 ? sx1 : sx2;
    AreaRun r;
    r.lead = (sx1 - fsx1 > 1e-3) ? 1 : 0;
    r.k_end = r.lead + (sx2 - sx1);
    r.tail = fsx2 - sx2 > 1e-3;
    double at = fsx2 - sx2;
    at = at < 1. ? at : 1.;
    at = at < cell ? at : cell;
    r.a_lead = (float)((sx1 - fsx1) / cell); r.a_full = (float)(1.0 / cell); r.a_tail = (float)(at / cell);
    r.n = r.k_end + (r.tail ? 1 : 0);
    r.first = sx1 - r.lead;
    return r;
}

// The run as a record of eight weights, for the kernels that keep a table of them in LDS and index it.  A run has at most
// floor(ratio) + 2 taps: the callers admit ratios below AREA_TAPS_RATIO only.
constexpr int AREA_TAPS = 8;
constexpr double AREA_TAPS_RATIO = 6.0;
struct AreaTaps {
    int n, first;
    float a[AREA_TAPS];
    VSTAB_HD float w(int k) const { return a[k]; }
};

VSTAB_HD void area_taps(int d, int ssize, double scale, AreaTaps& t)
{
    const AreaRun r = area_run(d, ssize, scale);
    t.n = r.n;
    t.first = r.first;
#pragma unroll
    for (int k = 0; k < AREA_TAPS; k++) t.a[k] = (k < r.lead) ? r.a_lead : (k < r.k_end) ? r.a_full : (k == r.k_end && r.tail) ? r.a_tail : 0.f;
}

// ---- one output sample.  px(row, col) fetches a source byte as an int: from global memory, LDS or a host array ----

// the box paths: the exact 2 x 2 form, else the integer sum of the kx x ky box at (x, y) scaled in f32
template <class Fetch>
VSTAB_HD int area_box_px(int mode, int kx, int ky, int x, int y, Fetch px)
{
    if (mode == AREA_BOX2) return (px(2 * y, 2 * x) + px(2 * y, 2 * x + 1) + px(2 * y + 1, 2 * x) + px(2 * y + 1, 2 * x + 1) + 2) >> 2;
    int sum = 0;
    for (int j = 0; j < ky; j++)
        for (int i = 0; i < kx; i++) sum += px(y * ky + j, x * kx + i);
    return sat_u8_round(sum * (1.f / (kx * ky)));
}

// the general path (ResizeArea_Invoker): a row's products are added to `buf` from 0.f on, the rows' terms to `sum`, the
// first of them assigned.  Taps: AreaRun or AreaTaps.
template <class Taps, class Fetch>
VSTAB_HD int area_taps_px(const Taps& ax, const Taps& ay, Fetch px)
{
    float sum = 0.f;
    for (int j = 0; j < ay.n; j++) {
        float buf = 0.f;
        for (int k = 0; k < ax.n; k++) buf += px(ay.first + j, ax.first + k) * ax.w(k);
        const float term = ay.w(j) * buf;
        sum = (j == 0) ? term : sum + term;
    }
    return sat_u8_round(sum);
}

// whichever of the three paths `mode` names (kx, ky: the box sides); ax / ay are read on the general path only
template <class Taps, class Fetch>
VSTAB_HD int area_px(int mode, int kx, int ky, int x, int y, const Taps& ax, const Taps& ay, Fetch px)
{
    return mode != AREA_GENERAL ? area_box_px(mode, kx, ky, x, y, px) : area_taps_px(ax, ay, px);
}
