// vstab_area.hip -- cv2.resize(..., INTER_AREA) u8 -> u8 on the device, any ratio >= 1: the one resize entry of the gray
// pass (every working size its fused kernel does not form itself) and of the DIS pyramid (the finest level, and every
// further level where pyramid_tail_kernel does not run).  The arithmetic is vstab_area.h's; here are only the launch forms.
#include "vstab_internal.h"
#include "vstab_area.h"

namespace {

// One thread per output, grid (blocks, frames): blockIdx.y is the frame and the index inside it is 32-bit, so that
// splitting it into (row, column) is one 32-bit division.
#define FRAME_OUTPUTS(t) \
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < (unsigned)(dh * dw); t += gridDim.x * blockDim.x)

// The box paths.  AREA_BOX4_DWORD: exact 4x4 boxes on dword-aligned rows (the 960x540 -> 240x135 level of every 1080p / 4K
// clip: four dword loads and four v_sad_u8 per output instead of sixteen byte loads).
constexpr int AREA_BOX4_DWORD = 3;
__global__ __launch_bounds__(256) void area_box_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int sh, int sw, int dh,
                                                       int dw, int mode, int kx, int ky)
{
    const uint8_t* S = src + (size_t)blockIdx.y * sh * sw;
    uint8_t* D = dst + (size_t)blockIdx.y * dh * dw;
    FRAME_OUTPUTS(t) {
        const int y = (int)(t / (unsigned)dw), x = (int)(t - (unsigned)y * (unsigned)dw);
        int o;
        if (mode == AREA_BOX4_DWORD) {
            const unsigned* p = reinterpret_cast<const unsigned*>(S + (size_t)(4 * y) * sw + 4 * x);
            const int rs = sw >> 2;
            unsigned sum = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) sum = __builtin_amdgcn_sad_u8(p[(size_t)j * rs], 0u, sum);
            o = sat_u8_round((int)sum * (1.f / 16));
        } else {
            o = area_box_px(mode, kx, ky, x, y, [=](int row, int col) { return (int)S[(size_t)row * sw + col]; });
        }
        D[t] = (uint8_t)o;
    }
}

// General ratio with the taps in run form, computed per output (fp64 with three divisions per axis): no table, so no limit
// on the width or the ratio.  The sizes that matter go through area_general_rows_kernel.
__global__ __launch_bounds__(256) void area_run_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int sh, int sw, int dh,
                                                       int dw, double scale_x, double scale_y)
{
    const uint8_t* S = src + (size_t)blockIdx.y * sh * sw;
    uint8_t* D = dst + (size_t)blockIdx.y * dh * dw;
    FRAME_OUTPUTS(t) {
        const int y = (int)(t / (unsigned)dw), x = (int)(t - (unsigned)y * (unsigned)dw);
        D[t] = (uint8_t)area_taps_px(area_run(x, sw, scale_x), area_run(y, sh, scale_y), [=](int row, int col) { return (int)S[(size_t)row * sw + col]; });
    }
}

// General ratio with the tap tables in LDS: one workgroup per (frame, AREA_ROWS output rows) forms the column table once
// and one row table per output row (per output pixel the fp64 tap rule made the three small pyramid levels of a 1080p
// clip cost more than the 4x4 level that reads sixteen times the bytes).
constexpr int AREA_ROWS = 32, AREA_MAX_COLS = 1024;
__global__ __launch_bounds__(256) void area_general_rows_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int sh, int sw,
                                                                int dh, int dw, double scale_x, double scale_y)
{
    __shared__ AreaTaps s_x[AREA_MAX_COLS];
    __shared__ AreaTaps s_y[AREA_ROWS];
    const int groups = (dh + AREA_ROWS - 1) / AREA_ROWS;
    const int f = (int)blockIdx.x / groups, y0 = ((int)blockIdx.x % groups) * AREA_ROWS;
    const int rows = min(AREA_ROWS, dh - y0);
    for (int x = threadIdx.x; x < dw; x += blockDim.x) area_taps(x, sw, scale_x, s_x[x]);
    if ((int)threadIdx.x < rows) area_taps(y0 + (int)threadIdx.x, sh, scale_y, s_y[threadIdx.x]);
    __syncthreads();
    const uint8_t* S = src + (size_t)f * sh * sw;
    uint8_t* D = dst + ((size_t)f * dh + y0) * dw;
    const auto px = [=](int row, int col) { return (int)S[(size_t)row * sw + col]; };
    for (int t = threadIdx.x; t < rows * dw; t += blockDim.x) {
        const int ry = t / dw, x = t - ry * dw;
        D[t] = (uint8_t)area_taps_px(s_x[x], s_y[ry], px);
    }
}

}  // namespace

int vstab_area_resize_u8(hipStream_t st, const uint8_t* src, uint8_t* dst, int n, int sh, int sw, int dh, int dw)
{
    VSTAB_REQUIRE(src && dst && n > 0 && dh > 0 && dw > 0 && dh <= sh && dw <= sw && (long long)dh * dw < 0x7fffffffLL,
                  "area resize: %d x %dx%d -> %dx%d is not a downscale to fewer than 2^31 samples", n, sw, sh, dw, dh);
    const AreaPlan pl = plan_area(sh, sw, dh, dw);
    int mode = pl.mode;
    if (mode == AREA_BOX && pl.isx == 4 && pl.isy == 4 && sw % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0) mode = AREA_BOX4_DWORD;
    // the eight-weight records hold a run of either axis only below AREA_TAPS_RATIO
    const bool rows_form = mode == AREA_GENERAL && dw <= AREA_MAX_COLS && pl.scale_x < AREA_TAPS_RATIO && pl.scale_y < AREA_TAPS_RATIO;
    const int groups = (dh + AREA_ROWS - 1) / AREA_ROWS;
    // the frame is a grid dimension (y: at most 65535; the rows form folds it into x): more frames are served in slices
    const int slice = rows_form ? 0x7fffffff / groups : 65535;
    for (int f0 = 0; f0 < n; f0 += slice) {
        const int nf = n - f0 < slice ? n - f0 : slice;
        const uint8_t* S = src + (size_t)f0 * sh * sw;
        uint8_t* D = dst + (size_t)f0 * dh * dw;
        // (blocks, frames), near 8192 workgroups in all: a thread then strides over a few outputs
        const dim3 grid(capped_grid((long long)dh * dw, nf < 8192 ? 8192 / nf : 1), (unsigned)nf);
        if (rows_form)
            hipLaunchKernelGGL(area_general_rows_kernel, dim3((unsigned)(nf * groups)), dim3(256), 0, st, S, D, sh, sw, dh, dw, pl.scale_x, pl.scale_y);
        else if (mode == AREA_GENERAL)
            hipLaunchKernelGGL(area_run_kernel, grid, dim3(256), 0, st, S, D, sh, sw, dh, dw, pl.scale_x, pl.scale_y);
        else
            hipLaunchKernelGGL(area_box_kernel, grid, dim3(256), 0, st, S, D, sh, sw, dh, dw, mode, pl.isx, pl.isy);
        VSTAB_HIP(hipGetLastError());
    }
    return 0;
}
