// vstab_internal.h -- shared between the translation units of libvstab.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <type_traits>
#include "../../include/vstab.h"

void vstab_set_error(const char* fmt, ...);

#define VSTAB_HIP(call)                                                                  \
    do {                                                                                 \
        hipError_t _e = (call);                                                          \
        if (_e != hipSuccess) {                                                          \
            vstab_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e),       \
                            __FILE__, __LINE__);                                         \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

#define VSTAB_REQUIRE(cond, ...)                                                         \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            vstab_set_error(__VA_ARGS__);                                                \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

// What the context holds releases itself with it; none of these is copied.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

// A grow-only device/pinned-host scratch buffer.
struct ScratchBuf : NoCopy {
    void* ptr = nullptr;
    size_t bytes = 0;
    bool pinned_host = false;
    ~ScratchBuf() { release(); }
    int reserve(size_t need);
    void release();
};

// Coherent, device-mapped host memory, zero-filled: a kernel writes through dev<T>() what the host reads through
// host<T>(), with no copy on the stream.
struct MappedBuf : NoCopy {
    size_t bytes = 0;
    ~MappedBuf();
    // No-op if `need` bytes are there; else drains `stream` (a queued kernel may still write into the old block) and reallocates.
    int reserve(size_t need, hipStream_t stream);
    template <class T> T* host() const { return static_cast<T*>(h); }
    template <class T> T* dev() const { return static_cast<T*>(d); }
private:
    void *h = nullptr, *d = nullptr;
};

// An event (timing disabled unless asked otherwise) / a non-blocking stream, created by the first ensure().
struct LazyEvent : NoCopy {
    hipEvent_t ev = nullptr;
    ~LazyEvent() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};
struct LazyStream : NoCopy {
    hipStream_t st = nullptr;
    ~LazyStream() { if (st) (void)hipStreamDestroy(st); }
    hipError_t ensure() { return st ? hipSuccess : hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
    operator hipStream_t() const { return st; }
};

struct EventPair {
    LazyEvent start, stop;
    bool pending = false;        // a start/stop pair has been recorded and not yet folded into the totals
    double total_ms = 0.0;       // folded launches since vstab_set_timing(ctx, 1)
    int launches = 0;
};

// TV-L1 (vstab_tvl1.hip): the grow-only workspace, and one 64-bit word of coherent host memory that the inner kernel's
// last workgroup writes, (launch number << 32) | active pairs; gen numbers the inner launches.
struct TvState {
    ScratchBuf work;
    MappedBuf word;
    unsigned gen = 0;
};
// Folds a finished, still pending measurement into the totals (blocks until the stop event has passed).
int vstab_timer_fold(EventPair* ev);

struct vstab_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool timing = false;
    bool timing_detail = false;                 // vstab_set_timing(ctx, 2): also events around the stages INSIDE a DIS call
    bool timing_warp_only = false;              // vstab_set_timing(ctx, 3): events around the warp launches only (the roofline kernel)
    bool dis_first_pair_is_clip_start = true;   // see vstab_dis_set_clip_start
    std::map<std::string, EventPair> timers;
    // staging for small per-call parameter tables (pinned host + device mirror)
    ScratchBuf h_params, d_params;
    LazyEvent ev_params_free;  // recorded after the H2D copy of h_params
    // DIS / fit workspaces (grow-only)
    ScratchBuf d_dis, d_fit, h_fit, d_gray_tmp, d_range;
    ScratchBuf d_mask_rows;   // estimation mask: the dilated rows between the two kernels of vstab_mask_block_grid
    ScratchBuf d_sfill;       // spatial fill: the pyramid records of one chunk of frames and their per-frame words (vstab_fill.hip)
    TvState tvl1;
    // Device-side failure reports: one host-resident word (coherent, device-mapped).  A kernel ORs a VSTAB_STATUS_*
    // bit into word [0] through its device pointer; the host reads it after any stream synchronisation at no cost.
    // (The words behind it: VSTAB_PEAKS_DONE_WORD and the others below.)
    MappedBuf status;
    // F0's per-frame maxima as the gray pass reports them, mirrored into coherent host memory by the kernel that forms them
    // (frame_max_kernel) -- no copy and no event on the stream (those cost the stream ~25 us between the gray pass and the
    // pyramid, profiles/r05_dis_small_steps.md).  peaks_target counts the frames of all range passes since the context was created; the pass
    // that completes it writes that number into status[VSTAB_PEAKS_DONE_WORD] behind the values (vstab_last_frame_peaks polls it).
    MappedBuf peaks;
    int peaks_frames = 0;
    unsigned peaks_target = 0;
    ScratchBuf d_peaks_count;   // device memory: frames finished since the context was created
    // The plain warp's per-frame padded-pixel counts reach the host the same way: a one-workgroup kernel behind the warp
    // copies them into coherent host memory and sets status[VSTAB_COUNTS_DONE_WORD] to the call's generation number, which
    // vstab_last_pad_counts polls -- the step's last host wait costs the flag's round trip instead of a copy + a stream
    // synchronisation (~30 us of GPU idle between two steps).
    MappedBuf counts;
    int counts_n = 0;
    unsigned counts_gen = 0;
    // bulk host <-> device transfers (vstab_xfer.hip): pinned ring, its events, a copy stream
    ScratchBuf h_xfer;
    ScratchBuf d_xfer;   // device side of the coded forms: landing slots of byte-coded upload chunks / the packed mask
    LazyEvent ev_xfer[4];
    LazyEvent ev_xfer_sync;
    LazyStream xfer_stream;
    // speculative device-side plan (vstab_plan.hip): the plan's outputs on the device (final float32 matrices, warp
    // table, path / target) and their pinned host copy, an event behind each asynchronous download
    ScratchBuf d_plan, h_plan;
    LazyEvent ev_fit_done, ev_plan_done;
    int fit_pairs_pending = 0, plan_frames = 0, plan_params = 0;
    // The downloads behind the speculative plan (fit records, plan results) run on a stream of their own, behind ONE event
    // recorded after plan_kernel: a copy queued on the call's stream sat between fit -> plan -> warp as two engine hand-overs
    // (19 + 27 us of idle GPU per C2 step, profiles/r05_dis_small_steps.md).  fit_copy_bytes > 0: the fit records'
    // download has not been issued yet (vstab_flow_plan_device issues it on the side stream, vstab_sample_fit_batch_end on
    // the call's stream if no plan call came in between).
    unsigned* plan_zero_ptr = nullptr;     // registered for the next plan kernel to zero (vstab_flow_plan_zero_counts)
    int plan_zero_n = 0;
    unsigned* plan_zeroed_ptr = nullptr;   // what the last plan kernel zeroed: the planned warp skips its own fill for it
    LazyStream side_stream;
    LazyEvent ev_side;
    size_t fit_copy_bytes = 0;
    // DIS: the per-level image preparation (pad, gradients, structure tensor) runs on its own stream beside the
    // coarse-to-fine chain, one event per pyramid level (vstab_dis.hip)
    LazyStream prep_stream;
    LazyEvent ev_prep[16];   // MAX_LEVELS of vstab_dis.hip
    LazyEvent ev_pyramid;
};

enum { VSTAB_PEAKS_DONE_WORD = 4, VSTAB_COUNTS_DONE_WORD = 5, VSTAB_XFER_OTHER_WORD = 6 };      // index into ctx->status (the status word itself is [0])
enum { VSTAB_STATUS_PIS_TIMEOUT = 1 };   // DIS patch search: a bounded intra-workgroup dependency wait expired

// Call after a host synchronisation of ctx->stream: turns a device-side failure report into a non-zero return
// (rc 3) with vstab_last_error() set, and clears the word.
int vstab_check_device_status(vstab_ctx* ctx, const char* who);

// Upload `bytes` of host data through the pinned staging buffer; returns device pointer.
int vstab_stage_params(vstab_ctx* ctx, const void* host, size_t bytes, void** dev_out);

// cv2.resize(..., INTER_AREA) of n gray images [sh][sw] -> [dh][dw] on `st`, any ratio >= 1 (vstab_area.hip; the rule
// itself is vstab_area.h): the gray pass's and the DIS pyramid's resize.
int vstab_area_resize_u8(hipStream_t st, const uint8_t* src, uint8_t* dst, int n, int sh, int sw, int dh, int dw);

// Brackets the kernels of one API call with HIP events recorded on the call's stream (no host
// sync here: vstab_last_kernel_ms waits for the stop event when the number is asked for).
EventPair* vstab_timer_slot(vstab_ctx* ctx, const char* kind);

// DETAIL: the same around one stage inside a call, only under vstab_set_timing(ctx, 2): the events sit between dependent
// kernels, where they lengthen the chain a little, and a kind used twice in one call folds (waits for) its previous
// measurement -- for a measurement pass of its own, never inside a timed loop.
struct KernelTimer {
    enum Scope { CALL, DETAIL };
    vstab_ctx* ctx;
    EventPair* ev = nullptr;
    KernelTimer(vstab_ctx* c, const char* k, Scope scope = CALL) : ctx(c) {
        // (level 3: an event pair costs the stream ~10 us -- 0.05-0.1 ms over the four stages of a C2 step, measured -- so a
        // timed loop keeps them around the one kernel whose per-launch time it reports, profiles/r05_dis_small_steps.md)
        if (ctx->timing && (scope == DETAIL ? ctx->timing_detail : (!ctx->timing_warp_only || strncmp(k, "warp", 4) == 0))) {
            ev = vstab_timer_slot(ctx, k);
            // the previous launch of this kind finished long ago (every pipeline pass synchronises with the host
            // between two launches of the same kind), so folding it costs no wait
            if (ev && ev->pending) (void)vstab_timer_fold(ev);
            if (ev) (void)hipEventRecord(ev->start, ctx->stream);
        }
    }
    ~KernelTimer() {
        if (ev) {
            (void)hipEventRecord(ev->stop, ctx->stream);
            ev->pending = true;
        }
    }
};

// cv::invert for a 3x3 CV_64F matrix (closed form); returns false (and zeros) if singular.  One definition for the host
// (vstab_warp_batch inverts the caller's matrices) and the device (plan_kernel writes the warp's table itself): IEEE fp64
// operations in one fixed order, no contraction (-ffp-contract=off), so both produce the same bits.
__host__ __device__ inline bool vstab_invert3x3_hd(const double* S, double* D)
{
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) +
               S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (d == 0.0) {
        for (int i = 0; i < 9; i++) D[i] = 0.0;
        return false;
    }
    d = 1.0 / d;
    double t[9];
    t[0] = (S[4] * S[8] - S[5] * S[7]) * d;
    t[1] = (S[2] * S[7] - S[1] * S[8]) * d;
    t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
    t[3] = (S[5] * S[6] - S[3] * S[8]) * d;
    t[4] = (S[0] * S[8] - S[2] * S[6]) * d;
    t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
    t[6] = (S[3] * S[7] - S[4] * S[6]) * d;
    t[7] = (S[1] * S[6] - S[0] * S[7]) * d;
    t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
    for (int i = 0; i < 9; i++) D[i] = t[i];
    return true;
}
bool vstab_invert3x3(const double* S, double* D);

// The pair mapping of the scene-cut score and of the deflicker's measurement (include/vstab.h states it once, under
// vstab_pair_residual_batch): a pixel p = (x, y) of the FROM frame through the pair's transition, widened to fp64.
struct PairMatrix {
    double m[9];
};
// one pixel of the rule: returns true and *q (pixel index into the TO frame) if p lands inside
__device__ __forceinline__ bool vstab_pair_lookup(const PairMatrix& A, int x, int y, int h, int w, int* q)
{
    const double dx = (double)x, dy = (double)y;
    const double X = (A.m[0] * dx + A.m[1] * dy) + A.m[2];
    const double Y = (A.m[3] * dx + A.m[4] * dy) + A.m[5];
    const double W = (A.m[6] * dx + A.m[7] * dy) + A.m[8];
    if (!(W > 0.0 && W <= 1.7976931348623157e308)) return false;   // w <= 0 or not finite
    // (X / 1.0 is X: the division is skipped where it changes no bit)
    const double qx = (W == 1.0) ? X : X / W, qy = (W == 1.0) ? Y : Y / W;
    const double rx = rint(qx), ry = rint(qy);          // half-to-even; NaN / inf fail the comparisons below
    if (!(rx >= 0.0 && rx <= (double)(w - 1) && ry >= 0.0 && ry <= (double)(h - 1))) return false;
    *q = (int)ry * w + (int)rx;
    return true;
}

// The warp kernels' per-(frame, sample) transform record and how it is filled from a float32 matrix
// (cv::warpPerspective: M.convertTo(CV_64F), invert).
struct WarpXform {
    double m[9];     // inverse (output -> source) matrix, as cv::warpPerspective builds it
    double wq;       // affine only: m8 ? 32/m8 : 0
    double wn;       // affine only: m8 ? 1/m8 : 0
    int affine;      // m6 == 0 && m7 == 0
    int pad_;
};
__host__ __device__ inline void vstab_fill_xform(const float* m32, WarpXform* xf)
{
    double M[9];
    for (int i = 0; i < 9; i++) M[i] = (double)m32[i];
    vstab_invert3x3_hd(M, xf->m);
    xf->affine = (xf->m[6] == 0.0 && xf->m[7] == 0.0) ? 1 : 0;
    const double W = xf->m[8];
    xf->wq = (W != 0.0) ? 32.0 / W : 0.0;
    xf->wn = (W != 0.0) ? 1.0 / W : 0.0;
    xf->pad_ = 0;
}
// float32 matrices [count, 9] -> WarpXform table -> the call's staged parameters on the device (vstab_warp.hip).
int vstab_stage_xforms(vstab_ctx* ctx, const float* m32, size_t count, const WarpXform** dev_out);

// Host-side checks and launch geometry of every warp-shaped entry point (vstab_warp.hip; vstab_neighbour.hip uses them too).
int vstab_check_sizes(const char* who, int n, int sh, int sw, int dh, int dw);
int vstab_check_subpix(const char* who, int subpix);
int vstab_check_common(const char* who, vstab_ctx* ctx, const void* src, int n, int sh, int sw, const void* mats,
                       int dh, int dw, int interp, const float* border, int subpix, const void* dst);
void vstab_set_block_width(int dh, int dw, int* bw0, int* bw0_pow2);
int vstab_tile_grid(const char* who, int n, int dh, int dw, int tx, int nt, int* tiles_x, int* tiles_y, unsigned* grid);

// ---- mesh warp ----
constexpr int MESH_MAX_VERTS = 65;   // vertices per axis (64 cells): the residual (vstab_mesh.hip) and the warp (vstab_warp.hip)

// ---- the scalar pieces of the warp's arithmetic that other translation units use too (the rest: the guarded section below) ----

// std::max((double)INT_MIN, std::min((double)INT_MAX, v)) followed by cvRound
__device__ __forceinline__ int clamp_round_i32(double v)
{
    const double hi = 2147483647.0, lo = -2147483648.0;
    double m = (v < hi) ? v : hi;
    double r = (lo < m) ? m : lo;
    return (int)__builtin_rint(r);
}

// cv::saturate_cast<short>(int)
__device__ __forceinline__ int sat_short(int v)
{
    return v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
}

// OpenCV's WarpPerspectiveInvoker evaluates its row-start terms once per block of this many output columns.
inline int vstab_warp_block_width(int dh, int dw)
{
    const int BLOCK_SZ = 32;
    const int bh0 = BLOCK_SZ / 2 < dh ? BLOCK_SZ / 2 : dh;
    return BLOCK_SZ * BLOCK_SZ / bh0 < dw ? BLOCK_SZ * BLOCK_SZ / bh0 : dw;
}

// INTER_NEAREST coverage of the source position (qx, qy) = (Xn * Wn, Yn * Wn) by an sw x sh source: the warp's mask rule
// in its general form (the plain warp's affine fast path gives the same answer where it applies).
__device__ __forceinline__ bool vstab_nn_covered(double qx, double qy, int sh, int sw)
{
    const int nx = sat_short(clamp_round_i32(qx));
    const int ny = sat_short(clamp_round_i32(qy));
    return (unsigned)nx < (unsigned)sw && (unsigned)ny < (unsigned)sh;
}

// The maximum of v over the 64 lanes of a wavefront, valid in lane 63: a DPP scan inside each row of 16 lanes (row_shr
// 1/2/4/8), then lane 15 of rows 0 and 2 into rows 1 and 3 (row_bcast:15), then lane 31 into rows 2 and 3 (row_bcast:31).
// `old` is the lane's own value and bound_ctrl is off, so a lane without a source lane keeps what it has.  No LDS traffic
// and no wait on it; float max is order-independent as long as the caller keeps NaN out of the result (the range passes
// carry a NaN flag of their own).  Every lane of the wavefront must reach the call.
__device__ __forceinline__ float wave_max_lane63(float v)
{
#define VSTAB_DPP_MAX(CTRL, ROW_MASK)                                                                                             \
    v = __builtin_fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), (CTRL), (ROW_MASK), 0xf, false)))
    VSTAB_DPP_MAX(0x111, 0xf);   // row_shr:1
    VSTAB_DPP_MAX(0x112, 0xf);   // row_shr:2
    VSTAB_DPP_MAX(0x114, 0xf);   // row_shr:4
    VSTAB_DPP_MAX(0x118, 0xf);   // row_shr:8
    VSTAB_DPP_MAX(0x142, 0xa);   // row_bcast:15 into rows 1 and 3
    VSTAB_DPP_MAX(0x143, 0xc);   // row_bcast:31 into rows 2 and 3
#undef VSTAB_DPP_MAX
    return v;
}

// ---- the block-level integer sum: THE tail of every pass that ends in exact integer sums ----
// Integer addition is associative, so neither the order of lanes and waves nor the order of the atomics behind it shows in
// a result.  The mechanism (shuffles, then LDS) is stated here and nowhere else.

// NC sums of type T (unsigned, unsigned long long, long long) over an NT-thread workgroup.  The kernel declares one
// `__shared__`; every thread calls put() with its own NC values (each wave's sums go to LDS); behind the kernel's own
// __syncthreads() any thread reads total(c), slot c over the waves, accumulated in U.  Which thread finishes which slot, the
// gate and the atomics stay with the kernel.  part[wave][slot]: threads that finish consecutive slots read consecutive
// words.  An object is used once per kernel execution (a second put() would need a barrier in front of it).
template <class T, int NC, int NT>
struct BlockSums {
    static_assert(NT % 64 == 0, "whole wavefronts");
    T part[NT / 64][NC];
    // The wave's sum of a slot is a __shfl_down chain 32 .. 1, valid in lane 0.  The chain stands in this loop and not in a
    // function of its own: behind a `wave_sum(T)` the compiler allocates the plain warp's registers differently all through
    // the kernel (profiles/r29_block_sums.md); written here, the benchmark's kernel is the same instruction sequence as before.
    __device__ __forceinline__ void put(const T (&v)[NC])
    {
        if constexpr (NC >= 2 && NC <= 4) {
            // a few slots: their chains side by side, so that one slot's shuffle latency hides another's (one after the other
            // cost the temporal fill 1 %, profiles/r29_block_sums.md)
            T s[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) s[c] = v[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int c = 0; c < NC; c++) s[c] += __shfl_down(s[c], off);
            }
            if ((threadIdx.x & 63) == 0) {
#pragma unroll
                for (int c = 0; c < NC; c++) part[threadIdx.x >> 6][c] = s[c];
            }
        } else {
            // many slots: one after the other, a slot's registers are free once it is stored (side by side, the 17 / 31
            // 64-bit slots of the anchor sums cost a wave per SIMD)
#pragma unroll
            for (int c = 0; c < NC; c++) {
                T s = v[c];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
                if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = s;
            }
        }
    }
    template <class U = T>
    __device__ __forceinline__ U total(int c) const
    {
        U s = part[0][c];
#pragma unroll
        for (int k = 1; k < NT / 64; k++) s += part[k][c];
        return s;
    }
};

// Per-thread counts of an NT-thread block -> one atomic per counter and block, only if non-zero and asked for
// (out[c] != nullptr); out[c] is a per-frame array.  All threads of the block call it (barrier).
template <int NC, int NT = 256>
__device__ __forceinline__ void block_count_add(const unsigned (&v)[NC], unsigned* const (&out)[NC], int frame)
{
    __shared__ BlockSums<unsigned, NC, NT> s_cnt;
    s_cnt.put(v);
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const unsigned total = s_cnt.total(c);
            if (total && out[c]) atomicAdd(out[c] + frame, total);
        }
    }
}

// ---- the residual of the global fit at a grid sample and the median of a workgroup's residuals: the per-vertex form
// (vstab_mesh.hip) and the per-row form (vstab_rolling.hip) ----
__device__ __forceinline__ bool finite_f(float v) { return __builtin_fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN

// The grid sample at (x, y) with flow (u, v) against the 3x3 fit A: where the flow takes the point minus where the fit does,
// every operation fp64 and rounded on its own.  false: a flow or a residual that is not finite (not a sample).
__device__ __forceinline__ bool vstab_fit_residual(const double (&A)[9], double x, double y, float u, float v, float& rx, float& ry)
{
    const double X = (A[0] * x + A[1] * y) + A[2];
    const double Y = (A[3] * x + A[4] * y) + A[5];
    const double W = (A[6] * x + A[7] * y) + A[8];
    rx = (float)((x + (double)u) - X / W);
    ry = (float)((y + (double)v) - Y / W);
    return finite_f(u) && finite_f(v) && finite_f(rx) && finite_f(ry);
}

// The medians of s_rx[0..n) and s_ry[0..n), n >= 1, values in LDS that a barrier has made visible; called by all 256 threads
// of the workgroup.  Every thread counts the rank of its elements against all others: the element of rank (n-1)/2 and the
// one of rank n/2 are the middle(s).  Thread 0 writes the two medians to out[0], out[1].
__device__ __forceinline__ void vstab_median_pair(const float* s_rx, const float* s_ry, int n, float* out)
{
    __shared__ float s_mid[2][2];          // [axis][lo, hi]
    // rank of element i: values below it, and equal values in front of it -- a permutation of 0..n-1
    const int klo = (n - 1) >> 1, khi = n >> 1;
    for (int i = threadIdx.x; i < n; i += 256) {
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
    }
}

// What the two residual entry points check alike: context, pointers, sizes, grid == ceil(work / step), and the launch grid of
// per_pair workgroups per pair.
int vstab_check_residual(const char* who, vstab_ctx* ctx, const void* grid_flow, const void* transitions, const void* residual,
                         const void* count, int pairs, int gh, int gw, int step, int work_h, int work_w, long long per_pair,
                         unsigned* blocks);

// ---- the warp's arithmetic proper: samplers, tile shell, warp_pixel, the kernel body ----
// Compiled only where a translation unit defines VSTAB_WARP_ARITHMETIC in front of this include (vstab_warp.hip,
// vstab_rolling.hip and vstab_neighbour.hip).  It lives here because profiles/warp_traffic.json is tied to the hash of vstab_warp.hip + this
// file: whatever decides the plain warp's instructions stays inside the two.
#ifdef VSTAB_WARP_ARITHMETIC
constexpr int TILE_PX = 2;       // pixels per thread along x, strided by the tile width (profiles/r01_warp_tile_sweep.md)
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

// warp_pixel's displacement hook, of two kinds.  OUTPUT == false: a functor evaluated at the source position
// q = (Xn * Wn, Yn * Wn) that gives the offset (cx, cy) taken off it before the roundings.  OUTPUT == true: `solve`, evaluated
// on the output pixel in front of the matrix (MeshInverseDisplacement).  NoDisplacement is the plain warp: nothing of the
// hook is compiled.
struct NoDisplacement {
    static constexpr bool ACTIVE = false;
    static constexpr bool OUTPUT = false;
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
// warp_kernel under every Args (plain, mesh and rolling shutter, forward and inverse), cover_extent_kernel and the
// neighbour passes (vstab_neighbour.hip).  `q5(X, Y)` samples at the 1/32-px coordinates, `exact(fsx, fsy)`
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

// The displacement a kernel's arguments ask for.  Plain warp: none.  Arguments derived from WarpArgs bring an overload of
// their own, in their own namespace (the mesh forms: vstab_warp.hip; the rolling-shutter forms: vstab_rolling.hip).
__device__ __forceinline__ NoDisplacement make_displacement(const WarpArgs&, int) { return {}; }

// One 64 x 8 (TILE_TX = 32) tile of the warp: every pixel through warp_pixel, RGB + mask stored, padded pixels counted.
// Args = WarpArgs is the plain warp, Args = MeshWarpArgs the mesh warp, Args = MeshUnwarpArgs its inverse, Args =
// RollingWarpArgs / RollingUnwarpArgs the rolling-shutter warp and its inverse (the rules are in
// include/vstab.h): the same body with the displacement its arguments ask for.  Arguments of an OUTPUT-kind displacement
// carry the second counter, `unconverged`.
// Like every kernel of the library it sits in the translation unit's anonymous namespace: internal linkage, and the
// profilers' kernel names keep the prefix the tools under tools/ select the library's kernels by.
// The body stays in the kernel: inlined from a device function that receives the
// arguments by reference, the compiler issued the two epilogue stores in another order and the plain warp ran 0.3-1 %
// slower (profiles/r11_one_warp_arithmetic.md).
namespace {
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
    unsigned unconv = 0;      // OUTPUT kind only: this thread's pixels whose solve hit its step limit or was refused

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
        // (the count is within the spread of repeated launches of the plain warp at 256 x 1080p, and so is a per-wavefront
        // ballot form of it: tools/warp_count_cost.py, profiles/r28_range_tail.md)
        if (WITH_MASK && a.pad_count != nullptr) block_count_add<1>(padded, {a.pad_count}, frame);
    }
}
}  // namespace

// The displaced warps' launch: the SUBPIX x MASK instantiation of the bilinear 64 x 8 tile for these arguments.
template <class Args>
void vstab_launch_displaced(const Args& a, unsigned blocks, int subpix, bool with_mask, size_t lds_bytes, hipStream_t stream)
{
    constexpr int BILINEAR = VSTAB_INTERP_BILINEAR, Q5 = VSTAB_SUBPIX_Q5, EXACT = VSTAB_SUBPIX_EXACT;
    const dim3 grid(blocks), block(256);
    if (subpix == EXACT) {
        if (with_mask) hipLaunchKernelGGL((warp_kernel<BILINEAR, EXACT, true, 32, Args>), grid, block, lds_bytes, stream, a);
        else hipLaunchKernelGGL((warp_kernel<BILINEAR, EXACT, false, 32, Args>), grid, block, lds_bytes, stream, a);
    } else {
        if (with_mask) hipLaunchKernelGGL((warp_kernel<BILINEAR, Q5, true, 32, Args>), grid, block, lds_bytes, stream, a);
        else hipLaunchKernelGGL((warp_kernel<BILINEAR, Q5, false, 32, Args>), grid, block, lds_bytes, stream, a);
    }
}

// The displaced warps' preparation, behind the caller's checks (vstab_warp.hip): the device, one staged table of the n
// transform records followed by `tail_bytes` of the caller's own (the staging buffer holds one table per call; *d_tail: where
// they lie on the device), the geometry, the 32 x 256 tile grid, and zeroed counters (pad_count, second; each may be NULL).
int vstab_prepare_displaced(const char* who, vstab_ctx* ctx, WarpArgs& a, const float* src, int n, int sh, int sw,
                            const float* matrices, int dh, int dw, const float* border, float* dst, float* mask,
                            uint32_t* pad_count, uint32_t* second, const void* tail, size_t tail_bytes, const void** d_tail,
                            unsigned* blocks);
#endif  // VSTAB_WARP_ARITHMETIC
