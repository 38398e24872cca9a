// vstab_internal.h -- shared between the translation units of libvstab.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <map>
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

// ---- mesh warp ----
constexpr int MESH_MAX_VERTS = 65;   // vertices per axis (64 cells): the residual (vstab_mesh.hip) and the warp (vstab_warp.hip)

// ---- the scalar pieces of the warp's arithmetic that other translation units use too (the rest: vstab_warp.hip) ----

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
