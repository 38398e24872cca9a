/*
 * vstab.h -- C ABI of libvstab.so, the MI355X (gfx950) implementation of the
 * dense-flow stabilization hot path of nomadoor/ComfyUI-Video-Stabilizer.
 *
 * The reference is pure Python and has no FFI of its own; every entry point
 * below replaces a group of OpenCV/NumPy calls made by the reference's Python
 * (file:line cited per function, paths relative to the reference root).  The
 * Python host layer (comfyui-video-stabilizer_amd/) binds these with ctypes;
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every call returns 0 on success, non-zero on failure;
 *     vstab_last_error() returns a thread-local message for the last failure.
 *     A failure detected by a kernel (e.g. an expired dependency wait inside the
 *     DIS patch search) is recorded in a host-visible status word and reported
 *     -- return value 3 -- by the next call that synchronises with the host
 *     (vstab_sample_fit_batch, vstab_synchronize).
 *   - "dev" pointers are HIP device pointers owned by the caller (e.g.
 *     torch.Tensor.data_ptr()); "host" pointers are ordinary host memory.
 *     The library never frees caller memory and never returns owned memory.
 *   - work is enqueued on the context's stream (vstab_set_stream; default: the
 *     null stream).  Calls that return host results synchronise that stream;
 *     the others are asynchronous.
 *   - images are row-major, channel-last: frames [N,H,W,3] f32 0..1,
 *     masks [N,H,W] f32, gray [N,h,w] u8, flow [P,h,w,2] f32 (x,y).
 *   - 3x3 matrices are row-major, 9 values.
 */
#ifndef VSTAB_H
#define VSTAB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSTAB_ABI_VERSION 1

typedef struct vstab_ctx vstab_ctx;

enum vstab_interp { VSTAB_INTERP_BILINEAR = 0, VSTAB_INTERP_BICUBIC = 1 };
/* sub-pixel model of the interpolating warp: Q5 = OpenCV legacy kernels (source
 * coordinates rounded to 1/32 px), EXACT = full f32 coordinates (OpenCV >= 4.11
 * INTER_LINEAR kernels; bilinear only). */
enum vstab_subpix { VSTAB_SUBPIX_Q5 = 0, VSTAB_SUBPIX_EXACT = 1 };
enum vstab_mode { VSTAB_MODE_TRANSLATION = 0, VSTAB_MODE_SIMILARITY = 1, VSTAB_MODE_PERSPECTIVE = 2 };

/* ---- context ------------------------------------------------------------ */
int vstab_abi_version(void);
const char* vstab_last_error(void);
/* device < 0: use the current HIP device */
/* 1 in the test build (-DVSTAB_TEST_HOOKS -> lib/libvstab_hooks.so: the fault injectors VSTAB_DEBUG_PLAN_PERTURB,
 * VSTAB_DEBUG_PIS_SPIN_LIMIT, VSTAB_DEBUG_XFER_SPAWN_FAIL are read from the environment), 0 in the shipped library,
 * which reads none of them. */
int vstab_test_hooks(void);
int vstab_create(vstab_ctx** out, int device);
int vstab_destroy(vstab_ctx* ctx);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = null stream */
int vstab_set_stream(vstab_ctx* ctx, void* hip_stream);
int vstab_synchronize(vstab_ctx* ctx);
/* Kernel timing with HIP events recorded on the call's own stream, per kind of call ("warp", "warp_blur",
 * "gray", "dis", "fit", "gftt", "lk", "phase").  vstab_set_timing(ctx, 1) enables it and clears the totals;
 * vstab_set_timing(ctx, 2) also brackets the stages INSIDE a DIS call ("dis_prep", "dis_pis4_L<level>",
 * "dis_level_L<level>", "dis_final": for a measurement pass of its own, the events lengthen the chain).
 * vstab_set_timing(ctx, 3) records events around the warp launches only ("warp", "warp_blur"): what a timed loop keeps.
 * vstab_last_kernel_ms: milliseconds of the most recent call of that kind (waits for it to finish).
 * vstab_kernel_ms_stats: sum and number of all calls of that kind since timing was enabled -- no
 * synchronisation is needed inside a timed loop, bench.py reads the totals after its closing fence
 * for the roofline line. */
int vstab_set_timing(vstab_ctx* ctx, int enabled);
int vstab_last_kernel_ms(vstab_ctx* ctx, const char* kind, float* ms_out);
int vstab_kernel_ms_stats(vstab_ctx* ctx, const char* kind, double* total_ms, int* launches);

/* ---- F0 / F16: the node boundary's bulk transfers ---------------------------------------------
 * ComfyUI hands CPU tensors in and takes CPU tensors back (nodes/stabilizer_utils.py:96-147, :200-221): 6.37 GB in and
 * 8.49 GB out for a 256 x 1080p clip.  vstab_upload / vstab_download move `bytes` between ordinary (pageable) host
 * memory and device memory through a ring of page-locked buffers filled / drained by several host threads
 * (VSTAB_XFER_THREADS, default 16, capped at the core count) while the DMA engine moves the previous chunk.
 * vstab_upload returns when every byte has left host_src (the copy into dev_dst completes asynchronously; work
 * enqueued afterwards on the context's stream is ordered behind it).  vstab_download starts after the work already
 * enqueued on the context's stream and returns when host_dst is complete. */
int vstab_upload(vstab_ctx* ctx, const void* host_src, void* dev_dst, size_t bytes);
int vstab_download(vstab_ctx* ctx, const void* dev_src, void* host_dst, size_t bytes);
/* The same two transfers with fewer bytes on PCIe where the DATA allow it; the destination holds the source's bits either way.
 * vstab_upload_f32_coded: `count` float32 values.  A ComfyUI IMAGE decoded from 8-bit video holds float32(k) / float32(255)
 * and nothing else (what nodes/stabilizer_utils.py:122-126 itself produces for uint8 input): a chunk (2^25 values) whose values
 * all have exactly the bits of such a quotient crosses as bytes and is expanded on the device by the same correctly rounded
 * division; the first chunk with a value of any other kind, and everything behind it, crosses as float32.  *coded_chunks
 * (may be NULL) = chunks that crossed as bytes.  dev_dst 16-byte aligned.
 * vstab_download_mask_coded: `count` float32 mask values (nodes/stabilizer_utils.py:1055-1077).  If every value is 0.0f or
 * 1.0f (the Flow node's mask, nodes/video_stabilizer_flow.py:583-586) they cross as bytes and the host threads expand them;
 * otherwise (Motion Apply's soft mask under motion blur) this is vstab_download.  *coded (may be NULL) = 1 / 0.
 * vstab_upload_u8_as_f32: `count` uint8 values k arrive on the device as float32(k) / float32(255) -- _to_numpy_frame's uint8
 * branch, `arr.astype(np.float32); arr /= 255.0` (nodes/stabilizer_utils.py:122-126), without the host ever holding the floats.
 */
int vstab_upload_f32_coded(vstab_ctx* ctx, const float* host_src, float* dev_dst, size_t count, size_t* coded_chunks);
int vstab_upload_u8_as_f32(vstab_ctx* ctx, const unsigned char* host_src, float* dev_dst, size_t count);
int vstab_download_mask_coded(vstab_ctx* ctx, const float* dev_src, float* host_dst, size_t count, int* coded);
/* The motion-blur warp's soft mask (nodes/motion_apply.py:195-199) holds 1 - c / S for c = 0 .. S covered samples, values below
 * 1e-3 set to 0: S + 1 different floats.  vstab_download_mask_levels(levels = S) sends c as a byte and the host threads look the
 * float up (formed with the same IEEE float32 subtraction and division); a mask with any other value takes vstab_download.
 * levels = 1 is vstab_download_mask_coded. */
int vstab_download_mask_levels(vstab_ctx* ctx, const float* dev_src, float* host_dst, size_t count, int levels, int* coded);

/* ---- F13 / A3: per-frame warp with padding mask ---------------------------
 * Replaces the loop at nodes/video_stabilizer_flow.py:560-588 and
 * nodes/motion_apply.py:92-120:
 *   cv2.warpPerspective(frame, M, (out_w,out_h), INTER_LINEAR|INTER_CUBIC, BORDER_CONSTANT, rgb)
 *   cv2.warpPerspective(ones,  M, (out_w,out_h), INTER_NEAREST, BORDER_CONSTANT, 0)
 *   mask = 1 - (content > 0.5); mask[mask < 1e-3] = 0
 * src        dev  [n, src_h, src_w, 3] f32
 * matrices   host [n, 9] f32, forward (source -> output) as the reference passes them
 * border_rgb host [3] f32 (padding_rgb / 255 computed in f32)
 * dst        dev  [n, out_h, out_w, 3] f32
 * mask       dev  [n, out_h, out_w] f32 or NULL (masks_zero path, motion_apply.py:103-106)
 * pad_count  dev  [n] u32 or NULL: number of mask==1 pixels per frame
 *                 (mask.mean() = count/(out_h*out_w), flow.py:587)
 */
int vstab_warp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w,
                     const float* matrices, int out_h, int out_w, int interp,
                     const float* border_rgb, int subpix, float* dst, float* mask,
                     uint32_t* pad_count);

/* ---- A5: multi-sample motion-blur warp -------------------------------------
 * Replaces nodes/motion_apply.py:125-202 (_blurred_matrix_samples +
 * _warp_with_motion_blur).  matrices: host [n,9] f64 motion matrices; the
 * library forms the S sample matrices M[i] + (M[i+1]-M[i])*t_k, t = linspace(0,
 * blur, S) in f64, casts each to f32 and inverts in f64 exactly as the plain warp does.
 * ts: host [samples] f64 = numpy.linspace(0, blur, samples) supplied by the caller
 * (keeps NumPy's own linspace rounding on the Python side of the boundary).
 * Output frame = sum_k warp_k / float(samples); mask = 1 - coverage_sum/samples,
 * values < 1e-3 -> 0.  mask may be NULL.
 */
int vstab_warp_blur_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w,
                          const double* matrices, const double* ts, int samples, int out_h,
                          int out_w, int interp, const float* border_rgb, int subpix,
                          float* dst, float* mask);

/* Shardable form of vstab_warp_blur_batch ("blur needs the next frame's matrix (replicated JSON) but never
 * another rank's pixels"): src holds frames [clip_first, clip_first + n) of a clip whose motion_meta has clip_total
 * matrices; clip_matrices is the whole host [clip_total,9] f64 table, so the sample delta of a frame at a shard edge
 * uses its true neighbour (M[i+1] - M[i]; the clip's last frame: M[i] - M[i-1], motion_apply.py:129-132).
 * vstab_warp_blur_batch(…, matrices, …) == vstab_warp_blur_clip_batch(…, matrices, n, 0, …). */
int vstab_warp_blur_clip_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w,
                               const double* clip_matrices, int clip_total, int clip_first,
                               const double* ts, int samples, int out_h, int out_w, int interp,
                               const float* border_rgb, int subpix, float* dst, float* mask);

/* ---- A4: the shutter sample matrices themselves (host arithmetic only, no GPU involved) --------
 * nodes/motion_apply.py:125-134 (_blurred_matrix_samples) followed by the float32 cast of motion_apply.py:172, for
 * frames [first, first+count) of a clip of `total` f64 matrices: out host [count, S', 9] f32 with S' = samples, or 1
 * for a single-matrix clip (motion_apply.py:126-127).  This is the routine vstab_warp_blur_*batch runs internally;
 * exported so that the reference-generated golden vectors pin the shipped arithmetic (tests/test_abi_cpu.py). */
int vstab_blur_sample_matrices(const double* matrices, int total, int first, int count,
                               const double* ts, int samples, float* out);

/* ---- F2: grayscale + INTER_AREA downscale to the estimation size ------------
 * Replaces nodes/stabilizer_utils.py:236-242 (_make_gray: cv2.cvtColor RGB2GRAY
 * on f32, clip(gray*255,0,255).astype(uint8)) and :271-276 (cv2.resize INTER_AREA).
 * work_h/work_w == src_h/src_w means "no downscale" (working_size None).
 * frames dev [n,src_h,src_w,3] f32 -> gray dev [n,work_h,work_w] u8.
 */
int vstab_gray_downscale(vstab_ctx* ctx, const float* frames, int n, int src_h, int src_w,
                         int work_h, int work_w, uint8_t* gray);

/* ---- F0 + F2: the same pass with the value-range sniff of the input adaptation folded in ------
 * nodes/stabilizer_utils.py:127-131 decides PER FRAME whether float input is 0..255 (`float(arr.max()) > 1.5` -> /255):
 * one more full read of every frame.  The gray pass reads every sample anyway, so it can report the per-frame maximum
 * (NaN if the frame holds one, as numpy's max) in the same 24.9 MB read: frame_max dev [n] f32.  The caller runs the
 * estimation optimistically on the tensor as given and, in the rare case that a maximum exceeds 1.5, rescales those
 * frames and repeats it (host_math.resolve_value_range).
 * vstab_frame_range: the sniff alone (Motion Apply has no estimation pass), an HBM-bound read of the clip. */
int vstab_gray_downscale_range(vstab_ctx* ctx, const float* frames, int n, int src_h, int src_w,
                               int work_h, int work_w, uint8_t* gray, float* frame_max);
/* The per-frame maxima of the latest vstab_gray_downscale_range call, on the host (n = that call's frame count): the
 * kernel that forms them also writes them into coherent host memory, so this waits for that kernel only -- nothing is
 * copied and no event is recorded on the stream.  The host side of `float(arr.max()) > 1.5` per frame
 * (nodes/stabilizer_utils.py:127-131). */
int vstab_last_frame_peaks(vstab_ctx* ctx, int n, float* out);
int vstab_frame_range(vstab_ctx* ctx, const float* frames, int n, int h, int w, float* frame_max);
/* The rule itself, out of place: out[f] = frames[f] / 255 (IEEE float32 division, numpy's `arr /= 255.0`) where
 * frame_max[f] > 1.5, else a copy.  frames, frame_max, out: dev.  The caller's tensor is never modified. */
int vstab_apply_value_range(vstab_ctx* ctx, const float* frames, int n, int h, int w,
                            const float* frame_max, float* out);

/* ---- F3 (+F4): DIS dense optical flow over consecutive pairs ---------------
 * Replaces cv2.DISOpticalFlow (PRESET_MEDIUM, finestScale 2, patchSize 8,
 * patchStride 4, spatial propagation) created at nodes/video_stabilizer_flow.py:82-86
 * and called at :140, for pairs (i, i+1), i in [0, n-1).
 * gray        dev [n,h,w] u8
 * flow        dev [n-1,h,w,2] f32 or NULL (full field; tests / debugging)
 * grid_flow   dev [n-1,gh,gw,2] f32 or NULL: the flow sampled at y=0,step,.. x=0,step,..
 *             (gh = ceil(h/step), gw = ceil(w/step)) -- the only values the
 *             reference consumes (flow.py:141-147)
 */
int vstab_dis_flow_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w,
                         float* flow, float* grid_flow, int sample_step);

/* OpenCV's DIS object is stateful for tiny images: its first calc() may auto-select patch size / scales
 * (autoSelectPatchSizeAndScales) and keeps the new finest scale for the following calls.  The reference
 * creates one object per clip (flow.py:316), so the first pair of a CLIP can use a different pyramid than
 * the rest.  A rank that processes a later shard of the clip clears this flag (default: 1). */
int vstab_dis_set_clip_start(vstab_ctx* ctx, int first_pair_is_clip_start);

/* ---- F4 + F5: model fit on the sampled flow -------------------------------
 * Replaces nodes/video_stabilizer_flow.py:141-210 for every pair: RANSAC
 * homography (cv2.findHomography 2.5 px / 2000 / 0.992, accept >= 0.15),
 * RANSAC similarity (cv2.estimateAffinePartial2D 2.0 px / 2000 / 0.992, accept
 * >= 0.1) and per-axis median translation.  All candidate models at or below
 * `requested_mode` are evaluated for every pair; the host applies the
 * sequential "sticky active_mode" rule (flow.py:324-339) to pick one.
 * grid_flow dev [pairs,gh,gw,2]; step = sample stride used to build the grid.
 * results host [pairs * 3] records indexed [pair*3 + mode].
 */
typedef struct vstab_fit_record {
    float matrix[9];   /* 3x3 f32 at working resolution */
    double confidence; /* inlier ratio (translation: valid/total), as the reference's Python float */
    double residual;   /* mean |model(p) - q| over all valid samples, both axes */
    int32_t accepted;  /* 1 if this mode's acceptance test passed */
    int32_t computed;  /* 1 if this mode was evaluated */
    int32_t valid_points; /* finite samples (flow.py:150-154) */
    int32_t total_points;
} vstab_fit_record;
int vstab_sample_fit_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw,
                           int step, int requested_mode, vstab_fit_record* results);
/* The same in two halves, so that work can be queued on the stream between the launch and the host's wait:
 * _begin launches the fits and queues the download of the records behind them; vstab_fit_records_device is the
 * device copy of those records ([pairs * 3], valid until the next fit call of this context); _end waits for the
 * download only (not for anything queued after _begin) and hands out the host records. */
int vstab_sample_fit_batch_begin(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw,
                                 int step, int requested_mode);
const vstab_fit_record* vstab_fit_records_device(vstab_ctx* ctx);
int vstab_sample_fit_batch_end(vstab_ctx* ctx, int pairs, vstab_fit_record* results);

/* ---- Estimation mask (not a reference feature): keep moving subjects out of the fit ------------
 * The fit answers "what does the largest coherent set of samples do"; a subject that owns more samples than the
 * background becomes the estimate.  A caller that knows where the subject is (a segmentation MASK per frame, or one
 * mask for a burnt-in logo) names the samples the fit must not use.  The rule:
 *   - a full-resolution pixel is SUBJECT iff its mask value is > 0.5 or is not finite;
 *   - a working pixel (X, Y) is COVERED iff a subject pixel lies in its INTER_AREA footprint
 *     x in [floor(X*src_w/work_w), ceil((X+1)*src_w/work_w)), y likewise (the pixel itself without a downscale);
 *   - grid sample (gx*step, gy*step) of a frame is BLOCKED iff a covered working pixel lies in the square
 *     |dX| <= margin, |dY| <= margin around it, clipped to the image (margin in working pixels, 0..64);
 *   - sample g of pair (i, i+1) is ADMITTED iff it is blocked neither in frame i nor in frame i+1.
 * vstab_mask_block_grid: mask dev [n_masks,src_h,src_w] f32 with n_masks == n_frames, or 1 (one mask for the whole
 * clip: reduced once, written to every frame) -> blocked dev [n_frames,gh,gw] u8 (0 / 1; gh = ceil(work_h/step),
 * gw = ceil(work_w/step)).  Every mask value is read once; asynchronous on the context's stream; timing kind "mask".
 * src_w <= 8192.
 */
int vstab_mask_block_grid(vstab_ctx* ctx, const float* mask, int n_masks, int n_frames, int src_h, int src_w,
                          int work_h, int work_w, int step, int margin, uint8_t* blocked);
/* vstab_sample_fit_batch / _begin on the admitted samples only: blocked dev [pairs+1,gh,gw] u8 (frame i of the clip
 * at row i).  The fit is flow.py:141-210 with prev_points restricted to the admitted grid positions, order kept: same
 * validity filter, same `< 12` rule, same RANSAC sample sequence for that point count; total_points = admitted samples
 * (translation confidence = valid / admitted).  With nothing blocked the records are those of vstab_sample_fit_batch,
 * byte for byte; otherwise matrix, accepted, residual, valid_points and the similarity / perspective confidence are
 * what vstab_sample_fit_batch returns for the same grid with NaN written into the samples that are not admitted.
 * The records of _begin_masked are collected as those of _begin (vstab_fit_records_device, vstab_fit_records_copy,
 * vstab_sample_fit_batch_end). */
int vstab_sample_fit_batch_masked(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw,
                                  int step, int requested_mode, const uint8_t* blocked, vstab_fit_record* results);
int vstab_sample_fit_batch_begin_masked(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw,
                                        int step, int requested_mode, const uint8_t* blocked);

/* ---- Scene cuts (not a reference feature): the motion-compensated residual of every consecutive pair ------------
 * A hard cut is the one pair whose two images no camera move explains.  The score of pair i is the mean absolute
 * difference of its two estimation images AFTER the pair's own transition A_i (x_{i+1} = A_i x_i, the direction the
 * fit reports, flow.py:133-210): frame i is the FROM image, frame i+1 the TO image, and no matrix is inverted.  The rule,
 * for pair i and every pixel p = (x, y) of frame i (x, y as fp64 integers, A = the float32 matrix widened to fp64):
 *   - X = (A0*x + A1*y) + A2,  Y = (A3*x + A4*y) + A5,  W = (A6*x + A7*y) + A8  -- separate IEEE multiplies and adds in
 *     exactly this association, nothing fused;
 *   - W <= 0 or W not finite: the pixel does not count.  Otherwise q = (X / W, Y / W), each coordinate rounded to the
 *     nearest integer, ties to even (rint); a coordinate that is not finite does not count (so a matrix with a non-finite
 *     entry counts nothing);
 *   - q inside frame i+1 (0 <= qx <= w-1 and 0 <= qy <= h-1): inside_i += 1 and sum_abs_i += |gray_i[p] - gray_{i+1}[q]|.
 * Both accumulators are integers, so the result does not depend on the order of the reduction.
 * vstab_pair_residual_batch: gray dev [n,h,w] u8 (n >= 2), transitions host [n-1,9] f32 at working resolution ->
 * sum_abs dev [n-1] u64, inside dev [n-1] u32 (both zeroed by the call).  One streaming pass of about 2*h*w bytes per pair;
 * asynchronous on the context's stream; timing kind "cut".  What is decided from the two numbers (scene_cuts.py):
 * score = sum_abs / inside, overlap = inside / (h*w), a cut iff overlap < 0.25 or score >= the threshold.
 */
int vstab_pair_residual_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const float* transitions,
                              uint64_t* sum_abs, uint32_t* inside);

/* ---- Drift correction (not a reference feature): the normal equations of aligning a frame to its keyframe ----------
 * Consecutive-pair estimates chain their bias; a frame registered directly against a keyframe does not.  One launch forms,
 * for every frame i with an anchor a = anchor[i], the Gauss-Newton sums of the inverse-compositional alignment of the
 * template T = gray[a] to the image I = gray[i] under R_i, the row-major affine 2x3 (fp64) that maps an anchor pixel into
 * frame i.  anchor[i] == -1: the frame's 17 numbers are zero.  For every template pixel (x, y), 1 <= x <= w-2, 1 <= y <= h-2:
 *   1. X = (R0*x + R1*y) + R2,  Y = (R3*x + R4*y) + R5  -- fp64, separate IEEE multiplies and adds in exactly this
 *      association, nothing fused;
 *   2. ix = rint(32 X), iy = rint(32 Y), ties to even;
 *   3. the pixel takes part iff 0 <= ix <= 32 (w-1) and 0 <= iy <= 32 (h-1), compared in fp64 before any conversion (NaN
 *      and inf fail);
 *   4. x0 = ix >> 5, fx = ix & 31, x1 = min(x0 + 1, w-1); y0, fy, y1 likewise;
 *   5. v = (32-fx)(32-fy) I[y0,x0] + fx (32-fy) I[y0,x1] + (32-fx) fy I[y1,x0] + fx fy I[y1,x1]   (an integer, 0..261120);
 *   6. r = v - 1024 T[y,x];
 *   7. |r| > 1024 cap: capped += 1 and nothing else is added (the truncated-L2 guard against moving subjects; cap is an
 *      integer in 0..255 grey levels, and 255 caps nothing);
 *   8. gx = T[y,x+1] - T[y,x-1],  gy = T[y+1,x] - T[y-1,x],  u = 2x - (w-1),  q = 2y - (h-1);
 *   9. J = (gx, gy, gx u + gy q, gy u - gx q)   -- twice the derivative of T along a shift in x, in y, and four times along
 *      a zoom and a rotation about the image centre ((w-1)/2, (h-1)/2);
 *  10. out[i] += [1, 0, |r|, J0 r, J1 r, J2 r, J3 r, J0J0, J0J1, J0J2, J0J3, J1J1, J1J2, J1J3, J2J2, J2J3, J3J3], i.e.
 *      out[i] = [count, capped, sum|r|, b0..b3, H00, H01, H02, H03, H11, H12, H13, H22, H23, H33].
 * Everything summed is an integer, so the result does not depend on the order of the reduction.  max(h, w) <= 1024 is
 * required: then |J2|, |J3| <= 2*255*1023 < 2^19, |r| < 2^18, fewer than 2^20 pixels take part, and no sum reaches 2^59.
 * h < 3 or w < 3: zeros.
 * vstab_anchor_sums_batch: gray dev [n,h,w] u8 (n >= 1), anchor host [n] i32 (-1 or a frame index in 0..n-1), R host
 * [n][6] f64, cap 0..255 -> out dev [n][VSTAB_ANCHOR_SLOTS] i64 (zeroed by the call).  One streaming pass of about 2*h*w
 * bytes per anchored frame; asynchronous on the context's stream; timing kind "anchor".  What is solved from the sums
 * (drift_correction.py): H d' = b / 1024, d = (2 d'0, 2 d'1, 4 d'2, 4 d'3), R <- R W(d)^-1.
 */
#define VSTAB_ANCHOR_SLOTS 17
int vstab_anchor_sums_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const int32_t* anchor,
                            const double* R, int cap, int64_t* out);
/* Exposure-matched, masked form (off by default; drift_exposure / drift_mask).  Auto-exposure changes the brightness between a
 * frame and a keyframe up to a whole spacing away, and a masked subject must not pull the alignment.  The rule is the one
 * above with three changes; steps 1-5 (mapping, Q5 rounding, the inside test, the bilinear integer v) and 8-9 (gx, gy, u, q,
 * J0..J3) are unchanged:
 *   - photometric prediction: every frame carries two host-given i32, G (gain in units of 1/1024, 256..4096) and O (offset
 *     in units of 1/1024 grey level, |O| <= 2^20), and step 6 becomes r = v - (G T[y,x] + O).  G = 1024, O = 0 is the r above.
 *   - mask (blocked != NULL only; blocked is vstab_mask_block_grid's [n,gh,gw] u8 grid of the clip at `step`, gh =
 *     ceil(h/step), gw = ceil(w/step)): tested behind the inside test (step 3) and before the cap (step 7).  With integer
 *     divisions throughout, the pixel is MASKED iff
 *       blocked[a][min((y + step/2) / step, gh-1)][min((x + step/2) / step, gw-1)] != 0   -- the template pixel's nearest
 *       grid sample in the anchor a -- or
 *       blocked[i][min((yn + step/2) / step, gh-1)][min((xn + step/2) / step, gw-1)] != 0 with xn = min((ix + 16) >> 5, w-1),
 *       yn = min((iy + 16) >> 5, h-1)   -- the nearest grid sample of the nearest pixel of the sample position in frame i.
 *     A masked pixel adds 1 to `masked` and nothing else.  A grid sample is blocked iff a covered pixel lies within
 *     mask_margin of it, and a pixel is up to step/2 from its nearest sample per axis: with mask_margin < step / 2 a subject
 *     pixel can lie nearer to an unblocked sample than to a blocked one, and the rule then does not cover every subject pixel.
 *   - cap: |r| > 1024 cap on the compensated r gives capped += 1 and nothing else, as above.
 *   - two more regression columns: J4 = T[y,x] (the gain's) and J5 = 1 (the offset's).
 * out[i] = [count, capped, masked, sum|r|, b0..b5, H00, H01, ..., H55]: b_k = sum J_k r, and H the 21 sums J_j J_k for
 * j <= k, row-major over the upper triangle (H00 H01 H02 H03 H04 H05 H11 H12 ... H45 H55).  Everything summed is an integer,
 * exact in any order.  Bounds: v <= 261120 and |G T + O| <= 4096*255 + 2^20 < 2^21, so r fits 32 bits; every counted pixel
 * has |r| <= 1024*255 < 2^18 by the cap test itself; J4 <= 255 and J5 = 1 are smaller than J0..J3; so with max(h, w) <= 1024
 * the argument above carries over and no sum reaches 2^59.  anchor[i] == -1, h < 3 or w < 3: zeros.
 * vstab_anchor_sums_ex_batch: gray, anchor, R, cap as above; gain, offset host [n] i32 (both required); blocked dev
 * [n,gh,gw] u8 or NULL (step >= 1 is checked either way, gh and gw only with blocked) -> out dev [n][VSTAB_ANCHOR_EX_SLOTS]
 * i64 (zeroed by the call).  Asynchronous on the context's stream; timing kind "anchor_ex".  What is solved from the sums
 * (drift_correction.py): the model I(R p) = g T(W(d) p) + o gives, to first order, v - G T - O = dG T + dO + (G + dG)
 * (J[0..3] . d'), so H theta = b with theta = ((G + dG) d'_0..3, dG, dO), d'_k = theta_k / (G + dG), and d, R as above.
 */
#define VSTAB_ANCHOR_EX_SLOTS 31
int vstab_anchor_sums_ex_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const int32_t* anchor,
                               const double* R, const int32_t* gain, const int32_t* offset, int cap, const uint8_t* blocked,
                               int step, int gh, int gw, int64_t* out);

/* ---- N1 (crop framing): coverage analysis for the keep_fov crop solver ---------
 * Replaces the per-frame cv2 calls of nodes/stabilizer_utils.py:611-643
 * (finalize_with_masks: warpPerspective(ones, NEAREST) > 0.5, dilate 3x3, erode 3x3, bounding box of
 * the remaining content) and :763-787 (_refine_no_padding_crop: AND of the coverage masks of all
 * frames, erode 3x3).  One pass over the n matrices serves both.
 * matrices host [n,9] f32 (source -> output);  source src_h x src_w, output out_h x out_w.
 * bbox     host [n,4] i32: x_min, y_min, x_max, y_max of the closed coverage, or -1,-1,-1,-1 if empty
 * common   host [out_h*out_w] u8: 1 where every frame covers the pixel, after the 3x3 erosion
 *          (pixels outside the image do not constrain the erosion, as cv2.erode's default border)
 */
int vstab_crop_analysis(vstab_ctx* ctx, const float* matrices, int n, int src_h, int src_w,
                        int out_h, int out_w, int32_t* bbox, uint8_t* common);

/* Motion Apply's crop framing (nodes/motion_apply.py:205-227, _common_valid_mask): AND over all frames of
 * warpPerspective(ones, M, INTER_NEAREST) > 0.5 -- no morphology, no bounding boxes.
 * matrices host [n,9] f32;  common host [out_h*out_w] u8 (1 = covered by every frame). */
int vstab_common_coverage(vstab_ctx* ctx, const float* matrices, int n, int src_h, int src_w,
                          int out_h, int out_w, uint8_t* common);

/* ---- N1 (Classic estimator): sparse features + pyramidal LK ------------------
 * Replaces nodes/video_stabilizer_classic.py:76-96 (`_estimate_motion_pair`) for a whole clip.
 *
 * vstab_gftt_batch: cv2.goodFeaturesToTrack(gray, maxCorners, qualityLevel, minDistance, blockSize)
 * (classic.py:76-83: 400 / 0.01 / 7 / 21; no mask, min-eigenvalue score, 3x3 Sobel) on every frame.
 *   gray    dev [n,h,w] u8
 *   corners dev [n,max_corners,2] f32 (x, y), strongest first;  counts dev [n] i32
 *
 * vstab_lk_track_batch: cv2.calcOpticalFlowPyrLK(frame i, frame i+1, corners of frame i, None,
 * winSize=(win,win), maxLevel, criteria=(EPS|COUNT, max_count, epsilon)) (classic.py:88-96: 31 / 3 /
 * 50 / 0.01) for the n-1 consecutive pairs of the clip.
 *   points      dev [n-1,max_points,2] f32, counts dev [n-1] i32 (rows of vstab_gftt_batch's output)
 *   point_pairs dev [n-1,max_points,4] f32: prev.x, prev.y, next.x, next.y; next = NaN where the
 *               tracker's status is 0 -- the input layout of vstab_points_fit_batch
 *   next_points dev [n-1,max_points,2] f32 or NULL (raw tracker output, also for status 0)
 *   status      dev [n-1,max_points] u8 or NULL
 * vstab_lk_levels: number of pyramid levels above level 0 that buildOpticalFlowPyramid keeps.
 *
 * vstab_points_fit_batch: the model-fit cascade of classic.py:98-160 on the tracked pairs: fewer
 * than 12 features or fewer than 8 tracked points -> no candidate; otherwise the same three
 * estimators as vstab_sample_fit_batch (translation confidence = tracked / features).
 *   results host [pairs*3] records indexed [pair*3 + mode] (residual is filled but unused by Classic)
 */
int vstab_gftt_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, int max_corners,
                     double quality, double min_distance, int block_size, float* corners, int* counts);
int vstab_lk_levels(int h, int w, int win, int max_level);
int vstab_lk_track_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const float* points,
                         const int* counts, int max_points, int win, int max_level, int max_count,
                         double epsilon, float* point_pairs, float* next_points, uint8_t* status);
int vstab_points_fit_batch(vstab_ctx* ctx, const float* point_pairs, const int* counts, int pairs,
                           int max_points, int requested_mode, vstab_fit_record* results);

/* ---- N2 (fallback estimator): phase correlation -------------------------------------
 * Replaces cv2.phaseCorrelate(prev_gray.astype(float32), curr_gray.astype(float32)) of
 * nodes/video_stabilizer_flow.py:110-130 (`_estimate_motion_phase_correlate`, the branch of the pair loop
 * flow.py:325-330 taken when no dense-flow backend could be created, flow.py:90-107) for the n-1 consecutive
 * pairs of a clip: zero-pad to the optimal DFT size, normalised cross-power spectrum, inverse DFT, first
 * maximum of the centred correlation surface, 5x5 weighted centroid.
 *   gray    dev [n,h,w] u8 (estimation images; padded sizes up to 2048)
 *   results host [pairs*3] records indexed [pair*3 + mode], or NULL: only the translation row is
 *           computed/accepted (matrix = [1 0 tx; 0 1 ty; 0 0 1], confidence = response, residual 0; a
 *           non-finite result becomes tx = ty = confidence = 0 as flow.py:115-120 does) -- the reference reports
 *           every pair of this estimator as "translation" whatever mode was requested
 *   shifts  host [pairs*3] f64 (tx, ty, response) as cv2.phaseCorrelate returns them, or NULL
 * Synchronises with the host (results are host values).  Timing kind: "phase".
 */
int vstab_phase_correlate_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w,
                                vstab_fit_record* results, double* shifts);

/* ---- N2 (second dense estimator): Dual TV-L1 optical flow ------------------------------------
 * Replaces cv2.optflow.DualTVL1OpticalFlow_create() (nodes/video_stabilizer_flow.py:76-80, the backend
 * _select_flow_backend tries after DIS, :90-107) and its calc(prev, curr, None) in the pair loop (:140) for the
 * pairs (i, i+1), i in [0, n-1).  Restated from OpenCV 4.x contrib optflow/src/tvl1flow.cpp in
 * tests/tvl1_restatement.py (unpinned against OpenCV); the HIP kernels follow it bit for bit.  The error sum of
 * each inner iteration is a stated deviation: a pairwise tree in double over each row, then over the rows.
 * The fields of vstab_tvl1_params are OpenCV's, with its defaults (vstab_tvl1_default_params):
 *   tau 0.25, lambda 0.15, theta 0.3, epsilon 0.01, scale_step 0.8, gamma 0, nscales 5, warps 5,
 *   inner_iterations 30, outer_iterations 10, median_filtering 5, use_initial_flow 0.
 * gamma != 0 and use_initial_flow != 0 are rejected (the reference uses neither); median_filtering is 1 (off) or 5.
 * chunk_pairs: pairs per workspace chunk (0: as many as fit ~4 GB; results do not depend on it).
 * poll_interval: inner launches between two reads of the host-mirrored active count (0: 8).
 *   gray        dev [n,h,w] u8, 16 <= h, w <= 2048 (the finest level; coarser levels below 16 end the pyramid)
 *   flow        dev [n-1,h,w,2] f32 or NULL (full field)
 *   grid_flow   dev [n-1,gh,gw,2] f32 or NULL: the flow at y=0,step,.. x=0,step,.. (as vstab_dis_flow_batch)
 *   iterations  dev [n-1,nscales,warps] int32 or NULL: inner iterations run at each (scale, warp), scale 0 = finest
 *               (0 for the scales the pyramid does not reach)
 * Asynchronous apart from a bounded host wait every poll_interval inner launches.  Timing kind: "tvl1".
 */
typedef struct vstab_tvl1_params {
    double tau, lambda, theta, epsilon, scale_step, gamma;
    int nscales, warps, inner_iterations, outer_iterations, median_filtering, use_initial_flow;
    int chunk_pairs, poll_interval;
} vstab_tvl1_params;
void vstab_tvl1_default_params(vstab_tvl1_params* params);
/* params NULL: the defaults */
int vstab_tvl1_flow_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, const vstab_tvl1_params* params,
                          float* flow, float* grid_flow, int sample_step, int32_t* iterations);

/* ---- F7 + F8: trajectory (prefix sum, box smoothing, strength blend), fp64 ---
 * Replaces nodes/video_stabilizer_flow.py:356-371 and
 * nodes/stabilizer_utils.py:361-383 (_smooth_path: moving average, edge padded,
 * window from fps).  deltas host [n-1,p]; path/target host [n,p]; any p >= 1 (the columns are independent: the mesh
 * warp sends its 2 * mw * mh vertex-path columns through the same call).
 * Host arithmetic since round 4 (a few thousand doubles; ctx is not used): the same operation order as the
 * device plan below, so the two agree bit for bit on equal deltas.
 */
int vstab_trajectory(vstab_ctx* ctx, const double* deltas, int n, int p, double smooth,
                     double fps, double strength, int camera_lock, double* path,
                     double* target);

/* ---- F6-F12 on the device, speculatively: fit records -> the warp's transform table, no host round trip ----
 * Replaces the stretch of nodes/video_stabilizer_flow.py:324-371 and :472-521 between the last model fit and the first
 * warp for framing_mode "crop_and_pad" / "expand" (any of the three models): sticky active_mode walk, rescale to full
 * resolution, parameter deltas of the requested model, path / _smooth_path / strength blend, _params_to_matrix,
 * _compute_bounding_boxes, the common region, the recentring shift and final = T @ M (float32), inverted as
 * cv2.warpPerspective inverts it.  One kernel on the context's stream.
 *   d_records  dev [pairs*3] (vstab_fit_records_device, or a gathered table of the whole clip)
 *   up, down   as for vstab_transitions_to_params (NULL: estimated at full size)
 * The plan stays on the device for vstab_warp_batch_planned; its float32 final matrices, path, target and the common
 * region (x0, y0, x1, y1) are downloaded behind the kernel and handed out by vstab_flow_plan_result (waits for that
 * download only).  The device forms atan2 / log / exp / cos / sin with its own fp64 library, the reference with the host's
 * libm (a perspective plan has no such call, but its final = T @ M holds sums of two inexact float32 terms, which NumPy's matmul
 * may or may not fuse): the caller computes the plan on the host as well (vstab_transitions_to_params ... vstab_bounding_boxes),
 * compares the final matrices bit for bit and warps a frame again where they differ -- see flow_pipeline.py. */
/* Optional, before vstab_flow_plan_device: the planned warp's padded-pixel count array (dev [n] u32); the plan kernel zeroes
 * it, and vstab_warp_batch_planned with the same pointer skips its own fill -- one launch less between plan and warp. */
int vstab_flow_plan_zero_counts(vstab_ctx* ctx, uint32_t* pad_count, int n);
/* framing (last argument of vstab_flow_plan_device): 0 = crop_and_pad -- `region` = the frames' common region, the matrices are
 * recentred on it (flow.py:500-529); 1 = expand -- `region` = the frames' union x_min, y_min, x_max, y_max, the matrices are
 * shifted by (-x_min, -y_min) (stabilizer_utils.py:386-406); the caller forms the canvas size ceil(x_max - x_min) x
 * ceil(y_max - y_min) from vstab_flow_plan_result's region before it queues the warp. */
int vstab_flow_plan_device(vstab_ctx* ctx, const vstab_fit_record* d_records, int pairs, int requested_mode,
                           const double* up, const double* down, double smooth, double fps, double strength,
                           int camera_lock, int width, int height, int segments, const int* seg_pairs, int seg_rows, int framing);
/* segments = 0: d_records is [pairs*3].  segments = world > 0 (multi-GPU): d_records is the receive buffer of the ranks'
 * all-gather as RCCL leaves it -- one block of seg_rows pairs per rank, of which the first seg_pairs[r] are valid -- so the
 * gathered table feeds the plan where it lands (no compaction pass, no host copy before the warp). */
/* Copies the records of the last vstab_sample_fit_batch_begin (device) to dst (device, >= pairs*3 records), stream-ordered:
 * how a rank places its records in its all-gather send buffer. */
int vstab_fit_records_copy(vstab_ctx* ctx, void* dst_dev, int pairs);
int vstab_flow_plan_result(vstab_ctx* ctx, int frames, float* final32, double* path, double* target, double* region);
/* vstab_warp_batch for frames [first, first + n) of the clip planned by the last vstab_flow_plan_device of this context
 * (src: those n frames). */
int vstab_warp_batch_planned(vstab_ctx* ctx, const float* src, int first, int n, int src_h, int src_w, int out_h,
                             int out_w, int interp, const float* border_rgb, int subpix, float* dst, float* mask,
                             uint32_t* pad_count);
/* The per-frame padded-pixel counts of the latest vstab_warp_batch / vstab_warp_batch_planned call that was given a
 * pad_count array, on the host (n = that call's frame count): a one-workgroup kernel behind the warp mirrors them into
 * coherent host memory, this call waits for it -- the host side of `mask.mean()` per frame (video_stabilizer_flow.py:583-588)
 * without a copy or a stream synchronisation of the caller's. */
int vstab_last_pad_counts(vstab_ctx* ctx, int n, uint32_t* out);

/* ---- temporal fill: padding pixels taken from neighbouring frames (beyond the reference, off by default) ----
 * After a warp, an output pixel with mask == 1.0f saw no content of its own frame.  Per output pixel of frame first + f:
 *   - mask != 1.0f: pixel, mask and every other output are left untouched (nothing is stored).
 *   - otherwise the candidates k = 0 .. K-1 are walked in order.  A candidate with cand_frame == -1, or whose float32 matrix
 *     has a zero / non-finite fp64 determinant or inverse (cv::invert would refuse it), is skipped.  Candidate k is VALID at
 *     the pixel iff the source coordinate -- computed exactly as vstab_warp_batch computes it for that matrix (float32
 *     forward matrix inverted in fp64, fp64 coordinate terms per OpenCV column block, 1/32-px rounding, or the float32
 *     coordinates of VSTAB_SUBPIX_EXACT) -- has every interpolation tap inside the source frame:
 *     bilinear 0 <= sx < src_w-1 && 0 <= sy < src_h-1, bicubic 1 <= sx < src_w-2 && 1 <= sy < src_h-2 (sx, sy the integer
 *     parts).  No border colour can enter a filled pixel.
 *   - the first valid candidate wins: dst = the bits vstab_warp_batch(src[cand_frame], that matrix) writes at that pixel,
 *     mask = 0, filled_from = k.  No valid candidate: untouched, filled_from = -1.
 * src         dev  [clip_frames, src_h, src_w, 3] f32: the whole clip (must not alias dst)
 * first, n    output frames [first, first + n) of the clip; matrices / cand_frame / dst / mask / outputs hold those n frames
 * matrices    host [n, K, 9] f32 FORWARD (source frame cand_frame[f][k] -> output canvas of frame first + f)
 * cand_frame  host [n, K] i32 clip frame index, -1 = no candidate;  K in 1..64
 * dst, mask   dev  [n, out_h, out_w, 3] / [n, out_h, out_w] f32, in and out
 * filled_from dev  [n, out_h, out_w] i8 or NULL;  fill_count / pad_count dev [n] u32 or NULL: pixels filled per frame /
 *             pixels whose mask is still 1.0f afterwards.  Timing kind "fill". */
int vstab_temporal_fill_batch(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                              const float* matrices, const int32_t* cand_frame, int K, int out_h, int out_w, int interp,
                              int subpix, float* dst, float* mask, int8_t* filled_from, uint32_t* fill_count,
                              uint32_t* pad_count);

/* ---- blended temporal fill: exposure-matched candidates and a feathered seam (beyond the reference, off by default) ----
 * vstab_temporal_fill_batch writes a hard cut: the raw value of a neighbour frame next to the frame's own content.  The two
 * entries below take the same candidates (matrices, cand_frame: as above, and skipped as above) plus the frame's OWN forward
 * matrix (own_matrices host [n, 9] f32, source frame first + f -> its output canvas; "usable" = a candidate's matrix test).
 * Both are VSTAB_SUBPIX_Q5 only (VSTAB_SUBPIX_EXACT is refused), bilinear and bicubic.  "Q5 coordinate" = the integers X, Y
 * (1/32 px) that vstab_warp_batch forms for a matrix at an output pixel; "inside" = the interior rule above on X >> 5, Y >> 5.
 *
 * vstab_fill_gain_sums -- per output frame f and candidate k, over the lattice of output pixels with
 * x % VSTAB_FILL_GAIN_STRIDE == VSTAB_FILL_GAIN_STRIDE / 2 && y % VSTAB_FILL_GAIN_STRIDE == VSTAB_FILL_GAIN_STRIDE / 2:
 *   - a lattice pixel COUNTS for (f, k) iff its Q5 coordinate under the own matrix is inside AND its Q5 coordinate under
 *     candidate k is inside.  A skipped candidate counts nothing; a non-usable own matrix counts nothing for the frame.
 *   - own value = dst[f, y, x, c] as the warp left it; candidate value = the sample vstab_temporal_fill_batch would write
 *     for that candidate.  q(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0 (a NaN gives 0).
 *   - sums[f, k] = { count, sum q(own r), q(own g), q(own b), sum q(cand r), q(cand g), q(cand b) }: integer sums, the same
 *     whatever the order of addition.  The call zeroes them itself.  It only reads dst: queue it in front of the fill.
 * dst   dev [n, out_h, out_w, 3] f32 (read only);  sums dev [n, K, 7] u64.  Timing kind "fill_gain".
 * The gain the host forms from them (temporal_fill.gains_from_sums) relates candidate and frame over their own overlap, so
 * nothing accumulates along a chain.  The stride of 8 is a choice (1/64 of the pixels: thousands of samples at 1080p), not a
 * calibration. */
#define VSTAB_FILL_GAIN_STRIDE 8
int vstab_fill_gain_sums(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                         const float* matrices, const int32_t* cand_frame, int K, const float* own_matrices, int out_h,
                         int out_w, int interp, int subpix, const float* dst, uint64_t* sums);

/* vstab_temporal_fill_blend_batch -- per output pixel, with Fe = 32 * feather_px:
 *   - mask == 1.0f (padded): the candidates are walked exactly as vstab_temporal_fill_batch walks them.  The first valid
 *     candidate k with sample s writes dst_c = gains[f, k, c] * s_c (one float32 multiply; nothing of the old pixel is read,
 *     so a NaN in the padding cannot leak), mask = 0, filled_from = k, and counts in fill_count.  None valid: untouched.
 *   - mask != 1.0f (own), only with feather_px > 0 and a usable own matrix: with X, Y the Q5 coordinate under the own matrix,
 *     d32 = the distance to the tap-interior border, formed without 32-bit overflow:
 *       bilinear  d32 = min(X, Y, 32 * (src_w - 1) - X, 32 * (src_h - 1) - Y)
 *       bicubic   d32 = min(X - 32, Y - 32, 32 * (src_w - 2) - X, 32 * (src_h - 2) - Y)
 *     and w = (float)min(max(d32, 0), Fe) / (float)Fe.  w == 1.0f: untouched, nothing is stored.  Otherwise the candidates
 *     are walked as for a padded pixel; the first valid one gives c_c = gains[f, k, c] * s_c and
 *       dst_c = (w == 0) ? c_c : own_c * w + c_c * (1.0f - w)     (float32, separate roundings, nothing fused)
 *     with own_c the pixel's value before the call; the mask stays as it is, filled_from = k, and the pixel counts in
 *     blend_count.  None valid: untouched.  So the ring of own pixels the padding colour was interpolated into (d32 <= 0,
 *     mask 0) is replaced by neighbour content, and the seam fades over feather_px source pixels.
 *   - feather_px == 0 and every gain == 1.0f: dst, mask, filled_from, fill_count and pad_count are those of
 *     vstab_temporal_fill_batch, bit for bit, and blend_count is 0.
 * gains       host [n, K, 3] f32;  feather_px in 0..VSTAB_FILL_FEATHER_MAX
 * blend_count dev  [n] u32 or NULL;  pad_count: the pixels whose mask is still 1.0f afterwards, as above.
 * filled_from is -1 where a pixel was neither filled nor blended.  Timing kind "fill_blend". */
#define VSTAB_FILL_FEATHER_MAX 64
int vstab_temporal_fill_blend_batch(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                                    const float* matrices, const int32_t* cand_frame, int K, const float* own_matrices,
                                    const float* gains, int feather_px, int out_h, int out_w, int interp, int subpix,
                                    float* dst, float* mask, int8_t* filled_from, uint32_t* fill_count, uint32_t* pad_count,
                                    uint32_t* blend_count);

/* ---- mesh warp (not a reference feature, off by default): the residual motion one global fit leaves ------------
 * One matrix per frame cannot express parallax, rolling-shutter skew or lens breathing.  What it leaves is measured on a
 * coarse mesh of mw x mh vertices (MeshFlow, Liu et al., ECCV 2016: per-vertex motion profiles) and taken out by a second,
 * per-vertex displacement inside the warp.
 *
 * vstab_mesh_residual_batch -- the rule, for pair i (frames i, i+1; x_{i+1} = A_i x_i) of a work_w x work_h estimation image:
 *   - vertex (a, b), a in 0..mw-1, b in 0..mh-1, sits at vx = (double)a * (work_w - 1) / (mw - 1), vy = (double)b * (work_h - 1)
 *     / (mh - 1) (fp64: the multiply, then the divide); a cell is cw = (double)(work_w - 1) / (mw - 1) wide and
 *     ch = (double)(work_h - 1) / (mh - 1) high.
 *   - grid sample (gx, gy) sits at (x, y) = (gx*step, gy*step) and has flow (u, v).  With A = the float32 matrix widened to
 *     fp64 and x, y as fp64 integers: X = (A0*x + A1*y) + A2, Y = (A3*x + A4*y) + A5, W = (A6*x + A7*y) + A8 (separate IEEE
 *     multiplies and adds in this association, nothing fused), and the residual is
 *     r = ( (float)((x + (double)u) - X / W), (float)((y + (double)v) - Y / W) ); it lives at (x, y) of frame i.
 *   - the sample is ADMITTED to vertex (a, b) iff u, v and both components of r are finite, it is blocked neither in frame i
 *     nor in frame i+1 (the estimation mask's pair rule; blocked == NULL: nothing is), and |x - vx| < cw and |y - vy| < ch
 *     (fp64, strict): the samples inside the four cells that touch the vertex, MeshFlow's neighbourhood.
 *   - count = the number of admitted samples.  count >= VSTAB_MESH_MIN_SAMPLES: the vertex value is, per axis, the median
 *     of the admitted residuals as numpy.median gives it on float32: the middle element of the sorted values for an odd
 *     count, (lo + hi) / 2 in float32 of the two middle elements for an even one.  Fewer: residual (0, 0), true count.
 * A median does not depend on the order of its inputs, so the result equals the NumPy restatement exactly.
 *   grid_flow   dev  [pairs, gh, gw, 2] f32, gh = ceil(work_h/step), gw = ceil(work_w/step)
 *   transitions host [pairs, 9] f32, working resolution: the matrices the plan used (after the sticky-mode selection)
 *   blocked     dev  [pairs+1, gh, gw] u8 (vstab_mask_block_grid) or NULL
 *   residual    dev  [pairs, mh, mw, 2] f32;  count dev [pairs, mh, mw] i32
 * 2 <= mw, mh <= 65; work_w, work_h >= 2.  One workgroup per (pair, vertex), rank counting in LDS; a neighbourhood of
 * more than 16384 grid positions is refused.  Asynchronous on the context's stream; timing kind "mesh_residual".
 */
#define VSTAB_MESH_MIN_SAMPLES 4
int vstab_mesh_residual_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h,
                              int work_w, const float* transitions, const uint8_t* blocked, int mw, int mh,
                              float* residual, int32_t* count);
/* vstab_mesh_warp_batch -- vstab_warp_batch (bilinear) with a per-vertex displacement of the SOURCE frame: the content at
 * source position x is moved to x + c(x) before the frame's matrix is applied.  The rule, per output pixel (x, y):
 *   - Xn, Yn, W (fp64 coordinate terms per OpenCV column block) and Wn = 1/W, Wq = 32 * Wn (affine: the two constants of the
 *     frame) are formed exactly as vstab_warp_batch forms them from the float32 forward matrix inverted in fp64.
 *   - q = (Xn*Wn, Yn*Wn) is the unrounded source coordinate.  For the lookup only, each coordinate is clamped to the frame:
 *     t = (q > 0) ? q : 0 (a NaN becomes 0), t = (t < S-1) ? t : S-1 with S = src_w / src_h.  Vertex (a, b) sits at
 *     (a*(src_w-1)/(mw-1), b*(src_h-1)/(mh-1)); g = t * (double)(m-1) / (double)(S-1) (multiply, then divide),
 *     i = min((int)g, m-2), f = g - i with m = mw / mh -> cell (ia, ib), fractions (fa, fb).  With c00 = offsets[ib][ia],
 *     c10 = offsets[ib][ia+1], c01 = offsets[ib+1][ia], c11 = offsets[ib+1][ia+1] widened to fp64, per axis:
 *     c = (c00*(1-fa) + c10*fa) * (1-fb) + (c01*(1-fa) + c11*fa) * fb -- IEEE fp64, this association, nothing fused.
 *   - s = q - c(q), a one-step inverse of the forward map x -> x + c(x): exact for a constant c, otherwise an approximation
 *     whose error is of order |c| * |grad c|.  It enters the plain warp's three roundings as
 *       1/32-px coordinate:  cvRound(Xn*Wq - 32.0*cx), cvRound(Yn*Wq - 32.0*cy)   (VSTAB_SUBPIX_Q5)
 *       float32 coordinate:  (float)((double)fsx - cx), (float)((double)fsy - cy)  (VSTAB_SUBPIX_EXACT; fsx, fsy the plain
 *                            warp's float32 chain)
 *       nearest (mask):      cvRound(Xn*Wn - cx), cvRound(Yn*Wn - cy)
 *     and everything behind them is vstab_warp_batch's: INT clamp and short saturation, taps, border colour, the mask rule,
 *     pad_count.
 * Invariant: all-zero offsets give dst, mask and pad_count bit-identical to vstab_warp_batch (c = +0.0, and v - 0.0 == v).
 *   offsets dev [n, mh, mw, 2] f32 (x, y), full-resolution px;  2 <= mw, mh <= 65;  src_w, src_h >= 2.
 * The other arguments are vstab_warp_batch's, interp fixed to bilinear, and are checked as vstab_warp_batch checks them
 * (same error texts under this function's name); a 1-px source and a vertex count out of range are refused in front of the
 * launch with texts of their own.  Each workgroup stages its frame's vertex table in
 * LDS; apart from that it is the same HBM stream as the plain warp (same tile, same XCD remap).  Timing kind "mesh_warp". */
int vstab_mesh_warp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                          int out_h, int out_w, const float* border_rgb, int subpix, const float* offsets, int mw, int mh,
                          float* dst, float* mask, uint32_t* pad_count);
/* vstab_mesh_unwarp_batch -- the inverse of vstab_mesh_warp_batch's displacement: vstab_warp_batch (bilinear) whose OUTPUT
 * pixel is moved by the inverse of the mesh displacement before the frame's matrix is applied.  The mesh lies over the output
 * canvas, out_w x out_h: the source canvas of the forward mesh warp being undone.  That warp sampled its source at
 * s = g(q) = q - c(q); restoring needs q = g^-1(p) = p + c(q), which has no closed form on a bilinear vertex table.  The rule,
 * per output pixel (x, y):
 *   - fixed point: q_0 = (x, y) as fp64 integers.  Step k = 0, 1, ...: c_k = c(q_k), vstab_mesh_warp_batch's lookup unchanged
 *     (clamp, cell, fraction, bilinear association) with S = out_w / out_h; q_{k+1} = (x + c_k.x, y + c_k.y).  The step is the
 *     last one if |q_{k+1}.x - q_k.x| <= VSTAB_MESH_UNWARP_TOL and |q_{k+1}.y - q_k.y| <= VSTAB_MESH_UNWARP_TOL (two fp64
 *     subtractions; a NaN does not meet the test), or if it is step number VSTAB_MESH_UNWARP_MAX_STEPS.  e = c of the last
 *     step taken.  A pixel whose last step did not meet the test is UNCONVERGED; it uses e all the same.
 *     2^-7 is a quarter of the 1/32-px coordinate step: for a field with Lipschitz constant L <= 1/2 the remaining error is
 *     L/(1-L) * 2^-7 <= 2^-7, below half a Q5 step.  A smooth field stops within 3 steps; independent vertex offsets of
 *     full amplitude are not a contraction everywhere, which is why the limit and the count exist.
 *   - Xn, Yn, W are formed exactly as vstab_warp_batch forms them (float32 forward matrix inverted in fp64 to m, OpenCV
 *     column-block terms).  If e.x == 0 and e.y == 0 (zeros of either sign) NOTHING is added: Xd = Xn, Yd = Yn, Wd = W and the
 *     float32 chain is the plain warp's, which settles every sign-of-zero corner in favour of the invariant below.
 *     Otherwise Xd = Xn + (m0*e.x + m1*e.y), Yd = Yn + (m3*e.x + m4*e.y), Wd = W + (m6*e.x + m7*e.y) -- separate IEEE fp64
 *     operations in this association, nothing fused.  For an affine m (m6 == m7 == 0) the frame's constants Wn / Wq are
 *     used as they are and Wd is not formed; otherwise Wn = (Wd != 0) ? 1/Wd : 0, Wq = 32 * Wn.
 *   - Xd, Yd, Wd enter the three roundings in place of Xn, Yn, W:
 *       1/32-px coordinate:  cvRound(Xd*Wq), cvRound(Yd*Wq)                          (VSTAB_SUBPIX_Q5)
 *       float32 coordinate:  with the plain warp's float32 numerators nx, ny and denominator w (a moved pixel only):
 *                            nx += (float)(m0*e.x + m1*e.y), ny += (float)(m3*e.x + m4*e.y), w += (float)(m6*e.x + m7*e.y)
 *                            (the fp64 sums above, rounded to float32; w also for an affine m), then fsx = nx / w,
 *                            fsy = ny / w                                             (VSTAB_SUBPIX_EXACT)
 *       nearest (mask):      cvRound(Xd*Wn), cvRound(Yd*Wn)
 *     and everything behind them is vstab_warp_batch's.
 * Invariant: all-zero offsets give dst, mask and pad_count bit-identical to vstab_warp_batch, and unconverged == 0.
 *   offsets dev [n, mh, mw, 2] f32 (x, y), px of the output canvas;  2 <= mw, mh <= 65;  out_w, out_h >= 2.
 *   unconverged dev [n] u32 or NULL: unconverged pixels per frame.
 * The other arguments are vstab_mesh_warp_batch's and are checked as it checks them (same error texts under this function's
 * name; the 2x2 minimum applies to the output, where the mesh lies).  Same tile, XCD remap and LDS staging of the vertex
 * table as the forward kernel; the iteration is a bounded per-lane loop.  Timing kind "mesh_unwarp". */
#define VSTAB_MESH_UNWARP_TOL 0.0078125      /* 2^-7 px */
#define VSTAB_MESH_UNWARP_MAX_STEPS 8
int vstab_mesh_unwarp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                            int out_h, int out_w, const float* border_rgb, int subpix, const float* offsets, int mw, int mh,
                            float* dst, float* mask, uint32_t* pad_count, uint32_t* unconverged);

/* ---- rolling shutter (not a reference feature, off by default): the per-row readout correction of the final warp ----
 * A sensor read out row by row over the fraction rho of the frame interval (the READOUT; negative: bottom to top) shows a
 * point that a global shutter would show at q at s = q + tau(s_y) * v(q) instead, tau(y) = rho * (y/(H-1) - 1/2) in frame
 * intervals and v(q) = V * (q_x, q_y, 1) the image velocity in px per frame interval, a 2x3 V per frame (rolling_shutter.py
 * forms it from the transitions).  The equation is linear in s_y: tau = rho*(q_y/(H-1) - 1/2) / (1 - rho*v_y/(H-1)).
 *
 * vstab_rolling_warp_batch -- vstab_warp_batch (bilinear) that samples the source at s instead of q: vstab_mesh_warp_batch's
 * rule with another displacement c = -tau * v in s = q - c(q).  Xn, Yn, W, Wn, Wq, q = (qx, qy) = (Xn*Wn, Yn*Wn), the three
 * roundings c enters and everything behind them are stated there.  c, with H = src_h, V = the frame's six coefficients and
 * rho = readout -- every operation IEEE fp64 and rounded on its own, nothing fused:
 *   - yc = (qy > 0) ? qy : 0 (a NaN becomes 0), yc = (yc < H-1) ? yc : H-1
 *   - vx = (V0*qx + V1*qy) + V2, vy = (V3*qx + V4*qy) + V5
 *   - D = 1 - (rho*vy) / (H-1); if D >= 0.5 does not hold (a NaN included), D = 0.5: a row velocity that would fold the
 *     readout over itself is not believed
 *   - tau = (rho * (yc/(H-1) - 0.5)) / D
 *   - cx = -(tau*vx), cy = -(tau*vy); if either is not finite, both are 0.
 * Invariant: all-zero velocity or readout == 0 give dst, mask and pad_count bit-identical to vstab_warp_batch (c is a zero,
 * and v - c == v for every v that is not a zero of c's sign, which rounds and samples as its counterpart does).
 *   velocity host [n, 6] f64 (V0..V5), full-resolution px per frame interval, staged with the transform records
 *   readout  in [-1, 1]; src_h >= 2
 * The other arguments are vstab_warp_batch's, interp fixed to bilinear, and are checked as vstab_warp_batch checks them (same
 * error texts under this function's name).  Kernel (vstab_rolling.hip): the plain warp's 64 x 8 tile and XCD remap; the
 * frame's coefficients and the readout are uniform, there is no table in LDS.  Timing kind "rolling_warp".
 *
 * vstab_rolling_unwarp_batch -- the inverse of vstab_rolling_warp_batch's displacement: vstab_warp_batch (bilinear) whose OUTPUT
 * pixel is moved in front of the frame's matrix, vstab_mesh_unwarp_batch's rule with a closed form in place of the fixed point.
 * The forward warp sampled its source at s = q + tau(s_y) * v(q).  Restoring, the output pixel is s itself, so tau is known
 * from the output row, and with v(q) = L q + t the equation (I + tau*L) q = s - tau*t is a 2x2 solve:
 * e = q - s = -tau * (I + tau*L)^-1 * v(s).  With (x, y) the output pixel as fp64 integers, hm1 = out_h - 1, V = the frame's
 * six coefficients and rho = readout -- every operation IEEE fp64 and rounded on its own, nothing fused:
 *   - tau = rho * (y / hm1 - 0.5)
 *   - a = 1 + tau*V0, b = tau*V1, c = tau*V3, d = 1 + tau*V4;  det = a*d - b*c
 *   - vx = (V0*x + V1*y) + V2, vy = (V3*x + V4*y) + V5;  rx = tau*vx, ry = tau*vy
 *   - e.x = -((d*rx - b*ry) / det), e.y = -((a*ry - c*rx) / det)
 *   - if det >= VSTAB_ROLLING_UNWARP_MIN_DET does not hold (a NaN included) or e.x or e.y is not finite, e = (0, 0) and the
 *     pixel is UNSOLVED: it is warped by the matrix alone.  0.25 is a choice, not a calibration, the counterpart of the
 *     forward warp's D >= 0.5: a row whose (I + tau*L) has lost three quarters of its area is one the forward warp folded.
 *   - e enters Xn, Yn, W and the float32 chain exactly as vstab_mesh_unwarp_batch's e does (e == 0, zeros of either sign: nothing
 *     is added), and everything behind them is vstab_warp_batch's.
 * Invariant: all-zero velocity or readout == 0 give dst, mask and pad_count bit-identical to vstab_warp_batch and unsolved == 0
 * (tau*v is a zero of either sign, and so is e).
 * Region of validity: the pair is an exact inverse (up to the roundings of two samplings) only where neither of the forward
 * warp's two clamps binds -- D >= 0.5, and q_y inside [0, H-1].  Where the forward warp clamped, it did not sample at
 * s = q + tau(s_y) v(q), and this function undoes a displacement that was not applied.  The lever of the forward warp is its
 * SOURCE's height; here it is the OUTPUT's: the canvas being restored.
 *   velocity host [n, 6] f64, readout in [-1, 1]: as for vstab_rolling_warp_batch;  out_h >= 2
 *   unsolved dev [n] u32 or NULL: unsolved pixels per frame, zeroed by the call as pad_count is.
 * The other arguments are vstab_rolling_warp_batch's and are checked as it checks them (same error texts under this function's
 * name; the 2-row minimum applies to the output).  The same kernel template as the forward warp with another displacement
 * functor; tau, a..d and det depend on the row only and are shared by a thread's pixels.  Timing kind "rolling_unwarp".
 *
 * vstab_row_residual_batch -- what the readout is estimated from: per pair i and grid row gy, the per-axis median of the
 * global fit's residual over the row's admitted samples.  A rolling shutter leaves a residual that is linear in the row.
 *   - the residual r of grid sample (gx, gy) at (x, y) = (gx*step, gy*step) is vstab_mesh_residual_batch's, unchanged:
 *     r = ( (float)((x + (double)u) - X / W), (float)((y + (double)v) - Y / W) ) with X, Y, W as stated there.
 *   - the sample is ADMITTED iff u, v and both components of r are finite and it is blocked neither in frame i nor in
 *     frame i+1 (blocked == NULL: nothing is).
 *   - count = the number of admitted samples of the row.  count >= VSTAB_ROW_MIN_SAMPLES: per axis the median as
 *     numpy.median gives it on float32 (an even count: (lo + hi) / 2.0f).  Fewer: residual (0, 0), true count.
 * A median does not depend on the order of its inputs, so the result equals the NumPy restatement exactly.
 *   grid_flow, transitions, blocked: as for vstab_mesh_residual_batch
 *   residual dev [pairs, gh, 2] f32;  count dev [pairs, gh] i32
 * work_w, work_h >= 2; a row of more than 4096 grid positions is refused.  One workgroup per (pair, row), rank counting in
 * LDS.  Asynchronous on the context's stream; timing kind "row_residual".  VSTAB_ROW_MIN_SAMPLES is a choice, not a
 * calibration: a median of fewer values is hardly one. */
#define VSTAB_ROW_MIN_SAMPLES 8
int vstab_rolling_warp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                             int out_h, int out_w, const float* border_rgb, int subpix, const double* velocity,
                             double readout, float* dst, float* mask, uint32_t* pad_count);
#define VSTAB_ROLLING_UNWARP_MIN_DET 0.25
int vstab_rolling_unwarp_batch(vstab_ctx* ctx, const float* src, int n, int src_h, int src_w, const float* matrices,
                               int out_h, int out_w, const float* border_rgb, int subpix, const double* velocity,
                               double readout, float* dst, float* mask, uint32_t* pad_count, uint32_t* unsolved);
int vstab_row_residual_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h,
                             int work_w, const float* transitions, const uint8_t* blocked, float* residual, int32_t* count);

/* vstab_rectify_samples_batch -- the flow grid's samples as point pairs whose two ends are corrected for the readout, so that
 * the pair transitions can be fitted again on what a global shutter would have shown (rolling_refit; rolling_shutter.py).  The
 * warp corrects rows; a fit on the raw samples has already taken part of the shear for rotation and scale.  For pair k and
 * grid sample g = gy*gw + gx, in grid order:
 *   - p = ((float)(gx*step), (float)(gy*step));  c = p + flow[k][g] in float32, the fit's own load (vstab_sample_fit_batch).
 *   - the sample is ADMITTED iff it is blocked neither in frame k nor in frame k+1 (blocked == NULL: every sample is): the
 *     estimation mask's rule.  A sample whose flow is not finite is admitted like any other.
 *   - the RECTIFIED position of an observed point s of a frame with velocity V is q = s + e, with e exactly
 *     vstab_rolling_unwarp_batch's e for (x, y) = s as fp64, hm1 = work_h - 1 and rho = readout -- tau, a..d, det, vx, vy, rx,
 *     ry and e as stated there, every operation IEEE fp64 and rounded on its own, nothing fused -- with one addition: the row
 *     that enters tau is clamped as the forward rule clamps yc, yr = (y < 0) ? 0 : y, yr = (yr > hm1) ? hm1 : yr (a NaN stays
 *     a NaN), tau = rho * (yr / hm1 - 0.5); vx and vy take y itself.  VSTAB_ROLLING_UNWARP_MIN_DET and the non-finite test
 *     apply unchanged: an UNSOLVED point gets e = (0, 0) and is counted.
 *   - prev = p rectified with V[k], next = c rectified with V[k+1]; each coordinate of q is rounded once to float32.
 *   - if c.x or c.y is not finite (a flow sample that is not), next = (NaN, NaN) -- vstab_lk_track_batch's "untracked" form --
 *     its solve is not attempted and not counted; prev is written as for any sample.
 *   - output, admitted samples only, compacted, grid order kept:
 *       point_pairs dev [pairs, gh*gw, 4] f32 (prev.x, prev.y, next.x, next.y): vstab_points_fit_batch's input layout with
 *                   max_points = gh*gw; the rows from counts[k] on are NaN (0x7fc00000, as the untracked form), so the whole
 *                   array can be compared in bits
 *       counts      dev [pairs] i32: admitted samples
 *       unsolved    dev [pairs] u32: unsolved points, prev and next counted one each
 * Invariant: readout == 0 or all-zero velocities give prev == p and next == c in bits (e is a zero of either sign, and
 * neither p nor c is ever a negative zero).
 * The refit is vstab_points_fit_batch on point_pairs and counts, unchanged.  Its thresholds are the Classic rule's -- fewer
 * than 12 points or fewer than 8 finite ones give no candidate -- where the grid fit asks for 12 finite ones; on any real grid
 * (thousands of samples) the difference is immaterial.  total_points is the admitted count, as in the masked grid fit, and
 * the translation confidence finite / admitted.
 *   grid_flow dev [pairs, gh, gw, 2] f32;  blocked dev [pairs+1, gh, gw] u8 or NULL: as for vstab_sample_fit_batch_masked
 *   velocity  host [pairs+1, 6] f64 (V0..V5 per frame), px of the WORKING image per frame interval, staged by the call
 *   readout in [-1, 1];  work_h >= 2;  gh == ceil(work_h / step);  gh*gw <= 16384, as the fit requires
 * One workgroup per pair: an ordered block compaction of the admitted samples (the fit kernel's wavefront scan); the two
 * frames' coefficients and the readout are uniform.  Asynchronous on the context's stream; timing kind "rectify". */
int vstab_rectify_samples_batch(vstab_ctx* ctx, const float* grid_flow, int pairs, int gh, int gw, int step, int work_h,
                                const double* velocity, double readout, const uint8_t* blocked, float* point_pairs,
                                int32_t* counts, uint32_t* unsolved);

/* ---- dynamic zoom (not a reference feature, off by default): how far a warp's own coverage reaches around the centre ----
 * A per-frame zoom that hides the frame's own border needs to know the largest centred rectangle of the canvas the warp
 * covers.  Closed-form geometry would drift from the warp at the nearest-rounding boundary and does not exist for a mesh,
 * so the measure is taken per output pixel with the warp's own coordinate arithmetic.  The rule, for frame f:
 *   - pixel (x, y) of the out_h x out_w canvas is UNCOVERED iff vstab_warp_batch (offsets == NULL) or
 *     vstab_mesh_warp_batch (offsets given) would write mask == 1.0f there for the same matrix, sizes and subpix: the
 *     nearest-neighbour coverage of those rules (vstab_nn_covered, same column-block terms, displacement and roundings).
 *   - e(x, y) = max(|2x - (out_w-1)| * (out_h-1), |2y - (out_h-1)| * (out_w-1)) as unsigned 32-bit integers: the Chebyshev
 *     distance from the canvas centre in units in which the canvas edge is at E = (out_w-1) * (out_h-1) on both axes.
 *   - extent[f] = the minimum of e over the uncovered pixels, 0xFFFFFFFF if every pixel is covered.
 * An integer minimum does not depend on the order of its reduction, so the result equals a NumPy restatement exactly.
 * Every pixel with e < extent[f] is covered, and those pixels form a full centred integer rectangle; for a matrix warp the
 * covered set is convex, so the continuous rectangle they span is covered too (under a mesh it need not be).
 * What is decided from the number is host arithmetic (dynamic_zoom.py): the zoom about the canvas centre that brings the
 * covered rectangle, less VSTAB_ZOOM_MARGIN_PX pixels on every side, out to the canvas edge.
 *   matrices host [n, 9] f32 forward (source -> output), inverted as vstab_warp_batch inverts them
 *   offsets  dev  [n, mh, mw, 2] f32 as for vstab_mesh_warp_batch (2 <= mw, mh <= 65; src_w, src_h >= 2), or NULL (mw, mh unused)
 *   extent   dev  [n] u32; preset by the call itself (a small kernel in front of the pass)
 * out_w < 2, out_h < 2 or (out_w-1) * (out_h-1) >= 2^31 is refused in front of any launch; the other sizes are checked as
 * vstab_warp_batch checks them.  Kernel (vstab_warp.hip; it calls warp_pixel of vstab_internal.h with samplers that load nothing):
 * the warp's 64 x 8 tile and XCD remap, no image memory read or written; per thread -> wave shuffle -> LDS -> one atomic
 * minimum per workgroup and frame, skipped when the workgroup saw no uncovered pixel.  Asynchronous on the context's stream;
 * timing kind "cover_extent". */
#define VSTAB_ZOOM_MARGIN_PX 2
int vstab_cover_extent_batch(vstab_ctx* ctx, const float* matrices, int n, int src_h, int src_w, int out_h, int out_w,
                             int subpix, const float* offsets, int mw, int mh, uint32_t* extent);

/* ---- spatial fill: push-pull inpainting of the pixels that stay padding (beyond the reference, off by default) ----
 * What the warp (and temporal fill) leave as padding is filled per frame from the frame's own valid pixels by pyramid
 * push-pull (Gortler et al., "The Lumigraph", 1996).  The rule -- float32, per frame and per channel, separate IEEE
 * operations in the association written here, nothing fused:
 *   - Holes.  A pixel is a hole iff !(mask <= 0.5f): > 0.5 or not finite (the estimation mask's convention).  Level 0 is the
 *     frame itself with V_0 = !hole.
 *   - Pull.  Level l+1 is h' = (h_l + 1) >> 1 by w' = (w_l + 1) >> 1.  Cell (Y, X) has the taps t00 = (2Y, 2X),
 *     t01 = (2Y, 2X+1), t10 = (2Y+1, 2X), t11 = (2Y+1, 2X+1) of level l; a tap outside the level or with V_l == 0 enters as
 *     +0.0f; n = the number of valid taps.  n == 0: V = 0, C = +0.0f.  Otherwise V = 1 and
 *     C = ((t00 + t01) + (t10 + t11)) / (float)n.  Levels go on until 1 x 1.
 *   - Push, from the top level down.  F_top = C_top if V_top.  V_top == 0: the whole frame is hole, it is left untouched
 *     and fill_count = 0.  Otherwise F_l(y, x) = V_l ? C_l : up(F_{l+1})(y, x), the centre-aligned x2 bilinear upsample:
 *     along an axis with index i the near coarse index is i >> 1, the far one near - 1 (even i) or near + 1 (odd i),
 *     clamped to the coarse level; horizontally first r(row) = F[row][x_near] * 0.75f + F[row][x_far] * 0.25f, then
 *     up = r(y_near) * 0.75f + r(y_far) * 0.25f.  F_0 at the hole pixels is the result.
 *   - Valid pixels of dst are not stored to.  mask is not written at all: these pixels are invented, not seen, and a
 *     downstream in-painter still needs to know where they are (temporal fill, whose pixels are real, clears it).
 * dst   dev [n, h, w, 3] f32, in and out;  mask dev [n, h, w] f32, read only.
 * chunk_frames  frames per pass over the workspace, 0 = as many as keep it at or below 1 GiB; the result does not depend on it.
 * hole_count / fill_count  dev [n] u32 or NULL: holes found / pixels written (== hole_count, or 0 for an all-hole frame).
 * The pyramid lives in the context's grow-only workspace, one float4 {r, g, b, valid} record per cell of levels >= 1 (a
 * third of a frame's pixels).  Kernels (vstab_fill.hip): one pass over dst and mask forms levels 1..3 in LDS and counts the
 * holes; one workgroup per frame takes the levels that fit its LDS to 1 x 1 and back; push kernels go down the rest and
 * store only invalid cells, at level 0 only hole pixels.  Workgroups of a frame without holes (or without a valid pixel)
 * return on a per-frame flag.  Asynchronous on the context's stream; timing kind "sfill". */
int vstab_spatial_fill_batch(vstab_ctx* ctx, float* dst, const float* mask, int n, int h, int w, int chunk_frames,
                             uint32_t* hole_count, uint32_t* fill_count);

/* ---- stability report: masked squared error between frames, as exact integers (beyond the reference, off by default) ----
 * The inter-frame transformation fidelity (ITF) of the stabilization literature is the mean PSNR between consecutive frames,
 * here over the pixels both frames really show.  This entry point forms its sums on the device; the logarithm is host
 * arithmetic on the downloaded integers (stability.py).  It compares frame a[k] with frame b[k] for k in 0..n-1.  The rule:
 *   - A pixel is VALID in a frame iff mask <= 0.5f (spatial fill's convention: a NaN, an inf and anything above 0.5 are not
 *     valid); a NULL mask makes every pixel of its frames valid.  A pixel COUNTS for pair k iff it is valid in a[k] and in
 *     b[k]; count[k] is the number of such pixels.
 *   - For every counting pixel and every channel: d = a - b, one IEEE float32 subtraction; e = (double)d * (double)d, exact
 *     in fp64; e = (e < 4.0) ? e : 4.0, so that a NaN or inf difference contributes the cap; q = (uint64_t)(e * 4294967296.0),
 *     the multiply by 2^32 exact and the conversion truncating.
 *   - sse[k] is the sum of q over the counting pixels and the three channels as a 64-bit integer: it does not depend on the
 *     order of the additions, so the result equals a NumPy restatement exactly.  One pixel contributes at most 3 * 2^34, a
 *     frame of 8.3 Mpixel stays below 2^59: no wrap.  A pair without a counting pixel has count = 0 and sse = 0.
 * a, b            dev [n, h, w, 3] f32.  They may overlap in any way: b = a + h*w*3 with n = N - 1 is the consecutive-frame
 *                 form.  Nothing is written to a, b or the masks.
 * mask_a, mask_b  dev [n, h, w] f32 or NULL, each independently of the other.
 * sse             dev [n] u64;  count  dev [n] u32.  The call zeroes both itself.
 * n >= 1, h, w >= 1, h * w < 2^31.  Kernel (vstab_stability.hip): one launch over all pairs reads the frames as flat float
 * arrays, float4 per lane where a[k] and b[k] sit at the same offset from a 16-byte boundary (a scalar head and tail of up
 * to 3 floats each), one float per lane where they do not; the reduction runs per thread, by wavefront shuffle, in LDS, and
 * ends in one 64-bit and one 32-bit atomic add per workgroup and pair, skipped when the workgroup counted nothing.
 * Asynchronous on the context's stream; timing kind "stability". */
int vstab_frame_sse_batch(vstab_ctx* ctx, const float* a, const float* mask_a, const float* b, const float* mask_b,
                          int n, int h, int w, uint64_t* sse, uint32_t* count);

/* ---- subject lock: where a mask's subject is, per frame, as exact integers (beyond the reference, off by default) ----
 * Stabilizing ON a subject (subject_lock.py) needs the subject's absolute position in every frame; a per-frame segmentation
 * mask gives it without drift.  This entry point reduces a clip of masks to seven integers per frame; everything formed
 * from them (centroid, area ratio, transitions) is host arithmetic on the downloaded 28 bytes.  The rule:
 *   - Pixel (x, y) of frame k is SUBJECT iff mask[k, y, x] > 0.5f: a NaN is not subject, +inf is.  This deliberately
 *     differs from the estimation mask, where a non-finite value means subject -- the conservative choice for exclusion;
 *     here a NaN must not attract the track.
 *   - sums[k] = {count, sum_x, sum_y}: the number of subject pixels and the sums of their x and of their y, 64-bit.
 *   - bbox[k] = {x0, y0, x1, y1}: the inclusive bounding box of the subject pixels; a frame without one reports
 *     {-1, -1, -1, -1} and sums of 0.
 * Integer sums, minima and maxima do not depend on the order of their reduction, so the result equals a NumPy restatement
 * exactly.  sum_x < 2^31 * 2^15: no wrap.
 *   mask dev [n, h, w] f32, read only;  sums dev [n, 3] u64;  bbox dev [n, 4] i32.  The call presets both outputs itself.
 * n >= 1;  1 <= w, h <= 32768 (32-bit coordinates per thread);  h * w < 2^31.  Kernel (vstab_subject.hip, shaped as
 * frame_sse_kernel is): one launch reads every frame as the flat float array it is, float4 per lane behind a scalar head of
 * up to 3 floats where a frame does not start on a 16-byte boundary (frame k of a clip whose h * w is no multiple of 4 starts
 * (k * h * w) mod 4 floats past one), and a tail of up to 3; (x, y) of a float4's first pixel from one division, the others
 * by stepping with wrap; per thread -> wavefront shuffle -> LDS -> three 64-bit atomic adds, two unsigned atomic minima
 * (x0, y0 preset to 0xFFFFFFFF) and two signed atomic maxima (x1, y1 preset to -1) per workgroup and frame, skipped when the
 * workgroup counted nothing -- so an empty frame reads as four -1 without a finishing pass.  Asynchronous on the context's
 * stream; timing kind "mask_moments". */
int vstab_mask_moments_batch(vstab_ctx* ctx, const float* mask, int n, int h, int w, uint64_t* sums, int32_t* bbox);

/* ---- sharpness transfer: shake-blurred frames repaired from sharper neighbours (beyond the reference, off by default) ----
 * A camera jolt blurs the frames it hits; once the picture stands still those frames read as a sharpness pulse.  Matsushita
 * et al. ("Full-frame video stabilization with motion inpainting", PAMI 2006, section 5) transfer pixels from sharper
 * neighbouring frames, registered by the transitions the stabilizer already has.  Two entries: a per-frame sharpness measure
 * and the weighted transfer (sharpness_transfer.py forms the ratios between them on the host).
 *
 * vstab_frame_sharpness_batch -- the gradient energy of every frame as one exact integer:
 *   - q(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0, the blended fill's q (a NaN gives 0).
 *   - Y(x, y) = (q(r) + 2 * q(g) + q(b)) >> 2, an integer in 0..65536.
 *   - over 0 <= x < w - 1, 0 <= y < h - 1:  gx = Y(x + 1, y) - Y(x, y),  gy = Y(x, y + 1) - Y(x, y).
 *   - energy[k] = the 64-bit integer sum of gx * gx + gy * gy over those pixels of frame k.
 * One pixel contributes at most 2^33 and h * w <= 2^30 is required, so nothing wraps; w == 1 or h == 1 gives 0.  An integer
 * sum does not depend on the order of addition, so the result equals a NumPy restatement exactly.
 *   frames dev [n, h, w, 3] f32, read only;  energy dev [n] u64, zeroed by the call.  n >= 1.
 * Kernel (vstab_sharp.hip): a workgroup per 64 x 32 tile, Y once per pixel into LDS with a one-column, one-row halo, the
 * differences from LDS, per thread -> wavefront shuffle -> LDS -> one 64-bit atomic add per workgroup and frame, skipped where
 * the tile is flat.  Asynchronous on the context's stream; timing kind "sharpness". */
int vstab_frame_sharpness_batch(vstab_ctx* ctx, const float* frames, int n, int h, int w, uint64_t* energy);

/* vstab_sharp_transfer_batch -- src, clip_frames, first, n, matrices, cand_frame, K: the candidates of
 * vstab_temporal_fill_batch, skipped as there (cand_frame -1, a matrix cv::invert would refuse); "sample" and "valid" are the
 * blended fill's: the value vstab_temporal_fill_batch would write for that candidate, taken where every interpolation tap
 * of the Q5 coordinate lies inside the candidate's frame (the interior rule above).  Per output pixel of frame first + f:
 *   - mask == 1.0f (padded): untouched, nothing is stored.  mask == NULL: every pixel is own (`crop` framing).
 *   - otherwise o = the pixel's value before the call, num = (0, 0, 0), den = 0, and the candidates k = 0 .. K-1 are walked
 *     in order.  Candidate k CONTRIBUTES iff ratio[f, k] > 0, it is not skipped, it is valid at the pixel, and
 *     D < INFINITY with D = (|s_r - o_r| + |s_g - o_g|) + |s_b - o_b| for its sample s (a NaN in either value makes the
 *     comparison false).  A contributing candidate adds, in float32, every operation rounded on its own, nothing fused:
 *         w = ratio / (ratio + alpha * D);    num_c = num_c + w * s_c;    den = den + w
 *   - after the walk, den > 0: dst_c = (o_c + num_c) / (1.0f + den), and the pixel counts in transfer_count.  Otherwise
 *     nothing is stored.  Both divisions are the correctly rounded ones.
 *   - the mask is never written.  dst is read only at the pixel itself and the candidates sample src, so working in place
 *     is free of races (dst must not alias src).
 * The own value has weight 1, a neighbour at most 1 (D == 0) and less the more it disagrees: a misregistered or occluded
 * sample fades out instead of ghosting.  There is no "first wins": every contributing candidate is sampled.
 *   ratio  host [n, K] f32, finite and >= 0 (sharpness_transfer.ratios_from_energy: E_j / E_i, 0 below 1.1)
 *   alpha  finite and >= 0;  dst dev [n, out_h, out_w, 3] f32, in and out;  mask dev [n, out_h, out_w] f32 or NULL
 *   transfer_count dev [n] u32 or NULL, zeroed by the call.  K in 1..64.
 * VSTAB_SUBPIX_Q5 only (VSTAB_SUBPIX_EXACT is refused), bilinear and bicubic.  Only frames with a contributing candidate get
 * workgroups: a call whose ratios are all 0 launches no kernel.  Timing kind "sharp_transfer". */
int vstab_sharp_transfer_batch(vstab_ctx* ctx, const float* src, int clip_frames, int src_h, int src_w, int first, int n,
                               const float* matrices, const int32_t* cand_frame, int K, const float* ratio, float alpha,
                               int out_h, int out_w, int interp, int subpix, float* dst, const float* mask,
                               uint32_t* transfer_count);

/* ---- mask hand-off: hold, grow and feather the padding mask for a generative outpainter (beyond the reference, off by default) ----
 * The reference's workflows put ComfyUI's GrowMask (scipy grey_dilation, 3 x 3, once per pixel of growth, on one CPU thread)
 * between the stabilizer and the outpainter, and users chain a feather behind it by hand.  Both, and a temporal hold that
 * keeps the repaint region from jittering, are maxima; a maximum is the same in any order, so what these two entries return
 * equals a NumPy restatement (tests/mask_handoff_restatement.py) in bits whatever decomposition the kernels use.
 *
 * m is a float32 mask [n, h, w].  A NaN reads as 1.0f: an unknown pixel is to be repainted (the spatial fill's convention).
 * Every other value, infinities included, reads as itself.  Values are ordered as IEEE 754 orders them, -0.0f below +0.0f
 * (the total order of the sign-magnitude bits), so that a maximum never has to choose between equals with different bits.
 * Nothing crosses from one frame into another except in the hold.
 *
 * vstab_mask_hold_batch -- 1. Hold, T = hold in 0..VSTAB_MASK_HOLD_MAX:
 *   - held_i(p) = max of m_j(p) over |j - i| <= T, 0 <= j < n, and shot[j] == shot[i].
 *   - shot  host [n] i32, non-decreasing (refused otherwise), or NULL: one shot.
 *   - T = 0 returns the input's bits, its NaNs included; T > 0 reads a NaN as 1.0f like every other maximum here.
 *   mask dev [n, h, w] f32, read only;  out dev [n, h, w] f32, must not overlap mask.
 * Kernel (vstab_handoff.hip): streaming, one 16-byte load per lane and window frame where h * w is a multiple of 4 and both
 * pointers are 16-byte aligned, one float per lane otherwise; the windows come down as a host-formed table.  A pixel's
 * 2T + 1 reads are whole-frame re-reads.  T = 0 is one device copy.  Timing kind "mask_hold".
 *
 * vstab_mask_grow_batch -- 2. Grow, g = grow in -VSTAB_MASK_GROW_MAX..VSTAB_MASK_GROW_MAX, footprint VSTAB_GROW_TAPERED (the
 * L1 ball |dx| + |dy| <= |g|) or VSTAB_GROW_SQUARE (the L-infinity ball max(|dx|, |dy|) <= |g|):
 *   - G(p) = max (g > 0) or min (g < 0) of the mask over the ball around p, clipped to the frame.  g = 0 is the identity
 *     (G holds the input's bits, a NaN included).
 *   - This is ComfyUI's GrowMask: |g| iterations of scipy's 3 x 3 grey_dilation / grey_erosion (cross or full footprint,
 *     mode="reflect") equal the clipped-ball extremum, because a reflected neighbour is an in-frame pixel no farther away.
 * 3. Feather, f = feather in 0..VSTAB_MASK_FEATHER_MAX, outward, in the norm of the chosen footprint.  f = 0: out = G, float
 * for float.  f > 0, with dist the L1 or L-infinity distance:
 *   - Q(p) = max(0, max over q in the clipped ball of radius f of [ q16(G(q)) - dist(p, q) * step ])
 *   - step = 65536 / (f + 1) in integer division;  q16(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0, the blended
 *     fill's quantiser, with a NaN of G read as 1.0f first (so q16 = 65536);  out = (float)Q / 65536, which is exact.
 *   For a 0 / 1 mask this is the ramp 1 - d * step / 65536 over the chamfer distance d <= f, and 0 beyond.
 * 4. Count.  count_out[k] = the number of pixels of out frame k that are > 0.5f.
 *   mask dev [n, h, w] f32, read only;  out dev [n, h, w] f32, must not overlap mask;  count_out dev [n] u32 or NULL, zeroed
 *   by the call.  h * w < 2^31.
 * Kernel (vstab_handoff.hip): balls and cones of one norm compose, so the |g| + f one-pixel steps are cut into passes of at
 * most 16.  In a pass a workgroup of 256 threads stages a 64 x 32 core tile and a halo of the pass's steps in LDS as integer
 * order keys, rows packed densely, relaxes it step by step over a shrinking region between two LDS buffers (flat steps
 * first, then the quantised integer ones with the decrement; a thread keeps, per cell, the number of steps the cell takes
 * part in), keeps the cells outside the frame at the identity, and stores the core once; the last pass counts (one atomic
 * add per workgroup and frame).  Passes alternate between out and a workspace of the context, a chunk of frames (at most
 * 1 GiB) at a time.  Asynchronous on the context's stream; timing kind "mask_grow". */
#define VSTAB_GROW_TAPERED 0
#define VSTAB_GROW_SQUARE 1
#define VSTAB_MASK_HOLD_MAX 16
#define VSTAB_MASK_GROW_MAX 64
#define VSTAB_MASK_FEATHER_MAX 64
int vstab_mask_hold_batch(vstab_ctx* ctx, const float* mask, int n, int h, int w, int hold, const int32_t* shot, float* out);
int vstab_mask_grow_batch(vstab_ctx* ctx, const float* mask, int n, int h, int w, int grow, int footprint, int feather,
                          float* out, uint32_t* count_out);

/* ---- deflicker: registered exposure gains between consecutive frames, and their correction (beyond the reference, off by default) ----
 * Auto exposure and auto white balance hunt while the camera shakes; once the picture stands still the brightness steps are
 * what is left to see.  The transitions register consecutive frames, so frame k+1 can be compared with frame k pixel against
 * the same scene point: what differs is exposure, not content.  Two measuring entries and one that applies per-frame gains;
 * median, band, smoothing and the gains themselves are host arithmetic on the downloaded integers (deflicker.py).
 *
 * The measurement rule, for pair k (frames a = k, b = k + 1 of src) and its full-resolution transition A_k (float32 widened
 * to fp64).  It uses integers only, so the result is the same in any order of summation:
 *   - Lattice: the pixels p = (x, y) of frame a with x % S == S/2 && y % S == S/2, S = VSTAB_DEFLICKER_STRIDE.
 *   - Mapping: vstab_pair_residual_batch's, literally (one device function serves both): X, Y, W in that association, W <= 0
 *     or not finite excluded, q = (rint(X / W), rint(Y / W)) with ties to even.  p is INSIDE iff q lies in frame b
 *     (0 <= qx <= w-1 and 0 <= qy <= h-1).  Nothing is interpolated: both values are stored pixels.
 *   - Levels: qa_c = q(src[a, y, x, c]), qb_c = q(src[b, qy, qx, c]), q the blended fill's 16-bit quantiser
 *     q(v) = v > 0 ? (v < 1 ? (uint32)(v * 65536.0f) : 65536) : 0 (a NaN gives 0).
 *   - An inside pixel is WELL EXPOSED iff all six levels lie in [VSTAB_DEFLICKER_LO, VSTAB_DEFLICKER_HI]: clipped highlights
 *     and crushed blacks break a gain model.
 *   - Four ratio channels: 0..2 are r, g, b; channel 3 is the sum of the three levels in each frame (qa_3 = qa_0 + qa_1 + qa_2,
 *     qb_3 likewise).  bin_c = min((qb_c * 256) / qa_c, 1023) in unsigned integer division: the ratio in units of 1/256.
 *     qa_c >= 2048 and qb_3 * 256 <= 3 * 63488 * 256 < 2^26: everything fits 32 bits.
 * vstab_pair_gain_hist_batch: hist[k, c, bin_c] += 1 for every well-exposed pixel and channel; stats[k] = {inside,
 * well_exposed}.  vstab_pair_gain_sums_batch: sums[k, c] = {count, sum qa_c, sum qb_c} over the well-exposed pixels whose
 * bin_c lies in band[k, c] = [lo, hi], both inclusive; lo > hi counts nothing.  The median of the histogram ignores a moving
 * subject, a flash in part of the frame or a misregistered region while they own less than half of the samples; the second
 * pass gives a fine estimate inside a band around that median.
 *   src          dev  [n, h, w, 3] f32, read only (n >= 2)
 *   transitions  host [n-1, 9] f32, full resolution, x_{k+1} = A_k x_k
 *   active       host [n-1] u8 or NULL (all active): a pair with active == 0 reads nothing and reports zeros
 *   hist         dev  [n-1, 4, 1024] u32;  stats dev [n-1, 2] u32;  sums dev [n-1, 4, 3] u64: zeroed by the call
 *   band         host [n-1, 4, 2] i32
 * h * w < 2^31.  A sum stays below 2^31 / 16 * 3 * 2^16 < 2^46.  Kernel (vstab_deflicker.hip): one body, two instantiations;
 * a workgroup takes a share of one active pair's lattice, a lane a lattice pixel (a gather of 12 B at a 48-B pitch in frame
 * a, 12 B wherever the transition points in frame b); the histogram is counted in LDS with integer atomics and its non-zero
 * bins are flushed with global atomics, the sums go per thread -> wavefront shuffle -> LDS -> one 64-bit atomic per workgroup
 * and number.  Asynchronous on the context's stream; timing kinds "gain_hist" and "gain_sums".
 * The stride of 4 (1/16 of the pixels) and the level bounds 2048 / 63488 (1/32 from either end of the range) are
 * choices, not calibrations; so are the band of 1/8, the minimum count of 256 and the clamp of the correction in deflicker.py.
 *
 * The apply rule, vstab_apply_gain_batch, per pixel of frame f and channel c with g = gains[f, c] and v the stored value:
 *   - mask[f, y, x] == 1.0f: the pixel is untouched, so padding keeps its colour.  mask == NULL: every pixel is own.
 *   - g == 1.0f exactly: the channel is untouched.  A frame whose three gains are all 1.0f is not read at all.
 *   - v is a NaN: untouched (a NaN stays the NaN it was).
 *   - otherwise out = v * g, one float32 multiply; if out > 1.0f && v <= 1.0f then out = 1.0f and the value counts in
 *     clamped[f].  A value is never pushed out of range; one that already was out of range stays scaled.
 *   frames  dev [n, h, w, 3] f32, in and out;  mask dev [n, h, w] f32 or NULL;  gains host [n, 3] f32
 *   clamped dev [n] u32 or NULL, zeroed by the call.  n >= 1, h * w < 2^31.
 * Kernel: shaped as frame_sse_kernel is.  A frame is read as the flat float array it is, a float4 per lane behind a scalar
 * head of up to 3 floats where it does not start on a 16-byte boundary and a tail of up to 3; channel and pixel come from the
 * flat index; only frames with a gain other than 1.0f get workgroups.  An in-place streaming pass of 24 B per pixel plus 4 B
 * of mask, with ordinary (temporal) stores: the passes behind it read the frames again at once.  Timing kind "apply_gain". */
#define VSTAB_DEFLICKER_STRIDE 4
#define VSTAB_DEFLICKER_LO 2048
#define VSTAB_DEFLICKER_HI 63488
#define VSTAB_DEFLICKER_BINS 1024
int vstab_pair_gain_hist_batch(vstab_ctx* ctx, const float* src, int n, int h, int w, const float* transitions,
                               const uint8_t* active, uint32_t* hist, uint32_t* stats);
int vstab_pair_gain_sums_batch(vstab_ctx* ctx, const float* src, int n, int h, int w, const float* transitions,
                               const uint8_t* active, const int32_t* band, uint64_t* sums);
int vstab_apply_gain_batch(vstab_ctx* ctx, float* frames, const float* mask, int n, int h, int w, const float* gains,
                           uint32_t* clamped);

/* ---- horizon level: which way is up, per estimation image, as exact integers (beyond the reference, off by default) ----
 * Everything else measures pairs; this measures one frame.  Man-made and natural structure is mostly vertical or horizontal,
 * so the histogram of gradient orientations, folded modulo 90 degrees, peaks at the frame's roll (horizon_level.py finds
 * the peak and turns it into one offset per shot on the host).  This entry point reduces every estimation image to 2K + 1
 * integers, K = VSTAB_ORIENTATION_K.  The rule, for every pixel (x, y) with all eight neighbours (1 <= x <= w - 2,
 * 1 <= y <= h - 2) of every frame g, all in integers:
 *   gx = 3 * (g[y-1][x+1] - g[y-1][x-1]) + 10 * (g[y][x+1] - g[y][x-1]) + 3 * (g[y+1][x+1] - g[y+1][x-1])
 *   gy = 3 * (g[y+1][x-1] - g[y-1][x-1]) + 10 * (g[y+1][x] - g[y-1][x]) + 3 * (g[y+1][x+1] - g[y-1][x+1])
 *   m2 = gx * gx + gy * gy                      (|gx|, |gy| <= 4080: m2 < 2^26)
 * (the Scharr derivative: the 3x3 Sobel weights 1 2 1 bias the orientation of a smooth edge by degrees, these by tenths).
 * A pixel with m2 < min_mag2 or m2 == 0 adds nothing.  Otherwise, with a = |gx|, b = |gy|:
 *   j = (2 * K * min(a, b) + max(a, b)) / (2 * max(a, b))     integer division: round(K * min / max), 0 .. K
 *   k = sign(gx * gy) * (a >= b ? 1 : -1) * j
 *   hist[frame][k + K] += m2
 * The bins are uniform in the slope, so nothing transcendental runs on the device: bin k stands for the orientation
 * atan(k / K), the gradient's direction folded into [-45, 45] degrees.  Bins -K and +K are the same orientation (a == b
 * lands in one of them by the sign of gx * gy); the host folds them.  Content rotated by the point matrix
 * [[c, -s], [s, c]] in pixel coordinates (x right, y down) puts its axis-aligned edges at +theta.
 * Integer sums do not depend on the order of their reduction, so the result equals a NumPy restatement exactly; a frame's
 * total is below 2^31 * 2^26: no wrap.
 *   gray dev [n, h, w] u8, read only;  hist dev [n, 2K + 1] u64, 8-byte aligned.  The call presets its own output.
 * n >= 1;  1 <= w, h <= 32768;  h * w < 2^31.  h < 3 or w < 3 is valid and gives an all-zero histogram.
 * Kernel (vstab_level.hip, shaped as the scene-cut residual's is): one launch over all frames, a workgroup per 16 rows of a
 * frame, a lane per 16 pixels of a row -- three aligned 16-byte loads and six halo bytes where w % 16 == 0 and gray is
 * 16-byte aligned, byte loads otherwise; a lane merges its run of equal bins in a 64-bit register and adds it to its wave's
 * copy of the histogram in LDS when the bin changes; behind a barrier the copies are summed and every non-zero bin goes out
 * with one 64-bit atomic add per workgroup and frame.  Asynchronous on the context's stream; timing kind
 * "orientation_hist". */
#define VSTAB_ORIENTATION_K 256
int vstab_orientation_hist_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, uint32_t min_mag2, uint64_t* hist);

/* ---- clean plate: the per-pixel temporal median of a registered shot, its fill and its matte (beyond the reference, off by default) ----
 * Every other pass behind the warp looks at one frame, a pair or a window of neighbours.  A locked shot (camera_lock at
 * strength 1) registers every output frame to its shot's first frame, so one pixel position shows one scene point all through
 * the shot: the median over time of what the frames really show there is the background with everything that moves taken
 * out, the ideal border is that one still image, and its difference to a frame is a matte of what moves.  A selection on
 * integers is the same in any order, so all three results equal a NumPy restatement in bits.
 *
 * vstab_plate_median_batch -- 1. Plate, per shot s (row s of sample_frame) and pixel p:
 *   - Sample j (a frame index of the row) of pixel p is VALID iff mask_j(p) <= 0.5f; a NaN mask is not valid (the stability
 *     report's convention).  mask == NULL: every sample is valid.  count_s(p) = the number of valid samples.
 *   - Per channel, the valid values are ordered by their float32 order keys: the total order of the sign-magnitude bits, -0.0f
 *     below +0.0f (the mask hand-off's order); every NaN is first mapped to the largest key.
 *   - plate_s(p, c) = the LOWER median, the element of 0-based rank (count - 1) / 2, returned with the sample's own bits; a
 *     NaN returns as 0x7FC00000.  count == 0 gives 0.0f in all three channels.
 *   - Nothing crosses from one row to another.
 *   frames        dev  [n, h, w, 3] f32, read only;  mask dev [n, h, w] f32, read only, or NULL
 *   sample_frame  host [shots, S] i32, S in 1..VSTAB_PLATE_SAMPLES_MAX: every row holds strictly increasing frame indices in
 *                 0..n-1 followed by -1 padding only, and at least one index; anything else is refused by name
 *   plate         dev  [shots, h, w, 3] f32;  count dev [shots, h, w] i32.  h * w < 2^31.
 * Kernels (vstab_plate.hip): [h, w, 3] is a flat array of elements e with mask index e / 3, so consecutive lanes load
 * consecutive floats of one frame and every frame and mask value crosses HBM once.  The widest row decides the form.  Up to
 * VSTAB_PLATE_REGISTER_MAX samples: a lane per element, the keys in 4 / 8 / 16 / 32 / 64 registers.  Beyond: a workgroup of 256
 * threads per 64 elements, the keys staged in LDS as [sample][element] in 128 / 256 rows (64 KiB at 256: two workgroups
 * per CU), then 16 lanes x 4 quarters of the samples per element, their counts joined by two shuffles.  Both select the key of
 * rank r as the largest v with #{key < v} <= r, from the top bit down: 32 counting passes.  A sample that is not valid is
 * staged as the largest key, which r < count never reaches.  Asynchronous on the context's stream; timing kind "plate_median".
 *
 * vstab_plate_fill_batch -- 2. Plate fill, for frame i with s = shot[i] (shot == NULL: every frame is of shot 0):
 *   - Pixel p is FILLED iff !(mask_i(p) <= 0.5f) && count_s(p) >= min_count.  A NaN mask pixel is filled.
 *   - A filled pixel takes the plate's three floats, its mask becomes 0.0f -- it was seen, not invented: the temporal fill's
 *     convention -- and it counts in filled_count[i].  Every other pixel keeps its bits in both tensors.
 *   dst dev [n, h, w, 3] f32 and mask dev [n, h, w] f32, both in and out;  plate, count as above, read only
 *   shot host [n] i32, non-decreasing, values in 0..shots-1, or NULL;  min_count in 1..VSTAB_PLATE_SAMPLES_MAX
 *   filled_count dev [n] u32 or NULL, zeroed by the call.
 *
 * vstab_plate_matte_batch -- 3. Matte: matte_i(p) = 1.0f iff all three hold, else 0.0f:
 *   - the pixel is own: mask_i(p) <= 0.5f, or mask == NULL;
 *   - count_s(p) >= min_count;
 *   - for some channel c, !(fabsf(f_c - plate_c) <= threshold): one float32 subtraction per channel, and a NaN on either side
 *     reads as "differs" (the estimation mask's convention: the unknown is subject).
 *   frames dev [n, h, w, 3] f32 and mask dev [n, h, w] f32 or NULL, read only;  threshold finite and >= 0
 *   matte dev [n, h, w] f32;  matte_count dev [n] u32 or NULL, zeroed by the call: the pixels of frame i with matte 1.
 * Kernels: streaming, workgroups per frame.  Where h * w is a multiple of 4 and every pointer is 16-byte aligned a lane takes
 * four whole pixels with 16-byte accesses (the fill reads the mask first and touches neither the frame nor the plate where none
 * of the four is padding); otherwise a lane takes one whole pixel -- never a single float of one, because the fill writes the
 * mask value that decides the pixel's other two channels.  The per-frame counts go through BlockSums: one atomic add per
 * workgroup and frame.  Asynchronous on the context's stream; timing kinds "plate_fill" and "plate_matte".
 * The 256 samples are a choice, not a calibration (clean_plate.py holds the others). */
#define VSTAB_PLATE_SAMPLES_MAX 256
#define VSTAB_PLATE_REGISTER_MAX 64
int vstab_plate_median_batch(vstab_ctx* ctx, const float* frames, const float* mask, int n, int h, int w,
                             const int32_t* sample_frame, int shots, int S, float* plate, int32_t* count);
int vstab_plate_fill_batch(vstab_ctx* ctx, float* dst, float* mask, int n, int h, int w, const float* plate, const int32_t* count,
                           const int32_t* shot, int shots, int min_count, uint32_t* filled_count);
int vstab_plate_matte_batch(vstab_ctx* ctx, const float* frames, const float* mask, int n, int h, int w, const float* plate,
                            const int32_t* count, const int32_t* shot, int shots, float threshold, int min_count, float* matte,
                            uint32_t* matte_count);

/* ---- F6 / F9 host helper: element-wise libm over fp64 arrays (host pointers, no GPU involved) ----
 * nodes/stabilizer_utils.py:300-358 (_matrix_to_params / _params_to_matrix) call math.sqrt/atan2/log and
 * math.exp/cos/sin per frame; this runs the same libm functions over a whole clip in one call.
 * b is only read by VSTAB_HOST_ATAN2 (out = atan2(a, b)). */
enum { VSTAB_HOST_SQRT = 0, VSTAB_HOST_ATAN2 = 1, VSTAB_HOST_LOG = 2, VSTAB_HOST_EXP = 3, VSTAB_HOST_COS = 4, VSTAB_HOST_SIN = 5 };
int vstab_host_math(int op, const double* a, const double* b, int n, double* out);

/* ---- F6 / F9 for a whole clip (host pointers, no GPU involved) ----
 * vstab_transitions_to_params: nodes/video_stabilizer_flow.py:340-346 per transition --
 *   _rescale_transform_to_full (stabilizer_utils.py:279-297; skipped when up == down == NULL: estimated at full size)
 *   then _matrix_to_params (stabilizer_utils.py:300-324) of the requested mode.
 *   work_mats host [count,9] f32 (working resolution); up = {1/sx, 1/sy, 1}, down = {sx, sy, 1} with
 *   sx = working_w / source_w, sy = working_h / source_h (fp64, as the reference forms them);
 *   full_mats host [count,9] f32; params host [count, 2 | 4 | 8] f64.
 * vstab_params_to_matrices: _params_to_matrix (stabilizer_utils.py:327-358): params host [count, 2|4|8] f64 ->
 *   mats host [count,9] f32.  mode = VSTAB_MODE_*.
 * Replicated on every rank of a multi-GPU run for the whole clip (the serial part of a rank's step): one call each
 * instead of ~25 NumPy / ctypes calls.  Same libm, same rounding points as the per-item Python forms. */
int vstab_transitions_to_params(const float* work_mats, int count, int mode, const double* up, const double* down,
                                float* full_mats, double* params);
int vstab_params_to_matrices(const double* params, int count, int mode, float* mats);

/* F10 for a whole clip (host pointers): _compute_bounding_boxes (stabilizer_utils.py:1010-1034) -- the four frame corners
 * through each f32 matrix in fp64, projective division, per-axis min / max (NaN-propagating, as numpy.minimum / maximum).
 * mats host [count,9] f32; mins, maxs host [count,2] f64. */
int vstab_bounding_boxes(const float* mats, int count, double width, double height, double* mins, double* maxs);

#ifdef __cplusplus
}
#endif
#endif /* VSTAB_H */
