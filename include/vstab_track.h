/*
 * vstab_track.h -- the template track of libvstab.so: one box, followed through a clip (beyond the reference, off by default).
 *
 * A second public header beside vstab.h, which it includes and whose conventions it keeps; the entry point below is exported
 * from the same libvstab.so.  It stands apart because vstab.h, its signature table and VSTAB_ABI_VERSION are frozen by the
 * binding's call records; the Python side binds this header through a table of its own (native._TRACK_SIGNATURES).
 *
 * The rule (tests/track_restatement.py restates it in NumPy; the kernel equals it in bits).  All arithmetic is integer.
 *
 *   Template.  The box (bx, by, bw, bh) lies inside frame `key` of gray [n,h,w] u8, bw >= 8, bh >= 8.  With the stride
 *     s = ceil(max(bw, bh) / 64), nx = bw / s and ny = bh / s (integer division), the template is the nx x ny samples
 *     T[j][i] = gray[key][by + j*s][bx + i*s], so n_s = nx * ny <= 4096.
 *     tsums = (n_s, sum T, sum T^2).  J_T = n_s * sum T^2 - (sum T)^2 is the template's own variance times n_s^2; a caller
 *     refuses J_T == 0 (no texture) on the host.
 *
 *   Chain.  pos[key] = (bx, by).  The frames are visited in the order key+1 .. n-1, then key-1 .. 0; frame k > key follows
 *     frame k-1, frame k < key follows frame k+1, and starts from the position p of the frame it follows.
 *
 *   Cost.  For a frame with start p and every (dx, dy) in [-R, R]^2, q = p + (dx, dy):
 *     if a sample of the box at q lies outside the frame -- q.x < 0, q.y < 0, q.x + (nx-1)*s > w-1 or q.y + (ny-1)*s > h-1 --
 *     the cost is the sentinel VSTAB_TRACK_SENTINEL = 2^64 - 1.  Otherwise, with C[j][i] = gray[k][q.y + j*s][q.x + i*s] and
 *     d = C - T per sample,
 *         J = n_s * sum d^2 - (sum d)^2,
 *     the zero-mean sum of squared differences times n_s^2: at most 4096 * 4096 * 255^2 < 2^40, an exact integer in any
 *     order of summation, and unchanged by a brightness offset between template and frame.
 *
 *   Pick.  The minimum of (J, dx^2 + dy^2, dy, dx) in lexicographic order: among equal costs the nearest candidate, so a flat
 *     region stays where it was, not in a corner of the window.  pos[k] = p + pick, best[k] = its J.  Where every candidate
 *     is the sentinel the pick is (0, 0) by that same order: the position is carried and best[k] is the sentinel.
 *     near[k][(ey+1)*3 + (ex+1)], ex, ey in -1..1, is the cost of the candidate pick + (ex, ey), the sentinel where that
 *     candidate lies outside the window (and, as everywhere, where its box leaves the frame).
 *     surface (optional, NULL if not wanted) [n, 2R+1, 2R+1]: surface[k][dy+R][dx+R], every cost of frame k.
 *     Frame `key` is not searched: best 0, and near / surface hold 0 at (0, 0) and the sentinel elsewhere.
 *
 * Kernels (csrc/vstab_track.hip): track_template_kernel (frame key: template, its sums, the key frame's outputs) and one
 * track_search_kernel launch per searched frame, queued back to back on the context's stream, one workgroup per dy row.  A
 * workgroup writes its row's costs and its row minimum; every workgroup of the NEXT launch reduces the previous frame's
 * 2R+1 row minima to find its own start, and workgroup 0 of it writes pos / best / near of that previous frame.  A last
 * one-workgroup launch per direction resolves the direction's final frame.  No host round trip between frames, no waiting
 * between workgroups, no cooperative launch.
 *
 * work: device scratch of VSTAB_TRACK_WORK_WORDS(radius) 64-bit words, contents undefined before and after: the template's
 * bytes, then two alternating slots of one cost surface and 2R+1 row minima (cost, dx) each.
 * All pointers but gray are written.  Asynchronous on the context's stream; timing kind "track_template".
 */
#ifndef VSTAB_TRACK_H
#define VSTAB_TRACK_H

#include "vstab.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSTAB_TRACK_SENTINEL 0xFFFFFFFFFFFFFFFFull
#define VSTAB_TRACK_RADIUS_MAX 48
#define VSTAB_TRACK_MIN_BOX 8
#define VSTAB_TRACK_MAX_SAMPLES 4096
/* the widest span of one staged frame row: 2R + (nx-1)*s + 1 bytes */
#define VSTAB_TRACK_MAX_SPAN 16384
#define VSTAB_TRACK_WORK_WORDS(radius) \
    (VSTAB_TRACK_MAX_SAMPLES / 8 + 2 * ((2 * (radius) + 1) * (2 * (radius) + 1) + 2 * (2 * (radius) + 1)))

int vstab_track_template_batch(vstab_ctx* ctx, const uint8_t* gray, int n, int h, int w, int bx, int by, int bw, int bh, int stride,
                               int radius, int key, uint64_t* tsums, int32_t* pos, uint64_t* best, uint64_t* near,
                               uint64_t* surface, uint64_t* work);

#ifdef __cplusplus
}
#endif

#endif  /* VSTAB_TRACK_H */
