// vstab_deflicker.hip -- deflicker: the registered exposure ratios of consecutive frames as exact integers
// (vstab_pair_gain_hist_batch, vstab_pair_gain_sums_batch) and the per-frame gains applied in place
// (vstab_apply_gain_batch).  Not a reference feature; both rules are stated in include/vstab.h.
//
//   pair_gain_kernel<false>  the ratio histograms: counted in LDS with integer atomics (16 KiB per workgroup), the non-zero
//                            bins flushed with global atomics; inside / well-exposed counts through BlockSums (vstab_internal.h)
//   pair_gain_kernel<true>   the banded sums: BlockSums, thread k finishes number k with one 64-bit atomic per workgroup
//   apply_gain_kernel        shaped as frame_sse_kernel: the frame as a flat float array, float4 per lane behind a scalar
//                            head, a scalar tail; channel and pixel from the flat index
// One body serves both measurements, so that lattice, mapping, levels and bins cannot differ between the two passes.  A lane
// takes one lattice pixel: 12 B of frame a at a 48-B pitch along a row, 12 B of frame b where the transition points.  Only
// 3/16 of the bytes of the rows the lattice touches are used (every fourth row is touched at all), so the pass is bound by
// the number of memory transactions, not by bytes -- vstab_fill_gain_sums' cost warning.
#include "vstab_internal.h"

namespace {

constexpr int DF_THREADS = 256;
constexpr int DF_S = VSTAB_DEFLICKER_STRIDE;
constexpr int DF_BINS = VSTAB_DEFLICKER_BINS;
constexpr unsigned DF_LO = VSTAB_DEFLICKER_LO, DF_HI = VSTAB_DEFLICKER_HI;
constexpr unsigned DF_ITEMS_PER_BLOCK = 4096;     // lattice pixels a workgroup takes at least (16 per lane) where the pair has them:
                                                  // a flush of up to 4096 bins then costs less than the counting did
constexpr unsigned DF_TARGET_BLOCKS = 8192;       // over all pairs; beyond it the kernel's loop takes the rest

// a pair that takes part: its transition, where its outputs go, and (sums only) its bands
struct DfPair {
    float m[9];
    int pair;
    int band[8];     // [c][lo, hi]
};

// the blended fill's quantiser (vstab_neighbour.hip: gain_q)
__device__ __forceinline__ unsigned df_q(float v) { return v > 0.f ? (v < 1.f ? (unsigned)(v * 65536.0f) : 65536u) : 0u; }

// grid (blocks_per_pair * active pairs); lw x lh lattice pixels per pair
template <bool SUMS>
__global__ __launch_bounds__(DF_THREADS) void pair_gain_kernel(const float* __restrict__ src, const DfPair* __restrict__ recs, int h, int w,
                                                               int lw, int lh, unsigned blocks_per_pair, unsigned* __restrict__ hist,
                                                               unsigned* __restrict__ stats, unsigned long long* __restrict__ sums)
{
    __shared__ unsigned s_hist[SUMS ? 1 : 4 * DF_BINS];
    const unsigned t = threadIdx.x;
    const unsigned slot_pair = blockIdx.x / blocks_per_pair, slot = blockIdx.x - slot_pair * blocks_per_pair;
    const DfPair& rec = recs[slot_pair];
    const int pair = rec.pair;
    PairMatrix A;
    for (int k = 0; k < 9; k++) A.m[k] = (double)rec.m[k];
    const size_t frame = (size_t)h * w * 3;
    const float* __restrict__ fa = src + (size_t)pair * frame;
    const float* __restrict__ fb = fa + frame;

    if (!SUMS) {
        for (unsigned i = t; i < 4u * DF_BINS; i += DF_THREADS) s_hist[i] = 0u;
        __syncthreads();
    }
    unsigned inside = 0u, well = 0u;
    unsigned cnt[4] = {0u, 0u, 0u, 0u};
    unsigned long long sa[4] = {0ull, 0ull, 0ull, 0ull}, sb[4] = {0ull, 0ull, 0ull, 0ull};
    const unsigned items = (unsigned)lw * (unsigned)lh;     // < 2^27
    for (unsigned item = slot * DF_THREADS + t; item < items; item += blocks_per_pair * DF_THREADS) {
        const unsigned ly = item / (unsigned)lw, lx = item - ly * (unsigned)lw;
        const int x = (int)lx * DF_S + DF_S / 2, y = (int)ly * DF_S + DF_S / 2;     // < w, < h by the lattice's size
        int q;
        if (!vstab_pair_lookup(A, x, y, h, w, &q)) continue;
        inside += 1u;
        const float* __restrict__ pa = fa + ((size_t)y * w + x) * 3;
        const float* __restrict__ pb = fb + (size_t)q * 3;
        unsigned qa[4], qb[4];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            qa[c] = df_q(pa[c]);
            qb[c] = df_q(pb[c]);
            ok = ok && qa[c] >= DF_LO && qa[c] <= DF_HI && qb[c] >= DF_LO && qb[c] <= DF_HI;
        }
        if (!ok) continue;
        well += 1u;
        qa[3] = qa[0] + qa[1] + qa[2];
        qb[3] = qb[0] + qb[1] + qb[2];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const unsigned bin = min((qb[c] * 256u) / qa[c], (unsigned)(DF_BINS - 1));
            if (SUMS) {
                if ((int)bin >= rec.band[2 * c] && (int)bin <= rec.band[2 * c + 1]) {
                    cnt[c] += 1u;
                    sa[c] += qa[c];
                    sb[c] += qb[c];
                }
            } else {
                atomicAdd(&s_hist[c * DF_BINS + bin], 1u);
            }
        }
    }

    if (SUMS) {
        __shared__ BlockSums<unsigned long long, 12, DF_THREADS> s_sum;
        unsigned long long v[12];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            v[3 * c] = cnt[c];
            v[3 * c + 1] = sa[c];
            v[3 * c + 2] = sb[c];
        }
        s_sum.put(v);
        __syncthreads();
        if (t < 12) {
            const unsigned long long total = s_sum.total(t);
            if (total) atomicAdd(&sums[(size_t)pair * 12 + t], total);      // (a zero count comes with zero sums)
        }
    } else {
        __shared__ BlockSums<unsigned, 2, DF_THREADS> s_stat;
        s_stat.put({inside, well});
        __syncthreads();      // also: every lane's LDS atomics are done
        if (t < 2) {
            const unsigned total = s_stat.total(t);
            if (total) atomicAdd(&stats[(size_t)pair * 2 + t], total);
        }
        unsigned* __restrict__ out = hist + (size_t)pair * 4 * DF_BINS;
        for (unsigned i = t; i < 4u * DF_BINS; i += DF_THREADS) {
            const unsigned v = s_hist[i];
            if (v) atomicAdd(&out[i], v);
        }
    }
}

// ---- apply ------------------------------------------------------------------------------------------------------------
constexpr unsigned AG_TILE_FLOATS = 3072;             // 1024 pixels: 768 float4, three per thread
constexpr unsigned AG_TILE_VECS = AG_TILE_FLOATS / 4;
constexpr unsigned AG_TILE_PIXELS = AG_TILE_FLOATS / 3;
constexpr unsigned AG_TARGET_BLOCKS = 4096;

typedef float ag_f4 __attribute__((ext_vector_type(4)));

struct AgFrame {
    int frame;
    float g[3];
};

// one value of the rule; own: the pixel's mask is not 1.0f
__device__ __forceinline__ float ag_value(float v, float g, bool own, unsigned* clamped)
{
    if (!own || g == 1.0f || !(v == v)) return v;
    float out = v * g;
    if (out > 1.0f && v <= 1.0f) {
        out = 1.0f;
        *clamped += 1u;
    }
    return out;
}

__device__ __forceinline__ bool ag_own(const float* mask, size_t p) { return mask == nullptr || !(mask[p] == 1.0f); }

// grid (blocks_per_frame * frames with a gain); px = h * w < 2^31
__global__ __launch_bounds__(DF_THREADS) void apply_gain_kernel(float* __restrict__ frames, const float* __restrict__ mask,
                                                                const AgFrame* __restrict__ recs, unsigned px, unsigned blocks_per_frame,
                                                                unsigned* __restrict__ clamped_out)
{
    __shared__ BlockSums<unsigned, 1, DF_THREADS> s_cl;
    const unsigned t = threadIdx.x;
    const unsigned slot_frame = blockIdx.x / blocks_per_frame, slot = blockIdx.x - slot_frame * blocks_per_frame;
    const AgFrame rec = recs[slot_frame];
    const size_t floats = (size_t)px * 3;
    float* __restrict__ f = frames + (size_t)rec.frame * floats;
    const float* __restrict__ m = mask ? mask + (size_t)rec.frame * px : nullptr;
    const float g0 = rec.g[0], g1 = rec.g[1], g2 = rec.g[2];
    auto gain = [&](unsigned c) { return c == 0u ? g0 : (c == 1u ? g1 : g2); };      // (selects: no indexed register array)
    unsigned clamped = 0u;

    const unsigned head = (4u - (unsigned)(((uintptr_t)f >> 2) & 3)) & 3u;
    const unsigned vecs = floats > head ? (unsigned)((floats - head) >> 2) : 0u;   // < 3 * 2^29
    float4* __restrict__ vf = reinterpret_cast<float4*>(f + head);
    const unsigned tiles = (vecs + AG_TILE_VECS - 1) / AG_TILE_VECS;
    for (unsigned tile = slot; tile < tiles; tile += blocks_per_frame) {
        const unsigned v0 = tile * AG_TILE_VECS;
#pragma unroll
        for (unsigned r = 0; r < AG_TILE_VECS / DF_THREADS; r++) {
            const unsigned vl = t + r * DF_THREADS;   // float4 within the tile
            if (v0 + vl >= vecs) break;
            // the float4 holds the floats head + 4 * (v0 + vl) + {0..3} of the frame: the last 3 - c0 channels of pixel p0 and
            // the first c0 + 1 of pixel p0 + 1 (whose first float is in the frame, so p0 + 1 < px)
            const unsigned jl = head + 4u * vl;
            const unsigned pl = jl / 3u, c0 = jl - 3u * pl;
            const size_t p0 = (size_t)tile * AG_TILE_PIXELS + pl;
            const bool o0 = ag_own(m, p0), o1 = ag_own(m, p0 + 1);
            if (!o0 && !o1) continue;                 // both padded: nothing is loaded, nothing stored
            float4 x = vf[v0 + vl];
            // channels of the four floats: c0, c0+1, c0+2, c0+3 (mod 3); the pixel changes behind channel 2
            const unsigned c1 = c0 == 2u ? 0u : c0 + 1u, c2 = c1 == 2u ? 0u : c1 + 1u;
            x.x = ag_value(x.x, gain(c0), o0, &clamped);
            x.y = ag_value(x.y, gain(c1), c0 == 2u ? o1 : o0, &clamped);
            x.z = ag_value(x.z, gain(c2), c0 == 0u ? o0 : o1, &clamped);
            x.w = ag_value(x.w, gain(c0), o1, &clamped);
#ifdef VSTAB_DEFLICKER_NT_STORES      // the measured alternative: a second build with this define, timed by tools/deflicker_report.py; not shipped
            __builtin_nontemporal_store(ag_f4{x.x, x.y, x.z, x.w}, reinterpret_cast<ag_f4*>(vf + v0 + vl));
#else
            vf[v0 + vl] = x;
#endif
        }
    }
    // the floats in front of and behind the float4s: at most 6, by the frame's first workgroup
    if (slot == 0 && t < 6) {
        const size_t tail0 = (size_t)head + 4 * (size_t)vecs;
        const size_t j = t < 3 ? (size_t)t : tail0 + (t - 3);
        const bool mine = t < 3 ? (t < head && j < floats) : (j < floats);
        if (mine) {
            const size_t p = j / 3;
            f[j] = ag_value(f[j], gain((unsigned)(j - 3 * p)), ag_own(m, p), &clamped);
        }
    }

    if (clamped_out == nullptr) return;
    s_cl.put({clamped});
    __syncthreads();
    if (t == 0) {
        const unsigned total = s_cl.total(0);
        if (total) atomicAdd(&clamped_out[rec.frame], total);
    }
}

// The two measuring entries behind their argument checks: the records of the active pairs, the launch geometry, the launch.
template <bool SUMS>
int pair_gain_launch(vstab_ctx* ctx, const char* who, const char* kind, const float* src, int n, int h, int w, const float* transitions,
                     const uint8_t* active, const int32_t* band, uint32_t* hist, uint32_t* stats, uint64_t* sums)
{
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 2 && h >= 1 && w >= 1, "%s: needs at least two frames of a positive size (n=%d, %dx%d)", who, n, w, h);
    VSTAB_REQUIRE(src != nullptr && transitions != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE(SUMS ? (band != nullptr && sums != nullptr) : (hist != nullptr && stats != nullptr), "%s: NULL pointer argument", who);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)hist & 3) == 0 && ((uintptr_t)stats & 3) == 0 && ((uintptr_t)sums & 7) == 0,
                  "%s: a pointer argument is not aligned to its element size", who);
    const int pairs = n - 1;
    // lattice pixels per axis: x = S/2 + S * i < w
    const int lw = (w + DF_S - 1 - DF_S / 2) / DF_S, lh = (h + DF_S - 1 - DF_S / 2) / DF_S;
    std::vector<DfPair> recs;
    recs.reserve((size_t)pairs);
    for (int k = 0; k < pairs; k++) {
        if (active != nullptr && active[k] == 0) continue;
        DfPair r;
        memcpy(r.m, transitions + (size_t)k * 9, sizeof(r.m));
        r.pair = k;
        for (int j = 0; j < 8; j++) r.band[j] = SUMS ? band[(size_t)k * 8 + j] : 0;
        recs.push_back(r);
    }
    VSTAB_HIP(hipSetDevice(ctx->device));
    if (SUMS) {
        VSTAB_HIP(hipMemsetAsync(sums, 0, (size_t)pairs * 12 * sizeof(uint64_t), ctx->stream));
    } else {
        VSTAB_HIP(hipMemsetAsync(hist, 0, (size_t)pairs * 4 * DF_BINS * sizeof(uint32_t), ctx->stream));
        VSTAB_HIP(hipMemsetAsync(stats, 0, (size_t)pairs * 2 * sizeof(uint32_t), ctx->stream));
    }
    const size_t items = (size_t)lw * (size_t)lh;
    if (recs.empty() || items == 0) return 0;         // nothing to read: the zeros are the answer
    size_t per_pair = (items + DF_ITEMS_PER_BLOCK - 1) / DF_ITEMS_PER_BLOCK;
    const size_t cap = (DF_TARGET_BLOCKS + recs.size() - 1) / recs.size();
    if (per_pair > cap) per_pair = cap;
    VSTAB_REQUIRE(per_pair * recs.size() <= 0x7fffffffull, "%s: n=%d frames exceed the grid", who, n);
    void* d_recs = nullptr;
    if (int rc = vstab_stage_params(ctx, recs.data(), recs.size() * sizeof(DfPair), &d_recs)) return rc;
    KernelTimer timer(ctx, kind);
    hipLaunchKernelGGL(pair_gain_kernel<SUMS>, dim3((unsigned)(per_pair * recs.size())), dim3(DF_THREADS), 0, ctx->stream, src,
                       static_cast<const DfPair*>(d_recs), h, w, lw, lh, (unsigned)per_pair, hist, stats,
                       reinterpret_cast<unsigned long long*>(sums));
    VSTAB_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int vstab_pair_gain_hist_batch(vstab_ctx* ctx, const float* src, int n, int h, int w, const float* transitions,
                                          const uint8_t* active, uint32_t* hist, uint32_t* stats)
{
    return pair_gain_launch<false>(ctx, "vstab_pair_gain_hist_batch", "gain_hist", src, n, h, w, transitions, active, nullptr, hist, stats,
                                   nullptr);
}

extern "C" int vstab_pair_gain_sums_batch(vstab_ctx* ctx, const float* src, int n, int h, int w, const float* transitions,
                                          const uint8_t* active, const int32_t* band, uint64_t* sums)
{
    return pair_gain_launch<true>(ctx, "vstab_pair_gain_sums_batch", "gain_sums", src, n, h, w, transitions, active, band, nullptr, nullptr,
                                  sums);
}

extern "C" int vstab_apply_gain_batch(vstab_ctx* ctx, float* frames, const float* mask, int n, int h, int w, const float* gains,
                                      uint32_t* clamped)
{
    const char* who = "vstab_apply_gain_batch";
    VSTAB_REQUIRE(ctx != nullptr, "%s: NULL context", who);
    VSTAB_REQUIRE(n >= 1 && h >= 1 && w >= 1, "%s: bad shape n=%d h=%d w=%d", who, n, h, w);
    VSTAB_REQUIRE(frames != nullptr && gains != nullptr, "%s: NULL pointer argument", who);
    VSTAB_REQUIRE((long long)h * w < (1ll << 31), "%s: %d x %d pixels per frame, the limit is 2^31 - 1", who, w, h);
    VSTAB_REQUIRE((((uintptr_t)frames | (uintptr_t)mask | (uintptr_t)clamped) & 3) == 0,
                  "%s: a pointer argument is not aligned to its element size", who);
    std::vector<AgFrame> recs;
    for (int k = 0; k < n; k++) {
        const float* g = gains + (size_t)k * 3;
        if (g[0] == 1.0f && g[1] == 1.0f && g[2] == 1.0f) continue;      // not read at all
        recs.push_back(AgFrame{k, {g[0], g[1], g[2]}});
    }
    VSTAB_HIP(hipSetDevice(ctx->device));
    if (clamped != nullptr) VSTAB_HIP(hipMemsetAsync(clamped, 0, (size_t)n * sizeof(uint32_t), ctx->stream));
    if (recs.empty()) return 0;
    const unsigned px = (unsigned)((long long)h * w);
    const size_t tiles = ((size_t)px * 3 + AG_TILE_FLOATS - 1) / AG_TILE_FLOATS;
    size_t per_frame = (AG_TARGET_BLOCKS + recs.size() - 1) / recs.size();
    if (per_frame > tiles) per_frame = tiles;
    VSTAB_REQUIRE(per_frame * recs.size() <= 0x7fffffffull, "%s: n=%d frames exceed the grid", who, n);
    void* d_recs = nullptr;
    if (int rc = vstab_stage_params(ctx, recs.data(), recs.size() * sizeof(AgFrame), &d_recs)) return rc;
    KernelTimer timer(ctx, "apply_gain");
    hipLaunchKernelGGL(apply_gain_kernel, dim3((unsigned)(per_frame * recs.size())), dim3(DF_THREADS), 0, ctx->stream, frames, mask,
                       static_cast<const AgFrame*>(d_recs), px, (unsigned)per_frame, clamped);
    VSTAB_HIP(hipGetLastError());
    return 0;
}
