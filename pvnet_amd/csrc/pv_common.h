// pv_common.h -- what every stage of the voting library shares: constants,
// the reference's exact arithmetic, the counter RNG, the mask / vertex views,
// the workspace layout, agent-scope loads and stores, and the wave / row /
// block reductions.  No kernels; everything is inline in namespace pvv
// (hidden visibility: nothing here is exported from libpvvote.so).
//
// -ffp-contract=off matters (pvnet_amd/build.py): every expression that
// restates reference arithmetic must round after each operation.  The few
// fused multiply-adds the kernels want (the approximate vote test) are
// written as explicit fmaf() calls.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <array>
#include <atomic>

#include <algorithm>
#include <type_traits>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pvvote.h"
#include "pv_tunables.h"
#include "pv_rng.h"
#include "pv_hypclass.h"

namespace pvv __attribute__((visibility("hidden"))) {

constexpr int kWave = 64;
constexpr int kCompactChunk = 256;           // pixels per compaction block (one per thread)
constexpr int kVoteChunk = 256;              // pixels per LDS-staged sub-chunk of the vote waves
constexpr int kRefineNJ = PVV_REFINE_NJ;     // refine blocks per (image, keypoint)
constexpr int kRT = PVV_REFINE_T;            // refine block threads
// a refine block's published partial: 5 least-squares sums (fp64) + its winner
// (ratio, index), each value as one 16-B pair of tagged 8-B granules
constexpr int kRefineGran = 6;
constexpr int kRefineLdsHyp = 1024;          // hypotheses per keypoint kept in LDS (more: k_refine_solve<true>)
// domain of the fast test's error bound (the hypotheses' side, kHypMax / kLattice / kMHypMax, hyp_exact_only
// and hyp_class: pv_hypclass.h, included above)
constexpr float kN1Max = 1.0e18f;            // |direction| above -> exact-only pixel
// The two norm1 tests of a pixel on its squared norm s (fl(fl(nx nx) + fl(ny ny)),
// the reference's own sum): the correctly rounded sqrtf is monotone, so
// sqrtf(s) <= c holds exactly for s <= T with T the largest float whose root
// rounds to <= c.  c = 1e-6f = 0x1.0c6f7ap-20: c^2 = 0x1.19799812...p-40; T =
// 0x1.19799ap-40 has sqrtf(T) = c and its successor's root is c's successor.
// c = 1e18f = 0x1.bc16d6p+59: c^2 = 0x1.812f9b7d...p+119; T = 0x1.812f9cp+119
// likewise.  NaN fails both forms; +inf and every s above T fail both, a
// subnormal or zero s passes both.  tests/test_norm_constants.py checks the
// equivalence around both constants and over the whole positive range.
constexpr float kN1SqLow = 0x1.19799ap-40f;  // sqrtf(s) <= 1e-6f   <=>  s <= kN1SqLow
constexpr float kN1SqMax = 0x1.812f9cp+119f; // sqrtf(s) <= kN1Max  <=>  s <= kN1SqMax

__host__ __device__ inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// --------------------------------------------------------------------------
// exact reference arithmetic (contraction is off for the whole library)
// --------------------------------------------------------------------------

// KU's guards compare a float against the double 1e-6: (double)x < 1e-6 holds
// exactly when x <= 1e-6f (the float nearest 1e-6 lies below it), so the
// guard runs in f32 without the two f64 conversions (NaN: false either way)
__device__ __forceinline__ bool below_1e6(float x) { return x <= 1e-6f; }

// KU:107-125: one (h, v, t) decision.
__device__ __forceinline__ bool exact_vote(float nx, float ny, float cx, float cy, float hx, float hy,
                                           float thr) {
    float dx = hx - cx;
    float dy = hy - cy;
    float norm1 = sqrtf(nx * nx + ny * ny);
    float norm2 = sqrtf(dx * dx + dy * dy);
    if (below_1e6(norm1) || below_1e6(norm2)) return false;
    float angle_dist = (dx * nx + dy * ny) / (norm1 * norm2);
    return angle_dist > thr;
}

// exact_vote's decision for K6's one hypothesis per keypoint, settled by a
// squared comparison where that is provably the same (*und: not settled, the
// exact sequence must decide): on the domain below
// (squared norms in [1e-11, 1e18]: KU's 1e-6 guards pass, nothing over- or
// underflows) the exact sequence's angle is dot / (|n| |d|) within 4 roundings
// (2.4e-7 relative) and dot^2 / (thr^2 |n|^2 |d|^2) is within 5 roundings of
// its square, so outside a 2e-6 band around equality both decide alike;
// inside the band, outside the domain, or for thr outside [1e-3, 1] (`fast`
// false), the exact sequence decides.  `thr2` = thr * thr.
__device__ __forceinline__ void refine_vote_pre(float nx, float ny, float cx, float cy, float hx, float hy,
                                                float thr2, bool fast, bool *inl, bool *und) {
    const float dx = hx - cx, dy = hy - cy;
    const float nn1 = nx * nx + ny * ny;
    const float nn2 = dx * dx + dy * dy;
    const float dot = dx * nx + dy * ny;   // the exact sequence's numerator, bit for bit
    const bool dom = fast && nn1 >= 1e-11f && nn1 <= 1e18f && nn2 >= 1e-11f && nn2 <= 1e18f;
    const float l = dot * dot, r = thr2 * nn1 * nn2;
    const bool pos = dot > 0.f;            // else angle <= 0 < thr (or NaN): outlier
    const bool in = pos && l > r * (1.f + 2e-6f);
    const bool out = !pos || l < r * (1.f - 2e-6f);
    *inl = dom && in;
    *und = !dom || !(in || out);
}

// KU:28-48: intersection of the lines through two pixels. false = degenerate.
__device__ __forceinline__ bool exact_intersect(float dx0, float dy0, float cx0, float cy0, float dx1, float dy1,
                                                float cx1, float cy1, float *ox, float *oy) {
    float nx0 = dy0, ny0 = -dx0;
    float nx1 = dy1, ny1 = -dx1;
    float d0 = nx1 * ny0 - nx0 * ny1;
    if (below_1e6(fabsf(d0))) return false;
    float d1 = ny1 * nx0 - ny0 * nx1;
    if (below_1e6(fabsf(d1))) return false;
    float p0 = nx0 * cx0 + ny0 * cy0;
    float p1 = nx1 * cx1 + ny1 * cy1;
    *oy = (nx1 * p0 - nx0 * p1) / d0;
    *ox = (ny1 * p0 - ny0 * p1) / d1;
    return true;
}

__device__ __forceinline__ uint64_t ballot(bool x) { return __ballot(x); }

__device__ __forceinline__ int lane_id() { return __lane_id(); }

__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ float bcast(float x, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), lane));
}

// plain POD read through the constant address space -> s_load (scalar) loads
struct alignas(16) F4 { float x, y, z, w; };

// operands and result of v_mfma_f32_32x32x8_f16 (k_vote_mfma, k_debug_mfma_sums)
typedef _Float16 h4f __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// (the counter RNG -- mix64, hash32, rand_index, rand_unit -- is pv_rng.h, included above)

// --------------------------------------------------------------------------
// masks
// --------------------------------------------------------------------------
struct MaskView {
    const void *p;
    int64_t s0, s1, s2, s3;
};

// foreground predicate.  V3: RV:533 `mask.byte()` != 0.  EVD: RV:340 `mask == 1`.
// SEG: argmax over 2 logits == 1 (torch.argmax: first max wins, NaN is max).
template <int KIND, bool EVD>
__device__ __forceinline__ bool is_fg(const MaskView &m, int b, int r, int c) {
    if constexpr (KIND == PV_MASK_SEG_F32 || KIND == PV_MASK_SEG_F16) {
        int64_t o = b * m.s0 + r * m.s2 + c * m.s3;
        float s0, s1;
        if constexpr (KIND == PV_MASK_SEG_F32) {
            s0 = ((const float *)m.p)[o];
            s1 = ((const float *)m.p)[o + m.s1];
        } else {
            s0 = __half2float(((const __half *)m.p)[o]);
            s1 = __half2float(((const __half *)m.p)[o + m.s1]);
        }
        if (isnan(s0)) return false;
        if (isnan(s1)) return true;
        return s1 > s0;
    } else {
        int64_t o = b * m.s0 + r * m.s1 + c * m.s2;
        int64_t v;
        if constexpr (KIND == PV_MASK_I64) v = ((const int64_t *)m.p)[o];
        else if constexpr (KIND == PV_MASK_I32) v = ((const int32_t *)m.p)[o];
        else v = ((const uint8_t *)m.p)[o];
        if constexpr (EVD) return v == 1;
        else return (uint8_t)v != 0;
    }
}

// the [b,H,W,vn,2] vertex field through its strides (elements)
struct VertexView {
    const void *p;
    int kind;
    int64_t s[5];
    int32_t extent;     // bytes spanned by one image's [h,w,vn,2] view (< 2^31: buffer-load range)
    // multi-object calls (ncls >= 1; 0: one object per image): the view holds
    // ncls * vn keypoint channels, extent spans all of them, and the pipeline's
    // image index is the virtual image bv = bi * ncls + c
    int32_t ncls;
    int64_t cs;         // elements between two classes' first channels (vn * s[3])
};

// Image `b`'s base (bytes from vx.p) and the bytes from there to the end of the
// image's view: the buffer descriptor of its loads.  MC: b is a virtual image,
// the base is shifted to its class's channels and the range shortened by as
// much, so a clamped load still ends inside the tensor.
template <bool MC>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t image_rsrc(const VertexView &vx, int b, int es) {
    int64_t base = (int64_t)b * vx.s[0] * es;
    int32_t range = vx.extent;
    if constexpr (MC) {
        const int bi = b / vx.ncls, c = b - bi * vx.ncls;
        const int64_t shift = c * vx.cs * es;
        base = (int64_t)bi * vx.s[0] * es + shift;
        range = vx.extent - (int32_t)shift;
    }
    return __builtin_amdgcn_make_buffer_rsrc((void *)((const char *)vx.p + base), (short)0, range, 0x00020000);
}

// --------------------------------------------------------------------------
// workspace
// --------------------------------------------------------------------------
struct Workspace {
    // the hypotheses' classes (pv_hypclass.h), the workspace's first bytes: per 32 hypotheses of a keypoint the
    // ballot of the fast ones and the ballot of the exact-only ones, OR-ed in by the producers (compact_hyp,
    // k_hyp_gen) and read by the pipeline's k_vote_mfma; nset = 4 * ceil(nh / 128), bits past nh stay 0
    uint32_t *hypcls;   // [b][vn][nset][2] zeroed by k_fg_count
    int32_t *counts;    // [b][vn][nh]   zeroed by k_fg_count
    uint4 *refslot;     // [b][vn][kRefineNJ][kRefineGran] zeroed by k_fg_count: k_refine_solve's tagged partials
    int32_t *dsagg;     // [b][nblk]     zeroed by k_fg_count: downsampled count + 1 per block (look-back)
    int32_t *confc;     // [b][vn][2]    zeroed by k_fg_count: v5 confidence count, ticket
    int64_t zero_words; // hypcls + counts + refslot + dsagg + confc (contiguous, from hypcls)
    int32_t *tn;        // [b] compacted pixels (0 = image skipped)
    int32_t *fgtot;     // [b] foreground before downsampling
    int32_t *blkcnt;    // [b][nblk]
    int32_t *grpcnt;    // [b][ceil(nblk / kFgWideCPB)]: the wide k_fg_count blocks' sums (large grids only)
    uint64_t *fgbits;   // [b][nblk][4] foreground ballot of each wave of a k_fg_count block
    uint64_t *keptbits; // [b][nblk][4] downsampled images: k_compact's kept ballots (for compact_hyp)
    float4 *pex;        // [b][vn][P]   exact pixel data (cx, cy, nx, ny): reference operands
    float2 *hyp;        // [b][nh][vn]  (reference layout)
    float2 *hypv;       // [b][vn][nh]  keypoint-major copy (pre-generated hypotheses)
    size_t total;
};

// 32-hypothesis sets per keypoint in Workspace::hypcls: four per 128-hypothesis group of the vote's work index
__host__ __device__ inline int64_t hyp_sets(int nh) { return 4 * (((int64_t)nh + 2 * kWave - 1) / (2 * kWave)); }

inline Workspace carve(void *base, int b, int H, int W, int vn, int nh) {
    Workspace w{};
    int64_t P = (int64_t)H * W;
    int64_t nblk = (P + kCompactChunk - 1) / kCompactChunk;
    char *p = (char *)base;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char *q = p ? p + off : nullptr; off = align_up(off + bytes, 256); return q; };
    const int64_t ncnt = align_up((int64_t)b * vn * nh, 4);            // refslot 16-B aligned
    const int64_t nslot = (int64_t)b * vn * kRefineNJ * kRefineGran;
    const int64_t ncls = align_up(2 * (int64_t)b * vn * hyp_sets(nh), 4);
    w.zero_words = ncls + ncnt + 4 * nslot + b * nblk + 2 * (int64_t)b * vn;
    w.hypcls = (uint32_t *)take(4 * w.zero_words);
    w.counts = w.hypcls ? (int32_t *)(w.hypcls + ncls) : nullptr;
    w.refslot = w.counts ? (uint4 *)(w.counts + ncnt) : nullptr;
    w.dsagg = w.counts ? (int32_t *)(w.refslot + nslot) : nullptr;
    w.confc = w.counts ? w.dsagg + b * nblk : nullptr;
    w.tn = (int32_t *)take(4 * b);
    w.fgtot = (int32_t *)take(4 * b);
    w.blkcnt = (int32_t *)take(4 * b * nblk);
    w.grpcnt = (int32_t *)take(4 * b * ((nblk + 7) / 8));
    w.fgbits = (uint64_t *)take(8 * 4 * b * nblk);
    w.keptbits = (uint64_t *)take(8 * 4 * b * nblk);
    w.pex = (float4 *)take(16 * b * vn * P);
    w.hyp = (float2 *)take(8 * (int64_t)b * nh * vn);
    w.hypv = (float2 *)take(8 * (int64_t)b * nh * vn);
    w.total = (size_t)off;
    return w;
}

// agent-scope (device-wide) relaxed atomics for the in-kernel hand-offs
template <typename T>
__device__ __forceinline__ void st_agent(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T ld_agent(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }


// --------------------------------------------------------------------------
// wave / row / block reductions (blocks of 256 threads = 4 waves), all on the
// VALU: DPP moves within each row of 16 lanes, v_permlane16_swap /
// v_permlane32_swap across the rows -- no ds_bpermute round trips (six serial
// LDS latencies in the __shfl_xor form)
// --------------------------------------------------------------------------
// wave sums (every lane gets the sum)
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ int wave_sum_i(int x) {
    x += dpp_i<0xB1>(x);
    x += dpp_i<0x4E>(x);
    x += dpp_i<0x141>(x);
    x += dpp_i<0x140>(x);
    const auto r16 = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    x = (int)(r16[0] + r16[1]);
    const auto r32 = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return (int)(r32[0] + r32[1]);
}
__device__ __forceinline__ double wave_sum_d(double x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// sum over each 16-lane row of the wave (every lane of a row gets its row's
// sum) by DPP moves: xor 1, xor 2, half-row mirror, row mirror -- VALU
// operations, not the LDS-routed ds_bpermute of __shfl_xor
template <int CTRL>
__device__ __forceinline__ double dpp_d(double x) {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t u) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t row_max_u64(uint64_t x) {
    uint64_t o;
    o = dpp_u64<0xB1>(x); x = o > x ? o : x;
    o = dpp_u64<0x4E>(x); x = o > x ? o : x;
    o = dpp_u64<0x141>(x); x = o > x ? o : x;
    o = dpp_u64<0x140>(x); x = o > x ? o : x;
    return x;
}
__device__ __forceinline__ double row_sum_d(double x) {
    x += dpp_d<0xB1>(x);    // quad_perm [1,0,3,2]
    x += dpp_d<0x4E>(x);    // quad_perm [2,3,0,1]
    x += dpp_d<0x141>(x);   // row_half_mirror: quad q <-> 1-q within each half row
    x += dpp_d<0x140>(x);   // row_mirror: half rows swapped
    return x;
}

// Wave-wide min / max (result in every lane), all on the VALU: DPP within
// each row of 16 lanes (quad xor 1, quad xor 2, half-row mirror, row
// mirror), then v_permlane16_swap and v_permlane32_swap across the rows
// (no LDS round trips, unlike ds_swizzle / ds_bpermute).
template <int CTRL>
__device__ __forceinline__ float dpp_f(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
template <bool MAX>
__device__ __forceinline__ float wave_reduce(float x) {
    auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); };
    x = op(x, dpp_f<0xB1>(x));    // quad_perm [1,0,3,2]
    x = op(x, dpp_f<0x4E>(x));    // quad_perm [2,3,0,1]
    x = op(x, dpp_f<0x141>(x));   // row_half_mirror
    x = op(x, dpp_f<0x140>(x));   // row_mirror
    const auto r16 = __builtin_amdgcn_permlane16_swap(__float_as_int(x), __float_as_int(x), false, false);
    x = op(__int_as_float(r16[0]), __int_as_float(r16[1]));
    const auto r32 = __builtin_amdgcn_permlane32_swap(__float_as_int(x), __float_as_int(x), false, false);
    return op(__int_as_float(r32[0]), __int_as_float(r32[1]));
}
__device__ __forceinline__ float wave_min(float x) { return wave_reduce<false>(x); }
__device__ __forceinline__ float wave_max(float x) { return wave_reduce<true>(x); }

// sum over the block of (x, y); `sh` holds >= 8 ints
__device__ __forceinline__ int2 block_sum2(int x, int y, int *sh) {
    x = wave_sum_i(x);
    y = wave_sum_i(y);
    __syncthreads();
    if (lane_id() == 0) { sh[threadIdx.x / 64] = x; sh[4 + threadIdx.x / 64] = y; }
    __syncthreads();
    return make_int2(sh[0] + sh[1] + sh[2] + sh[3], sh[4] + sh[5] + sh[6] + sh[7]);
}

// --------------------------------------------------------------------------
// host: a stage's run() instantiated for the call's mask kind and foreground
// predicate (F<KIND, EVD>::run(args...))
// --------------------------------------------------------------------------
template <template <int, bool> class F, typename... A>
int dispatch_mask(int kind, bool evd, A... args) {
    switch (kind) {
#define PV_CASE(K)                                                    \
    case K:                                                           \
        return evd ? F<K, true>::run(args...) : F<K, false>::run(args...);
        PV_CASE(PV_MASK_I64)
        PV_CASE(PV_MASK_U8)
        PV_CASE(PV_MASK_I32)
        PV_CASE(PV_MASK_SEG_F32)
        PV_CASE(PV_MASK_SEG_F16)
#undef PV_CASE
    default:
        return PV_EINVAL;
    }
}

}  // namespace pvv
