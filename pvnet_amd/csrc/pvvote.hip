// pvvote.hip -- MI355X (gfx950, CDNA4) implementation of PVNet's pixel-wise
// RANSAC keypoint voting, exported through the C ABI in include/pvvote.h.
//
// Reference (kennege/pvnet):
//   KU  lib/ransac_voting_gpu_layer/src/ransac_voting_kernel.cu
//   BND lib/ransac_voting_gpu_layer/src/ransac_voting.cpp
//   RV  lib/ransac_voting_gpu_layer/ransac_voting_gpu.py
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
// (see pvnet_amd/build.py).  -ffp-contract=off matters: every expression that
// restates reference arithmetic must round after each operation.  The few
// fused multiply-adds this file wants (the approximate vote test) are written
// as explicit fmaf() calls.
//
// Design notes (DESIGN.md has the long form):
//   * The (hypothesis, pixel) vote test runs in the pixel's rotated frame:
//     5 FMAs and a compare, no sqrt or division.  A rigorous error bound
//     puts a guard band around the threshold; pairs inside it, and
//     hypotheses / pixels outside the bound's domain, are re-decided with
//     the reference's exact IEEE sequence (KU:116-125), so every decision is
//     bit-identical to the reference's.
//   * v3 / EVD never materialise the [hn,vn,tn] inlier mask: the fused
//     vote/count kernel keeps per-hypothesis counts in registers (lane =
//     hypothesis, pixels broadcast from LDS).  The byte mask is produced only
//     by the API entry point voting_for_hypothesis, as coalesced 8-byte
//     stores (lane = 8 pixels, hypotheses broadcast from LDS).
//
// Files: this one holds the fused vote/count -- k_vote_mfma, k_vote_count,
// k_hyp_gen, their host side (fast_constants, launch_vote) and the entries
// that are the vote's own (pv_vote_counts, two debug hooks).  Every stage has
// its own translation unit, reached by the pipeline through pv_stages.h:
//   pvpipeline.hip the pipeline (front_half, v3 / v5 / motion / EVD) and the
//                  general C ABI (version, build config, errors, streams)
//   pvcompact.hip  k_fg_count, k_compact (+ the fused hypotheses)
//   pvrefine.hip   k_refine_solve, k_point_conf (v5 confidence)
//   pvevd.hip      k_evd_with_mean, k_evd_topk, k_motion_vote
//   pvapi.hip      the stand-alone API kernels the pipeline never launches:
//                  k_generate_api, k_vote_bytes (byte masks), VP, debug kernels
// Shared headers: pv_tunables.h (every -D default with its measurement),
// pv_common.h (constants, exact reference arithmetic, RNG, views, workspace,
// reductions), pv_host.h (rc / last / cu_count).
#include "pv_stages.h"

// Per-wave timestamp traces (tools/vote_trace.py, tools/compact_trace.py)
// exist only in trace builds (-DPVV_TRACE); the product kernels carry none.
#ifdef PVV_TRACE
#define PVV_TRACE_ON(a) ((a).trace != nullptr)
#else
#define PVV_TRACE_ON(a) false
#endif

namespace {

using namespace pvv;

// ==========================================================================
// K4: hypotheses (KU:11-49) + fused vote/count.
// counts[b][v][h] += #{t : inlier(h, v, t)}.
//
// k_vote_count (hn not a multiple of 512, or the test hook) makes its own
// hypotheses in the pipeline (pixel pairs from the caller or the counter RNG,
// RV:553; item_hyp) in its prologue, beside its first pixel loads; the unit
// whose range starts at pixel 0 of a (b, v, group) stores them in the
// reference layout (refine stage, diagnostics).  k_vote_mfma makes none: its
// hypotheses and their classes come from compact_hyp or k_hyp_gen.
//
// k_vote_count: lane = hypothesis (kHypLane = 2 per lane, groups of 128 per
// wave); the (image, keypoint, group, pixel) space is cut into equal
// contiguous ranges over persistent units.  With hn a multiple of 512 a unit
// is a block whose four waves take four groups against the same pixels, which
// the block stages once per 256-pixel sub-chunk in LDS; every wave then reads
// a pixel's four fast operands with one broadcast ds_read_b128, and the
// per-lane inlier count is one v_addc on the compare's VCC.
//
// The test (fast path) works in the pixel's rotated frame: with u the unit
// predicted direction and d = h - c,
//     x' = u.d,  y' = u x d,    cos(u,d) > thr  <=>  x' tau - |y'| > 0,
//     tau = sqrt(1 - thr^2) / thr   (0 < thr < 1),
// i.e. 2 subs + 4 mul/fma + 1 fma + compare: no sqrt, rsq or division.
// A pair is decided by the fast path only when |z| = |x' tau - |y'|| exceeds
// gz * D, where D >= |d| bounds the distance to every pixel of the chunk and
// gz covers both the fast path's rounding and the reference's own (<= 8 ulp
// on the cosine, KU:119-123); the rest (and hypotheses / pixels outside the
// bound's domain) are re-decided with the reference's exact sequence.  See
// DESIGN.md "Exactness of the fast vote test" for the derivation.
// ==========================================================================
// Share of unit w when the units come in four dispatch rounds of B = n / 4
// blocks each weighted rw[r]: a SIMD issues age-first, so a CU's first-
// dispatched block runs ahead of its later ones; weighting the earlier
// rounds more makes the four end together.  Contiguous and exact: unit w
// starts at total * (B * sum(rw[<r]) + i * rw[r]) / (B * sum(rw)).
// (rw[3] == 0: three rounds of n / 3 blocks)
__device__ __forceinline__ void round_share(uint32_t total, uint32_t n, uint32_t w, const int32_t *rw, uint32_t *lo,
                                            uint32_t *hi) {
    const uint32_t nr = rw[3] > 0 ? 4u : 3u;
    const uint64_t B = n / nr, W = (uint64_t)rw[0] + rw[1] + rw[2] + rw[3];
    auto pos = [&](uint32_t u) -> uint32_t {
        if (u >= n) return total;
        const uint32_t r = u / (uint32_t)B, i = u % (uint32_t)B;
        uint64_t pre = 0;
        for (uint32_t k = 0; k < r; ++k) pre += (uint64_t)rw[k];
        return (uint32_t)((uint64_t)total * (B * pre + (uint64_t)i * rw[r]) / (B * W));
    };
    *lo = pos(w);
    *hi = pos(w + 1);
}

// image b's compacted pixel count, clamped to [0, P]: the vote kernels size
// and index their work from it, so whatever the workspace holds (a caller
// that hands one workspace to two calls in flight), every pex / hypothesis
// index stays inside the image's P records
template <class A>
__device__ __forceinline__ int tn_at(const A &a, int b) {
    const int n = a.tn_dev ? a.tn_dev[b] : a.tn_host;
    return min(max(n, 0), a.P);
}

// the reference's operands of pixel t: (cx, cy, nx, ny)
template <bool PREPPED, class A>
__device__ __forceinline__ F4 pixel_exact(const A &a, int b, int v, int t) {
    if constexpr (PREPPED) {
        const float4 e = a.pex[((int64_t)b * a.vn + v) * a.P + t];
        return F4{e.x, e.y, e.z, e.w};
    } else {
        const float2 c = a.coords[(int64_t)b * a.P + t];
        const float2 d = a.raw[(int64_t)b * a.vn * a.P + (int64_t)v * a.raw_v + (int64_t)t * a.raw_t];
        return F4{c.x, c.y, d.x, d.y};
    }
}

// the hypothesis of lane h (exact value; (0, 0) for a degenerate pair, KU:33-41)
template <bool GEN, bool PREPPED>
__device__ __forceinline__ float2 item_hyp(const VoteArgs &a, int b, int v, int h, bool hl, int n, bool store) {
    float x = 0.f, y = 0.f;
    if (GEN) {
        if (hl) {
            int64_t gid = ((int64_t)b * a.nh + h) * a.vn + v;
            int t0, t1;
            if (a.idxs) {
                t0 = min(max(a.idxs[gid * 2], 0), n - 1);
                t1 = min(max(a.idxs[gid * 2 + 1], 0), n - 1);
            } else {
                const uint64_t key = (uint64_t)((((int64_t)a.b0 + b) * a.nh + h) * a.vn + v);
                t0 = rand_index(a.seed, key * 2, n);
                t1 = rand_index(a.seed, key * 2 + 1, n);
            }
            const F4 e0 = pixel_exact<PREPPED>(a, b, v, t0), e1 = pixel_exact<PREPPED>(a, b, v, t1);
            float ox, oy;
            if (exact_intersect(e0.z, e0.w, e0.x, e0.y, e1.z, e1.w, e1.x, e1.y, &ox, &oy)) { x = ox; y = oy; }
            if (store) {
                a.hyp_out[gid] = make_float2(x, y);
                if (a.diag_hyp) { a.diag_hyp[gid * 2] = x; a.diag_hyp[gid * 2 + 1] = y; }
            }
        }
    } else if (hl) {
        float2 q = a.hyp[b * a.hyp_sb + v * a.hyp_sv + h * a.hyp_sh];
        x = q.x; y = q.y;
    }
    return make_float2(x, y);
}

// wave w's share [lo, hi) of `total` items cut evenly over `nwaves` (32-bit: the callers keep total < 2^31)
__device__ __forceinline__ void even_share(uint32_t total, uint32_t nwaves, uint32_t w, uint32_t *lo, uint32_t *hi) {
    const uint32_t q = total / nwaves, rem = total - q * nwaves;
    *lo = w * q + min(w, rem);
    *hi = *lo + q + (w < rem ? 1u : 0u);
}

// fast data of one pixel from its raw direction (API path without a prepped array)
__device__ __forceinline__ float4 prep_pixel(float cx, float cy, float nx, float ny) {
    float n1 = sqrtf(nx * nx + ny * ny);                 // exactly the reference's norm1
    bool ok = !below_1e6(n1);
    double N = sqrt((double)nx * nx + (double)ny * ny);
    return make_float4(ok ? cx : __builtin_nanf(""), cy, (float)(nx / N), (float)(ny / N));
}

// fast data of a compacted pipeline pixel (cx, cy, nx, ny), made while the
// vote kernel stages it: validity by the reference's own norm1 (KU:119-121),
// the direction rounded per component after scaling by rsq (the fast test
// needs only its direction); *exo: votes, but outside the fast domain
__device__ __forceinline__ float4 prep_compacted(const F4 &e, bool *exo) {
    // norm1 = sqrtf(s) is only compared here, and sqrtf is monotone: the two
    // tests are made on s against kN1SqLow / kN1SqMax (pv_common.h), no root
    const float s = e.z * e.z + e.w * e.w;
    const bool valid = !(s <= kN1SqLow);
    const float rs = __builtin_amdgcn_rsqf(fmaf(e.z, e.z, e.w * e.w));
    *exo = valid && !(s <= kN1SqMax);
    return make_float4(valid ? e.x : __builtin_nanf(""), e.y, e.z * rs, e.w * rs);
}

__device__ __forceinline__ bool pixel_exotic(float nx, float ny) {
    float n1 = sqrtf(nx * nx + ny * ny);
    return !below_1e6(n1) && !(n1 <= kN1Max);     // votes, but outside the fast domain
}

// One segment = pixels [ts, te) of one (image b, keypoint v, hypothesis group
// hg) against the group's kGroup hypotheses (kHypLane per lane; pv_stages.h).
//
// Pixels are staged per sub-chunk of 256 in two LDS slabs of the wave: the
// fast operands (ux, uy, -k1, -k2) with k1 = u.c', k2 = u x c' and c' = c - o
// relative to the sub-chunk origin o (an integer corner of its bounding box,
// so c' is exact for pixel centres), and the reference's operands (cx, cy,
// nx, ny) for the rare exact decisions.  For h' = h - o:
//     x' = u.h' - k1,  y' = u x h' - k2,  z = x' tau - |y'|
// = 4 fma + 1 fma, a compare for the count and a min for the guard band.
// The band is gzf * B + gzr * D: B >= |h'| + |c'| bounds the fast path's own
// rounding (per sub-chunk), D >= |h - c| the reference's (per 64-pixel
// quarter, from the quarter's bounding box).

// The wave's slab of exact operands.  Pipeline pixels are integer centres
// below 65536 (check_desc), packed as cx | cy << 16: 12 B per pixel keeps a
// block at 28 KiB of LDS (5 blocks per CU); API coordinates are any floats.
template <bool PACKED, int N = kVoteChunk>
struct ExactSlab {
    float2 n[N];
    uint32_t c[N];
    __device__ __forceinline__ void put(int j, const F4 &e) {
        n[j] = make_float2(e.z, e.w);
        c[j] = (uint32_t)e.x | ((uint32_t)e.y << 16);
    }
    __device__ __forceinline__ F4 get(int j) const {
        const float2 d = n[j];
        const uint32_t q = c[j];
        return F4{(float)(q & 0xffffu), (float)(q >> 16), d.x, d.y};
    }
};
template <int N>
struct ExactSlab<false, N> {
    F4 e[N];
    __device__ __forceinline__ void put(int j, const F4 &x) { e[j] = x; }
    __device__ __forceinline__ F4 get(int j) const { return e[j]; }
};

// LDS of one sub-chunk: fast operands and exact operands
template <bool PREPPED>
struct VoteSlab {
    F4 stage[kVoteChunk];
    ExactSlab<PREPPED> x;
};
// block-shared staging: the four quarter bounding boxes and exotic flags
struct QuarterBoxes {
    float4 box[4];
    uint32_t exo[4];
};

//
// SH (block-shared staging): the block's four waves take the same pixels
// against four different hypothesis groups, so a sub-chunk is loaded and
// staged once per block (one pixel per thread, double-buffered slabs, one
// barrier per sub-chunk) instead of once per wave.  Its origin is the
// sub-chunk's first pixel (known to every wave without a reduction); the
// quarter boxes come through LDS.
template <bool PREPPED, bool SH>
__device__ __forceinline__ void vote_segment(const VoteArgs &a, VoteSlab<PREPPED> *slabs, QuarterBoxes *qbs, float2 *hlds, int &buf, int b, int v, int hg,
                                             int ts, int te, int n, uint32_t rem_after, uint32_t prio_hi, uint32_t prio_mid, int &nfix,
                                             uint64_t &tloop) {
    const int lane = lane_id();
    const int wid = SH ? (int)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave) : 0;
    // Issue priority from the work this wave still has (0..3): the SIMD's
    // arbiter otherwise favours the oldest wave, so equal shares finish
    // staggered and the last waves run alone; this keeps them level.
    // (levels 0..2: 3 is the prologue's, above every hot loop; the caller's
    // thresholds are ceil(2 (total + 1) / 3) and ceil((total + 1) / 3), so
    // the comparisons need no 64-bit products: 32-bit, wave-uniform)
    auto set_prio = [&](uint32_t remaining) {
        if (remaining >= prio_hi) __builtin_amdgcn_s_setprio(2);
        else if (remaining >= prio_mid) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
    };
    const float tau = a.tau;
    constexpr float kBig = 3.0e38f;

    // SH: the loads of a sub-chunk (this thread's pixel, the first pixel for
    // the origin); the first sub-chunk's are issued before the hypothesis
    // generation so that the two memory round trips overlap
    struct SubLoad {
        F4 f0, e;
    };
    auto load_sub = [&](int s0, int np) {
        SubLoad L;
        const int t = wid * kWave + lane;
        L.f0 = pixel_exact<PREPPED>(a, b, v, s0);
        L.e = F4{0.f, 0.f, 0.f, 0.f};
        if (t < np) L.e = pixel_exact<PREPPED>(a, b, v, s0 + t);
        return L;
    };
    SubLoad L;               // (loaded at the end of the previous sub-chunk: not live across its hot loop)
    if (SH) L = load_sub(ts, min(kVoteChunk, te - ts));

    // exact hypotheses (the reference's operands): SH keeps them in the wave's
    // LDS row (read per sub-chunk and by the rare exact decisions), which
    // frees their registers for the hot loop
    float2 he_r[kHypLane];
    auto he_set = [&](int i, float2 x) {
        if (SH) hlds[i * kWave + lane] = x;
        else he_r[i] = x;
    };
    auto he = [&](int i) -> float2 { return SH ? hlds[i * kWave + lane] : he_r[i]; };
    bool hf[kHypLane];       // decided by the fast test
    bool hxo[kHypLane];      // outside the fast test's domain: exact only
    int cnt[kHypLane];
#pragma unroll
    for (int i = 0; i < kHypLane; ++i) {
        const int h = hg * kGroup + i * kWave + lane;
        const bool hl = h < a.nh;
        // the pipeline (PREPPED) makes its hypotheses here: every block of
        // (b, v, group) intersects the same pixel pairs, the one whose range
        // starts at pixel 0 stores them (reference layout, for the refine /
        // EVD stages and the diagnostics); the API path reads the caller's
        const float2 hv = item_hyp<PREPPED, PREPPED>(a, b, v, h, hl, n, PREPPED && ts == 0);
        he_set(i, hv);
        const bool fin = isfinite(hv.x) && isfinite(hv.y);    // non-finite: never an inlier
        hxo[i] = hl && fin && hyp_exact_only(hv.x, hv.y);
        hf[i] = hl && fin && !hxo[i];
        cnt[i] = 0;
    }

    for (int s0 = ts; s0 < te; s0 += kVoteChunk) {
        const int np = min(kVoteChunk, te - s0);
        VoteSlab<PREPPED> &S = slabs[SH ? buf : 0];
        F4 *stage = S.stage;
        ExactSlab<PREPPED> &stagex = S.x;
        QuarterBoxes &QB = qbs[SH ? buf : 0];
        if (SH) buf ^= 1;
        float qxl = kBig, qxh = -kBig, qyl = kBig, qyh = -kBig;
        float cxl = kBig, cxh = -kBig, cyl = kBig, cyh = -kBig;
        float ox, oy, R;
        bool slow = !a.fast;
        if (SH) {
            const int t = wid * kWave + lane;
            ox = floorf(L.f0.x);
            oy = floorf(L.f0.y);
            if (!(fabsf(ox) <= 1.6e7f && fabsf(oy) <= 1.6e7f)) { ox = 0.f; oy = 0.f; }
            F4 q{__builtin_nanf(""), 0.f, 0.f, 0.f};
            float xl = kBig, xh = -kBig;
            bool exo_p = false;
            if (t < np) {
                const F4 e = L.e;
                if (PREPPED) {
                    const float4 f = prep_compacted(e, &exo_p);
                    q = F4{f.x, f.y, f.z, f.w};
                } else {
                    const float4 f = prep_pixel(e.x, e.y, e.z, e.w);
                    q = F4{f.x, f.y, f.z, f.w};
                    exo_p = pixel_exotic(e.z, e.w);
                }
                stagex.put(t, e);
                xl = e.x;
                xh = e.x;
            }
            {
                const float cx = q.x - ox, cy = q.y - oy;
                const float k1 = fmaf(q.z, cx, q.w * cy);
                const float k2 = fmaf(q.z, cy, -(q.w * cx));
                // a pixel that never votes (prep: cx NaN; the slab's padding):
                // u = 0, -k1 = -1e30 -> z = -1e30 tau < 0 and far outside the band
                stage[t] = q.x == q.x ? F4{q.z, q.w, -k1, -k2} : F4{0.f, 0.f, -1.0e30f, 0.f};
            }
            if (wid * kWave < np) {
                const float mn = wave_min(xl), mx = wave_max(xh);
                float yn, yx;
                if (PREPPED) {
                    yn = bcast(q.y, 0);
                    yx = bcast(q.y, min(kWave - 1, np - 1 - wid * kWave));
                } else {
                    const bool in = t < np;
                    yn = wave_min(in ? q.y : kBig);
                    yx = wave_max(in ? q.y : -kBig);
                }
                const uint32_t ex = __builtin_amdgcn_ballot_w64(exo_p) != 0;
                if (lane == 0) {
                    QB.box[wid] = make_float4(mn, mx, yn, yx);
                    QB.exo[wid] = ex;
                }
            } else if (lane == 0) {
                QB.box[wid] = make_float4(kBig, -kBig, kBig, -kBig);
                QB.exo[wid] = 0;
            }
            __syncthreads();
            uint32_t ex = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 Q = QB.box[k];
                cxl = fminf(cxl, Q.x); cxh = fmaxf(cxh, Q.y);
                cyl = fminf(cyl, Q.z); cyh = fmaxf(cyh, Q.w);
                ex |= QB.exo[k];
            }
            slow |= ex != 0;
            slow = __builtin_amdgcn_readfirstlane(slow);
            const float ax = fmaxf(cxh - ox, ox - cxl), ay = fmaxf(cyh - oy, oy - cyl);
            R = __builtin_amdgcn_sqrtf(fmaf(ax, ax, ay * ay)) * 1.00001f;
        } else {
        F4 q4[kVoteChunk / kWave];
        float xl[kVoteChunk / kWave], xh[kVoteChunk / kWave];
        bool exo_p = false;
#pragma unroll
        for (int k = 0; k < kVoteChunk / kWave; ++k) {
            const int j = k * kWave + lane;
            F4 q{__builtin_nanf(""), 0.f, 0.f, 0.f};
            xl[k] = kBig;
            xh[k] = -kBig;
            if (j < np) {
                const F4 e = pixel_exact<PREPPED>(a, b, v, s0 + j);
                if (PREPPED) {
                    bool xo;
                    const float4 f = prep_compacted(e, &xo);
                    q = F4{f.x, f.y, f.z, f.w};
                    exo_p |= xo;
                } else {
                    const float4 f = prep_pixel(e.x, e.y, e.z, e.w);
                    q = F4{f.x, f.y, f.z, f.w};
                    exo_p |= pixel_exotic(e.z, e.w);
                }
                stagex.put(j, e);
                xl[k] = e.x;
                xh[k] = e.x;
            }
            q4[k] = q;
        }
        slow |= __builtin_amdgcn_ballot_w64(exo_p) != 0;
        slow = __builtin_amdgcn_readfirstlane(slow);
        // per-quarter bounding boxes (lane k of qxl..qyh holds quarter k); the
        // compacted pixels are row-major, so a quarter's rows run from its
        // first pixel to its last (the API path takes arbitrary coordinates)
#pragma unroll
        for (int k = 0; k < kVoteChunk / kWave; ++k) {
            if (k * kWave < np) {
                const float mn = wave_min(xl[k]), mx = wave_max(xh[k]);
                float yn, yx;
                if (PREPPED) {
                    yn = bcast(q4[k].y, 0);
                    yx = bcast(q4[k].y, min(kWave - 1, np - 1 - k * kWave));
                } else {
                    const bool in = k * kWave + lane < np;
                    yn = wave_min(in ? q4[k].y : kBig);
                    yx = wave_max(in ? q4[k].y : -kBig);
                }
                if (lane == k) { qxl = mn; qxh = mx; qyl = yn; qyh = yx; }
                cxl = fminf(cxl, mn); cxh = fmaxf(cxh, mx);
                cyl = fminf(cyl, yn); cyh = fmaxf(cyh, yx);
            }
        }
        const bool empty = !(cxl <= cxh) || !(cyl <= cyh);
        ox = empty ? 0.f : floorf(cxl);
        oy = empty ? 0.f : floorf(cyl);
        R = empty ? 0.f : __builtin_amdgcn_sqrtf(fmaf(cxh - ox, cxh - ox, (cyh - oy) * (cyh - oy))) * 1.00001f;
        // stage the fast operands (ux, uy, -k1, -k2)
#pragma unroll
        for (int k = 0; k < kVoteChunk / kWave; ++k) {
            const F4 q = q4[k];
            const float cx = q.x - ox, cy = q.y - oy;          // exact for pixel centres
            const float k1 = fmaf(q.z, cx, q.w * cy);          // NaN for invalid pixels
            const float k2 = fmaf(q.z, cy, -(q.w * cx));
            stage[k * kWave + lane] = q.x == q.x ? F4{q.z, q.w, -k1, -k2} : F4{0.f, 0.f, -1.0e30f, 0.f};
        }
        __builtin_amdgcn_wave_barrier();
        }
        // lane constants of this sub-chunk
        float hx[kHypLane], hy[kHypLane], Bv[kHypLane], gd[kHypLane];
#pragma unroll
        for (int i = 0; i < kHypLane; ++i) {
            const float2 hv = he(i);
            hx[i] = hf[i] ? hv.x - ox : __builtin_nanf("");
            hy[i] = hf[i] ? hv.y - oy : __builtin_nanf("");
            Bv[i] = (__builtin_amdgcn_sqrtf(fmaf(hx[i], hx[i], hy[i] * hy[i])) + R) * 1.00001f + 1e-30f;
            gd[i] = 0.f;
        }
        // band of quarter k
        auto set_band = [&](int k) {
            float xn, xx, yn, yx;
            if (SH) {   // the block's quarter boxes are still in LDS: no registers held across the loop
                const float4 Q = QB.box[k];
                xn = Q.x - ox; xx = Q.y - ox; yn = Q.z - oy; yx = Q.w - oy;
            } else {
                xn = bcast(qxl, k) - ox; xx = bcast(qxh, k) - ox;
                yn = bcast(qyl, k) - oy; yx = bcast(qyh, k) - oy;
            }
#pragma unroll
            for (int i = 0; i < kHypLane; ++i) {
                const float ax = fmaxf(fabsf(hx[i] - xn), fabsf(hx[i] - xx));
                const float ay = fmaxf(fabsf(hy[i] - yn), fabsf(hy[i] - yx));
                const float D = fmaf(__builtin_amdgcn_sqrtf(fmaf(ax, ax, ay * ay)), 1.00001f, Bv[i] * 1e-6f);
                const float g = fmaf(a.gzr, D, a.gzf * Bv[i]);
                // a hypothesis outside the fast test (hx, hy NaN -> g NaN) gets
                // -1: its z is NaN, never counted, and it must never trigger
                // the band (the exact-only loop below decides it)
                gd[i] = g >= 0.f ? g : -1.f;
            }
        };
        if (!slow) {
            auto zval = [&](const F4 &q, float hxi, float hyi) {
                const float xr = fmaf(q.x, hxi, fmaf(q.y, hyi, q.z));      // u.h' - k1
                const float yr = fmaf(q.x, hyi, fmaf(-q.y, hxi, q.w));     // u x h' - k2
                return fmaf(xr, tau, -fabsf(yr));
            };
            // rare: some pair of pixels [j, j+4) is inside the band.  One (pixel,
            // hypothesis) pair per iteration, not unrolled, so the hot loop's
            // registers stay free; the exact operands come from the LDS slab.
            auto fix_step = [&](int j) {
#pragma unroll 1
                for (int pi = 0; pi < 4 * kHypLane; ++pi) {
                    const int p = pi / kHypLane, i = pi % kHypLane;
                    const float2 h0 = he(0);
                    float hxi = hx[0], hyi = hy[0], gdi = gd[0], ex = h0.x, ey = h0.y;
#pragma unroll
                    for (int k = 1; k < kHypLane; ++k) {
                        if (i == k) { const float2 hk = he(k); hxi = hx[k]; hyi = hy[k]; gdi = gd[k]; ex = hk.x; ey = hk.y; }
                    }
                    const float zz = zval(stage[j + p], hxi, hyi);
                    const bool u = fabsf(zz) <= gdi;
                    if (__builtin_amdgcn_ballot_w64(u)) {
                        const F4 e = stagex.get(j + p);
                        const int r = (u && exact_vote(e.z, e.w, e.x, e.y, ex, ey, a.thr)) ? 1 : 0;
                        const int f = (u && !signbit(zz)) ? 1 : 0;   // what the sign count took
#pragma unroll
                        for (int k = 0; k < kHypLane; ++k) cnt[k] += i == k ? r - f : 0;
                    }
                }
            };
            // 4 pixels x kHypLane hypotheses per step, LDS reads one step ahead
            // into two named buffers (no register copies).  The band is checked
            // once per step on min |z| per hypothesis (v_min ignores NaN, so
            // non-fast hypotheses never trigger it).
            // The fast count is a sign count: v_perm gathers the sign bytes
            // (0xff / 0x00) of 4 z values and v_sad_u8 adds them, 255 per
            // negative z -- 1 VALU op per pair instead of a compare and an
            // add-with-carry.  Pairs inside the band are re-decided by
            // fix_step, which also takes back what the sign count gave them.
            uint32_t neg[kHypLane];
#pragma unroll
            for (int i = 0; i < kHypLane; ++i) neg[i] = 0;
            uint64_t hitmask = 0;    // steps (4 pixels each) with a pair in the band
            auto step = [&](F4 q0, F4 q1, F4 q2, F4 q3, int j) {
                float m[kHypLane];
#pragma unroll
                for (int i = 0; i < kHypLane; ++i) m[i] = kBig;
                const F4 *qs[4] = {&q0, &q1, &q2, &q3};
                float z[4][kHypLane];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
#pragma unroll
                    for (int i = 0; i < kHypLane; ++i) {
                        z[p][i] = zval(*qs[p], hx[i], hy[i]);
                        m[i] = fminf(m[i], fabsf(z[p][i]));
                    }
                }
#pragma unroll
                for (int i = 0; i < kHypLane; ++i) {
                    const uint32_t p01 = __builtin_amdgcn_perm(__float_as_uint(z[1][i]), __float_as_uint(z[0][i]), 0x0c0c0b09u);
                    const uint32_t p23 = __builtin_amdgcn_perm(__float_as_uint(z[3][i]), __float_as_uint(z[2][i]), 0x0b090c0cu);
                    // p01 and p23 have no byte in common: sum |p01 - p23| = sum of both
                    neg[i] = __builtin_amdgcn_sad_u8(p01, p23, neg[i]);
                }
                // (one ballot per compare: the compare's VCC is the ballot)
                uint64_t hit = 0;
#pragma unroll
                for (int i = 0; i < kHypLane; ++i) hit |= __builtin_amdgcn_ballot_w64(m[i] <= gd[i]);
                // a step with a pair in the band is only noted here (bit j / 4 of
                // a wave-uniform mask) and re-decided after the loop: the exact
                // sequence's registers are then not live beside the hot loop's
                if (hit) hitmask |= 1ull << (j >> 2);
            };
            // the slab past np holds never-voting pixels (negative z, never in
            // the band), so the loop runs whole 8-pixel iterations
            const int nit = (np + 7) >> 3;
            F4 a0 = stage[0], a1 = stage[1], a2 = stage[2], a3 = stage[3];
            if (PVV_TRACE_ON(a) && tloop == 0) tloop = __builtin_amdgcn_s_memrealtime();   // (debug traces only)
            for (int it = 0; it < nit; ++it) {
                const int j = it * 8;
                if ((j & (kWave - 1)) == 0) {
                    set_band(j / kWave);
                    set_prio(rem_after + (uint32_t)(te - s0 - j));
                }
                const F4 b0 = stage[j + 4], b1 = stage[j + 5], b2 = stage[j + 6], b3 = stage[j + 7];
                step(a0, a1, a2, a3, j);
                const int jn = (j + 8) & (kVoteChunk - 1);
                a0 = stage[jn]; a1 = stage[jn + 1]; a2 = stage[jn + 2]; a3 = stage[jn + 3];
                step(b0, b1, b2, b3, j + 4);
            }
            // the band pairs, by the reference's sequence, under the band of
            // their own quarter (set_band is deterministic: the same gd as in the loop)
            {
                uint64_t hm = hitmask;
                int kq = -1;
                while (hm) {
                    const int j = __builtin_ctzll(hm) * 4;
                    hm &= hm - 1;
                    if ((j >> 6) != kq) { kq = j >> 6; set_band(kq); }
                    ++nfix;
                    fix_step(j);
                }
            }
            // positives = pairs stepped - negatives (never-voting pixels and the
            // padding are negative); hypotheses outside the fast test count 0 here
#pragma unroll
            for (int i = 0; i < kHypLane; ++i) cnt[i] += hf[i] ? 8 * nit - (int)(neg[i] / 255u) : 0;
            // exact-only hypotheses (rare): lane = pixel, one hypothesis at a time
#pragma unroll
            for (int i = 0; i < kHypLane; ++i) {
                uint64_t m = __builtin_amdgcn_ballot_w64(hxo[i]);
                while (m) {
                    const int l = __builtin_ctzll(m);
                    m &= m - 1;
                    float ex, ey;
                    if (SH) { const float2 hl2 = hlds[i * kWave + l]; ex = hl2.x; ey = hl2.y; }
                    else { ex = bcast(he_r[i].x, l); ey = bcast(he_r[i].y, l); }
                    int c = 0;
#pragma unroll
                    for (int k = 0; k < kVoteChunk / kWave; ++k) {
                        const int jj = k * kWave + lane;
                        bool e = false;
                        if (jj < np) {
                            const F4 x = stagex.get(jj);
                            e = exact_vote(x.z, x.w, x.x, x.y, ex, ey, a.thr);
                        }
                        c += __popcll(__builtin_amdgcn_ballot_w64(e));
                    }
                    if (lane == l) cnt[i] += c;
                }
            }
        } else {
            // every pair through the reference sequence
#pragma unroll 1
            for (int j = 0; j < np; ++j) {
                const F4 e = stagex.get(j);
#pragma unroll
                for (int i = 0; i < kHypLane; ++i) {
                    const float2 hv = he(i);
                    cnt[i] += exact_vote(e.z, e.w, e.x, e.y, hv.x, hv.y, a.thr);
                }
            }
        }
        if (!SH) __builtin_amdgcn_wave_barrier();
        if (SH && s0 + kVoteChunk < te) L = load_sub(s0 + kVoteChunk, min(kVoteChunk, te - s0 - kVoteChunk));
    }
    int32_t *cp = a.counts + (int64_t)b * a.cnt_bs + (int64_t)v * a.cnt_v;
#pragma unroll
    for (int i = 0; i < kHypLane; ++i) {
        const int h = hg * kGroup + i * kWave + lane;
        if (h < a.nh && cnt[i]) atomicAdd(&cp[(int64_t)h * a.cnt_h], cnt[i]);
    }
}

// Balanced persistent waves: the (image, keypoint, hypothesis group, pixel)
// work space is linearised with pixels fastest and cut into equal contiguous
// ranges, one per wave, so every wave does the same number of pixel steps and
// generates each group's hypotheses once per range.  SH: the unit is a block
// (its four waves = four consecutive hypothesis groups on the same pixels),
// the space is (image, keypoint, group of four groups, pixel); needs
// hgn % 4 == 0 (hn a multiple of 512).
template <bool PREPPED, bool SH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 5))) void k_vote_count(VoteArgs a) {
    const int wave = uniform((int)(blockIdx.x * 4 + threadIdx.x / 64));
    const int unit = SH ? (int)blockIdx.x : wave;
    const int64_t nunits = SH ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
    const int gpu = SH ? 4 : 1;           // hypothesis groups per unit
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    // the prologue (hypotheses, first sub-chunk) at the top issue priority:
    // the hot loops rank 0..2 by the work they have left (set_prio), and a
    // wave still in its prologue would otherwise wait behind them
    __builtin_amdgcn_s_setprio(3);
    __shared__ VoteSlab<PREPPED> slab_all[SH ? 2 : 4];
    __shared__ QuarterBoxes qb_all[SH ? 2 : 1];
    __shared__ float2 hyp_all[SH ? 4 * kGroup : 1];   // SH: each wave's exact hypotheses
    VoteSlab<PREPPED> *slabs = SH ? slab_all : slab_all + threadIdx.x / 64;
    int buf = 0;
    const int ggn = a.hgn / gpu;          // unit groups per keypoint
    // 32-bit index math (the host splits launches so that the work stays < 2^31)
    uint32_t total = 0;
    for (int b = 0; b < a.b; ++b) total += (uint32_t)(a.vn * ggn) * (uint32_t)tn_at(a, b);
    uint32_t lo, hi;
    if (SH && a.rw[0] > 0 && nunits % 4 == 0)
        round_share(total, (uint32_t)nunits, (uint32_t)unit, a.rw, &lo, &hi);
    else
        even_share(total, (uint32_t)nunits, (uint32_t)unit, &lo, &hi);
    // issue-priority thresholds of the wave's share (vote_segment set_prio)
    const uint32_t w1 = hi - lo + 1u;
    const uint32_t prio_hi = uniform((int)((2ull * w1 + 2) / 3)), prio_mid = uniform((int)((w1 + 2) / 3));
    int nfix = 0, nseg = 0;   // diagnostics (trace)
    uint64_t tloop = 0;       // (trace) first hot-loop entry
    // walk the segments of [lo, hi)
    int b = 0;
    uint32_t base = 0;
    while (lo < hi && b < a.b) {
        const int n = tn_at(a, b);
        const uint32_t span = (uint32_t)(a.vn * ggn) * (uint32_t)n;
        if (lo >= base + span) { base += span; ++b; continue; }
        const uint32_t r = lo - base;
        const int g = (int)(r / (uint32_t)n);               // (v, unit group) index
        const int ts = (int)(r - (uint32_t)g * n);
        const int te = (int)min((uint32_t)n, ts + (hi - lo));
        const int v = g / ggn, gg = g - v * ggn;
        const int hg = SH ? gg * 4 + (int)__builtin_amdgcn_readfirstlane(threadIdx.x / 64) : gg;
        vote_segment<PREPPED, SH>(a, slabs, qb_all, SH ? hyp_all + (threadIdx.x / 64) * kGroup : hyp_all, buf, uniform(b), uniform(v), uniform(hg), uniform(ts), uniform(te), n,
                                       uniform((int)((hi - lo) - (uint32_t)(te - ts))), prio_hi, prio_mid, nfix, tloop);
        lo += te - ts;
        ++nseg;
    }
    if (PVV_TRACE_ON(a) && lane_id() == 0) {
        uint32_t hw;
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        a.trace[wave * 8] = t_start;
        a.trace[wave * 8 + 1] = __builtin_amdgcn_s_memrealtime();
        a.trace[wave * 8 + 2] = ((uint64_t)xcc << 32) | hw;
        a.trace[wave * 8 + 3] = ((uint64_t)nseg << 32) | (uint32_t)nfix;
        a.trace[wave * 8 + 4] = tloop;
    }
}

#ifdef PVV_PROFILE
// profiling builds only (pv_debug_set_ablation bit 32): a launch that does nothing
__global__ void k_abl_empty(int) {}
#endif

// Hypotheses once per launch (pipeline, hyp_pregen), one thread per
// (image, hypothesis, keypoint): the pixel pair (the caller's idxs or the
// counter RNG, RV:553) and its intersection (KU:11-49), stored in the
// reference layout and keypoint-major; images without a vote are left alone.
__global__ __launch_bounds__(256) void k_hyp_gen(VoteArgs a) {
    __shared__ uint32_t lcls[512];
    const int64_t per = (int64_t)a.nh * a.vn;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = gid < per * a.b;
    const int b = in ? (int)(gid / per) : 0;
    const int r = in ? (int)(gid - b * per) : 0;
    const int h = r / a.vn, v = r - h * a.vn;
    const bool act = in && tn_at(a, b) > 0;
    uint32_t cls = 0;
    if (act) {
        const float2 hv = item_hyp<true, true>(a, b, v, h, true, tn_at(a, b), true);
        a.hypv_out[((int64_t)b * a.vn + v) * a.nh + h] = hv;
        cls = hyp_class(hv.x, hv.y);
    }
    // the classes' ballots (every thread: block barriers)
    hypcls_block_put(a.hypcls, lcls, b, a.vn, a.nh, r, act, cls);
}

// ==========================================================================
// K5m: the fused vote/count on the matrix cores (block-shared layout, hn a
// multiple of 512).  The rotated-frame test's two forms are linear in the
// hypothesis:
//     X = tau (u.h' - u.c') = a_X . h' - b_X,   a_X = tau u
//     Y =      u x h' - u x c' = a_Y . h' - b_Y,   a_Y = (-u_y, u_x)
// and z = X - |Y| (= x' tau - |y'| of the VALU kernel above).  One
// v_mfma_f32_32x32x8_f16 evaluates both forms for 16 pixels x 32 hypotheses
// (rows = (pixel, form), columns = hypotheses) from hi/lo-split fp16
// operands, K = 8:
//     row (pixel form): [ax_hi, ax_hi, ax_lo, ay_hi | ay_hi, ay_lo, -b_hi, -b_lo]
//     col (hypothesis): [hx_hi, hx_lo, hx_hi, hy_hi | hy_lo, hy_hi,  s,     s   ]
// (products of fp16 are exact in the f32 accumulation; the lo x lo terms are
// dropped; s = 2^-k keeps |h' s| < 2^14 in fp16 range).  The VALU is left with
// z = X - |Y| (one fast-rate v_sub), the sign count (v_perm + v_sad_u8) and
// the band check (v_minimum3 of |z|): ~18 instructions per 8 pairs per lane
// instead of ~54 (tools/valu_rates.hip: add/fma/or issue at ~2.7 cycles per
// wave64 instruction, min/perm/sad at ~4.3).
//
// Exactness: the MFMA path's error is bounded by gzm * |a| * B with
// B >= |h'| + |c'| (fp16 splits, the f32 sum of the
// matrix core's 8 exact products -- bounded by 16 u sum|terms| for any
// order of roundings (mfma_gz), measured within 5.2 u on 2M random sums
// (tools/mfma_probe.hip) and tested on crafted cancellation sums --, the
// rounded h', c', b and tau u); a pair is decided by the fast sign only if
// |z| > (gzm + gzr) B s (cheap per hypothesis and sub-chunk); the few that
// are not are re-checked after the sub-chunk against gzm B + gzr D with the
// pair's own distance D, and decided by the reference's sequence when
// inside it -- every decision equals KU:116-125's.
// ==========================================================================
constexpr int kMB = 16;                        // pixels per MFMA batch (32 rows: 16 pixels x (X, Y))
// pixels per sub-chunk and band pairs queued per wave: pv_tunables.h
constexpr int kMChunk = PVM_CHUNK;
constexpr int kMSlots = (kMChunk + 255) / 256; // pixels per thread in the block's staging (2)
constexpr int kMBatch = kMChunk / kMB;         // batches per sub-chunk (24)
static_assert(kMChunk % kMB == 0 && kMBatch <= 32 && kMChunk <= 512, "hit masks: 2 x 64 bits; queue: 9-bit pixel");
constexpr int kMSet = 4;                       // 32-hypothesis column sets per wave (128 hypotheses)
// (kMHypMax, |hx|, |hy| from which a hypothesis is exact-only here: pv_hypclass.h, part of hyp_class)
constexpr float kMRMax = 30000.f;              // sub-chunk radius above -> exact sub-chunk (fp16 range of b)
constexpr int kMQueue = PVM_QUEUE;             // band pairs queued per wave before a reference pass
// flagged MFMAs re-checked at a time (2 measured the same as 1).  The re-check
// loop stays written over kMBandK entries, the form the measured kernel was
// compiled from: the scalar form is equivalent but schedules differently
constexpr int kMBandK = 1;

template <bool PREPPED>
struct MSlab {
    uint4 rows[kMBatch][2 * kMB];              // [batch][row = 2 pixel + form (X, Y)]: k 0..7 as 8 halves (12 KiB)
    ExactSlab<PREPPED, kMChunk> x;
};

__device__ __forceinline__ uint32_t pack_h2(_Float16 lo, _Float16 hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, lo) | ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
}

// a row of the A operand: features of one pixel form (ax, ay, b) as 8 halves
__device__ __forceinline__ uint4 form_row(float ax, float ay, float b) {
    const _Float16 axh = (_Float16)ax, axl = (_Float16)(ax - (float)axh);
    const _Float16 ayh = (_Float16)ay, ayl = (_Float16)(ay - (float)ayh);
    const float nb = -b;
    const _Float16 bh = (_Float16)nb, bl = (_Float16)(nb - (float)bh);
    return make_uint4(pack_h2(axh, axh), pack_h2(axl, ayh), pack_h2(ayh, ayl), pack_h2(bh, bl));
}

// k_vote_mfma's arguments: only what it reads.  It makes no hypotheses (the
// pipeline's come from compact_hyp or k_hyp_gen, pv_vote_counts' from the
// caller), so nothing of the generation (seed, idxs, the reference-layout
// copies) is here, and each instantiation has its own pixel source.  The
// layouts are the instantiation's, not arguments: the pipeline's hypotheses and
// counts are keypoint-major ([b][vn][nh]), pv_vote_counts' are [nh][vn] of one
// image.
template <bool PREPPED>
struct MVotePix {               // the pipeline: compacted records and the producers' classes
    const float4 *pex;          // [b][vn][P] exact data (cx, cy, nx, ny)
    const uint32_t *hypcls;     // [b][vn][4 hgn][2] ballots of the fast / the exact-only hypotheses (Workspace::hypcls)
};
template <>
struct MVotePix<false> {        // pv_vote_counts: the caller's arrays
    const float2 *coords;       // coords[t]
    const float2 *raw;          // raw[v * raw_v + t * raw_t]
    int32_t raw_v, raw_t;
};
template <bool PREPPED>
struct MVoteArgs : MVotePix<PREPPED> {
    const float2 *hyp;          // never null (launch_vote)
    int32_t *counts;
    const int32_t *tn_dev;      // [b] pixels per image, or nullptr (tn_host)
    int32_t P, tn_host, b, vn, nh, hgn, fast;
    float thr, tau, gzf, gzr;
    float gq, Kb;               // the band re-check's constants (BandConsts, pv_band.h)
#ifdef PVV_PROFILE
    int32_t abl;                // the two band ablations' sentinels (7777 / 7778)
#endif
#ifdef PVV_TRACE
    uint64_t *trace;            // per-wave stamps and phase cycles, or nullptr
#endif
};

// the 32 columns' bits of a set, for both lane halves (which hold the same columns)
__device__ __forceinline__ uint64_t both_halves(uint32_t w) { return (uint64_t)w | ((uint64_t)w << 32); }

template <bool PREPPED>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PVM_WPE, PVM_WPE))) void k_vote_mfma(MVoteArgs<PREPPED> a) {
    const int lane = lane_id();
    const int wid = (int)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int col = lane & 31, half = lane >> 5;
    const int unit = (int)blockIdx.x;
    const uint32_t nunits = gridDim.x;
    [[maybe_unused]] const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_setprio(3);
    __shared__ MSlab<PREPPED> slab[2];
    __shared__ QuarterBoxes qb_all[2];
    __shared__ float2 hyp_all[4 * kGroup];     // each wave's 128 exact hypotheses, [set][column]
    __shared__ uint32_t bq_all[4][kMQueue];     // each wave's band pairs awaiting the reference sequence
    __shared__ int32_t corr_all[4][kGroup];     // each wave's count corrections, [set][column]
    float2 *hlds = hyp_all + wid * kGroup;
    uint32_t *bq = bq_all[wid];
    int32_t *corr = corr_all[wid];
    const int ggn = a.hgn / 4;
    uint32_t total = 0;
    for (int b = 0; b < a.b; ++b) total += (uint32_t)(a.vn * ggn) * (uint32_t)tn_at(a, b);
    uint32_t lo, hi;
    even_share(total, nunits, (uint32_t)unit, &lo, &hi);   // (no weighted rounds here: k_vote_count's alone)
    // (the counters and stamps below: trace builds only read them)
    int buf = 0;
    [[maybe_unused]] int nfix = 0, nseg = 0, nslow = 0, nxo = 0, nqd = 0;   // (nqd: band pairs queued, trace builds)
    [[maybe_unused]] uint64_t tloop = 0, t_total = 0, t_hyp = 0;
    [[maybe_unused]] uint64_t c_stage = 0, c_hot = 0, c_fix = 0, c_seg = 0, c_mark = 0;   // debug: shader cycles per phase
    [[maybe_unused]] uint64_t c_band = 0, c_flush = 0, c_xo = 0;                            // (trace builds: parts of c_fix)
    auto cyc = [&]() -> uint64_t { return PVV_TRACE_ON(a) ? __builtin_amdgcn_s_memtime() : 0; };
    if (PVV_TRACE_ON(a)) t_total = __builtin_amdgcn_s_memrealtime();
    const float tau = a.tau;
    constexpr float kBig = 3.0e38f;
    int b = 0;
    uint32_t base = 0;
    while (lo < hi && b < a.b) {
        const int n = tn_at(a, b);
        const uint32_t span = (uint32_t)(a.vn * ggn) * (uint32_t)n;
        if (lo >= base + span) { base += span; ++b; continue; }
        const uint32_t r0 = lo - base;
        const int g = (int)(r0 / (uint32_t)n);
        const int ts = uniform((int)(r0 - (uint32_t)g * n));
        const int te = uniform((int)min((uint32_t)n, ts + (hi - lo)));
        const int v = uniform(g / ggn), gg = g - (g / ggn) * ggn;
        const int hg = uniform(gg * 4 + wid);
        // ---- segment: pixels [ts, te) of (b, v) against hypotheses hg*128 .. +127 ----
        c_mark = cyc();
        F4 L[kMSlots];
        auto load_px = [&](int s0, int np) {
#pragma unroll
            for (int k = 0; k < kMSlots; ++k) {
                const int t = k * 256 + wid * kWave + lane;
                L[k] = F4{0.f, 0.f, 0.f, 0.f};
                if (t < np) L[k] = pixel_exact<PREPPED>(a, b, v, s0 + t);
            }
        };
        load_px(ts, min(kMChunk, te - ts));
        // hypotheses: lane loads h = hg*128 + i*64 + lane (i = 0, 1) into
        // [set 2i + half][col] -- the same linear index -- of the wave's LDS row.
        // Their classes (hyp_class: fast / exact-only) as wave-uniform words,
        // bit c of wf[j] / wx[j] for column c of set j: the pipeline reads the
        // ballots that the hypotheses' producer stored with them (two scalar
        // loads: 85 blocks per keypoint used to classify the same 512 values
        // again); pv_vote_counts' hypotheses have no producer and are
        // classified here, two ballots per lane slot (half 0's lanes are set
        // 2i, half 1's set 2i + 1).  A lane's own class is then its bit of a
        // mask in scalar registers (inverse ballot), no vector instruction.
        uint32_t wf[kMSet], wx[kMSet];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int h = hg * kGroup + i * kWave + lane;
            const bool hl = h < a.nh;
            float2 hv = make_float2(0.f, 0.f);
            if (hl) hv = PREPPED ? a.hyp[((int64_t)b * a.vn + v) * a.nh + h] : a.hyp[(int64_t)h * a.vn + v];
            hlds[i * kWave + lane] = hv;
            if constexpr (!PREPPED) {
                const uint32_t c = hl ? hyp_class(hv.x, hv.y) : 0u;
                const uint64_t bf_ = __builtin_amdgcn_ballot_w64((c & kHypFast) != 0);
                const uint64_t bx_ = __builtin_amdgcn_ballot_w64((c & kHypExact) != 0);
                wf[2 * i] = (uint32_t)bf_; wf[2 * i + 1] = (uint32_t)(bf_ >> 32);
                wx[2 * i] = (uint32_t)bx_; wx[2 * i + 1] = (uint32_t)(bx_ >> 32);
            }
        }
        if constexpr (PREPPED) {
            typedef __attribute__((address_space(4))) const uint32_t cu32;   // constant address space: scalar loads
            // (a 32-bit word index in scalar registers: launch_vote keeps the launch's words below 2^31)
            const int ci = uniform(((b * a.vn + v) * (4 * a.hgn) + 4 * hg) * 2);
            const cu32 *cw = (const cu32 *)(a.hypcls + ci);
#pragma unroll
            for (int j = 0; j < kMSet; ++j) { wf[j] = cw[2 * j]; wx[j] = cw[2 * j + 1]; }
        }
        __builtin_amdgcn_wave_barrier();
        // (the exact hypotheses stay in LDS, hlds[set * 32 + col]: read where
        // needed rather than held in registers across the hot loop)
        const bool any_xo = (wx[0] | wx[1] | wx[2] | wx[3]) != 0;
        // is this lane's column of set j a fast hypothesis?  (j a constant)
        auto fast_col = [&](int j) -> bool { return __builtin_amdgcn_inverse_ballot_w64(both_halves(wf[j])); };
        int cnt[kMSet] = {0, 0, 0, 0};
        corr[lane] = 0;
        corr[64 + lane] = 0;
        if (PVV_TRACE_ON(a) && t_hyp == 0) t_hyp = __builtin_amdgcn_s_memrealtime();
        for (int s0 = ts; s0 < te; s0 += kMChunk) {
            {
                const uint64_t t = cyc();
                if (s0 == ts) c_seg += t - c_mark; else c_fix += t - c_mark;
                c_mark = t;
            }
            const int np = uniform(min(kMChunk, te - s0));
            MSlab<PREPPED> &S = slab[buf];
            QuarterBoxes &QB = qb_all[buf];
            buf ^= 1;
            // ---- stage: pixels t and 256 + t of thread t; the origin is the
            // centre of the sub-chunk's bounding box (block reduce), so |c'| <= R
            // is small ----
            const int t = wid * kWave + lane;
            bool exo_p = false;
            float xl = kBig, xh = -kBig;
            float4 q[kMSlots];
            float yq[kMSlots];
#pragma unroll
            for (int k = 0; k < kMSlots; ++k) {
                const int tt = k * 256 + t;
                q[k] = make_float4(__builtin_nanf(""), 0.f, 0.f, 0.f);
                yq[k] = 0.f;
                if (tt < np) {
                    const F4 e = L[k];
                    bool ex = false;
                    if (PREPPED) q[k] = prep_compacted(e, &ex);
                    else { q[k] = prep_pixel(e.x, e.y, e.z, e.w); ex = pixel_exotic(e.z, e.w); }
                    exo_p |= ex;
                    S.x.put(tt, e);
                    xl = fminf(xl, e.x); xh = fmaxf(xh, e.x); yq[k] = q[k].y;
                }
            }
            if (wid * kWave < np) {
                const float mn = wave_min(xl), mx = wave_max(xh);
                float yn, yx;
                if (PREPPED) {
                    // rows never decrease along the compacted order: the wave's
                    // first pixel (64 wid) and its last (slot 1 when it has one)
                    yn = bcast(yq[0], 0);
                    const bool s1 = kMSlots > 1 && 256 + wid * kWave < np;
                    yx = s1 ? bcast(yq[kMSlots - 1], min(kWave - 1, np - 1 - 256 - wid * kWave))
                            : bcast(yq[0], min(kWave - 1, np - 1 - wid * kWave));
                } else {
                    float mnq = kBig, mxq = -kBig;
#pragma unroll
                    for (int k = 0; k < kMSlots; ++k)
                        if (k * 256 + t < np) { mnq = fminf(mnq, yq[k]); mxq = fmaxf(mxq, yq[k]); }
                    yn = wave_min(mnq);
                    yx = wave_max(mxq);
                }
                const uint32_t ex = __builtin_amdgcn_ballot_w64(exo_p) != 0;
                if (lane == 0) { QB.box[wid] = make_float4(mn, mx, yn, yx); QB.exo[wid] = ex; }
            } else if (lane == 0) {
                QB.box[wid] = make_float4(kBig, -kBig, kBig, -kBig);
                QB.exo[wid] = 0;
            }
            // the form rows of the sub-chunk's pixels against origin (ox, oy)
            auto put_rows = [&](float ox, float oy, bool slow) {
#pragma unroll
                for (int k = 0; k < kMSlots; ++k) {
                    const int tt = k * 256 + t;
                    if (tt >= kMChunk) break;
                    uint4 rx = make_uint4(0u, 0u, pack_h2((_Float16)0.f, (_Float16)0.f),
                                          pack_h2((_Float16)(-60000.f), (_Float16)0.f));   // never votes: X = -6e4 s
                    uint4 ry = make_uint4(0u, 0u, 0u, 0u);
                    if (q[k].x == q[k].x && !slow) {
                        const float cx = q[k].x - ox, cy = q[k].y - oy;      // exact for pixel centres
                        const float axX = tau * q[k].z, ayX = tau * q[k].w;
                        rx = form_row(axX, ayX, fmaf(axX, cx, ayX * cy));
                        ry = form_row(-q[k].w, q[k].z, fmaf(-q[k].w, cx, q[k].z * cy));
                    }
                    S.rows[tt >> 4][2 * (tt & 15)] = rx;
                    S.rows[tt >> 4][2 * (tt & 15) + 1] = ry;
                }
            };
            // next sub-chunk's loads, in flight across the barriers and the hot loop
            if (s0 + kMChunk < te) load_px(s0 + kMChunk, min(kMChunk, te - s0 - kMChunk));
            __syncthreads();
            float cxl = kBig, cxh = -kBig, cyl = kBig, cyh = -kBig;
            uint32_t exq = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 Q = QB.box[k];
                cxl = fminf(cxl, Q.x); cxh = fmaxf(cxh, Q.y);
                cyl = fminf(cyl, Q.z); cyh = fmaxf(cyh, Q.w);
                exq |= QB.exo[k];
            }
            float ox = floorf(0.5f * cxl + 0.5f * cxh), oy = floorf(0.5f * cyl + 0.5f * cyh);
            if (!(fabsf(ox) <= 1.6e7f && fabsf(oy) <= 1.6e7f)) { ox = 0.f; oy = 0.f; }
            const float axr = fmaxf(cxh - ox, ox - cxl), ayr = fmaxf(cyh - oy, oy - cyl);
            const float R = __builtin_amdgcn_sqrtf(fmaf(axr, axr, ayr * ayr)) * 1.00001f;
            // (the fp16 b operands reach max(tau, 1) R: tau u.c' for X, u x c' for Y)
            bool slow = !a.fast || exq != 0 || !(R * fmaxf(tau, 1.f) <= kMRMax);
            slow = __builtin_amdgcn_readfirstlane(slow);
            nslow += slow ? 1 : 0;
            put_rows(ox, oy, slow);
            __syncthreads();
            if (!slow) {
                // ---- the hypotheses' B fragments and bands for this origin ----
                // hypothesis j's scale s = 2^-k (|h' s| < 2^14) and bound B >=
                // |h'| + |c'| + 1 (the +1 covers the fp16 subnormal terms) for
                // this origin; made again for the band pairs (not held across
                // the hot loop)
                auto hscale = [&](int j, bool fj, float &hx, float &hy, float &s, float &Bv) {
                    const float2 hv = hlds[j * 32 + col];
                    hx = hv.x - ox;
                    hy = hv.y - oy;
                    const float mag = fmaxf(fabsf(hx), fabsf(hy));
                    const int e = __builtin_amdgcn_frexp_expf(mag);       // mag < 2^e
                    const int k = fj ? max(0, e - 14) : 0;
                    s = __builtin_ldexpf(1.f, -k);
                    Bv = (__builtin_amdgcn_sqrtf(fmaf(hx, hx, hy * hy)) * 1.00001f + R) * 1.00001f + 1.f;
                };
                // The two lane halves hold the same columns: half 0 makes sets 0
                // and 1, half 1 sets 2 and 3 (the same operations on the same
                // values as one lane making all four), and v_permlane32_swap
                // hands every lane its words of the other half's sets.  A set's
                // fragment is {xh, xl | xh, yh} in half 0 and {yl, yh | s, s} in
                // half 1: swap(a, b) returns (a's low half, b's low half) and
                // (a's high half, b's high half), i.e. set i and set 2 + i with
                // each consumer half's own word.
                static_assert(kMSet == 4, "two sets per lane half");
                h4f bf[kMSet];
                float gb[kMSet];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int j = 2 * half + i;                           // the set this lane makes
                    const bool fj = __builtin_amdgcn_inverse_ballot_w64((uint64_t)wf[i] | ((uint64_t)wf[2 + i] << 32));
                    float hx, hy, s, Bv;
                    hscale(j, fj, hx, hy, s, Bv);
                    const float hxs = hx * s, hys = hy * s;               // exact
                    const _Float16 xh_ = (_Float16)hxs, xl_ = (_Float16)(hxs - (float)xh_);
                    const _Float16 yh_ = (_Float16)hys, yl_ = (_Float16)(hys - (float)yh_);
                    const _Float16 sh = (_Float16)s;
                    const uint32_t w0 = fj ? pack_h2(xh_, xl_) : 0u, w1 = fj ? pack_h2(xh_, yh_) : 0u;
                    const uint32_t w2 = fj ? pack_h2(yl_, yh_) : 0u, w3 = fj ? pack_h2(sh, sh) : 0u;
                    const float g = fj ? (a.gzf + a.gzr) * Bv * s * 1.00001f : -1.f;
                    const auto e0 = __builtin_amdgcn_permlane32_swap(w0, w2, false, false);
                    const auto e1 = __builtin_amdgcn_permlane32_swap(w1, w3, false, false);
                    const auto eg = __builtin_amdgcn_permlane32_swap(__float_as_uint(g), __float_as_uint(g), false, false);
                    bf[i] = __builtin_bit_cast(h4f, make_uint2(e0[0], e1[0]));
                    bf[i + 2] = __builtin_bit_cast(h4f, make_uint2(e0[1], e1[1]));
                    gb[i] = __uint_as_float(eg[0]);
                    gb[i + 2] = __uint_as_float(eg[1]);
                }
                uint32_t neg[kMSet] = {0u, 0u, 0u, 0u};
                uint64_t hm0 = 0, hm1 = 0;              // band hits: bit 4 p + set, batches 0-15 / 16-31
                const int nb = (np + kMB - 1) / kMB;
                const uint2 *arow = (const uint2 *)&S.rows[0][0];
                // the lane's A fragment of batch p: row (col) of the batch's 32
                // rows (pixel col>>1, form col&1), k half `half`
                auto afrag = [&](int p) -> h4f {
                    const uint2 w = arow[(p * kMB * 2 + col) * 2 + half];
                    return __builtin_bit_cast(h4f, w);
                };
                auto zvals = [&](const f32x16 &c, float z[8]) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) z[q] = c[2 * q] - fabsf(c[2 * q + 1]);
                };
                // z of the lane's 8 pairs -> sign count into neg, returns min |z|
                auto proc = [&](const f32x16 &c, uint32_t &ng) -> float {
                    float z[8];
                    zvals(c, z);
#pragma unroll
                    for (int q = 0; q < 8; q += 4) {
                        const uint32_t p01 = __builtin_amdgcn_perm(__float_as_uint(z[q + 1]), __float_as_uint(z[q]), 0x0c0c0b09u);
                        const uint32_t p23 = __builtin_amdgcn_perm(__float_as_uint(z[q + 3]), __float_as_uint(z[q + 2]), 0x0b090c0cu);
                        ng = __builtin_amdgcn_sad_u8(p01, p23, ng);
                    }
                    float mb = __builtin_elementwise_minimum(__builtin_elementwise_minimum(fabsf(z[0]), fabsf(z[1])), fabsf(z[2]));
                    mb = __builtin_elementwise_minimum(__builtin_elementwise_minimum(mb, fabsf(z[3])), fabsf(z[4]));
                    mb = __builtin_elementwise_minimum(__builtin_elementwise_minimum(mb, fabsf(z[5])), fabsf(z[6]));
                    return __builtin_elementwise_minimum(mb, fabsf(z[7]));
                };
                // software pipelined: the next MFMA is in flight while the
                // previous one's results are processed, the next batch's A
                // fragment is read one batch ahead, and the band ballots of a
                // batch are taken together at its end
                const f32x16 zero = {};
                if (PVV_TRACE_ON(a) && tloop == 0) tloop = __builtin_amdgcn_s_memrealtime();
                { const uint64_t t = cyc(); c_stage += t - c_mark; c_mark = t; }
                h4f A = afrag(0);
                f32x16 c0 = __builtin_amdgcn_mfma_f32_32x32x8f16(A, bf[0], zero, 0, 0, 0);
#pragma unroll 1
                for (int p = 0; p < nb; ++p) {
                    const h4f An = afrag(min(p + 1, kMBatch - 1));
                    const f32x16 c1 = __builtin_amdgcn_mfma_f32_32x32x8f16(A, bf[1], zero, 0, 0, 0);
                    const float m0 = proc(c0, neg[0]);
                    const f32x16 c2 = __builtin_amdgcn_mfma_f32_32x32x8f16(A, bf[2], zero, 0, 0, 0);
                    const float m1 = proc(c1, neg[1]);
                    const f32x16 c3 = __builtin_amdgcn_mfma_f32_32x32x8f16(A, bf[3], zero, 0, 0, 0);
                    const float m2 = proc(c2, neg[2]);
                    c0 = __builtin_amdgcn_mfma_f32_32x32x8f16(An, bf[0], zero, 0, 0, 0);   // (unused after the last batch)
                    const float m3 = proc(c3, neg[3]);
                    const uint32_t hb = (__builtin_amdgcn_ballot_w64(m0 <= gb[0]) != 0 ? 1u : 0u) |
                                        (__builtin_amdgcn_ballot_w64(m1 <= gb[1]) != 0 ? 2u : 0u) |
                                        (__builtin_amdgcn_ballot_w64(m2 <= gb[2]) != 0 ? 4u : 0u) |
                                        (__builtin_amdgcn_ballot_w64(m3 <= gb[3]) != 0 ? 8u : 0u);
                    const uint64_t hbs = (uint64_t)hb << ((p & 15) * kMSet);
                    if (p < 16) hm0 |= hbs; else hm1 |= hbs;
                    A = An;
                }
                // positives = slots - negatives (padding and never-voting rows are negative)
#pragma unroll
                for (int j = 0; j < kMSet; ++j) cnt[j] += fast_col(j) ? 8 * nb - (int)(neg[j] / 255u) : 0;
                { const uint64_t t = cyc(); c_hot += t - c_mark; c_mark = t; }
                // ---- band pairs: the same MFMA again (bit-identical); each pair
                // against its own distance, bounded from the MFMA's own forms:
                // D = |h - c| <= |x'| + |y'| = |X| / tau + |Y| (scaled by s;
                // the forms' own errors, < gzm B s, add < 1e-3 of G), and the
                // reference's sequence inside the band ----
#ifdef PVV_PROFILE   // ablation bit 64: band pairs keep the sign count's guess (counts wrong)
                if (a.abl == 7777) hm0 = hm1 = 0;
#endif
                // the queued pairs by the reference's sequence, one pair per lane;
                // a decision the sign count got wrong corrects (set, column)
                int nq = 0;
                auto flush = [&]() {
                    for (int k0 = 0; k0 < nq; k0 += kWave) {
                        if (k0 + lane < nq) {
                            const uint32_t en = bq[k0 + lane];
                            const int pix = (int)(en & 0x1ffu), jj = (int)((en >> 9) & 3u), cl = (int)((en >> 11) & 31u);
                            const int f = (int)(en >> 16) & 1;
                            const F4 e = S.x.get(pix);
                            const float2 hj = hlds[jj * 32 + cl];
                            const int r = exact_vote(e.z, e.w, e.x, e.y, hj.x, hj.y, a.thr) ? 1 : 0;
                            if (r != f) atomicAdd(&corr[jj * 32 + cl], r - f);
                        }
                    }
                    nq = 0;
                };
                // Each set's per-pair constant G = gzf B s (1.001), once: from
                // the hot-loop bound gb = (gzf + gzr) B s (1.00001) with the
                // same B and s, gb gzf / (gzf + gzr) 1.0011 >= gzf B s 1.001 --
                // not an hscale (LDS read, sqrt) per flagged MFMA.
                //
                // Round 5 tested each pair against g = G + kx |X| + ky |Y|
                // (~7 VALU a pair, ~90 per flagged MFMA: the band phase was
                // 12 % of the batch-1 stream, its VALU issued beside three
                // other waves' hot loops).  Now one FMA a pair decides whether
                // any pair of the lane can be inside: |Y| <= |X| + |z| for z =
                // X - |Y| (X >= 0: |Y| = X - z; X < 0: |Y| <= |z|), so |z| <= g
                // implies |z| (1 - ky) <= G + (kx + ky) |X|, i.e. t = |z| - K |X|
                // <= G' with K = (kx + ky) / (1 - ky) and G' = G / (1 - ky)
                // (both with a 2e-4 margin that also covers t's rounding;
                // tests/test_band_filter.py checks the inclusion in float32).  The pairs with t <= G' are queued for the
                // reference's sequence: a superset of round 5's queue, so every
                // decision still equals KU's.
                // K, and G' / gb, are functions of tau, gzf and gzr alone: made once on the
                // host (a.gq, a.Kb: band_consts in pv_band.h, the same float32 expressions)
                float Gs[kMSet];
#pragma unroll
                for (int j = 0; j < kMSet; ++j) Gs[j] = gb[j] * a.gq;
                const float Kb = a.Kb;
                // The candidates of flagged MFMA (batch p, set j) are the pairs with fj && pix < np
                // && ts[q] <= G.  Only ts[q] <= G is a per-lane test; the other two are wave masks
                // combined with its ballot in scalar registers:
                // - fj, whether column col of set j is a fast hypothesis: one ballot per flagged MFMA;
                // - pix < np, with pix = 16 p + off(q) + 2 half and off(q) = (q & 1) + 4 (q >> 1)
                //   (the MFMA's row layout), fails only past the sub-chunk's last pixel, i.e. in
                //   its last batch: with rem = np - 16 p pixels left from this batch on (>= 1, and
                //   above 15 in every batch but the last, where both tests hold for every q),
                //   slot q's pixel is inside for lane half 0 if off(q) < rem and for half 1 if
                //   off(q) + 2 < rem.
                // A queue entry is pix | j << 9 | col << 11 | the sign count's guess << 16: the
                // lane's part (col, half) plus the wave-uniform part (p, j, the guess as 1) once per
                // flagged MFMA, off(q) added per entry, and a negative z takes the guess back.
                auto band_test = [&](const f32x16 &c, int p, int j) {
                    const uint64_t fmj = both_halves(j == 0 ? wf[0] : j == 1 ? wf[1] : j == 2 ? wf[2] : wf[3]);
                    // (selects on the wave-uniform j: a dynamic index would put Gs / bf in scratch)
                    const float G = j == 0 ? Gs[0] : j == 1 ? Gs[1] : j == 2 ? Gs[2] : Gs[3];
                    float zs[8], ts[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const float X = c[2 * q], Y = c[2 * q + 1];
                        zs[q] = X - fabsf(Y);
                        ts[q] = fmaf(-Kb, fabsf(X), fabsf(zs[q]));
                    }
                    float mt = __builtin_elementwise_minimum(__builtin_elementwise_minimum(ts[0], ts[1]), ts[2]);
                    mt = __builtin_elementwise_minimum(__builtin_elementwise_minimum(mt, ts[3]), ts[4]);
                    mt = __builtin_elementwise_minimum(__builtin_elementwise_minimum(mt, ts[5]), ts[6]);
                    mt = __builtin_elementwise_minimum(mt, ts[7]);
#ifdef PVV_PROFILE   // ablation bit 128: the candidates found but never queued (counts wrong)
                    if (a.abl == 7778) mt = 3.0e38f;
#endif
                    if ((__builtin_amdgcn_ballot_w64(mt <= G) & fmj) != 0) {
                        const int rem = np - p * kMB;
                        uint32_t eb = (((uint32_t)col << 11) | (2u * (uint32_t)half)) +
                                      ((uint32_t)(p * kMB) | ((uint32_t)j << 9) | (1u << 16));
                        // (opaque to the optimiser, which otherwise keeps the lane's part plus off(q)
                        // in eight registers from the kernel's start)
                        asm volatile("" : "+v"(eb));
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const int off = (q & 1) + 4 * (q >> 1);
                            const uint64_t in = (off < rem ? 0x00000000ffffffffull : 0ull) |
                                                (off + 2 < rem ? 0xffffffff00000000ull : 0ull);
                            const uint64_t m = __builtin_amdgcn_ballot_w64(ts[q] <= G) & fmj & in;
                            if (m) {
                                if (nq > kMQueue - kWave) flush();
                                const uint32_t at = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, (uint32_t)nq));
                                const uint32_t neg = (uint32_t)((int32_t)__float_as_uint(zs[q]) >> 31);   // ~0: z's sign bit is set
                                if (__builtin_amdgcn_inverse_ballot_w64(m)) bq[at] = eb + (uint32_t)off + (neg << 16);
                                nq += __popcll(m);
                                nqd += __popcll(m);
                            }
                        }
                    }
                };
                static_assert(kMSet == 4, "band selects");
                auto bsel = [&](int j) -> h4f { return j == 0 ? bf[0] : j == 1 ? bf[1] : j == 2 ? bf[2] : bf[3]; };
                while (hm0 | hm1) {
                    int pk[kMBandK], jk[kMBandK], nk = 0;
#pragma unroll
                    for (int k = 0; k < kMBandK; ++k) {
                        pk[k] = 0; jk[k] = 0;
                        if (hm0 | hm1) {
                            int bit;
                            if (hm0) { bit = __builtin_ctzll(hm0); hm0 &= hm0 - 1; }
                            else { bit = 64 + __builtin_ctzll(hm1); hm1 &= hm1 - 1; }
                            pk[k] = bit / kMSet; jk[k] = bit % kMSet;
                            nk = k + 1;
                        }
                    }
                    nfix += nk;
                    h4f ak[kMBandK];
#pragma unroll
                    for (int k = 0; k < kMBandK; ++k) ak[k] = afrag(pk[k]);
                    f32x16 ck[kMBandK];
#pragma unroll
                    for (int k = 0; k < kMBandK; ++k)
                        ck[k] = __builtin_amdgcn_mfma_f32_32x32x8f16(ak[k], bsel(jk[k]), zero, 0, 0, 0);
#pragma unroll
                    for (int k = 0; k < kMBandK; ++k)
                        if (k < nk) band_test(ck[k], pk[k], jk[k]);
                }
                { const uint64_t t = cyc(); c_band += t - c_mark; c_fix += t - c_mark; c_mark = t; }
                flush();
                __builtin_amdgcn_wave_barrier();
                { const uint64_t t = cyc(); c_flush += t - c_mark; c_fix += t - c_mark; c_mark = t; }
                // exact-only hypotheses (rare: one wave-uniform test skips the
                // sets' ballots): lane = pixel, one hypothesis at a time
#pragma unroll
                for (int j = 0; any_xo && j < kMSet; ++j) {
                    uint64_t mm = wx[j];   // (half 0's lanes: one lane per column)
                    nxo += __popcll(mm);
                    while (mm) {
                        const int l = __builtin_ctzll(mm);
                        mm &= mm - 1;
                        const float2 hx2 = hlds[j * 32 + l];
                        int c = 0;
#pragma unroll
                        for (int k = 0; k < (kMChunk + kWave - 1) / kWave; ++k) {
                            const int jj = k * kWave + lane;
                            bool e = false;
                            if (jj < np) {
                                const F4 x = S.x.get(jj);
                                e = exact_vote(x.z, x.w, x.x, x.y, hx2.x, hx2.y, a.thr);
                            }
                            c += __popcll(__builtin_amdgcn_ballot_w64(e));
                        }
                        if (lane == l) cnt[j] += c;
                    }
                }
                { const uint64_t t = cyc(); c_xo += t - c_mark; c_fix += t - c_mark; c_mark = t; }
            } else {
                // every pair through the reference sequence (lane = hypothesis column;
                // the two lane halves take alternate pixels)
#pragma unroll 1
                for (int jj = half; jj < np; jj += 2) {
                    const F4 e = S.x.get(jj);
#pragma unroll
                    for (int j = 0; j < kMSet; ++j)
                        if (__builtin_amdgcn_inverse_ballot_w64(both_halves(wf[j] | wx[j]))) {
                            const float2 hv = hlds[j * 32 + col];
                            cnt[j] += exact_vote(e.z, e.w, e.x, e.y, hv.x, hv.y, a.thr);
                        }
                }
            }
        }
        // the reference pass's corrections (LDS atomics of this wave), then
        // the two lane halves hold the same hypotheses
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < kMSet; ++j) cnt[j] += half == 0 ? corr[j * 32 + col] : 0;
#pragma unroll
        for (int j = 0; j < kMSet; ++j) {
            const auto sw = __builtin_amdgcn_permlane32_swap(cnt[j], cnt[j], false, false);
            const int tot = (int)(sw[0] + sw[1]);   // both halves, VALU only
            const int h = hg * kGroup + j * 32 + col;
            if (half == 0 && h < a.nh && tot)
                atomicAdd(PREPPED ? &a.counts[((int64_t)b * a.vn + v) * a.nh + h] : &a.counts[(int64_t)h * a.vn + v], tot);
        }
        lo += te - ts;
        ++nseg;
        { const uint64_t t = cyc(); c_fix += t - c_mark; c_mark = t; }
    }
#ifdef PVV_TRACE
    if (PVV_TRACE_ON(a) && lane == 0) {
        const int wave = (int)(blockIdx.x * 4 + wid);
        uint64_t *q = a.trace + 65536 + wave * 8;
        q[0] = c_seg; q[1] = c_stage; q[2] = c_hot; q[3] = c_fix;
        q[4] = c_band; q[5] = c_flush; q[6] = c_xo; q[7] = (uint64_t)nqd;
    }
    if (PVV_TRACE_ON(a) && lane == 0) {
        const int wave = (int)(blockIdx.x * 4 + wid);
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        a.trace[wave * 8] = t_start;
        a.trace[wave * 8 + 1] = __builtin_amdgcn_s_memrealtime();
        a.trace[wave * 8 + 2] = ((uint64_t)xcc << 32) | hw;
        a.trace[wave * 8 + 3] = ((uint64_t)nseg << 32) | (uint32_t)nfix;
        a.trace[wave * 8 + 4] = tloop;
        a.trace[wave * 8 + 5] = ((uint64_t)nslow << 32) | (uint32_t)nxo;
        a.trace[wave * 8 + 6] = t_total;
        a.trace[wave * 8 + 7] = t_hyp;
    }
#endif
}

// The matrix-core vote (k_vote_mfma): its own fast-path constant (DESIGN.md
// section 5a): per form F the error is <= u |a_F| (37.7 + [X] 2 sqrt 2 tau) B
// (h', c' and b roundings 5.7, fp16 splits 12, b split 4, the matrix core's
// f32 sum of 8 exact products 16: any order of its 7 additions, each off by
// less than one f32 ulp of a partial sum <= sum|terms| -- truncating,
// k-ordered, or aligned to the largest product and truncated -- stays within
// 14 u sum|terms|, +1 u for the final rounding, +1 u margin; tested with
// crafted cancellation sums, test_mfma_sum_error_bound), z = X - |Y| adds
// u (tau + 1) B:
//   gzm = 2 (41.5 tau + 38.7) 2^-24 (2x margin);  gzr is fast_constants'.
float mfma_gz(float tau) { return (float)(2.0 * (41.5 * (double)tau + 38.7) / 16777216.0 * 1.0001); }

// persistent vote grid: every block resident at once (the occupancy limit of
// the kernel: LDS slabs, registers), fewer when the work is small (>= ~128
// pixel steps per wave)
int vote_grid_steps(int64_t pixel_steps, const void *kernel, int max_per_cu = 1 << 30) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu <= 0) per_cu = 4;
    per_cu = std::min(per_cu, max_per_cu);
    int64_t cap = (int64_t)cu_count() * per_cu;
    int64_t need = (pixel_steps / 128 + 3) / 4;
    return (int)(need < 1 ? 1 : (need < cap ? need : cap));
}

#ifdef PVV_TRACE
uint64_t *g_vote_trace = nullptr;   // trace builds only (pv_debug_set_vote_trace)
#endif

// Kernel selection and grid shapes are compile-time constants of the build
// (pvnet_amd/build.py; pv_build_config() reports them): no environment
// variable changes what the library runs, and the default build has no switch
// that drops work.  The A/B measurements behind each default are in the
// comments and DESIGN.md section 7; the variants measured and removed are in
// DESIGN.md's appendix "Removed variants".

// Test hook, not for production (not in pvvote.h, set only by explicit calls
// between launches, never during a capture): which fused vote/count kernel
// the pipeline runs (pv_debug_set_vote_kernel: the tests check both in one
// process).  Atomic, relaxed: concurrent caller threads read it on every call.
std::atomic<int> g_vote_kernel{0};   // 0: k_vote_mfma (hn a multiple of 512), 1: k_vote_count
bool vote_old() { return g_vote_kernel.load(std::memory_order_relaxed) == 1; }

// k_vote_mfma's arguments from the launch's VoteArgs (va.hyp set)
template <bool PREPPED>
MVoteArgs<PREPPED> mvote_args(const VoteArgs &va) {
    MVoteArgs<PREPPED> m{};
    if constexpr (PREPPED) {
        m.pex = va.pex; m.hypcls = va.hypcls;
    } else {
        m.coords = va.coords; m.raw = va.raw; m.raw_v = va.raw_v; m.raw_t = va.raw_t;
    }
    m.hyp = va.hyp; m.counts = va.counts; m.tn_dev = va.tn_dev;
    m.P = va.P; m.tn_host = va.tn_host; m.b = va.b; m.vn = va.vn; m.nh = va.nh; m.hgn = va.hgn; m.fast = va.fast;
    m.thr = va.thr; m.tau = va.tau; m.gzr = va.gzr;
    m.gzf = va.fast ? mfma_gz(va.tau) : 0.f;
    // (!fast: tau = 0, every sub-chunk takes the slow path and reads none of them)
    const BandConsts bk = va.fast ? band_consts(m.tau, m.gzf, m.gzr) : BandConsts{};
    m.gq = bk.gq; m.Kb = bk.Kb;
#ifdef PVV_PROFILE
    m.abl = (g_abl & 64) ? 7777 : (g_abl & 128) ? 7778 : 0;
#endif
#ifdef PVV_TRACE
    m.trace = va.trace;
#endif
    return m;
}

// (int: PV_EINVAL for a launch k_vote_mfma cannot take, nothing launched; launch errors are the caller's last())
template <bool PREPPED>
int launch_vote(const VoteArgs &va, int64_t pixel_steps, hipStream_t s) {
    if (va.hgn % 4 == 0 && !vote_old()) {
        // k_vote_mfma makes no hypotheses: it needs them made (and, in the pipeline, classified) before it,
        // in the layout its instantiation reads
        if (!va.hyp || (PREPPED ? !va.hypcls || va.hyp_sb != (int64_t)va.vn * va.nh || va.hyp_sv != va.nh ||
                                      va.hyp_sh != 1 || va.cnt_bs != va.vn * va.nh || va.cnt_v != va.nh || va.cnt_h != 1
                                : va.b != 1 || va.hyp_sv != 1 || va.hyp_sh != va.vn || va.cnt_v != 1 || va.cnt_h != va.vn))
            return PV_EINVAL;
        if (PREPPED && (int64_t)va.b * va.vn * hyp_sets(va.nh) * 2 >= (1ll << 31)) return PV_EINVAL;   // the class words' 32-bit index
        // blocks per CU of the persistent grid: with 3 of the 4 wave slots
        // of every SIMD one launch leaves room for the next image's blocks,
        // whose prologue (dependent loads) then overlaps this one's
        // matrix/VALU work; the work is cut evenly over the blocks
        const int grid = vote_grid_steps(pixel_steps, (const void *)k_vote_mfma<PREPPED>, PVV_VM_BPC);
        k_vote_mfma<PREPPED><<<grid, 256, 0, s>>>(mvote_args<PREPPED>(va));
    } else if (va.hgn % 4 == 0) {
        const int grid = vote_grid_steps(pixel_steps, (const void *)k_vote_count<PREPPED, true>, 4);
        VoteArgs vr = va;
        if (grid == 4 * cu_count()) {
            // four resident rounds: weight the earlier-dispatched ones (round_share;
            // measured: the rounds' mean ends 28.1/30.6/32.9/35.3 us with equal
            // shares, within ~2 us with 1080/1024/976/920, vote kernel -6 %;
            // these a further -1.5 %)
            constexpr int w[4] = {1110, 1035, 965, 890};
            for (int k = 0; k < 4; ++k) vr.rw[k] = w[k];
        }
        k_vote_count<PREPPED, true><<<grid, 256, 0, s>>>(vr);
    } else
        k_vote_count<PREPPED, false>
            <<<vote_grid_steps(pixel_steps, (const void *)k_vote_count<PREPPED, false>), 256, 0, s>>>(va);
    return PV_OK;
}

}  // namespace

namespace pvv __attribute__((visibility("hidden"))) {

// Constants of the rotated-frame test (DESIGN.md "Exactness of the fast vote
// test"): tau = sqrt(1-thr^2)/thr; band = gzf * B + gzr * D with
// B >= |h - o| + |c - o| and D >= |h - c|:
//   gzf = 2 * (9 tau + 8) * 2^-24   the fast path's rounding (7 tau + 6, plus
//                                   2 (tau + 1) for a rounded c - o when the
//                                   coordinates are not integers)
//   gzr = 2 * 9.5 (tau + 1/tau) * 2^-24   the reference's 8-ulp cosine error
//                                   (+1.5 ulp for its rounded d) mapped
//                                   through dz/dcos = |d| (tau + 1/tau)
// both with 2x margin.
void fast_constants(float thr, VoteArgs *va) {
    va->thr = thr;
    const double t = (double)thr;
    if (t >= 0.05 && t <= 0.999999) {
        const double tau = sqrt(1.0 - t * t) / t;
        const double u = 1.0 / 16777216.0;
        va->tau = (float)tau;
        va->gzf = (float)(2.0 * (9.0 * tau + 8.0) * u * 1.0001);
        va->gzr = (float)(2.0 * 9.5 * (tau + 1.0 / tau) * u * 1.0001);
        va->fast = 1;
    } else {   // outside the derivation's range: every pair takes the exact sequence
        va->tau = 0.f;
        va->gzf = 0.f;
        va->gzr = 0.f;
        va->fast = 0;
    }
}

// does front_half pre-generate the hypotheses (k_hyp_gen, keypoint-major in w.hypv)?
bool hyp_pregen_used(int nh) { return ((nh + kGroup - 1) / kGroup) % 4 == 0 && !vote_old(); }

void launch_hyp_gen(const VoteArgs &va, hipStream_t s) {
    const int64_t nt = (int64_t)va.b * va.nh * va.vn;
    if (!(g_abl & 2)) k_hyp_gen<<<(unsigned)((nt + 255) / 256), 256, 0, s>>>(va);
#ifdef PVV_PROFILE
    else if (g_abl & 32) k_abl_empty<<<1, 64, 0, s>>>(0);
#endif
}

int launch_pipeline_vote(const VoteArgs &va, int64_t pixel_steps, hipStream_t s) {
#ifdef PVV_TRACE
    VoteArgs vt = va;
    vt.trace = g_vote_trace;
    return launch_vote<true>(vt, pixel_steps, s);
#else
    return launch_vote<true>(va, pixel_steps, s);
#endif
}

}  // namespace pvv

extern "C" {

int pv_vote_counts(const float *direct, const float *coords, const float *hypo, int32_t *counts, int32_t tn,
                   int32_t vn, int32_t hn, float inlier_thresh, pv_stream_t stream) {
    if (!direct || !coords || !hypo || !counts || tn < 0 || vn <= 0 || hn < 0) return PV_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hn == 0) return PV_OK;
    // counts[h][v] (the layout of torch.sum(inliers, 2)): zero, then accumulate
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)hn * vn, s);
    if (e != hipSuccess) return rc(e);
    VoteArgs va{};
    va.coords = (const float2 *)coords; va.P = tn;
    va.raw = (const float2 *)direct; va.raw_v = 1; va.raw_t = vn;
    va.hyp = (const float2 *)hypo; va.hyp_sb = 0; va.hyp_sv = 1; va.hyp_sh = vn;
    va.counts = counts; va.cnt_bs = 0; va.cnt_v = 1; va.cnt_h = vn;
    va.tn_dev = nullptr; va.tn_host = tn;
    va.b = 1; va.vn = vn; va.nh = hn; va.hgn = (hn + kGroup - 1) / kGroup;
    fast_constants(inlier_thresh, &va);
    if (tn == 0) return PV_OK;
    if ((int64_t)vn * va.hgn * tn >= (1ll << 31)) return PV_EINVAL;   // the kernel's 32-bit work index
    const int r = launch_vote<false>(va, (int64_t)vn * va.hgn * tn, s);
    return r ? r : last();
}

#ifdef PVV_TRACE
// trace builds only: per-wave timestamps of the next pipeline vote launches
void pv_debug_set_vote_trace(uint64_t *buf) { g_vote_trace = buf; }
#endif
// test hook (not in pvvote.h): which fused vote/count kernel the pipeline runs
// (0 matrix-core k_vote_mfma, 1 VALU k_vote_count); returns the previous
int pv_debug_set_vote_kernel(int32_t which) {
    return g_vote_kernel.exchange(which == 1 ? 1 : 0, std::memory_order_relaxed);
}

}  // extern "C"
