// pvapi.hip -- the stand-alone API kernels of libpvvote.so, which the pipeline
// never launches: the reference's drop-in entry points on its own layouts
// (k_generate_api, k_vote_bytes for voting_for_hypothesis' byte masks, the
// vanishing-point pair k_generate_vp / k_vote_vp) and two debug kernels behind
// test hooks, each with its extern "C" entry (include/pvvote.h).  From the vote
// stage (pvvote.hip) it takes only fast_constants, on a scratch VoteArgs.
#include "pv_stages.h"

namespace {

using namespace pvv;

// ==========================================================================
// drop-in kernels on the reference layouts
// ==========================================================================

// KU:11-86
__global__ __launch_bounds__(256) void k_generate_api(const float *direct, const float *coords, const int32_t *idxs,
                                                      float *hypo, int tn, int vn, int hn) {
    int hv = blockIdx.x * 256 + threadIdx.x;
    if (hv >= hn * vn) return;
    int hi = hv / vn, vi = hv - hi * vn;
    int t0 = idxs[hi * vn * 2 + vi * 2], t1 = idxs[hi * vn * 2 + vi * 2 + 1];
    float x = 0.f, y = 0.f, ox, oy;
    if (t0 >= 0 && t0 < tn && t1 >= 0 && t1 < tn &&
        exact_intersect(direct[t0 * vn * 2 + vi * 2], direct[t0 * vn * 2 + vi * 2 + 1], coords[t0 * 2],
                        coords[t0 * 2 + 1], direct[t1 * vn * 2 + vi * 2], direct[t1 * vn * 2 + vi * 2 + 1],
                        coords[t1 * 2], coords[t1 * 2 + 1], &ox, &oy)) {
        x = ox; y = oy;
    }
    hypo[hi * vn * 2 + vi * 2] = x;
    hypo[hi * vn * 2 + vi * 2 + 1] = y;
}

// KU:88-167 with byte outputs: inliers[h][v][t] (U1, store-bound: hn*vn*tn
// bytes).  Mode OR writes only the inlier bytes (reference semantics: the
// caller's buffer keeps its other bytes), DENSE writes every byte.
//
// A wave takes one item: keypoint v, a window of 512 pixels w and 64
// consecutive hypotheses; lane l owns pixels t = 512w + 8l + j, j < 8, and
// writes their 8 bytes of each row (h, v) at R = (h*vn + v)*tn + t with one
// 8-byte store, unaligned as the rows are (measured as fast as aligned
// stores on gfx950).  One item per wave, every item's operand loads at the
// start of the launch, before the store stream fills the memory system.
// There is no prepass: with hn a multiple of 256 a block's four waves take
// four hypothesis groups of one window and stage the window once (raw
// operands, fast operands and the window's frame, in LDS); the grid is
// CU-balanced (full blocks a multiple of the CU count, the rest as quarter
// blocks).  The vote test is vote_segment's rotated-frame test (5 FMAs per
// pair); the inlier bytes are the signs of -z gathered with v_perm.  Pairs
// inside the guard band go to a per-wave LDS queue decided by the
// reference's sequence at the wave's end; hypotheses / pixels outside the
// fast domain take it for their whole row.
constexpr int kBytePix = 8;
constexpr int kByteWin = kWave * kBytePix;      // bytes of a row per segment
constexpr int kByteHB = PVV_BYTE_HB;             // hypothesis records per batch (rows per wave, <= 64)
static_assert(kByteHB <= 64 && kByteHB % 16 == 0, "row masks are 64-bit; quarter blocks take 16 rows");
constexpr uint32_t kQueuePerWave = 128;          // band pairs a wave queues for its end (LDS)

#ifdef PVVOTE_TRACE_U1
__device__ uint64_t *g_btrace;      // debug build only: per-wave phase stamps of k_vote_bytes
#endif

struct ByteArgs {
    const float *direct;   // [tn][vn][2]
    const float *coords;   // [tn][2]
    const float *hypo;     // [hn][vn][2]
    uint8_t *out;          // [hn][vn][tn]
    int tn, vn, hn, nwin, nhg, fast;
    float thr, tau, gzf, gzr;
    int dbg;               // test hook (pv_debug_set_bytes_mode): 4 = one-entry band queue
    int xcd;               // XCD-contiguous item ranges (grid a multiple of 8)
    // CU-balanced grid (bal_nt > 0): bal_t full blocks, then bal_nt quarter
    // blocks; per XCD bal_tnx / bal_ttx of each (see k_vote_bytes)
    int bal_t, bal_nt, bal_tnx, bal_ttx;
};

// Operands of pixel (t, v) in the byte-output kernel, made where they are
// staged (no prepass): (ux, uy, cx, cy) with u the direction rounded per
// component; (0, 0) for a pixel that never votes (norm1 < 1e-6 or NaN,
// KU:119-121, or non-finite coordinates) and ux = NaN for one outside the
// fast domain.
__device__ __forceinline__ float4 api_pixel(const float2 c, const float2 d) {
    const float n1 = sqrtf(d.x * d.x + d.y * d.y);
    const bool ok = !below_1e6(n1) && n1 == n1 && isfinite(c.x) && isfinite(c.y);
    const float rs = __builtin_amdgcn_rsqf(fmaf(d.x, d.x, d.y * d.y));
    float4 q = make_float4(0.f, 0.f, c.x, c.y);
    if (ok)
        q = (n1 <= kN1Max) ? make_float4(d.x * rs, d.y * rs, c.x, c.y)
                           : make_float4(__builtin_nanf(""), 0.f, c.x, c.y);
    return q;
}
__device__ __forceinline__ float2 api_coords(const ByteArgs &a, int t) {
    return *(const float2 *)(a.coords + (int64_t)t * 2);
}
__device__ __forceinline__ float2 api_direct(const ByteArgs &a, int t, int v) {
    return *(const float2 *)(a.direct + ((int64_t)t * a.vn + v) * 2);
}

// Issue priority from the rows a wave still has (0..3), as in vote_segment:
// otherwise the SIMD favours its oldest wave, equal shares finish staggered
// and the last waves of each SIMD run alone at a fraction of the issue rate.
// (levels 0..2: 3 is the setup's, above every hot loop)
__device__ __forceinline__ void prio_by_remaining(uint32_t remaining, uint32_t total) {
    const uint64_t r3 = (uint64_t)remaining * 3, w1 = (uint64_t)total + 1;
    if (r3 >= 2 * w1) __builtin_amdgcn_s_setprio(2);
    else if (r3 >= w1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

// A window's fast-test frame, shared by the waves that vote it: origin o
// (an integer point), the voting pixels' bounding box relative to o and its
// radius R >= |c - o|; slow = some pixel is outside the fast domain.
struct WinInfo {
    float ox, oy, bxl, bxh, byl, byh, Rw;
    int slow;
};

// rows h0 + i, i < nh (<= kByteHB), of keypoint v, pixels of window w
template <int MODE>
__device__ __forceinline__ void vote_bytes_seg(const ByteArgs &a, F4 *recs, uint8_t *band8, int v, int w, int h0,
                                               int nh, uint32_t rem_after, uint32_t wave_total, uint16_t *wq,
                                               uint32_t &qn, uint64_t *tsetup, const float4 *stage, float2 hq,
                                               const float4 *raw, const float2 *hraw, const WinInfo *win) {
    const uint32_t qcap = a.dbg == 4 ? 1u : kQueuePerWave;   // (dbg 4: test hook, a full queue)
    const int lane = lane_id();
    const float ntau = -a.tau;
    const int tb = kByteWin * w + kBytePix * lane;              // lane's first pixel
    const int64_t rstep = (int64_t)a.vn * a.tn;                 // R(h + 1) - R(h)
    // row i's bytes of this lane: wave-uniform offset (SGPRs) + 32-bit lane offset
    int64_t obase = ((int64_t)h0 * a.vn + v) * a.tn + (int64_t)kByteWin * w;
    obase = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(obase >> 32)) << 32 |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)obase));   // (SGPRs for the asm below)
    const uint32_t loff = kBytePix * lane;

    // ---- operands ----
    // hq: lane's hypothesis (row h0 + lane), loaded by the caller with the pixels
    uint32_t vmask = 0;
    float fu[kBytePix], fv[kBytePix], fk1[kBytePix], fk2[kBytePix];
    float ox = 0.f, oy = 0.f, Rw = 0.f, bxl = 0.f, bxh = 0.f, byl = 0.f, byh = 0.f;
    bool slow;
    if (stage) {
        // block-staged window: the fast operands and the window's bounds are
        // made once per block (stage_window); pixels past tn never vote
#pragma unroll
        for (int j = 0; j < kBytePix; ++j) {
            fu[j] = fv[j] = fk2[j] = 0.f;
            fk1[j] = -1.0e30f;
            if (tb + j < a.tn) {
                const float4 q = stage[j * kWave + lane];
                fu[j] = q.x; fv[j] = q.y; fk1[j] = q.z; fk2[j] = q.w;
                vmask |= 1u << j;
            }
        }
        slow = __builtin_amdgcn_readfirstlane(!a.fast || win->slow);
        ox = win->ox; oy = win->oy; Rw = win->Rw;
        bxl = win->bxl; bxh = win->bxh; byl = win->byl; byh = win->byh;
        __syncthreads();   // the staging area is the block's band masks from here on
    } else {
        // from the caller's arrays: all 16 loads in flight, then the operands
        uint32_t okmask = 0;
        bool exo = false;
        float2 c[kBytePix], d[kBytePix];
#pragma unroll
        for (int j = 0; j < kBytePix; ++j) {
            const int t = tb + j;
            c[j] = d[j] = make_float2(0.f, 0.f);
            if (t < a.tn) {
                c[j] = api_coords(a, t);
                d[j] = api_direct(a, t, v);
                vmask |= 1u << j;
            }
        }
#pragma unroll
        for (int j = 0; j < kBytePix; ++j) {
            const float4 q = api_pixel(c[j], d[j]);
            const bool in = vmask >> j & 1;
            fu[j] = in ? q.x : 0.f; fv[j] = in ? q.y : 0.f; fk1[j] = in ? q.z : 0.f; fk2[j] = in ? q.w : 0.f;
        }
#pragma unroll
        for (int j = 0; j < kBytePix; ++j) {
            exo |= fu[j] != fu[j];                                  // outside the fast domain
            if (fu[j] != 0.f || fv[j] != 0.f) okmask |= 1u << j;    // votes at all
        }
        slow = __builtin_amdgcn_readfirstlane(!a.fast || __builtin_amdgcn_ballot_w64(exo) != 0);
        // origin: an integer point at the first voting pixel; the voting pixels'
        // bounding box relative to it (R >= |c - o|, and D >= |h - c| per row)
        const uint64_t anyok = __builtin_amdgcn_ballot_w64(okmask != 0);
        if (anyok) {
            const int l0 = __builtin_ctzll(anyok);
            const int j0 = __builtin_ctz(__builtin_amdgcn_readlane(okmask, l0));
            float fx = fk1[0], fy = fk2[0];
#pragma unroll
            for (int j = 1; j < kBytePix; ++j)
                if (j == j0) { fx = fk1[j]; fy = fk2[j]; }
            ox = floorf(bcast(fx, l0));
            oy = floorf(bcast(fy, l0));
            float xl = 3.0e38f, xh = -3.0e38f, yl = 3.0e38f, yh = -3.0e38f;
#pragma unroll
            for (int j = 0; j < kBytePix; ++j)
                if (okmask >> j & 1) {
                    xl = fminf(xl, fk1[j] - ox); xh = fmaxf(xh, fk1[j] - ox);
                    yl = fminf(yl, fk2[j] - oy); yh = fmaxf(yh, fk2[j] - oy);
                }
            bxl = wave_min(xl); bxh = wave_max(xh);
            byl = wave_min(yl); byh = wave_max(yh);
            const float ax = fmaxf(-bxl, bxh), ay = fmaxf(-byl, byh);
            Rw = __builtin_amdgcn_sqrtf(fmaf(ax, ax, ay * ay)) * 1.00001f;
        }
        // fast operands (ux, uy, -k1, -k2) relative to the origin, in place;
        // pixels that never vote get u = 0, -k1 = -1e30: -z = 1e30 tau, far
        // above the band, for every finite h'
#pragma unroll
        for (int j = 0; j < kBytePix; ++j) {
            const bool ok = okmask >> j & 1;
            const float ux = fu[j], uy = fv[j];
            const float cx = fk1[j] - ox, cy = fk2[j] - oy;
            fu[j] = ok ? ux : 0.f;
            fv[j] = ok ? uy : 0.f;
            fk1[j] = ok ? -fmaf(ux, cx, uy * cy) : -1.0e30f;
            fk2[j] = ok ? -fmaf(ux, cy, -(uy * cx)) : 0.f;
        }
    }
    // hypothesis records (lane i -> row h0 + 8i): h - o, band, exact flag
    uint64_t flagged;                                   // rows the exact pass decides whole
    {
        // (flagged rows carry an infinite band, so the hot loop defers them
        // without testing the flag)
        F4 rec{0.f, 0.f, __builtin_inff(), 1.f};
        if (lane < nh) {
            // non-finite or outside the fast domain: the exact sequence decides
            const bool xo = !(isfinite(hq.x) && isfinite(hq.y)) || hyp_exact_only(hq.x, hq.y);
            if (!xo && !slow) {
                const float hx = hq.x - ox, hy = hq.y - oy;
                const float B = (__builtin_amdgcn_sqrtf(fmaf(hx, hx, hy * hy)) + Rw) * 1.00001f + 1e-30f;
                const float dx = fmaxf(fabsf(hx - bxl), fabsf(hx - bxh));
                const float dy = fmaxf(fabsf(hy - byl), fabsf(hy - byh));
                const float D = fmaf(__builtin_amdgcn_sqrtf(fmaf(dx, dx, dy * dy)), 1.00001f, B * 1e-6f);
                rec = F4{hx, hy, fmaf(a.gzr, D, a.gzf * B) * 1.00001f, 0.f};
            }
        }
        flagged = __builtin_amdgcn_ballot_w64(lane < nh && rec.w != 0.f);
        __builtin_amdgcn_wave_barrier();
        if (lane < kByteHB) recs[lane] = rec;
        __builtin_amdgcn_wave_barrier();
    }

    typedef uint64_t u64a1 __attribute__((aligned(1)));   // rows start at any byte
    auto store = [&](uint8_t *p, uint32_t lo, uint32_t hi, auto partial) {
        if (!decltype(partial)::value || vmask == 0xffu) {
            const uint64_t x = (uint64_t)hi << 32 | lo;
            if (MODE == PV_VOTE_DENSE) {
                *(u64a1 *)p = x;
            } else {
                // KU:125 sets inlier bytes to 1 and leaves the others
                const uint64_t old = *(const u64a1 *)p;
                *(u64a1 *)p = (old & ~(x * 0xffu)) | x;
            }
        } else if (vmask) {
            // a row's last pixels (vmask is a prefix): 4 + 2 + 1 bytes at most
            typedef uint32_t u32a1 __attribute__((aligned(1)));
            typedef uint16_t u16a1 __attribute__((aligned(1)));
            const int n = __builtin_popcount(vmask);
            uint64_t x = (uint64_t)hi << 32 | lo;
            int o = 0;
            if (n & 4) {
                const uint32_t y = (uint32_t)x;
                if (MODE == PV_VOTE_DENSE) *(u32a1 *)(p + o) = y;
                else *(u32a1 *)(p + o) = (*(const u32a1 *)(p + o) & ~(y * 0xffu)) | y;
                x >>= 32;
                o += 4;
            }
            if (n & 2) {
                const uint16_t y = (uint16_t)x;
                if (MODE == PV_VOTE_DENSE) *(u16a1 *)(p + o) = y;
                else *(u16a1 *)(p + o) = (uint16_t)((*(const u16a1 *)(p + o) & ~(y * 0xffu)) | y);
                x >>= 16;
                o += 2;
            }
            if (n & 1) {
                const uint8_t y = (uint8_t)x;
                if (MODE == PV_VOTE_DENSE) p[o] = y;
                else if (y) p[o] = 1;
            }
        }
    };
    // inlier bytes from the signs of nz = -z: v_perm's selectors 9 / 11
    // replicate the sign bit of its second / first operand into a byte, 12 is 0
    constexpr uint32_t kSgn01 = 0x0c0c0b09u;   // sign(z0) -> b0, sign(z1) -> b1
    constexpr uint32_t kSgn23 = 0x0b090c0cu;   // sign(z2) -> b2, sign(z3) -> b3
    auto pack4 = [&](float z0, float z1, float z2, float z3) {
        const uint32_t p01 = __builtin_amdgcn_perm(__float_as_uint(z1), __float_as_uint(z0), kSgn01);
        const uint32_t p23 = __builtin_amdgcn_perm(__float_as_uint(z3), __float_as_uint(z2), kSgn23);
        return (p01 | p23) & 0x01010101u;   // 1 where z > 0 (band pairs fixed below); one v_bitop3
    };
    // nz = -z = x' (-tau) + |y'|, and min |nz| for the band check
    auto zrow = [&](const F4 &rec, float nz[kBytePix]) {
        float m = 3.0e38f;
#pragma unroll
        for (int j = 0; j < kBytePix; ++j) {
            const float xr = fmaf(fu[j], rec.x, fmaf(fv[j], rec.y, fk1[j]));
            const float yr = fmaf(fu[j], rec.y, fmaf(-fv[j], rec.x, fk2[j]));
            nz[j] = fmaf(xr, ntau, fabsf(yr));
            m = fminf(m, fabsf(nz[j]));
        }
        return m;
    };

    if (tsetup && *tsetup == 0) *tsetup = __builtin_amdgcn_s_memrealtime();   // (trace builds only)
    // Hot loop: the fast decision of every pair, one 8-byte store per row.
    // A row with a pair inside the band records which (an 8-bit mask per lane
    // in LDS) and its word is stored with those bytes as the fast guess
    // (dense) or left out (OR); the exact pass rewrites just those bytes.
    // Flagged rows (outside the fast domain) are decided whole by the exact
    // pass.  Waves holding a partial word (row ends) use byte stores.
    // Queue this lane's band pairs of row i (bits of bm) in the wave's LDS
    // queue, decided at the wave's end (fix_queued): a wave prefix of the
    // per-lane counts (<= 8, four ballots).  False when the queue is full
    // (entries that fit are still written: deciding a pair twice is harmless,
    // both give the reference's byte).
    auto enqueue = [&](uint32_t bm, int i) {
        const uint32_t n = __builtin_popcount(bm);
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t m = __builtin_amdgcn_ballot_w64((n >> k) & 1u);
            pre += (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)) << k;
            tot += (uint32_t)__builtin_popcountll(m) << k;
        }
        const uint32_t base = qn;
        qn = min(base + tot, qcap);
        uint32_t k = base + pre;
#pragma unroll
        for (int j = 0; j < kBytePix; ++j) {
            if (bm >> j & 1) {
                // (row in the wave's batch, pixel in the window): 6 + 9 bits
                if (k < qcap) wq[k] = (uint16_t)(i << 9 | (kBytePix * lane + j));
                ++k;
            }
        }
        return base + tot <= qcap;
    };
    uint64_t dmask = 0;                                 // rows with exact work in this kernel (nh <= 64)
    uint32_t lof = loff;                                // (loop-carried through the asm below: no copies)
    auto row = [&](const F4 &rec, int i, uint32_t &lo, uint32_t &hi) {
        float nz[kBytePix];
        const float m = zrow(rec, nz);
        const uint64_t hit = __builtin_amdgcn_ballot_w64(m <= rec.z);   // flagged rows: rec.z = inf
        lo = pack4(nz[0], nz[1], nz[2], nz[3]);
        hi = pack4(nz[4], nz[5], nz[6], nz[7]);
        bool skip = false;
        if (hit) {
            dmask |= 1ull << i;
            if ((flagged >> i) & 1) {
                skip = MODE != PV_VOTE_DENSE;
            } else {
                uint32_t bm = 0;
#pragma unroll
                for (int j = 0; j < kBytePix; ++j) bm |= (fabsf(nz[j]) <= rec.z ? 1u : 0u) << j;
                int io = i;
                asm volatile("" : "+s"(io));   // address math here, not an induction variable of the hot loop
                band8[io * kWave + lane] = (uint8_t)bm;
                if (MODE != PV_VOTE_DENSE) {
                    lo &= ~((bm & 1u) | (bm & 2u) << 7 | (bm & 4u) << 14 | (bm & 8u) << 21);
                    hi &= ~((bm >> 4 & 1u) | (bm >> 4 & 2u) << 7 | (bm >> 4 & 4u) << 14 | (bm >> 4 & 8u) << 21);
                }
            }
        }
        return skip;
    };
    using gbyte = __attribute__((address_space(1))) uint8_t;
    // (the row offset is made opaque so that the address stays a scalar
    // base + 32-bit lane offset instead of a strength-reduced 64-bit VGPR pointer)
    auto store_row = [&](int i, uint32_t lo, uint32_t hi, bool skip, auto partial) {
        uint64_t rp = (uint64_t)(a.out + (obase + rstep * i));
        rp = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(rp >> 32)) << 32 |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)rp);
        gbyte *rowp = (gbyte *)rp;
        asm volatile("" : "+s"(rowp), "+v"(lof));
        if (!skip) store((uint8_t *)(rowp + lof), lo, hi, partial);
    };
    auto rows = [&](auto partial) {
        F4 ra = recs[0];
        int i = 0;
        for (; i + 1 < nh; i += 2) {
            const F4 rb = recs[i + 1];
            if ((i & 7) == 0) prio_by_remaining(rem_after + (uint32_t)(nh - i), wave_total);
            uint32_t lo0, hi0, lo1, hi1;
            const bool s0 = row(ra, i, lo0, hi0);
            ra = recs[min(i + 2, kByteHB - 1)];
            const bool s1 = row(rb, i + 1, lo1, hi1);
            store_row(i, lo0, hi0, s0, partial);
            store_row(i + 1, lo1, hi1, s1, partial);
        }
        if (i < nh) {
            uint32_t lo, hi;
            const bool sk = row(ra, i, lo, hi);
            store_row(i, lo, hi, sk, partial);
        }
    };
    if (__builtin_amdgcn_ballot_w64(vmask != 0xffu)) rows(std::true_type{});
    else rows(std::false_type{});

    // Band rows: their pairs go to k_fix_bytes' queue (outside the hot loop:
    // the queue's masks and atomics would crowd its registers).
    {
        uint64_t m = dmask & ~flagged;
        while (m) {
            const int i = __builtin_ctzll(m);
            m &= m - 1;
            if (enqueue(band8[i * kWave + lane], i)) dmask &= ~(1ull << i);
        }
    }
    // Exact pass over what is left -- flagged rows, and band rows that found
    // the queue full: the lane's pixels' reference operands are loaded once
    // (one memory round trip), then the reference's sequence decides.
    if (dmask) {
        float2 ec[kBytePix], ed[kBytePix];
#pragma unroll
        for (int j = 0; j < kBytePix; ++j) {
            const int t = tb + j;
            ec[j] = ed[j] = make_float2(0.f, 0.f);
            if (vmask >> j & 1) {
                if (raw) {
                    const float4 r = raw[j * kWave + lane];
                    ec[j] = make_float2(r.x, r.y);
                    ed[j] = make_float2(r.z, r.w);
                } else {
                    ec[j] = *(const float2 *)(a.coords + (int64_t)t * 2);
                    ed[j] = *(const float2 *)(a.direct + ((int64_t)t * a.vn + v) * 2);
                }
            }
        }
        while (dmask) {
            const int i = __builtin_ctzll(dmask);
            dmask &= dmask - 1;
            const float2 q = hraw[i];
            uint8_t *p = a.out + (obase + rstep * i) + loff;
            if ((flagged >> i) & 1) {
                uint32_t lo = 0, hi = 0;
#pragma unroll
                for (int j = 0; j < kBytePix; ++j) {
                    const uint32_t bit =
                        ((vmask >> j & 1) && exact_vote(ed[j].x, ed[j].y, ec[j].x, ec[j].y, q.x, q.y, a.thr)) ? 1u : 0u;
                    if (j < 4) lo |= bit << (8 * j);
                    else hi |= bit << (8 * (j - 4));
                }
                store(p, lo, hi, std::true_type{});
            } else {
                const uint32_t bm = band8[i * kWave + lane];
#pragma unroll
                for (int j = 0; j < kBytePix; ++j) {
                    if (bm >> j & 1) {
                        const bool e = exact_vote(ed[j].x, ed[j].y, ec[j].x, ec[j].y, q.x, q.y, a.thr);
                        if (MODE == PV_VOTE_DENSE) p[j] = e ? 1 : 0;
                        else if (e) p[j] = 1;
                    }
                }
            }
        }
    }
}

// A wave's queued band pairs, decided by the reference's sequence at its
// end: lane = entry; the operands are the reference's own (c, d, h) -- from
// the block's raw window in LDS when it is staged (no memory round trip at
// the wave's end), else loaded, up to 64 pairs in flight at once; the byte
// goes over the wave's own earlier fast guess (dense, program order) or is
// set (OR).
template <int MODE>
__device__ __forceinline__ void fix_queued(const ByteArgs &a, const uint16_t *wq, uint32_t qn, int v, int w, int h0,
                                           const float4 *raw, const float2 *hraw) {
    for (uint32_t k = lane_id(); k < qn; k += kWave) {
        const uint32_t e = wq[k];
        const uint32_t i = e >> 9, p = e & (kByteWin - 1);
        const uint32_t t = (uint32_t)(kByteWin * w) + p;
        const float2 q = hraw[i];
        float2 c, d;
        if (raw) {
            const float4 r = raw[(p % kBytePix) * kWave + p / kBytePix];
            c = make_float2(r.x, r.y);
            d = make_float2(r.z, r.w);
        } else {
            c = *(const float2 *)(a.coords + (int64_t)t * 2);
            d = *(const float2 *)(a.direct + ((int64_t)t * a.vn + v) * 2);
        }
        const bool in = exact_vote(d.x, d.y, c.x, c.y, q.x, q.y, a.thr);
        uint8_t *o = a.out + ((int64_t)(h0 + (int)i) * a.vn + v) * a.tn + t;
        if (MODE == PV_VOTE_DENSE) *o = in ? 1 : 0;
        else if (in) *o = 1;
    }
}

// One item per wave: (keypoint v, window w, hypothesis group g of kByteHB
// rows, or of 16 rows in a quarter block of the balanced grid), g fastest;
// a wave beyond the items exits.
template <int MODE, int WPB>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_vote_bytes(ByteArgs a) {
    __shared__ F4 recs_all[WPB][kByteHB];
    __shared__ alignas(16) uint8_t band_all[WPB][kByteHB * kWave];   // per deferred row: each lane's band-pair mask
    __shared__ uint16_t queue_all[WPB][kQueuePerWave];     // per wave: queued band pairs (row, pixel)
    __shared__ float2 hraw_all[WPB][kByteHB];              // per wave: its rows' hypotheses
    __shared__ float4 raw_win[WPB == 4 ? kByteWin : 1];    // block-staged window: (c, d) as given
    __shared__ float4 win_part[WPB];                       // per wave: its pixels' bounds (staging)
    __shared__ int win_exo[WPB];
    F4 *recs = recs_all[threadIdx.x / 64];
    uint8_t *band8 = band_all[threadIdx.x / 64];
    uint16_t *wq = queue_all[threadIdx.x / 64];
    float2 *hraw = hraw_all[threadIdx.x / 64];
    // setup at the top issue priority, above every hot loop (whose waves
    // rank 0..2 by the rows they have left, prio_by_remaining): a wave still
    // in its setup would otherwise wait for them -- and then finish last
    __builtin_amdgcn_s_setprio(3);
    int blk = (int)blockIdx.x;
#ifdef PVVOTE_TRACE_U1
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    uint64_t t_setup = 0;
    uint64_t *tsetup = &t_setup;
#else
    uint64_t *tsetup = nullptr;
#endif
    // Every load of the wave is issued at the launch's start, in one round
    // trip: the item's hypotheses, and the window's pixels.  With the
    // hypothesis groups in fours (hn a multiple of 256) a block's four items
    // share (v, w): the block stages the window's pixels in LDS once (the
    // band-mask area, free until the hot loop) instead of four times.
    const bool shared = WPB == 4 && a.nhg % 4 == 0;
    int wave, v, w, h0, nh;
    if (WPB == 4 && a.bal_nt > 0) {
        // CU-balanced grid (shared staging only): the bal_t full blocks (64
        // rows per wave) are a multiple of the CU count; the remaining units
        // are split four ways into quarter blocks (16 rows per wave),
        // dispatched after the full ones -- at most one beside a CU's full
        // blocks, so every CU carries the same rows to within a quarter block
        // instead of a whole fifth block on some.  Each XCD (blocks i, i + 8,
        // ... under round-robin dispatch) takes a contiguous share of both
        // kinds, full ones first.  (Speed only: any placement is correct.)
        const int x = blk % 8, k = blk / 8;
        int u, part = -1;
        if (k < a.bal_tnx) {
            u = x * a.bal_tnx + k;
            if (u >= a.bal_t) return;                     // (whole blocks)
        } else {
            const int i = x * a.bal_ttx + (k - a.bal_tnx);
            if (i >= a.bal_nt) return;
            u = a.bal_t + i / 4;
            part = i % 4;
        }
        const int G = a.nhg / 4, q = (int)(threadIdx.x / 64);
        const int gq = u % G, rest = u / G;
        v = rest % a.vn;
        w = (rest / a.vn + a.nwin - 1) % a.nwin;
        h0 = part < 0 ? gq * 4 * kByteHB + q * kByteHB : gq * 4 * kByteHB + part * kByteHB + q * (kByteHB / 4);
        nh = part < 0 ? kByteHB : kByteHB / 4;
        wave = uniform(blk * 4 + q);
    } else {
        if (a.xcd) {
            // blocks i, i + 8, ... run on one XCD (round-robin dispatch; speed
            // only, nothing depends on it): give each XCD a contiguous range of
            // items, whose windows' pixels its L2 then fetches once
            const int per = (int)gridDim.x / 8;   // (the host pads the grid to a multiple of 8)
            blk = (blk % 8) * per + blk / 8;
        }
        wave = uniform(blk * WPB + (int)(threadIdx.x / 64));
        const uint32_t nitems = (uint32_t)a.vn * a.nwin * a.nhg;   // < 2^31 (host-checked)
        // (shared: nitems is a multiple of 4, every wave of a block has an item)
        if ((uint32_t)wave >= nitems) return;
        // items (w, v, g), g fastest: a window's items are adjacent; the last
        // (partial) window first, so that its slower byte-store rows are not the
        // launch's tail
        const uint32_t g = (uint32_t)wave % a.nhg, rest = (uint32_t)wave / a.nhg;
        v = (int)(rest % (uint32_t)a.vn);
        w = (int)((rest / (uint32_t)a.vn + (uint32_t)a.nwin - 1) % (uint32_t)a.nwin);
        h0 = (int)g * kByteHB;
        nh = min(kByteHB, a.hn - h0);
    }
    v = uniform(v); w = uniform(w); h0 = uniform(h0); nh = uniform(nh);
    float2 hq = make_float2(0.f, 0.f);
    if (lane_id() < nh) hq = *(const float2 *)(a.hypo + ((int64_t)(h0 + lane_id()) * a.vn + v) * 2);
    if (lane_id() < kByteHB) hraw[lane_id()] = hq;
    const float4 *stage = nullptr, *raw = nullptr;
    WinInfo wi{};
    if (WPB == 4 && shared) {
        // the block's window, once: raw (c, d) for the exact decisions, the
        // fast operands (ux, uy, -k1, -k2) relative to the window's origin
        // (the floor of its first pixel), and the voting pixels' bounds
        float4 *st = (float4 *)&band_all[0][0];
        constexpr int kPer = kByteWin / 256;   // pixels per thread; loads first, then the operands
        const int t0 = kByteWin * w;
        float2 c[kPer], d[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int t = t0 + k * 256 + (int)threadIdx.x;
            if (t < a.tn) { c[k] = api_coords(a, t); d[k] = api_direct(a, t, v); }
        }
        const float2 c0 = api_coords(a, t0);
        const bool obad = !(isfinite(c0.x) && isfinite(c0.y));
        const float ox = obad ? 0.f : floorf(c0.x), oy = obad ? 0.f : floorf(c0.y);
        float xl = 3.0e38f, xh = -3.0e38f, yl = 3.0e38f, yh = -3.0e38f;
        bool exo = false;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int t = t0 + k * 256 + (int)threadIdx.x;
            // lane-interleaved: lane l's pixel j (k = 8l + j) at j * 64 + l, so
            // that each of the waves' eight reads is 64 consecutive float4
            const int kk = k * 256 + (int)threadIdx.x;
            if (t < a.tn) {
                const float4 q = api_pixel(c[k], d[k]);
                const bool ok = q.x != 0.f || q.y != 0.f;   // votes at all (NaN: outside the fast domain)
                exo |= q.x != q.x;
                const float cx = q.z - ox, cy = q.w - oy;
                float4 f = make_float4(0.f, 0.f, -1.0e30f, 0.f);   // never votes: -z = 1e30 tau
                if (ok) {
                    f = make_float4(q.x, q.y, -fmaf(q.x, cx, q.y * cy), -fmaf(q.x, cy, -(q.y * cx)));
                    xl = fminf(xl, cx); xh = fmaxf(xh, cx);
                    yl = fminf(yl, cy); yh = fmaxf(yh, cy);
                }
                st[(kk % kBytePix) * kWave + kk / kBytePix] = f;
                raw_win[(kk % kBytePix) * kWave + kk / kBytePix] = make_float4(c[k].x, c[k].y, d[k].x, d[k].y);
            }
        }
        xl = wave_min(xl); xh = wave_max(xh);
        yl = wave_min(yl); yh = wave_max(yh);
        const bool wexo = __builtin_amdgcn_ballot_w64(exo) != 0;
        if (lane_id() == 0) {
            win_part[threadIdx.x / 64] = make_float4(xl, xh, yl, yh);
            win_exo[threadIdx.x / 64] = wexo;
        }
        __syncthreads();
        float4 p = win_part[0];
        int ex = win_exo[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const float4 q = win_part[k];
            p.x = fminf(p.x, q.x); p.y = fmaxf(p.y, q.y);
            p.z = fminf(p.z, q.z); p.w = fmaxf(p.w, q.w);
            ex |= win_exo[k];
        }
        wi.slow = ex | obad;
        wi.ox = ox; wi.oy = oy;
        if (p.x <= p.y) {   // some pixel votes
            wi.bxl = p.x; wi.bxh = p.y; wi.byl = p.z; wi.byh = p.w;
            const float ax = fmaxf(-p.x, p.y), ay = fmaxf(-p.z, p.w);
            wi.Rw = __builtin_amdgcn_sqrtf(fmaf(ax, ax, ay * ay)) * 1.00001f;
        }
        stage = st;
        raw = raw_win;
    }
#ifdef PVVOTE_TRACE_U1
    const uint64_t t_staged = __builtin_amdgcn_s_memrealtime();
#endif
    uint32_t qn = 0;
    vote_bytes_seg<MODE>(a, recs, band8, uniform(v), uniform(w), uniform(h0), uniform(nh), 0u, (uint32_t)nh, wq, qn,
                         tsetup, stage, hq, raw, hraw, &wi);
#ifdef PVVOTE_TRACE_U1
    const uint64_t t_first = __builtin_amdgcn_s_memrealtime();
#endif
    __builtin_amdgcn_wave_barrier();
    fix_queued<MODE>(a, wq, qn, v, w, h0, raw, hraw);
#ifdef PVVOTE_TRACE_U1
    if (g_btrace && lane_id() == 0) {
        g_btrace[wave * 8] = t_start;
        g_btrace[wave * 8 + 1] = t_first;
        g_btrace[wave * 8 + 2] = __builtin_amdgcn_s_memrealtime();
        g_btrace[wave * 8 + 3] = t_setup;
        g_btrace[wave * 8 + 4] = t_staged;
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_btrace[wave * 8 + 5] = ((uint64_t)xcc << 32) | hw;
    }
#endif
}

// test hook of the matrix-core sums the vote kernel's error bound rests on
// (pv_debug_mfma_sums): tile i = A [32][8] fp16 x B [8][32] fp16 -> D
// [32][32] f32 by the instruction k_vote_mfma issues, with a zero accumulator
// as there; lane l holds A[l & 31][4 (l >> 5) + j] and B[4 (l >> 5) + j][l & 31]
__global__ __launch_bounds__(64) void k_debug_mfma_sums(const uint16_t *A, const uint16_t *B, float *D) {
    const int l = threadIdx.x, r = l & 31, h = l >> 5;
    const uint16_t *At = A + (int64_t)blockIdx.x * 256, *Bt = B + (int64_t)blockIdx.x * 256;
    h4f a, b;
    for (int j = 0; j < 4; ++j) {
        a[j] = __builtin_bit_cast(_Float16, At[r * 8 + 4 * h + j]);
        b[j] = __builtin_bit_cast(_Float16, Bt[(4 * h + j) * 32 + r]);
    }
    const f32x16 zero = {};
    const f32x16 c = __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, zero, 0, 0, 0);
    float *Dt = D + (int64_t)blockIdx.x * 1024;
    for (int i = 0; i < 16; ++i) Dt[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = c[i];
}

// test hook of wave_min / wave_max (pv_debug_wave_minmax)
__global__ __launch_bounds__(64) void k_debug_minmax(const float *in, float *out) {
    const float x = in[blockIdx.x * 64 + threadIdx.x];
    const float mn = wave_min(x), mx = wave_max(x);
    // every lane must hold the result
    const bool agree = __builtin_amdgcn_ballot_w64(mn != bcast(mn, 0) || mx != bcast(mx, 0)) == 0;
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = agree ? mn : __builtin_nanf("");
        out[2 * blockIdx.x + 1] = agree ? mx : __builtin_nanf("");
    }
}

// KU:170-229
__global__ __launch_bounds__(256) void k_generate_vp(const float *direct, const float *coords, const int32_t *idxs,
                                                     float *hypo, int tn, int vn, int hn) {
    int hv = blockIdx.x * 256 + threadIdx.x;
    if (hv >= hn * vn) return;
    int hi = hv / vn, vi = hv - hi * vn;
    int id0 = idxs[hi * vn * 2 + vi * 2], id1 = idxs[hi * vn * 2 + vi * 2 + 1];
    float x = 0.f, y = 0.f, z = 0.f;
    if (id0 >= 0 && id0 < tn && id1 >= 0 && id1 < tn) {
        float dx0 = direct[id0 * vn * 2 + vi * 2], dy0 = direct[id0 * vn * 2 + vi * 2 + 1];
        float cx0 = coords[id0 * 2], cy0 = coords[id0 * 2 + 1];
        float dx1 = direct[id1 * vn * 2 + vi * 2], dy1 = direct[id1 * vn * 2 + vi * 2 + 1];
        float cx1 = coords[id1 * 2], cy1 = coords[id1 * 2 + 1];
        float lx0 = dy0, ly0 = -dx0, lz0 = cy0 * dx0 - cx0 * dy0;
        float lx1 = dy1, ly1 = -dx1, lz1 = cy1 * dx1 - cx1 * dy1;
        x = ly0 * lz1 - lz0 * ly1;
        y = lz0 * lx1 - lx0 * lz1;
        z = lx0 * ly1 - ly0 * lx1;
        float vx0 = dx0 * (x - z * cx0), vx1 = dx1 * (x - z * cx1);
        float vy0 = dy0 * (y - z * cy0), vy1 = dy1 * (y - z * cy1);
        if (vx0 < 0 && vx1 < 0 && vy0 < 0 && vy1 < 0) { z = -z; x = -x; y = -y; }
        if (vx0 * vx1 < 0 || vy0 * vy1 < 0) { x = 0.f; y = 0.f; z = 0.f; }
    }
    hypo[hi * vn * 3 + vi * 3] = x;
    hypo[hi * vn * 3 + vi * 3 + 1] = y;
    hypo[hi * vn * 3 + vi * 3 + 2] = z;
}

// KU:268-310
__global__ __launch_bounds__(256) void k_vote_vp(const float *direct, const float *coords, const float *hypo,
                                                 uint8_t *inliers, int tn, int vn, int hn, float thr) {
    int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t tot = (int64_t)hn * vn * tn;
    if (gid >= tot) return;
    int ti = (int)(gid % tn);
    int vi = (int)((gid / tn) % vn);
    int hi = (int)(gid / ((int64_t)tn * vn));
    float cx = coords[ti * 2], cy = coords[ti * 2 + 1];
    float hx = hypo[(hi * vn + vi) * 3], hy = hypo[(hi * vn + vi) * 3 + 1], hz = hypo[(hi * vn + vi) * 3 + 2];
    float ddx = direct[(int64_t)ti * vn * 2 + vi * 2], ddy = direct[(int64_t)ti * vn * 2 + vi * 2 + 1];
    float fx = hx - cx * hz, fy = hy - cy * hz;
    float n1 = sqrtf(ddx * ddx + ddy * ddy);
    float n2 = sqrtf(fx * fx + fy * fy);
    if (below_1e6(n1) || below_1e6(n2)) return;
    float ad = (ddx * fx + ddy * fy) / (n1 * n2);
    float vx = fx * ddx, vy = fy * ddy;
    if (vx < 0 || vy < 0) return;
    if (fabsf(ad) > thr) inliers[gid] = 1;
}

// Test hook, not for production (not in pvvote.h, set only by explicit calls
// between launches, never during a capture): the byte kernel's band-queue
// capacity (pv_debug_set_bytes_mode 4: a queue of one entry, so the in-kernel
// exact pass runs).  Atomic, relaxed: concurrent caller threads read it on
// every call.
std::atomic<int> g_bytes_dbg{0};

}  // namespace

extern "C" {

int pv_generate_hypothesis(const float *direct, const float *coords, const int32_t *idxs, float *hypo, int32_t tn,
                           int32_t vn, int32_t hn, pv_stream_t stream) {
    if (!direct || !coords || !idxs || !hypo || tn <= 0 || vn <= 0 || hn < 0) return PV_EINVAL;
    if (hn == 0) return PV_OK;
    int64_t n = (int64_t)hn * vn;
    k_generate_api<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(direct, coords, idxs, hypo, tn, vn,
                                                                                  hn);
    return last();
}


int pv_voting_for_hypothesis(const float *direct, const float *coords, const float *hypo, uint8_t *inliers,
                             int32_t tn, int32_t vn, int32_t hn, float inlier_thresh, int32_t mode,
                             pv_stream_t stream) {
    if (!direct || !coords || !hypo || !inliers || tn < 0 || vn <= 0 || hn < 0) return PV_EINVAL;
    if (mode != PV_VOTE_OR && mode != PV_VOTE_DENSE) return PV_EINVAL;
    if (tn == 0 || hn == 0) return PV_OK;
    VoteArgs fc{};
    fast_constants(inlier_thresh, &fc);
    ByteArgs ba{};
    ba.direct = direct; ba.coords = coords; ba.hypo = hypo; ba.out = inliers;
    ba.tn = tn; ba.vn = vn; ba.hn = hn;
    ba.fast = fc.fast; ba.thr = fc.thr; ba.tau = fc.tau; ba.gzf = fc.gzf; ba.gzr = fc.gzr;
    ba.nwin = (tn + kByteWin - 1) / kByteWin;
    ba.nhg = (hn + kByteHB - 1) / kByteHB;
    ba.dbg = g_bytes_dbg.load(std::memory_order_relaxed);
    const int64_t items = (int64_t)vn * ba.nwin * ba.nhg;
    if (items >= (1ll << 31)) return PV_EINVAL;   // the kernel's 32-bit item index
    // one launch, no scratch: the operands are made where the blocks stage them
    unsigned grid = (unsigned)((items + 3) / 4);
    ba.xcd = PVV_BYTES_XCD;
    if (ba.xcd) grid = (grid + 7) / 8 * 8;
    if (PVV_BYTES_BAL && ba.nhg % 4 == 0 && ba.xcd) {
        // CU-balanced grid: full blocks a multiple of the CU count, the rest
        // as quarter blocks, when that leaves at most one quarter block per CU
        // beside four full ones (one resident round; see k_vote_bytes)
        const int64_t units = items / 4, cus = cu_count();
        const int64_t T = units / cus * cus, E = units - T;
        if (T > 0 && T <= 4 * cus && E > 0 && 4 * E <= cus) {
            ba.bal_t = (int)T;
            ba.bal_nt = (int)(4 * E);
            ba.bal_tnx = (int)((T + 7) / 8);
            ba.bal_ttx = (int)((4 * E + 7) / 8);
            grid = (unsigned)(8 * (ba.bal_tnx + ba.bal_ttx));
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (mode == PV_VOTE_DENSE)
        k_vote_bytes<PV_VOTE_DENSE, 4><<<grid, 256, 0, s>>>(ba);
    else
        k_vote_bytes<PV_VOTE_OR, 4><<<grid, 256, 0, s>>>(ba);
    return last();
}

int pv_generate_hypothesis_vp(const float *direct, const float *coords, const int32_t *idxs, float *hypo,
                              int32_t tn, int32_t vn, int32_t hn, pv_stream_t stream) {
    if (!direct || !coords || !idxs || !hypo || tn <= 0 || vn <= 0 || hn < 0) return PV_EINVAL;
    if (hn == 0) return PV_OK;
    int64_t n = (int64_t)hn * vn;
    k_generate_vp<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(direct, coords, idxs, hypo, tn, vn,
                                                                                 hn);
    return last();
}

int pv_voting_for_hypothesis_vp(const float *direct, const float *coords, const float *hypo, uint8_t *inliers,
                                int32_t tn, int32_t vn, int32_t hn, float inlier_thresh, pv_stream_t stream) {
    if (!direct || !coords || !hypo || !inliers || tn < 0 || vn <= 0 || hn < 0) return PV_EINVAL;
    int64_t n = (int64_t)hn * vn * tn;
    if (n == 0) return PV_OK;
    k_vote_vp<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(direct, coords, hypo, inliers, tn, vn, hn,
                                                                            inlier_thresh);
    return last();
}

// debug only (not in pvvote.h): ntiles products A[i] (32 x 8 fp16) x B[i] (8 x 32 fp16) -> D[i]
// (32 x 32 f32) on v_mfma_f32_32x32x8_f16 with a zero accumulator (the vote kernel's sums)
int pv_debug_mfma_sums(const uint16_t *A, const uint16_t *B, float *D, int32_t ntiles, pv_stream_t stream) {
    if (!A || !B || !D || ntiles <= 0) return PV_EINVAL;
    k_debug_mfma_sums<<<(unsigned)ntiles, 64, 0, (hipStream_t)stream>>>(A, B, D);
    return last();
}

// debug only (not in pvvote.h): wave min / max of 64 floats per wave -> out[2 * wave + {0, 1}]
int pv_debug_wave_minmax(const float *in, float *out, int32_t nwaves, pv_stream_t stream) {
    if (!in || !out || nwaves <= 0) return PV_EINVAL;
    k_debug_minmax<<<(unsigned)nwaves, 64, 0, (hipStream_t)stream>>>(in, out);
    return last();
}

// test hook (not in pvvote.h): the byte kernel's band-queue mode (4: one-entry
// queue, so band rows take the in-kernel exact pass); returns the previous
int pv_debug_set_bytes_mode(int32_t dbg) {
    return g_bytes_dbg.exchange(dbg == 4 ? 4 : 0, std::memory_order_relaxed);
}
#ifdef PVVOTE_TRACE_U1
int pv_debug_set_bytes_trace(uint64_t *buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_btrace), &buf, sizeof(buf)); }
#endif

}  // extern "C"
