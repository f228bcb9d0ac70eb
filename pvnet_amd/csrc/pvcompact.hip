// pvcompact.hip -- the pipeline's first stage: foreground count (k_fg_count),
// row-major stream compaction of the foreground pixels with their
// per-keypoint directions (k_compact) and, in k_compact's first blocks, the
// hypotheses (compact_hyp).  A multi-object call (pv_image_desc.ncls >= 1)
// runs k_label_count in k_fg_count's place: one read of each pixel's label
// for the ballots and counts of every class, the rest over b * ncls virtual
// images.  Host entry: pvv::compact (pv_stages.h).  The
// look-back test hook and the compaction trace live here with the device
// globals they set: a __device__ global belongs in the translation unit of
// both its kernels and its host-side setter (a global no host code of the
// file writes is folded away as a constant).
#include "pv_stages.h"

namespace {
using namespace pvv;

// ==========================================================================
// K1: foreground count per 256-pixel chunk (one pixel per thread and chunk)
// and the chunk's four wave ballots (k_compact reads 32 B instead of the mask
// again); zeroes the pipeline's counters.  A block takes CPB consecutive
// chunks, their mask loads issued together (clamped to the image, so no
// branch sits between them).  One chunk per block for grids that fit the
// chip at once (a one-image call: tools/lat_ab.sh, 1 chunk 52.1-52.4 us
// sequential latency, 2 chunks 52.8-53.1, 4 chunks 54.3); kFgWideCPB for
// larger grids, where one-chunk blocks -- one mask round trip each, eight
// per CU at a time -- left the kernel bound by block turnover (configs[2],
// 32 frames: 70 us).
// ==========================================================================
constexpr int kFgWideCPB = 8;
constexpr int64_t kFgWideAbove = PVV_FG_WIDE_ABOVE;   // blocks of one chunk above which the wide form runs
template <int KIND, bool EVD, int CPB>
__global__ __launch_bounds__(256) void k_fg_count(MaskView m, int H, int W, int32_t *blkcnt, uint64_t *fgbits,
                                                  int32_t *grpcnt, int nblk, int32_t *zero, int64_t zero_words) {
    static_assert(kCompactChunk == 256, "one pixel per thread");
    const int b = blockIdx.y, wid = threadIdx.x / 64;
    const int64_t P = (int64_t)H * W;
    {   // zero counts + tickets (read only by later kernels of this pipeline)
        int64_t g = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        int64_t G = (int64_t)gridDim.x * gridDim.y * 256;
        for (int64_t i = g; i < zero_words; i += G) zero[i] = 0;
    }
    __shared__ int sh[CPB][4];
    bool f[CPB];
#pragma unroll
    for (int k = 0; k < CPB; ++k) {
        const int blk = blockIdx.x * CPB + k;
        const int64_t p = (int64_t)blk * kCompactChunk + threadIdx.x;
        const uint32_t pc = (uint32_t)min(p, P - 1);   // every load in range: none behind a branch
        const bool v = is_fg<KIND, EVD>(m, b, (int)(pc / (uint32_t)W), (int)(pc % (uint32_t)W));
        f[k] = blk < nblk && p < P && v;
    }
#pragma unroll
    for (int k = 0; k < CPB; ++k) {
        const int blk = blockIdx.x * CPB + k;   // block-uniform
        if (blk >= nblk) break;
        const uint64_t bal = ballot(f[k]);
        if (lane_id() == 0) {
            fgbits[((int64_t)b * nblk + blk) * 4 + wid] = bal;
            sh[k][wid] = __popcll(bal);
        }
    }
    __syncthreads();
    const int blk = blockIdx.x * CPB + (int)threadIdx.x;
    if (threadIdx.x < CPB && blk < nblk)
        blkcnt[b * nblk + blk] = sh[threadIdx.x][0] + sh[threadIdx.x][1] + sh[threadIdx.x][2] + sh[threadIdx.x][3];
    if (CPB > 1 && threadIdx.x == 0) {   // the block's sum: k_compact's image totals read these
        int g = 0;
#pragma unroll
        for (int k = 0; k < CPB; ++k)
            if (blockIdx.x * CPB + k < nblk) g += sh[k][0] + sh[k][1] + sh[k][2] + sh[k][3];
        grpcnt[b * gridDim.x + blockIdx.x] = g;
    }
}

// ==========================================================================
// K1 of a multi-object call (ncls >= 1): every pixel's label read once -- the
// label map's value, or the argmax over the ncls + 1 logit planes (first
// maximum wins, NaN is the maximum: torch.argmax) -- and the ballots, chunk
// counts and group sums of all ncls classes written as k_fg_count would have
// for the stacked batch of b * ncls binary masks `label == c + 1` (virtual
// image bv = bi * ncls + c).  Same grids as k_fg_count over (chunks, b).
// Lane c of a wave keeps class c's ballot (ncls <= 64), so a wave stores a
// chunk's ncls ballots with one instruction.
// ==========================================================================
constexpr int kLabelPlanes = 4;   // logit planes of a pixel in flight together

template <int KIND>
__device__ __forceinline__ int read_label(const MaskView &m, int ncls, int b, int r, int c) {
    if constexpr (KIND == PV_MASK_SEG_F32 || KIND == PV_MASK_SEG_F16) {
        const int64_t o = b * m.s0 + r * m.s2 + c * m.s3;
        float best = 0.f;
        int lab = 0;
        for (int k0 = 0; k0 <= ncls; k0 += kLabelPlanes) {
            float v[kLabelPlanes];
#pragma unroll
            for (int u = 0; u < kLabelPlanes; ++u) {
                const int64_t q = o + (int64_t)min(k0 + u, ncls) * m.s1;   // clamped: none behind a branch
                if constexpr (KIND == PV_MASK_SEG_F32) v[u] = ((const float *)m.p)[q];
                else v[u] = __half2float(((const __half *)m.p)[q]);
            }
#pragma unroll
            for (int u = 0; u < kLabelPlanes; ++u) {
                const int k = k0 + u;
                if (k == 0) best = v[u];
                else if (k <= ncls && !isnan(best) && (isnan(v[u]) || v[u] > best)) { best = v[u]; lab = k; }
            }
        }
        return lab;
    } else {
        const int64_t o = b * m.s0 + r * m.s1 + c * m.s2;
        int64_t v;
        if constexpr (KIND == PV_MASK_I64) v = ((const int64_t *)m.p)[o];
        else if constexpr (KIND == PV_MASK_I32) v = ((const int32_t *)m.p)[o];
        else v = ((const uint8_t *)m.p)[o];
        return v >= 1 && v <= ncls ? (int)v : 0;   // the full value: 257 is no class
    }
}

template <int KIND, int CPB>
__global__ __launch_bounds__(256) void k_label_count(MaskView m, int H, int W, int ncls, int32_t *blkcnt,
                                                     uint64_t *fgbits, int32_t *grpcnt, int nblk, int32_t *zero,
                                                     int64_t zero_words) {
    static_assert(kCompactChunk == 256, "one pixel per thread");
    const int bi = blockIdx.y, wid = threadIdx.x / 64, lane = lane_id();
    const int64_t P = (int64_t)H * W;
    {   // zero counts + tickets of all b * ncls virtual images
        int64_t g = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
        int64_t G = (int64_t)gridDim.x * gridDim.y * 256;
        for (int64_t i = g; i < zero_words; i += G) zero[i] = 0;
    }
    __shared__ int sh[CPB][4][64];   // [chunk][wave][class]
    int lab[CPB];
#pragma unroll
    for (int k = 0; k < CPB; ++k) {
        const int blk = blockIdx.x * CPB + k;
        const int64_t p = (int64_t)blk * kCompactChunk + threadIdx.x;
        const uint32_t pc = (uint32_t)min(p, P - 1);   // every load in range
        const int v = read_label<KIND>(m, ncls, bi, (int)(pc / (uint32_t)W), (int)(pc % (uint32_t)W));
        lab[k] = blk < nblk && p < P ? v : 0;
    }
#pragma unroll
    for (int k = 0; k < CPB; ++k) {
        const int blk = blockIdx.x * CPB + k;   // block-uniform
        if (blk >= nblk) break;
        uint64_t mine = 0;
        for (int c = 0; c < ncls; ++c) {        // wave-uniform
            const uint64_t bal = ballot(lab[k] == c + 1);
            if (lane == c) mine = bal;
        }
        if (lane < ncls) {
            fgbits[(((int64_t)bi * ncls + lane) * nblk + blk) * 4 + wid] = mine;
            sh[k][wid][lane] = __popcll(mine);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CPB * ncls; i += 256) {
        const int k = i / ncls, c = i - k * ncls, blk = blockIdx.x * CPB + k;
        if (blk < nblk) blkcnt[((int64_t)bi * ncls + c) * nblk + blk] = sh[k][0][c] + sh[k][1][c] + sh[k][2][c] + sh[k][3][c];
    }
    if (CPB > 1 && (int)threadIdx.x < ncls) {   // the block's sum per class: k_compact's image totals read these
        const int c = threadIdx.x;
        int g = 0;
#pragma unroll
        for (int k = 0; k < CPB; ++k)
            if (blockIdx.x * CPB + k < nblk) g += sh[k][0][c] + sh[k][1][c] + sh[k][2][c] + sh[k][3][c];
        grpcnt[((int64_t)bi * ncls + c) * gridDim.x + blockIdx.x] = g;
    }
}

// foreground total of image b from the per-block counts (every block of K1b/K2 does this)
__device__ __forceinline__ int2 image_totals(const int32_t *cnt, int nblk, int upto, int *sh) {
    int all = 0, pre = 0;
    for (int j = threadIdx.x; j < nblk; j += 256) {
        int v = cnt[j];
        all += v;
        pre += j < upto ? v : 0;
    }
    return block_sum2(all, pre, sh);
}

// ==========================================================================
// K2: row-major stream compaction (RV:548-552): coords (x=col, y=row) and the
// per-keypoint raw directions, keypoint-major so the vote waves read them
// contiguously.  Reads the [b,H,W,vn,2] view through its strides, so the
// network's NCHW vertex_pred is gathered directly (no permute copy).
// ==========================================================================
// debug-only phase stamps (s_memrealtime) of the compaction blocks; see
// pv_debug_compact_trace
#ifdef PVV_TRACE
__device__ uint64_t g_ctrace[4096 * 4];
__device__ int g_ctrace_on;
__device__ __forceinline__ void cstamp(int blk, int k) {
    if (g_ctrace_on && threadIdx.x == 0 && blk < 4096) g_ctrace[blk * 4 + k] = __builtin_amdgcn_s_memrealtime();
}
#else
__device__ __forceinline__ void cstamp(int, int) {}
#endif

constexpr int kCompactKp = 12;   // keypoints whose vertex loads a compaction thread keeps in flight at once
constexpr uint64_t kLookbackSpin = 20000;   // s_memrealtime ticks (100 MHz): 200 us
__device__ int g_lb_self;   // debug (pv_debug_lookback_self): every look-back count worked out by the waiter

// one chunk (256 pixels) of image b: the whole of a k_compact block
// (block-uniform early returns; sh holds 8 ints, wcnt 4, pos 256 with TASKS)
template <int KIND, bool EVD, int VK, bool TASKS, bool MC>
__device__ __forceinline__ void compact_chunk(const VertexView &vx, int H, int W, int vn, const int32_t *blkcnt,
                                              const int32_t *grpcnt, const uint64_t *fgbits, int32_t *dsagg,
                                              int nblk, int min_num, int max_num, uint64_t seed, const uint8_t *keep,
                                              int32_t *tn, int32_t *fgtot, float4 *pex, const int b, const int blk,
                                              int *sh, int *wcnt, uint16_t *pos, uint64_t *keptbits) {
    static_assert(kCompactChunk == 256, "one pixel per thread");
    const int64_t P = (int64_t)H * W;
    const int wid = threadIdx.x / 64, lane = lane_id();
    cstamp(blk, 0);
    // a block without foreground has nothing to store; only blocks 0 and
    // nblk - 1 (which write tn / fgtot) run on.  The downsampling look-back
    // below takes such a predecessor's kept count as 0 from its k_fg_count
    // count, without waiting for it.
    if (blk != 0 && blk != nblk - 1 && blkcnt[b * nblk + blk] == 0) return;
    // one round trip: this wave's foreground ballot (k_fg_count) beside the
    // image's per-block counts (the total and this block's row-major offset)
    const uint64_t fw = fgbits[((int64_t)b * nblk + blk) * 4 + wid];
    int2 tot;
    if constexpr (TASKS) {
        // the image's total and this chunk's prefix from the wide k_fg_count
        // blocks' sums (8 chunks each) and the chunks before it in its group
        const int ng = (nblk + 7) / 8, g0 = blk / 8;
        int all = 0, pre = 0;
        for (int j = threadIdx.x; j < ng; j += 256) {
            const int v = grpcnt[b * ng + j];
            all += v;
            pre += j < g0 ? v : 0;
        }
        if (threadIdx.x < 8 && g0 * 8 + (int)threadIdx.x < blk) pre += blkcnt[b * nblk + g0 * 8 + threadIdx.x];
        tot = block_sum2(all, pre, sh);
    } else {
        tot = image_totals(blkcnt + b * nblk, nblk, blk, sh);
    }
    cstamp(blk, 1);
    const int fgb = tot.x;
    if (fgb < min_num) {
        if (blk == 0 && threadIdx.x == 0) { tn[b] = 0; fgtot[b] = fgb; }
        return;
    }
    const bool ds = fgb > max_num;
    int base = tot.y;
    if (!ds && blk == 0 && threadIdx.x == 0) {
        tn[b] = fgb;
        fgtot[b] = fgb;
    }
    const uint32_t p = (uint32_t)blk * kCompactChunk + threadIdx.x;   // H, W <= 65535: fits
    bool f = (fw >> lane) & 1;
    if (ds && f) f = keep ? keep[b * P + p] != 0 : rand_unit(seed, (uint64_t)b * P + p) < (float)max_num / (float)fgb;
    const uint64_t bal = ds ? ballot(f) : fw;
    const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
    if (lane == 0) wcnt[wid] = __popcll(bal);
    if (ds && keptbits && lane == 0) {
        // the kept ballots for compact_hyp, stored before this block's
        // look-back value is published (the barrier below orders them)
        st_agent(&keptbits[((int64_t)b * nblk + blk) * 4 + wid], bal);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // this pixel's vertex loads (all keypoints of a group in flight together),
    // issued before the block's offsets are known: buffer loads through a
    // per-image descriptor, one VGPR offset for the pixel and the keypoint /
    // component plane offsets in SGPRs (host check: the image's view spans
    // < 2 GiB)
    const int r = (int)(p / (uint32_t)W), c = (int)(p - (uint32_t)r * W);
    constexpr int ES = VK == PV_VERTEX_F32 ? 4 : 2;
    const __amdgpu_buffer_rsrc_t vr = image_rsrc<MC>(vx, b, ES);
    const int voff = (int)((r * vx.s[1] + c * vx.s[2]) * ES);
    float nx[kCompactKp], ny[kCompactKp];
    auto load_group = [&](int v0) {
#pragma unroll
        for (int u = 0; u < kCompactKp; ++u) {
            nx[u] = ny[u] = 0.f;
            if (f && v0 + u < vn) {
                const int so = uniform((int)((v0 + u) * vx.s[3] * ES));
                const int s4 = uniform((int)(vx.s[4] * ES));
                if constexpr (VK == PV_VERTEX_F32) {
                    nx[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vr, voff, so, 0));
                    ny[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vr, voff, so + s4, 0));
                } else {
                    nx[u] = __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(vr, voff, so, 0)));
                    ny[u] = __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(vr, voff, so + s4, 0)));
                }
            }
        }
    };
    if constexpr (!TASKS) load_group(0);
    __syncthreads();
    const int nsel = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    int off = below;
    for (int q = 0; q < wid; ++q) off += wcnt[q];
    if constexpr (TASKS) {
        if (f) pos[off] = (uint16_t)threadIdx.x;   // the block's selected pixels in rank order
    }
    if (ds) {
        // Downsampled offsets by look-back: publish this block's kept count
        // (+1, so 0 = not yet; k_fg_count zeroed the array), then add up the
        // earlier blocks' counts, waiting for each.  No dispatch order is
        // assumed: a count not seen within kLookbackSpin (a block not yet
        // scheduled) is worked out by the waiting thread itself from the
        // foreground ballots and the keep decisions, so every wait ends.
        int32_t *agg = dsagg + (int64_t)b * nblk;
        if (threadIdx.x == 0) {
            st_agent(&agg[blk], nsel + 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const bool self_all = g_lb_self != 0;
        int pre = 0;
        // one deadline per thread (not per predecessor): after kLookbackSpin
        // the thread stops waiting and counts every unseen predecessor itself,
        // so no thread waits longer than kLookbackSpin in all
        const uint64_t t_dead = __builtin_amdgcn_s_memrealtime() + kLookbackSpin;
        for (int j = threadIdx.x; j < blk; j += 256) {
            if (blkcnt[b * nblk + j] == 0) continue;   // no foreground: kept 0 (the block may not publish)
            int v = self_all ? 0 : ld_agent(&agg[j]);
            if (v == 0 && !self_all)
                while ((v = ld_agent(&agg[j])) == 0 && __builtin_amdgcn_s_memrealtime() < t_dead)
                    __builtin_amdgcn_s_sleep(1);
            if (v == 0) {   // block j's kept count from its ballots
                for (int q = 0; q < 4; ++q) {
                    uint64_t w = fgbits[((int64_t)b * nblk + j) * 4 + q];
                    while (w) {
                        const uint32_t pj = (uint32_t)j * kCompactChunk + q * 64 + __builtin_ctzll(w);
                        w &= w - 1;
                        v += keep ? keep[b * P + pj] != 0
                                  : rand_unit(seed, (uint64_t)b * P + pj) < (float)max_num / (float)fgb;
                    }
                }
                ++v;
            }
            pre += v - 1;
        }
        base = block_sum2(pre, 0, sh).x;
        if (blk == nblk - 1 && threadIdx.x == 0) { tn[b] = base + nsel; fgtot[b] = fgb; }
    }
    cstamp(blk, 2);
    // the selected pixel's records at t = base + its rank: consecutive
    // selected pixels write consecutive records of each keypoint
    float4 *eb = pex + (int64_t)b * vn * P;
    if constexpr (TASKS) {
        // one (selected pixel, keypoint) record per thread and pass, keypoint
        // major: the block's nsel x vn records spread over all its lanes (with
        // a sparse mask a lane-per-pixel store pass runs ~8 % of its lanes)
        __syncthreads();   // pos written
        const int n = nsel * vn;
        const int s4 = uniform((int)(vx.s[4] * ES));
        for (int i = (int)threadIdx.x; i < n; i += 256) {
            const int v = (int)((uint32_t)i / (uint32_t)nsel), k = i - v * nsel;
            const uint32_t pp = (uint32_t)blk * kCompactChunk + pos[k];
            const int rr = (int)(pp / (uint32_t)W), cc = (int)(pp - (uint32_t)rr * W);
            const int vo = (int)((rr * vx.s[1] + cc * vx.s[2] + v * vx.s[3]) * ES);
            float x, y;
            if constexpr (VK == PV_VERTEX_F32) {
                x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vr, vo, 0, 0));
                y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vr, vo, s4, 0));
            } else {
                x = __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(vr, vo, 0, 0)));
                y = __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(vr, vo, s4, 0)));
            }
            const int64_t t = base + k;   // (bounded as below)
            if (t < P) eb[(int64_t)v * P + t] = make_float4((float)cc, (float)rr, x, y);
        }
        cstamp(blk, 3);
        return;
    }
    const int64_t t = base + off;
    // t < fg <= P whenever the counts are this call's own; the bound keeps a
    // workspace shared by two calls in flight (a caller error) from writing
    // past the image's records
    const bool store = f && t < P;
    for (int v0 = 0; v0 < vn; v0 += kCompactKp) {
        if (v0 > 0) load_group(v0);
        if (store) {
#pragma unroll
            for (int u = 0; u < kCompactKp; ++u) {
                if (v0 + u >= vn) break;
                const int64_t o = (int64_t)(v0 + u) * P + t;
                // the reference's operands only: the vote kernel makes the fast
                // test's (prep_compacted) while it stages them
                eb[o] = make_float4((float)c, (float)r, nx[u], ny[u]);
            }
        }
    }
    cstamp(blk, 3);
}

// ==========================================================================
// K3 inside K2 (round 6): the hypotheses (KU:11-49, RV:553-557) made by the
// first `nhb` blocks of k_compact's grid, beside the compaction, instead of a
// k_hyp_gen launch after it.  Everything they need is k_fg_count's (the
// kernel before): the image's chunk counts give tn and a chunk prefix (LDS),
// a pair index t finds its chunk by binary search and its pixel by a bit
// select in that chunk's four wave ballots, and the pixel's direction is read
// from the input view -- the same (col, row, nx, ny) k_compact stores as its
// record, so the hypotheses are bit-identical to k_hyp_gen's.  Downsampled
// images (fg > max_num) rank the kept pixels: kept counts from the
// compaction blocks' look-back values (a count not seen within kLookbackSpin
// is worked out from the ballots and keep decisions), kept bits by the same
// keep decision.  One dependent trip more than a compaction block (the
// ballots), one kernel fewer in the call's chain: a k_hyp_gen launch costs
// the batch-1 stream ~9 % (profiles/r06/ablation.txt).
// ==========================================================================
template <int VK>
__device__ __forceinline__ void read_dir(const __amdgpu_buffer_rsrc_t &vr, int voff, int s4, float &x, float &y) {
    if constexpr (VK == PV_VERTEX_F32) {
        x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vr, voff, 0, 0));
        y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vr, voff, s4, 0));
    } else {
        x = __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(vr, voff, 0, 0)));
        y = __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(vr, voff, s4, 0)));
    }
}

// the q-th set bit (0-based) of the 256-bit mask w[0..3]; q < popcount
__device__ __forceinline__ int select_bit(const uint64_t (&w)[4], int q) {
    int base = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = __popcll(w[k]);
        if (q < c) {
            uint64_t x = w[k];
            uint32_t lo = (uint32_t)x;
            int off = 0;
            if (q >= __popc(lo)) { q -= __popc(lo); lo = (uint32_t)(x >> 32); off = 32; }
            // binary descent on the 32-bit half
            int pos = 0;
#pragma unroll
            for (int sh = 16; sh >= 1; sh >>= 1) {
                const int c2 = __popc(lo & ((1u << sh) - 1u));
                if (q >= c2) { q -= c2; lo >>= sh; pos += sh; }
            }
            return base + off + pos;
        }
        q -= c;
        base += 64;
    }
    return 255;
}

template <int KIND, bool EVD, int VK, bool MC>
__device__ void compact_hyp(const VertexView &vx, int H, int W, int nblk, const int32_t *blkcnt,
                            const uint64_t *fgbits, const int32_t *dsagg, int32_t *pre, int *sh, const HypGen &g,
                            int b, int hb) {
    const int64_t P = (int64_t)H * W;
    const int per = (nblk + 255) / 256;            // consecutive chunks per thread (<= 6)
    // ---- the image's chunk counts and their exclusive prefix (one trip)
    int c[6];
    const int j0 = (int)threadIdx.x * per;
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = k < per && j0 + k < nblk ? blkcnt[b * nblk + j0 + k] : 0;
    auto scan = [&](int (&v)[6]) -> int {        // block exclusive scan into pre[], returns the total
        int run = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) run += v[k];
        // inclusive wave scan of run (row shifts + row broadcasts)
        int x = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane_id() >= o) x += y;
        }
        __syncthreads();
        if (lane_id() == 63) sh[threadIdx.x / 64] = x;
        __syncthreads();
        int wpre = 0;
        for (int w = 0; w < (int)threadIdx.x / 64; ++w) wpre += sh[w];
        const int total = sh[0] + sh[1] + sh[2] + sh[3];
        int e = wpre + x - run;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (k < per && j0 + k < nblk) { pre[j0 + k] = e; e += v[k]; }
        if (threadIdx.x == 0) pre[nblk] = total;
        __syncthreads();
        return total;
    };
    const int fgb = scan(c);
    if (fgb < g.min_num) return;                   // tn = 0: no hypotheses (as k_hyp_gen)
    const bool ds = fgb > g.max_num;
    const float pk = (float)g.max_num / (float)fgb;
    auto kept = [&](int64_t p) -> bool {
        return g.keep ? g.keep[b * P + p] != 0 : rand_unit(g.kseed, (uint64_t)b * P + p) < pk;
    };
    int n = fgb;
    uint32_t seen = 0;                             // ds: chunks whose kept count (and ballots) were published
    if (ds) {
        // kept counts from the compaction blocks' look-back values (count + 1)
        const uint64_t t_dead = __builtin_amdgcn_s_memrealtime() + kLookbackSpin;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int j = j0 + k;
            if (!(k < per && j < nblk) || c[k] == 0) { c[k] = 0; continue; }
            int v = g_lb_self ? 0 : ld_agent(&dsagg[b * nblk + j]);
            while (v == 0 && !g_lb_self && __builtin_amdgcn_s_memrealtime() < t_dead) {
                __builtin_amdgcn_s_sleep(1);
                v = ld_agent(&dsagg[b * nblk + j]);
            }
            if (v != 0) seen |= 1u << k;
            if (v == 0) {                          // worked out from the ballots and keep decisions
                for (int q = 0; q < 4; ++q) {
                    uint64_t w = fgbits[((int64_t)b * nblk + j) * 4 + q];
                    while (w) {
                        v += kept((int64_t)j * kCompactChunk + q * 64 + __builtin_ctzll(w));
                        w &= w - 1;
                    }
                }
                ++v;
            }
            c[k] = v - 1;
        }
        n = scan(c);
        // which chunks' kept ballots are published: bit j of the LDS words
        // after pre[] (pre[nblk + 1 ...]); the rest are worked out below
        int32_t *pub = pre + nblk + 1;
        for (int q = (int)threadIdx.x; q < (nblk + 31) / 32; q += 256) pub[q] = 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if ((seen >> k) & 1u) atomicOr(&pub[(j0 + k) >> 5], 1 << ((j0 + k) & 31));
        __syncthreads();
    }
    n = min(n, (int)P);
    if (n <= 0) return;
    // ---- this thread's hypothesis: item i = (h, v) of image b; returns its class (hyp_class)
    const int i = hb * 256 + (int)threadIdx.x;
    const bool act = i < g.nh * g.vn;
    auto make = [&]() -> uint32_t {
        const int h = i / g.vn, v = i - h * g.vn;
        const int64_t gid = ((int64_t)b * g.nh + h) * g.vn + v;
        int t[2];
        if (g.idxs) {
            t[0] = min(max(g.idxs[gid * 2], 0), n - 1);
            t[1] = min(max(g.idxs[gid * 2 + 1], 0), n - 1);
        } else {
            const uint64_t key = (uint64_t)gid;
            t[0] = rand_index(g.seed, key * 2, n);
            t[1] = rand_index(g.seed, key * 2 + 1, n);
        }
        int jj[2], rr[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {                  // the last chunk with pre <= t (never an empty one)
            int lo = 0, hi = nblk - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= t[e]) lo = mid; else hi = mid - 1;
            }
            jj[e] = lo;
            rr[e] = t[e] - pre[lo];
        }
        uint64_t w0[4], w1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            w0[q] = fgbits[((int64_t)b * nblk + jj[0]) * 4 + q];
            w1[q] = fgbits[((int64_t)b * nblk + jj[1]) * 4 + q];
        }
        if (ds) {                                      // keep only the kept pixels' bits
            const int32_t *pub = pre + nblk + 1;
            const bool p0 = g.keptbits && ((pub[jj[0] >> 5] >> (jj[0] & 31)) & 1);
            const bool p1 = g.keptbits && ((pub[jj[1] >> 5] >> (jj[1] & 31)) & 1);
            // published: the compaction block's own kept ballots (one load)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (p0) w0[q] = ld_agent(&g.keptbits[((int64_t)b * nblk + jj[0]) * 4 + q]);
                if (p1) w1[q] = ld_agent(&g.keptbits[((int64_t)b * nblk + jj[1]) * 4 + q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (p0 && p1) break;
                uint64_t m0 = w0[q], m1 = w1[q], x0 = p0 ? 0 : w0[q], x1 = p1 ? 0 : w1[q];
                if (!p0) m0 = 0;
                if (!p1) m1 = 0;
                while (x0) { const int z = __builtin_ctzll(x0); x0 &= x0 - 1;
                             if (kept((int64_t)jj[0] * kCompactChunk + q * 64 + z)) m0 |= 1ull << z; }
                while (x1) { const int z = __builtin_ctzll(x1); x1 &= x1 - 1;
                             if (kept((int64_t)jj[1] * kCompactChunk + q * 64 + z)) m1 |= 1ull << z; }
                w0[q] = m0; w1[q] = m1;
            }
        }
        constexpr int ES = VK == PV_VERTEX_F32 ? 4 : 2;
        const __amdgpu_buffer_rsrc_t vr = image_rsrc<MC>(vx, b, ES);
        const int s4 = (int)(vx.s[4] * ES);
        float cx[2], cy[2], nx[2], ny[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int q = select_bit(e == 0 ? w0 : w1, rr[e]);
            const uint32_t p = (uint32_t)jj[e] * kCompactChunk + (uint32_t)q;
            const int r = (int)(p / (uint32_t)W), col = (int)(p - (uint32_t)r * W);
            cx[e] = (float)col;
            cy[e] = (float)r;
            read_dir<VK>(vr, (int)((r * vx.s[1] + col * vx.s[2] + v * vx.s[3]) * ES), s4, nx[e], ny[e]);
        }
        float x = 0.f, y = 0.f, ox, oy;
        if (exact_intersect(nx[0], ny[0], cx[0], cy[0], nx[1], ny[1], cx[1], cy[1], &ox, &oy)) { x = ox; y = oy; }
        g.hyp_out[gid] = make_float2(x, y);
        if (g.diag_hyp) { g.diag_hyp[gid * 2] = x; g.diag_hyp[gid * 2 + 1] = y; }
        g.hypv_out[((int64_t)b * g.vn + v) * g.nh + h] = make_float2(x, y);
        return hyp_class(x, y);
    };
    const uint32_t cls = act ? make() : 0u;
    // the classes' ballots, gathered per block in LDS (pre[] is free once every thread has its pixels)
    __syncthreads();
    hypcls_block_put(g.hypcls, (uint32_t *)pre, b, g.vn, g.nh, i, act, cls);
}

// TASKS (grids above kFgWideAbove blocks, i.e. batches): the records are
// written by (pixel, keypoint) tasks spread over the block instead of by the
// pixel's own lane (configs[2]'s 32 network frames, ~8 % foreground: 69 us).
// With g.nhb > 0 the grid's first g.nhb blocks per image make the hypotheses.
template <int KIND, bool EVD, int VK, bool TASKS, bool MC = false>
__global__ __launch_bounds__(256) void k_compact(MaskView, VertexView vx, int H, int W, int vn,
                                                 const int32_t *blkcnt, const int32_t *grpcnt,
                                                 const uint64_t *fgbits, int32_t *dsagg,
                                                 int nblk, int min_num, int max_num, uint64_t seed,
                                                 const uint8_t *keep, int32_t *tn, int32_t *fgtot, float4 *pex,
                                                 HypGen g) {
    __shared__ int sh[8];
    __shared__ int wcnt[4];
    __shared__ uint16_t pos[TASKS ? kCompactChunk : 1];
    __shared__ int32_t pre[kHypMaxChunks + 1 + (kHypMaxChunks + 31) / 32];
    if ((int)blockIdx.x < g.nhb) {
        compact_hyp<KIND, EVD, VK, MC>(vx, H, W, nblk, blkcnt, fgbits, dsagg, pre, sh, g, (int)blockIdx.y, (int)blockIdx.x);
        return;
    }
    compact_chunk<KIND, EVD, VK, TASKS, MC>(vx, H, W, vn, blkcnt, grpcnt, fgbits, dsagg, nblk, min_num, max_num, seed, keep, tn,
                                        fgtot, pex, (int)blockIdx.y, (int)blockIdx.x - g.nhb, sh, wcnt, pos,
                                        g.nhb > 0 ? g.keptbits : nullptr);
}

template <int KIND, bool EVD>
struct CompactStage {
    template <int VK, bool TASKS>
    static void launch_compact(const CompactArgs *a) {
        k_compact<KIND, EVD, VK, TASKS><<<dim3(a->nblk + a->hg.nhb, a->b), 256, 0, a->s>>>(
            a->m, a->vx, a->H, a->W, a->vn, a->ws.blkcnt, a->ws.grpcnt, a->ws.fgbits, a->ws.dsagg, a->nblk, a->min_num,
            a->max_num, a->seed, a->keep, a->ws.tn, a->ws.fgtot, a->ws.pex, a->hg);
    }
    static int run(const CompactArgs *a) {
        static_assert(kFgWideCPB == 8, "grpcnt: groups of 8 chunks");
        const bool wide = (int64_t)a->nblk * a->b > kFgWideAbove;
        if (g_abl & 16) {
        } else if (wide)
            k_fg_count<KIND, EVD, kFgWideCPB><<<dim3((a->nblk + kFgWideCPB - 1) / kFgWideCPB, a->b), 256, 0, a->s>>>(
                a->m, a->H, a->W, a->ws.blkcnt, a->ws.fgbits, a->ws.grpcnt, a->nblk, (int32_t *)a->ws.hypcls, a->ws.zero_words);
        else
            k_fg_count<KIND, EVD, 1><<<dim3(a->nblk, a->b), 256, 0, a->s>>>(a->m, a->H, a->W, a->ws.blkcnt, a->ws.fgbits,
                                                                          nullptr, a->nblk, (int32_t *)a->ws.hypcls,
                                                                          a->ws.zero_words);
        if (g_abl & 1) return last();
        const bool f32 = a->vx.kind == PV_VERTEX_F32;
        if (wide) f32 ? launch_compact<PV_VERTEX_F32, true>(a) : launch_compact<PV_VERTEX_F16, true>(a);
        else f32 ? launch_compact<PV_VERTEX_F32, false>(a) : launch_compact<PV_VERTEX_F16, false>(a);
        return last();
    }
};

// A multi-object call (a->ncls >= 1; a->b counts the b * ncls virtual images):
// k_label_count in k_fg_count's place, then k_compact with the class offset in
// its vertex view.  k_compact never reads the mask, so one mask kind's
// instantiation serves all of them.
template <int KIND>
int compact_multi(const CompactArgs *a) {
    const int bi = a->b / a->ncls;
    const bool wide = (int64_t)a->nblk * a->b > kFgWideAbove;   // the same for both kernels
    if (wide)
        k_label_count<KIND, kFgWideCPB><<<dim3((a->nblk + kFgWideCPB - 1) / kFgWideCPB, bi), 256, 0, a->s>>>(
            a->m, a->H, a->W, a->ncls, a->ws.blkcnt, a->ws.fgbits, a->ws.grpcnt, a->nblk, (int32_t *)a->ws.hypcls,
            a->ws.zero_words);
    else
        k_label_count<KIND, 1><<<dim3(a->nblk, bi), 256, 0, a->s>>>(a->m, a->H, a->W, a->ncls, a->ws.blkcnt,
                                                                   a->ws.fgbits, nullptr, a->nblk, (int32_t *)a->ws.hypcls,
                                                                   a->ws.zero_words);
    auto launch = [&](auto kernel) {
        kernel<<<dim3(a->nblk + a->hg.nhb, a->b), 256, 0, a->s>>>(
            a->m, a->vx, a->H, a->W, a->vn, a->ws.blkcnt, a->ws.grpcnt, a->ws.fgbits, a->ws.dsagg, a->nblk, a->min_num,
            a->max_num, a->seed, a->keep, a->ws.tn, a->ws.fgtot, a->ws.pex, a->hg);
    };
    const bool f32 = a->vx.kind == PV_VERTEX_F32;
    if (wide) f32 ? launch(k_compact<PV_MASK_I64, false, PV_VERTEX_F32, true, true>)
                  : launch(k_compact<PV_MASK_I64, false, PV_VERTEX_F16, true, true>);
    else f32 ? launch(k_compact<PV_MASK_I64, false, PV_VERTEX_F32, false, true>)
             : launch(k_compact<PV_MASK_I64, false, PV_VERTEX_F16, false, true>);
    return last();
}

}  // namespace

namespace pvv __attribute__((visibility("hidden"))) {
int compact(const CompactArgs &a) {
    if (a.ncls > 0) {
        switch (a.mask_kind) {
        case PV_MASK_I64: return compact_multi<PV_MASK_I64>(&a);
        case PV_MASK_U8: return compact_multi<PV_MASK_U8>(&a);
        case PV_MASK_I32: return compact_multi<PV_MASK_I32>(&a);
        case PV_MASK_SEG_F32: return compact_multi<PV_MASK_SEG_F32>(&a);
        case PV_MASK_SEG_F16: return compact_multi<PV_MASK_SEG_F16>(&a);
        default: return PV_EINVAL;
        }
    }
    return dispatch_mask<CompactStage>(a.mask_kind, a.evd, &a);
}
}  // namespace pvv

extern "C" {

// debug only (not in pvvote.h): the downsampling look-back counts every earlier
// block itself instead of reading its count (tests of the fallback path)
int pv_debug_lookback_self(int32_t on) {
    return rc(hipMemcpyToSymbol(HIP_SYMBOL(g_lb_self), &on, sizeof(on)));
}

#ifdef PVV_TRACE
int pv_debug_compact_trace(int on, uint64_t *host, int n) {
    if (host) return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_ctrace), sizeof(uint64_t) * (size_t)n);
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_ctrace_on), &on, sizeof(int));
}
#endif

}  // extern "C"
