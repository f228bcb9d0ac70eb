// pv_stages.h -- what the stages, each in its own translation unit, expose to
// the pipeline (pvpipeline.hip): each stage's host launcher and its argument
// struct.  Internal to libpvvote.so (namespace pvv, hidden visibility); the
// exported C ABI is include/pvvote.h.
#pragma once

#include "pv_band.h"
#include "pv_common.h"
#include "pv_host.h"

namespace pvv __attribute__((visibility("hidden"))) {

#ifdef PVV_PROFILE
// profiling builds only (tools/build_variant.py profile -DPVV_PROFILE): the
// ablation bits in effect (pv_debug_set_ablation, set between captures by the
// profiling tools; outputs wrong): 1 no k_compact, 2 no k_hyp_gen, 4 no vote,
// 8 no refine, 16 no k_fg_count, 32 an empty launch in k_hyp_gen's place,
// 64 k_vote_mfma's band pairs not re-checked, 128 found but not queued
extern int g_abl;
#else
constexpr int g_abl = 0;
#endif

// ---- compaction (pvcompact.hip) -------------------------------------------
constexpr int kHypMaxChunks = 1536;   // chunks per image the fused hypotheses handle (LDS prefix); more: k_hyp_gen
struct HypGen {
    int nhb;                    // hypothesis blocks per image (0: none, k_hyp_gen runs)
    int nh, vn, min_num, max_num;
    uint64_t seed;              // the hypotheses' counter RNG (VoteArgs::seed)
    uint64_t kseed;             // the downsampling keep decisions' (k_compact's seed)
    const int32_t *idxs;        // [b][nh][vn][2] pixel pairs, or nullptr (counter RNG)
    const uint8_t *keep;
    float2 *hyp_out;            // [b][nh][vn]
    float2 *hypv_out;           // [b][vn][nh]
    uint32_t *hypcls;           // [b][vn][nset][2] the classes' ballots (Workspace::hypcls, zeroed by k_fg_count)
    float *diag_hyp;            // [b][nh][vn][2] or nullptr
    uint64_t *keptbits;         // downsampled images: the compaction blocks' kept ballots [b][nblk][4]
};

struct CompactArgs {
    int mask_kind;      // PV_MASK_*
    bool evd;           // foreground predicate: EVD's `mask == 1` (else `mask.byte() != 0`)
    MaskView m;
    VertexView vx;
    int b, H, W, vn, nblk, min_num, max_num;   // b: the pipeline's images (b * ncls virtual ones when ncls > 0)
    int ncls;           // classes of a multi-object call (mask = label map, k_label_count); 0: one object per image
    uint64_t seed;
    const uint8_t *keep;
    Workspace ws;
    HypGen hg;          // hg.nhb > 0: k_compact's first blocks make the hypotheses
    hipStream_t s;
};

// k_fg_count + k_compact (+ the fused hypotheses) of one call
int compact(const CompactArgs &a);

// ---- hypotheses and the fused vote/count (pvvote.hip) ---------------------
constexpr int kHypLane = 2;                 // hypotheses per lane of a vote wave
constexpr int kGroup = kWave * kHypLane;    // hypotheses per wave: a hypothesis group, the unit of the vote's work index
static_assert(kGroup == 128, "hyp_sets (pv_common.h): four 32-hypothesis sets per group");

// The classes of a producer block's hypotheses into the classes' ballots (Workspace::hypcls, zeroed before).
// Every thread of the 256 calls it; an active one holds item r = h * vn + v of image b (consecutive threads
// hold consecutive items) and cls = hyp_class of the value it stored.  A block's items of one keypoint fall
// into a few 32-hypothesis sets, each shared with the neighbouring blocks: the bits are gathered in LDS at the
// slot of the set's first thread in the block (its leader), which ORs the two words into memory -- two or
// three atomics per word over the grid, not one per hypothesis on the same address.  lds: 512 words.
__device__ __forceinline__ void hypcls_block_put(uint32_t *hypcls, uint32_t *lds, int b, int vn, int nh, int r,
                                                 bool active, uint32_t cls) {
    const int t = (int)threadIdx.x;
    lds[t] = 0;
    lds[256 + t] = 0;
    __syncthreads();
    int lead = t, h = 0, v = 0;
    if (active) {
        h = r / vn;
        v = r - h * vn;
        const int r0 = max(r - t, 0);                       // the block's first item of this image
        const int hf = (r0 - v + vn - 1) / vn;              // keypoint v's first hypothesis in the block
        lead = t - (h - max(h & ~31, hf)) * vn;             // the thread of (that or the set's first one, v)
        if (cls & kHypFast) atomicOr(&lds[lead], 1u << (h & 31));
        if (cls & kHypExact) atomicOr(&lds[256 + lead], 1u << (h & 31));
    }
    __syncthreads();
    if (active && lead == t) {
        uint32_t *w = hypcls + (((int64_t)b * vn + v) * hyp_sets(nh) + (h >> 5)) * 2;
        const uint32_t f = lds[t], x = lds[256 + t];
        if (f) atomicOr(w, f);
        if (x) atomicOr(w + 1, x);
    }
}

struct VoteArgs {
    const float4 *pex;          // PREPPED: exact data (cx, cy, nx, ny), same layout
    const float2 *coords;       // !PREPPED: coords[b*P + t]
    const float2 *raw;          // !PREPPED: raw[b*vn*P + v*raw_v + t*raw_t]
    const float2 *hyp;          // !GEN: hyp[b*hyp_sb + v*hyp_sv + h*hyp_sh]
    float2 *hyp_out;            // GEN: generated hypotheses [b][nh][vn]
    float2 *hypv_out;           // k_hyp_gen: keypoint-major copy [b][vn][nh]
    uint32_t *hypcls;           // k_hyp_gen writes, the pipeline's k_vote_mfma reads: Workspace::hypcls [b][vn][nset][2]
    int64_t hyp_sb, hyp_sv, hyp_sh;
    float *diag_hyp;            // GEN: optional copy [b][nh][vn][2]
    const int32_t *idxs;        // GEN: pixel pairs [b][nh][vn][2], or nullptr (counter RNG)
    int32_t *counts;            // counts[b*cnt_bs + v*cnt_v + h*cnt_h]
    const int32_t *tn_dev;      // [b] pixels per image, or nullptr (tn_host)
    uint64_t seed;
    int32_t P, raw_v, raw_t, cnt_v, cnt_h, cnt_bs;
    int32_t tn_host, b, vn, nh, hgn, fast;
    int32_t b0;                 // GEN: batch index of image 0 of this launch (RNG key: the same pairs in any chunking)
    float thr, tau, gzf, gzr;
    uint64_t *trace;            // debug: per-wave (start, end) s_memrealtime stamps, or nullptr
    int32_t rw[4];              // k_vote_count, four resident rounds of blocks: work weights per round (0: even)
};

// thr, tau, gzf, gzr and fast of `va` from the inlier threshold (the byte kernel takes its own from a scratch VoteArgs)
void fast_constants(float thr, VoteArgs *va);
// does the pipeline pre-generate the hypotheses (keypoint-major in w.hypv: k_hyp_gen or k_compact's first blocks)?
bool hyp_pregen_used(int nh);
// k_hyp_gen over va's b images: hyp_out and hypv_out
void launch_hyp_gen(const VoteArgs &va, hipStream_t s);
// the fused vote/count of one launch chunk on compacted pixels (va.pex): k_vote_mfma, or k_vote_count
// (PV_EINVAL, nothing launched: k_vote_mfma's turn without pre-generated hypotheses and their classes)
int launch_pipeline_vote(const VoteArgs &va, int64_t pixel_steps, hipStream_t s);

// ---- refine and v5 confidence (pvrefine.hip) ------------------------------
// k_refine_solve over the workspace's counts; hypv: the hypotheses keypoint-major (w.hypv)
void launch_refine(const Workspace &w, bool hypv, int b, int vn, int nh, int64_t P, const pv_vote_params *prm,
                   float *out, const pv_v3_diag &dg, hipStream_t s);
void launch_point_conf(const Workspace &w, const float *pts, int b, int vn, int64_t P, float thr, float *conf,
                       hipStream_t s);

// ---- EVD and motion (pvevd.hip) -------------------------------------------
void launch_evd_with_mean(const Workspace &w, int b, int vn, int nh, int min_num, int min_hyp_num,
                          const float *mean, float *cov, hipStream_t s);
void launch_evd_topk(const Workspace &w, int b, int vn, int nh, int min_num, int topk, float *mean, float *cov,
                     hipStream_t s);
int launch_motion(int mask_kind, const MaskView &m, const VertexView &vx, int b, int H, int W, int vn, double *acc,
                  int32_t *cnt, int32_t *ticket, float *out, hipStream_t s);

}  // namespace pvv
