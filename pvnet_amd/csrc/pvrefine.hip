// pvrefine.hip -- the pipeline's last stage: the winning hypothesis of each
// (image, keypoint) and the least-squares refinement over its inliers
// (k_refine_solve), and v5's confidence of the refined point (k_point_conf).
// Host entries: pvv::launch_refine / launch_point_conf (pv_stages.h); the
// refine trace of trace builds lives here with the device global it sets.
#include "pv_stages.h"

namespace {
using namespace pvv;

// f32 2x2 inverse as LAPACK sgesv(A, I) (partial pivoting); false if a pivot is 0.
__device__ inline bool lu2_inv(float a00, float a01, float a10, float a11, float inv[4]) {
    bool sw = fabsf(a10) > fabsf(a00);
    if (sw) { float t0 = a00, t1 = a01; a00 = a10; a01 = a11; a10 = t0; a11 = t1; }
    if (a00 == 0.f) return false;
    float l = a10 / a00;
    float u11 = a11 - l * a01;
    if (u11 == 0.f) return false;
    for (int jc = 0; jc < 2; ++jc) {
        float e0 = (jc == 0) ? 1.f : 0.f, e1 = (jc == 1) ? 1.f : 0.f;
        float b0 = sw ? e1 : e0, b1 = sw ? e0 : e1;
        float y1 = b1 - l * b0;
        float x1 = y1 / u11;
        float x0 = (b0 - a01 * x1) / a00;
        inv[0 * 2 + jc] = x0;
        inv[1 * 2 + jc] = x1;
    }
    return true;
}

// ==========================================================================
// K6: winner per (image, keypoint) (RV:567-575) + least-squares partial sums
// over the winner's inliers (RV:584-599, fp64), kRefineNJ blocks per
// keypoint; the last block of each image gathers its image's partials, sums
// them per keypoint in a fixed order, solves (pts = b_inv(ATA) @ ATb, RV:600)
// with b_inv's batch-wide identity fallback (RV:503-518).
// Hand-off (cdna_hip_programming.md Guideline 16, R2: the data is the flag):
// every value travels as 8-B granules {32-bit half, tag}, a pair per 16-B
// sc1 store; the gathering block re-reads them with 16-B sc1 loads until
// every tag is set.  The granules are zeroed by k_fg_count every call; no
// ticket, no drain before a signal, one memory trip from publish to use.
// ==========================================================================
#ifdef PVV_TRACE
__device__ uint64_t *g_refine_trace;   // trace builds only: per-block phase stamps of k_refine_solve
#define PVR_STAMP(k)                                                                                      \
    if (g_refine_trace && threadIdx.x == 0)                                                               \
        g_refine_trace[(((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + (k)] = \
            __builtin_amdgcn_s_memrealtime()
#else
#define PVR_STAMP(k)
#endif
constexpr uint32_t kRefineTag = 1u;           // granule tag (slots zeroed every call)
constexpr uint32_t kRefineSpinMax = 1u << 21;  // gather polls before giving up (~seconds): outputs NaN
// BIG: nh > 1024 hypotheses (the winner's is fetched, not kept in LDS; the
// counts beyond the first 1024 read in a loop) -- its own instantiation, so
// the common one has no loop whose loads would make the compiler drain every
// load in flight before the argmax
template <bool BIG>
__global__ __launch_bounds__(kRT) void k_refine_solve(const int32_t *counts, const float2 *hyp, int64_t hsb, int hsv,
                                                      int hsh, const float4 *pex, const int32_t *tn, int64_t P, int vn,
                                                      int nh, float thr, uint4 *slot, float confidence, int max_iter,
                                                      float *out, pv_v3_diag diag) {
    const int j = blockIdx.x, v = blockIdx.y, b = blockIdx.z;
    PVR_STAMP(0);
    __shared__ uint64_t skey[kRT / 16];
    __shared__ double sacc[kRT / 16][5];   // row sums (16-lane rows)
    constexpr int HC = kRefineLdsHyp / kRT;         // counts / hypotheses per thread, in registers
    static_assert(kRefineLdsHyp % kRT == 0, "PVV_REFINE_T divides the LDS hypothesis capacity");
    __shared__ float2 shyp[kRefineLdsHyp];
    // Loads are issued in the order they are needed and return in that order:
    // the pixel count, the keypoint's vote counts and hypotheses (the argmax
    // needs only those), then this block's pixels (the winner's votes).
    const int n = min(max(tn[b], 0), (int)P);   // clamped like tn_at: loads stay inside the P records
    const int32_t *cnt = counts + ((int64_t)b * vn + v) * nh;
    const float2 *hb = hyp + b * hsb + (int64_t)v * hsv;
    constexpr bool lds_hyp = !BIG;
    int32_t c[HC];
    float2 hh[HC];
    // (every load unconditional, its index clamped into range, so that no
    // branch makes the compiler wait for all of them before the first use)
#pragma unroll
    for (int q = 0; q < HC; ++q) c[q] = cnt[min((int)threadIdx.x + q * kRT, nh - 1)];
#pragma unroll
    for (int q = 0; q < HC; ++q) hh[q] = hb[(int64_t)min((int)threadIdx.x + q * kRT, nh - 1) * hsh];
    constexpr int U = 32768 / (kRefineNJ * kRT);    // 32768 pixels per keypoint preloaded
    static_assert(U >= 1, "PVV_REFINE_NJ * PVV_REFINE_T must not exceed 32768 (preload depth)");
    static_assert(kRT % 64 == 0 && kRT <= 1024, "PVV_REFINE_T: whole waves, at most 1024 threads");
    // (guarded by the buffer's extent P, not by tn: the loads do not wait for
    // tn's; records at t >= tn are read but never used)
    const float4 *eb = pex + ((int64_t)b * vn + v) * P;
    const int t0 = j * kRT + threadIdx.x, tstep = kRefineNJ * kRT;
    float4 e[U];
#pragma unroll
    for (int u = 0; u < U; ++u) e[u] = eb[min(t0 + u * tstep, (int)P - 1)];
    // argmax over h, first index on ties: key = count << 32 | ~h
    uint64_t key = 0;
    auto take = [&](int32_t cv, int h) {
        const uint64_t k2 = ((uint64_t)(uint32_t)cv << 32) | (uint32_t)(0xffffffffu - (uint32_t)h);
        key = k2 > key ? k2 : key;
    };
#pragma unroll
    for (int q = 0; q < HC; ++q) {
        const int h = (int)threadIdx.x + q * kRT;
        take(h < nh ? c[q] : 0, h < nh ? h : -1);   // out of range: key 0 (the initial value)
    }
    if constexpr (BIG)
        for (int h = (int)threadIdx.x + kRefineLdsHyp; h < nh; h += kRT) take(cnt[h], h);
    if constexpr (lds_hyp)
#pragma unroll
        for (int q = 0; q < HC; ++q)
            if ((int)threadIdx.x + q * kRT < nh) shyp[threadIdx.x + q * kRT] = hh[q];
    key = row_max_u64(key);                      // DPP within 16-lane rows, rows through LDS
    if ((lane_id() & 15) == 0) skey[threadIdx.x / 16] = key;
    __syncthreads();
    PVR_STAMP(1);
    key = skey[0];
#pragma unroll
    for (int q = 1; q < kRT / 16; ++q) key = skey[q] > key ? skey[q] : key;
    const int win = (int)(0xffffffffu - (uint32_t)key);
    const int wcnt = (int)(key >> 32);
    // RV:570-575: ratio = count / tn; best starts at 0 and is replaced only on a strict increase
    const float ratio = n > 0 ? (float)wcnt / (float)n : 0.f;
    float2 best = make_float2(0.f, 0.f);
    if (n > 0 && 0.f < ratio) best = lds_hyp ? shyp[win] : hb[(int64_t)win * hsh];
#ifdef PVV_TRACE
    if (g_refine_trace) {   // trace builds: when the block's pixels have arrived
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        PVR_STAMP(7);
    }
#endif
    double acc[5] = {0, 0, 0, 0, 0};
    const bool fast = thr >= 1e-3f && thr <= 1.f;
    const float thr2 = thr * thr;
    // branch-free: the squared pre-test decides by selects; the exact sequence
    // runs only when some lane of the wave is undecided; an outlier adds zeros
    auto accum = [&](const float4 &q, bool valid) {   // (cx, cy, nx, ny)
        bool inl, und;
        refine_vote_pre(q.z, q.w, q.x, q.y, best.x, best.y, thr2, fast, &inl, &und);
        und = und && valid;
        if (__ballot(und)) {
            if (und) inl = exact_vote(q.z, q.w, q.x, q.y, best.x, best.y, thr);
        }
        inl = inl && valid;
        const float n0 = inl ? q.w : 0.f, n1 = inl ? -q.z : 0.f;   // RV:585-587 normal = (d_y, -d_x)
        const float bb = inl ? q.w * q.x + -q.z * q.y : 0.f;       // RV:597 (2-term fp32 sum)
        // f32 x f32 is exact in f64, so each fma equals the product-then-add
        const double d0 = n0, d1 = n1, db = bb;
        acc[0] = __fma_rn(d0, d0, acc[0]);
        acc[1] = __fma_rn(d0, d1, acc[1]);
        acc[2] = __fma_rn(d1, d1, acc[2]);
        acc[3] = __fma_rn(d0, db, acc[3]);
        acc[4] = __fma_rn(d1, db, acc[4]);
    };
#pragma unroll
    for (int u = 0; u < U; ++u) accum(e[u], t0 + u * tstep < n);
    for (int t = t0 + U * tstep; t < n; t += tstep) accum(eb[t], true);   // images larger than U * tstep
    PVR_STAMP(2);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double sr = row_sum_d(acc[k]);
        if ((lane_id() & 15) == 0) sacc[threadIdx.x / 16][k] = sr;
    }
    __syncthreads();
    PVR_STAMP(3);
    // ---- publish: this block's partial, the data as its own flag ----
    const __amdgpu_buffer_rsrc_t sr = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(slot + (int64_t)b * vn * kRefineNJ * kRefineGran), (short)0, 0x7fffffff, 0x00020000);
    static_assert(kRefineNJ <= 32, "gather: one pending bit per partial");
    if (threadIdx.x < kRefineGran) {
        const int k = threadIdx.x;
        uint64_t bits;
        if (k < 5) {
            double sk = sacc[0][k];
#pragma unroll
            for (int q = 1; q < kRT / 16; ++q) sk += sacc[q][k];
            bits = __builtin_bit_cast(uint64_t, sk);
        } else {
            bits = ((uint64_t)(uint32_t)(n > 0 ? win : 0) << 32) | __float_as_uint(ratio);
        }
        typedef int v4i __attribute__((ext_vector_type(4)));
        const v4i g = {(int)(uint32_t)bits, (int)kRefineTag, (int)(uint32_t)(bits >> 32), (int)kRefineTag};
        __builtin_amdgcn_raw_buffer_store_b128(g, sr, ((v * kRefineNJ + j) * kRefineGran + k) * 16, 0, 16);   // sc1
    }
    if (j == 0 && threadIdx.x == 0) {
        if (diag.win_ratio) diag.win_ratio[b * vn + v] = n > 0 ? ratio : 0.f;
        if (diag.win_idx) diag.win_idx[b * vn + v] = n > 0 ? win : 0;
    }
    PVR_STAMP(4);
    // the image's highest block gathers: dispatched last (in practice: only
    // speed depends on it), it mostly finds every partial already there
    if (j != kRefineNJ - 1 || v != vn - 1) return;
    // ---- gather.  Thread p polls value k of keypoint vv in a quarter of the
    // kRefineNJ partials (its loads in flight together); sums in partial
    // order, quarters then in order: deterministic ----
    constexpr int kGQ = kRefineNJ >= 4 ? 4 : kRefineNJ, kGJ = kRefineNJ / kGQ;
    __shared__ double sks[64][5];
    __shared__ double sq[64 * kRefineGran * kGQ];
    __shared__ float srat[64];
    __shared__ int sflag;   // bit 0: some matrix singular, bit 1: gather gave up
    if (threadIdx.x == 0) sflag = 0;
    __syncthreads();
    bool gave_up = false;
    for (int p = threadIdx.x; p < vn * kRefineGran * kGQ; p += kRT) {
        const int vk = p / kGQ, jq = p - vk * kGQ;
        const int vv = vk / kRefineGran, k = vk - vv * kRefineGran;
        const int base = (vv * kRefineNJ + jq * kGJ) * kRefineGran + k;
        uint64_t val[kGJ];
        uint32_t pend = (1u << kGJ) - 1;
        for (uint32_t spins = 0; pend; ++spins) {
            typedef int v4i __attribute__((ext_vector_type(4)));
            v4i g[kGJ];
#pragma unroll
            for (int jj = 0; jj < kGJ; ++jj)
                if (pend >> jj & 1) g[jj] = __builtin_amdgcn_raw_buffer_load_b128(sr, (base + jj * kRefineGran) * 16, 0, 16);
#pragma unroll
            for (int jj = 0; jj < kGJ; ++jj)
                if ((pend >> jj & 1) && (uint32_t)g[jj].y == kRefineTag && (uint32_t)g[jj].w == kRefineTag) {
                    val[jj] = ((uint64_t)(uint32_t)g[jj].z << 32) | (uint32_t)g[jj].x;
                    pend &= ~(1u << jj);
                }
            if (pend && spins >= kRefineSpinMax) { gave_up = true; break; }
            if (pend) __builtin_amdgcn_s_sleep(2);
        }
        if (gave_up) break;
        if (k < 5) {
            double sum = __builtin_bit_cast(double, val[0]);
#pragma unroll
            for (int jj = 1; jj < kGJ; ++jj) sum += __builtin_bit_cast(double, val[jj]);
            sq[p] = sum;
        } else if (jq == 0) {
            srat[vv] = __uint_as_float((uint32_t)val[0]);   // every block of a keypoint finds the same winner
        }
    }
    if (gave_up) sflag = 2;   // benign race: every writer stores 2
    __syncthreads();
    for (int q = threadIdx.x; q < vn * 5; q += kRT) {
        const int vv = q / 5, k = q - vv * 5;
        const double *sp = &sq[(vv * kRefineGran + k) * kGQ];
        double sum = sp[0];
#pragma unroll
        for (int jq = 1; jq < kGQ; ++jq) sum += sp[jq];
        sks[vv][k] = sum;
    }
    __syncthreads();
    PVR_STAMP(5);
    // ---- solve, one thread per keypoint (vn <= 64: wave 0) ----
    const int vv = threadIdx.x;
    const bool act = vv < vn;
    float A00 = 0, A01 = 0, A11 = 0, B0 = 0, B1 = 0, rat = 3.0e38f;
    float inv[4] = {1.f, 0.f, 0.f, 1.f};
    if (act) {
        A00 = (float)sks[vv][0]; A01 = (float)sks[vv][1]; A11 = (float)sks[vv][2];
        B0 = (float)sks[vv][3]; B1 = (float)sks[vv][4];
        rat = srat[vv];
        if (!lu2_inv(A00, A01, A01, A11, inv)) atomicOr(&sflag, 1);
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int flag = sflag;
    if (flag & 1) { inv[0] = 1.f; inv[1] = 0.f; inv[2] = 0.f; inv[3] = 1.f; }   // RV:514-517
    if (act) {
        float x = inv[0] * B0 + inv[1] * B1;
        float y = inv[2] * B0 + inv[3] * B1;
        if (n == 0) { x = 0.f; y = 0.f; }
        if (flag & 2) { x = __int_as_float(0x7fc00000); y = x; }   // gather gave up: loud
        out[((int64_t)b * vn + vv) * 2] = x;
        out[((int64_t)b * vn + vv) * 2 + 1] = y;
        if (diag.ata) {
            float *q = diag.ata + ((int64_t)b * vn + vv) * 4;
            q[0] = A00; q[1] = A01; q[2] = A01; q[3] = A11;
        }
        if (diag.atb) { diag.atb[((int64_t)b * vn + vv) * 2] = B0; diag.atb[((int64_t)b * vn + vv) * 2 + 1] = B1; }
    }
    if (diag.tn && vv == 0) diag.tn[b] = n;
    if (diag.iters) {
        // min ratio over keypoints -> iterations the reference's `while True` would run
        float r = rat;
        for (int o = 32; o > 0; o >>= 1) r = fminf(r, __shfl_xor(r, o));
        if (vv == 0) {
            int it = 0;
            if (n > 0) {
                long long hyp_num = 0;
                while (true) {
                    hyp_num += nh;
                    ++it;
                    float val = 1.f - powf(1.f - r * r, (float)hyp_num);
                    if (val > confidence || it > max_iter) break;
                }
            }
            diag.iters[b] = it;
        }
    }
    PVR_STAMP(6);
}

// ==========================================================================
// v5 confidence (RV:856-858): the inlier ratio of each refined keypoint at
// a second threshold (0.999), counted over the image's compacted pixels.
// ==========================================================================
__global__ __launch_bounds__(256) void k_point_conf(const float *pts, const float4 *pex, const int32_t *tn, int64_t P,
                                                    int vn, float thr, int32_t *confc, float *conf) {
    const int j = blockIdx.x, v = blockIdx.y, b = blockIdx.z;
    const int n = min(max(tn[b], 0), (int)P);   // clamped like tn_at: loads stay inside the P records
    __shared__ int sh[8];
    const float px = pts[((int64_t)b * vn + v) * 2], py = pts[((int64_t)b * vn + v) * 2 + 1];
    const float4 *eb = pex + ((int64_t)b * vn + v) * P;
    int c = 0;
    for (int t = j * 256 + threadIdx.x; t < n; t += kRefineNJ * 256) {
        const float4 e = eb[t];   // (cx, cy, nx, ny)
        c += exact_vote(e.z, e.w, e.x, e.y, px, py, thr) ? 1 : 0;
    }
    c = block_sum2(c, 0, sh).x;
    if (threadIdx.x == 0) {
        int32_t *cc = confc + ((int64_t)b * vn + v) * 2;
        if (c) atomicAdd(&cc[0], c);
        __threadfence();
        const int t = __hip_atomic_fetch_add(&cc[1], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == kRefineNJ - 1) {
            const int total = ld_agent(&cc[0]);
            conf[(int64_t)b * vn + v] = n > 0 ? (float)total / (float)n : 0.f;   // RV:858 float division
        }
    }
}

}  // namespace

namespace pvv __attribute__((visibility("hidden"))) {

void launch_refine(const Workspace &w, bool hypv, int b, int vn, int nh, int64_t P, const pv_vote_params *prm,
                   float *out, const pv_v3_diag &dg, hipStream_t s) {
    // hypotheses keypoint-major when the pipeline pre-generated them (coalesced), else the reference layout
    auto *kref = nh > kRefineLdsHyp ? k_refine_solve<true> : k_refine_solve<false>;
    kref<<<dim3(kRefineNJ, vn, b), kRT, 0, s>>>(w.counts, hypv ? w.hypv : w.hyp, (int64_t)nh * vn, hypv ? nh : 1,
                                                hypv ? 1 : vn, w.pex, w.tn, P, vn, nh, prm->inlier_thresh, w.refslot,
                                                prm->confidence, prm->max_iter, out, dg);
}

void launch_point_conf(const Workspace &w, const float *pts, int b, int vn, int64_t P, float thr, float *conf,
                       hipStream_t s) {
    k_point_conf<<<dim3(kRefineNJ, vn, b), 256, 0, s>>>(pts, w.pex, w.tn, P, vn, thr, w.confc, conf);
}

}  // namespace pvv

#ifdef PVV_TRACE
// trace builds only: per-block phase stamps of the next k_refine_solve launches
extern "C" int pv_debug_set_refine_trace(uint64_t *buf) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_refine_trace), &buf, sizeof(buf));
}
#endif
