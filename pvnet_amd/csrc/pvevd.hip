// pvevd.hip -- the two stages that reduce over all hypotheses or all pixels
// instead of refining a winner: the voting distribution's mean / covariance
// (k_evd_with_mean, k_evd_topk, after the pipeline's vote) and
// ransac_motion_voting (k_motion_vote, a pipeline of its own).  Host entries:
// pvv::launch_evd_with_mean / launch_evd_topk / launch_motion (pv_stages.h).
#include "pv_stages.h"

namespace {
using namespace pvv;

// ==========================================================================
// ransac_motion_voting (RV:966-987): per image and keypoint, the mean over
// the foreground (mask.byte() != 0) of vertex + (col, row) -- the vertex
// field holds offsets here.  fp64 sums (torch.mean's fp32 order is
// unspecified), block-local in LDS, then one device-scope add per block; the
// last block of each image divides.  Empty foreground -> zeros (RV:977-979).
// ==========================================================================
template <int KIND>
__global__ __launch_bounds__(256) void k_motion_vote(MaskView m, VertexView vx, int H, int W, int vn, double *acc,
                                                     int32_t *cnt, int32_t *ticket, float *out) {
    const int b = blockIdx.y, nblk = gridDim.x;
    __shared__ double sacc[64 * 2];
    __shared__ int scnt;
    for (int i = threadIdx.x; i < vn * 2; i += 256) sacc[i] = 0.0;
    if (threadIdx.x == 0) scnt = 0;
    __syncthreads();
    const uint32_t p = (uint32_t)blockIdx.x * 256 + threadIdx.x;
    if (p < (uint32_t)H * W) {
        const int r = (int)(p / (uint32_t)W), c = (int)(p - (uint32_t)r * W);
        if (is_fg<KIND, false>(m, b, r, c)) {
            atomicAdd(&scnt, 1);
            const int64_t vo = b * vx.s[0] + r * vx.s[1] + c * vx.s[2];
            for (int v = 0; v < vn; ++v) {
                float dx, dy;
                if (vx.kind == PV_VERTEX_F32) {
                    dx = ((const float *)vx.p)[vo + v * vx.s[3]];
                    dy = ((const float *)vx.p)[vo + v * vx.s[3] + vx.s[4]];
                } else {
                    dx = __half2float(((const __half *)vx.p)[vo + v * vx.s[3]]);
                    dy = __half2float(((const __half *)vx.p)[vo + v * vx.s[3] + vx.s[4]]);
                }
                atomicAdd(&sacc[v * 2], (double)(dx + (float)c));       // RV:983 vertex + coords (fp32 add)
                atomicAdd(&sacc[v * 2 + 1], (double)(dy + (float)r));
            }
        }
    }
    __syncthreads();
    if (scnt) {
        for (int i = threadIdx.x; i < vn * 2; i += 256) atomicAdd(&acc[(int64_t)b * vn * 2 + i], sacc[i]);
        if (threadIdx.x == 0) atomicAdd(&cnt[b], scnt);
    }
    __syncthreads();
    __shared__ int slast;
    if (threadIdx.x == 0) {
        __threadfence();
        slast = __hip_atomic_fetch_add(&ticket[b], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nblk - 1;
    }
    __syncthreads();
    if (!slast) return;
    const int n = ld_agent(&cnt[b]);
    for (int i = threadIdx.x; i < vn * 2; i += 256)
        out[(int64_t)b * vn * 2 + i] = n > 0 ? (float)(ld_agent(&acc[(int64_t)b * vn * 2 + i]) / n) : 0.f;
}

template <int KIND, bool EVD>
struct MotionStage {
    static int run(const MaskView *m, const VertexView *vx, int b, int H, int W, int vn, double *acc, int32_t *cnt,
                   int32_t *ticket, float *out, hipStream_t s) {
        dim3 grid((unsigned)(((int64_t)H * W + 255) / 256), (unsigned)b);
        k_motion_vote<KIND><<<grid, 256, 0, s>>>(*m, *vx, H, W, vn, acc, cnt, ticket, out);
        return PV_OK;
    }
};

// ==========================================================================
// EVD (RV:333-406, RV:263-331): per (image, keypoint) over all hypotheses.
// ==========================================================================
__global__ __launch_bounds__(256) void k_evd_with_mean(const int32_t *counts, const float2 *hyp, const int32_t *fg,
                                                       const int32_t *tn, int vn, int nh, int min_num,
                                                       int min_hyp_num, const float *mean, float *cov) {
    const int v = blockIdx.x, b = blockIdx.y;
    const int fgb = fg[b];
    const float mx = mean[(b * vn + v) * 2], my = mean[(b * vn + v) * 2 + 1];
    __shared__ double sacc[4][4];
    __shared__ float smax[4];
    float *cv = cov + ((int64_t)b * vn + v) * 4;
    if (fgb < min_num) {
        // RV:343-348: min_hyp_num zero hypotheses with ratio 1 (all kept by the max-0.1 rule)
        if (threadIdx.x == 0) {
            double dx = (double)(0.f - mx), dy = (double)(0.f - my);
            double w = (double)min_hyp_num;
            float den = (float)w + 1e-3f;
            cv[0] = (float)(w * dx * dx) / den;
            cv[1] = (float)(w * dx * dy) / den;
            cv[2] = (float)(w * dy * dx) / den;
            cv[3] = (float)(w * dy * dy) / den;
        }
        return;
    }
    const float fgf = (float)tn[b];   // RV:355 foreground re-counted after downsampling == tn
    const int32_t *cnt = counts + ((int64_t)b * vn + v) * nh;
    float m = -1.f;
    for (int h = threadIdx.x; h < nh; h += 256) m = fmaxf(m, (float)cnt[h] / fgf);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane_id() == 0) smax[threadIdx.x / 64] = m;
    __syncthreads();
    m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    const float thresh = m - 0.1f;                                   // RV:394
    double a[4] = {0, 0, 0, 0};
    for (int h = threadIdx.x; h < nh; h += 256) {
        float w = (float)cnt[h] / fgf;
        if (w < thresh) w = 0.f;                                     // RV:395
        float2 q = hyp[((int64_t)b * nh + h) * vn + v];
        float dx = q.x - mx, dy = q.y - my;                          // RV:398
        float wx = dx * w, wy = dy * w;                              // RV:399
        a[0] += (double)dx * wx;
        a[1] += (double)dx * wy;
        a[2] += (double)dy * wy;
        a[3] += (double)w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double s = wave_sum_d(a[k]);
        if (lane_id() == 0) sacc[threadIdx.x / 64][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s[4];
        for (int k = 0; k < 4; ++k) s[k] = sacc[0][k] + sacc[1][k] + sacc[2][k] + sacc[3][k];
        float den = (float)s[3] + 1e-3f;                             // RV:401
        cv[0] = (float)s[0] / den;
        cv[1] = (float)s[1] / den;
        cv[2] = (float)s[1] / den;
        cv[3] = (float)s[2] / den;
    }
}

// RV:320-329: top-k (ties: lowest index first) then weighted mean / covariance.
__global__ __launch_bounds__(256) void k_evd_topk(const int32_t *counts, const float2 *hyp, const int32_t *fg,
                                                  const int32_t *tn, int vn, int nh, int min_num, int topk,
                                                  float *mean, float *cov) {
    const int v = blockIdx.x, b = blockIdx.y;
    const int fgb = fg[b];
    float *mo = mean + ((int64_t)b * vn + v) * 2;
    float *cv = cov + ((int64_t)b * vn + v) * 4;
    if (fgb < min_num) {   // RV:276-281: zero hypotheses -> mean 0, cov 0
        if (threadIdx.x == 0) { mo[0] = 0.f; mo[1] = 0.f; cv[0] = cv[1] = cv[2] = cv[3] = 0.f; }
        return;
    }
    const float fgf = (float)tn[b];
    const int32_t *cnt = counts + ((int64_t)b * vn + v) * nh;
    __shared__ int sred[4];
    __shared__ double sacc[4][6];
    auto block_sum = [&](int x) {
        x = wave_sum_i(x);
        __syncthreads();
        if (lane_id() == 0) sred[threadIdx.x / 64] = x;
        __syncthreads();
        return sred[0] + sred[1] + sred[2] + sred[3];
    };
    // k-th largest count T: largest T with #{count >= T} >= k (binary search on the value)
    int k = min(topk, nh);
    int lo = 0, hi = 0;
    for (int h = threadIdx.x; h < nh; h += 256) hi = max(hi, cnt[h]);
    for (int o = 32; o > 0; o >>= 1) hi = max(hi, __shfl_xor(hi, o));
    __syncthreads();
    if (lane_id() == 0) sred[threadIdx.x / 64] = hi;
    __syncthreads();
    hi = max(max(sred[0], sred[1]), max(sred[2], sred[3]));
    while (lo < hi) {   // invariant: #{>= lo} >= k
        int mid = (lo + hi + 1) / 2;
        int c = 0;
        for (int h = threadIdx.x; h < nh; h += 256) c += cnt[h] >= mid;
        c = block_sum(c);
        if (c >= k) lo = mid; else hi = mid - 1;
    }
    const int T = lo;
    int ngt = 0;
    for (int h = threadIdx.x; h < nh; h += 256) ngt += cnt[h] > T;
    ngt = block_sum(ngt);
    const int need_eq = k - ngt;   // take the first `need_eq` hypotheses with count == T (index order)
    double a[6] = {0, 0, 0, 0, 0, 0};
    // pass 1: weights, weighted sums of x, y (mean, RV:323-324)
    int eq_base = 0;
    for (int h0 = 0; h0 < nh; h0 += 256) {
        int h = h0 + threadIdx.x;
        int c = h < nh ? cnt[h] : -1;
        bool eq = c == T;
        // exclusive prefix of eq inside this 256-slab
        uint64_t bal = ballot(eq);
        int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
        __syncthreads();
        if (lane_id() == 0) sred[threadIdx.x / 64] = __popcll(bal);
        __syncthreads();
        int woff = 0;
        for (int q = 0; q < (int)(threadIdx.x / 64); ++q) woff += sred[q];
        int slab = sred[0] + sred[1] + sred[2] + sred[3];
        bool sel = (c > T) || (eq && eq_base + woff + below < need_eq);
        if (h < nh && sel) {
            float w = (float)c / fgf;
            float2 q = hyp[((int64_t)b * nh + h) * vn + v];
            a[0] += (double)w;
            a[1] += (double)(w * q.x);
            a[2] += (double)(w * q.y);
        }
        eq_base += slab;
    }
    for (int kk = 0; kk < 3; ++kk) {
        double s = wave_sum_d(a[kk]);
        if (lane_id() == 0) sacc[threadIdx.x / 64][kk] = s;
    }
    __syncthreads();
    double W = sacc[0][0] + sacc[1][0] + sacc[2][0] + sacc[3][0];
    double SX = sacc[0][1] + sacc[1][1] + sacc[2][1] + sacc[3][1];
    double SY = sacc[0][2] + sacc[1][2] + sacc[2][2] + sacc[3][2];
    const float wsum = (float)W;
    const float mx = (float)SX / wsum, my = (float)SY / wsum;
    // pass 2: covariance about the mean (RV:326-329), every hypothesis, zero weight if not selected
    eq_base = 0;
    double c3[3] = {0, 0, 0};
    for (int h0 = 0; h0 < nh; h0 += 256) {
        int h = h0 + threadIdx.x;
        int c = h < nh ? cnt[h] : -1;
        bool eq = c == T;
        uint64_t bal = ballot(eq);
        int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
        __syncthreads();
        if (lane_id() == 0) sred[threadIdx.x / 64] = __popcll(bal);
        __syncthreads();
        int woff = 0;
        for (int q = 0; q < (int)(threadIdx.x / 64); ++q) woff += sred[q];
        int slab = sred[0] + sred[1] + sred[2] + sred[3];
        bool sel = (c > T) || (eq && eq_base + woff + below < need_eq);
        if (h < nh && sel) {
            float w = (float)c / fgf;
            float2 q = hyp[((int64_t)b * nh + h) * vn + v];
            float dx = q.x - mx, dy = q.y - my;
            c3[0] += (double)dx * (dx * w);
            c3[1] += (double)dx * (dy * w);
            c3[2] += (double)dy * (dy * w);
        }
        eq_base += slab;
    }
    __syncthreads();
    for (int kk = 0; kk < 3; ++kk) {
        double s = wave_sum_d(c3[kk]);
        if (lane_id() == 0) sacc[threadIdx.x / 64][3 + kk] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = sacc[0][3] + sacc[1][3] + sacc[2][3] + sacc[3][3];
        double s1 = sacc[0][4] + sacc[1][4] + sacc[2][4] + sacc[3][4];
        double s2 = sacc[0][5] + sacc[1][5] + sacc[2][5] + sacc[3][5];
        mo[0] = mx; mo[1] = my;
        cv[0] = (float)s0 / wsum;
        cv[1] = (float)s1 / wsum;
        cv[2] = (float)s1 / wsum;
        cv[3] = (float)s2 / wsum;
    }
}

}  // namespace

namespace pvv __attribute__((visibility("hidden"))) {

void launch_evd_with_mean(const Workspace &w, int b, int vn, int nh, int min_num, int min_hyp_num,
                          const float *mean, float *cov, hipStream_t s) {
    k_evd_with_mean<<<dim3(vn, b), 256, 0, s>>>(w.counts, w.hyp, w.fgtot, w.tn, vn, nh, min_num, min_hyp_num, mean,
                                                cov);
}

void launch_evd_topk(const Workspace &w, int b, int vn, int nh, int min_num, int topk, float *mean, float *cov,
                     hipStream_t s) {
    k_evd_topk<<<dim3(vn, b), 256, 0, s>>>(w.counts, w.hyp, w.fgtot, w.tn, vn, nh, min_num, topk, mean, cov);
}

int launch_motion(int mask_kind, const MaskView &m, const VertexView &vx, int b, int H, int W, int vn, double *acc,
                  int32_t *cnt, int32_t *ticket, float *out, hipStream_t s) {
    return dispatch_mask<MotionStage>(mask_kind, false, &m, &vx, b, H, W, vn, acc, cnt, ticket, out, s);
}

}  // namespace pvv
