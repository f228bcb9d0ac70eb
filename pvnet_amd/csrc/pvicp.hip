// pvicp.hip -- libpvicp.so (include/pvicp.h): one Gauss-Newton step of a projective point-to-plane
// ICP for a batch of poses, from each pose's rendered depth map and the sensor's.  One translation
// unit that includes no other file of csrc/.
//
// Everything is fp64 VALU with every operation rounded (-ffp-contract=off; no fused multiply-add, no
// MFMA: the definition rounds after each product and each sum), so tests/icp_ref.py's
// numpy float64 restatement reproduces every bit.
//
// k_linearise: block (pose, kPix consecutive pixels), a lane a run of kRun pixels.  A pixel whose
// rendered depth is not a surface costs one load; the stencil, the eight divides and the 28 products
// are paid only where the object is, and a wave none of whose lanes used a pixel skips the reduction
// too (its sums are +0 either way).  The 28 sums go through the header's tree: shuffles within a
// wave, LDS across the four, one partial row per block to the workspace.  No atomics.
// k_solve: one wave per pose.  Lane q adds sum q's partials in increasing block order; lane 0 then
// damps, factors, solves, limits and applies the step.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pvicp.h"

namespace {

constexpr int kThreads = PV_ICP_LANES;    // 4 waves per block
constexpr int kWaves = kThreads / 64;
constexpr int kRun = PV_ICP_RUN;          // consecutive pixels per lane
constexpr int kPix = kThreads * kRun;     // pixels per block
constexpr int kSum = PV_ICP_NSUM;
static_assert(kPix == PV_ICP_BLOCK && kThreads == 256 && kSum == 28, "the header's rule 4");

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
inline int last() { return rc(hipGetLastError()); }
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline int64_t chunks(int64_t n, int64_t per) { return (n + per - 1) / per; }

struct Args {
    const float *depth_test, *depth_est;
    const int32_t *img_id;
    const double *K;
    double *pose, *stats, *neq;
    int32_t *status, *iters, *cnt;
    double *part;           // [b][nblk][28]
    int32_t *pcnt;          // [b][nblk]
    int64_t K_stride, npix;
    double dist_max, edge_max, lambda, max_rot, max_trans, eps_rot, eps_trans;
    int32_t b, n_img, H, W, min_count, nblk;
};

__device__ __forceinline__ bool depth_ok(float z) { return z > 0.f && z < __builtin_inff(); }

__global__ __launch_bounds__(kThreads) void k_linearise(Args a) {
    __shared__ double wsum[kWaves][kSum];
    __shared__ int wcnt[kWaves];
    const int i = blockIdx.x / a.nblk, blk = blockIdx.x - i * a.nblk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (a.status[i] == PV_ICP_CONVERGED) return;
    const int img = a.img_id ? a.img_id[i] : i;
    if (img < 0 || img >= a.n_img) return;                             // k_solve reads no partial of this pose
    const double *K = a.K + (int64_t)i * a.K_stride;
    const double fx = K[0], sk = K[1], cx = K[2], fy = K[4], cy = K[5];
    const float *ze_ = a.depth_est + (int64_t)i * a.npix;
    const float *zt_ = a.depth_test + (int64_t)img * a.npix;
    const int W = a.W, H = a.H;

    double S[kSum];
#pragma unroll
    for (int q = 0; q < kSum; ++q) S[q] = 0.0;
    int n_used = 0;

    const int64_t p0 = (int64_t)blk * kPix + (int64_t)tid * kRun;
    int64_t x, y;
    if (a.npix <= INT32_MAX) {
        y = (uint32_t)p0 / (uint32_t)W;
        x = (uint32_t)p0 - (uint32_t)y * (uint32_t)W;
    } else {
        y = p0 / W;
        x = p0 - y * W;
    }
    for (int j = 0; j < kRun; ++j, ++x) {
        if (x >= W) {                                                  // W may be below kRun: more than one wrap
            y += x / W;
            x = x % W;
        }
        const int64_t p = p0 + j;
        if (p >= a.npix) break;
        if (x < 1 || x > W - 2 || y < 1 || y > H - 2) continue;
        const float zef = ze_[p];
        if (!depth_ok(zef)) continue;
        const float zlf = ze_[p - 1], zrf = ze_[p + 1], zuf = ze_[p - W], zdf = ze_[p + W], ztf = zt_[p];
        if (!(depth_ok(zlf) && depth_ok(zrf) && depth_ok(zuf) && depth_ok(zdf) && depth_ok(ztf))) continue;
        const double ze = zef, zl = zlf, zr = zrf, zu = zuf, zd = zdf, zt = ztf;
        if (!(fabs(zl - ze) <= a.edge_max && fabs(zr - ze) <= a.edge_max && fabs(zu - ze) <= a.edge_max &&
              fabs(zd - ze) <= a.edge_max))
            continue;
        const double xc = (double)x - cx, xl = (double)(x - 1) - cx, xr = (double)(x + 1) - cx;
        const double ay = ((double)y - cy) / fy, ayu = ((double)(y - 1) - cy) / fy, ayd = ((double)(y + 1) - cy) / fy;
        const double ax = (xc - sk * ay) / fx, axl = (xl - sk * ay) / fx, axr = (xr - sk * ay) / fx;
        const double axu = (xc - sk * ayu) / fx, axd = (xc - sk * ayd) / fx;
        const double P0 = ze * ax, P1 = ze * ay, P2 = ze;
        const double du0 = zr * axr - zl * axl, du1 = zr * ay - zl * ay, du2 = zr - zl;
        const double dv0 = zd * axd - zu * axu, dv1 = zd * ayd - zu * ayu, dv2 = zd - zu;
        const double m0 = du1 * dv2 - du2 * dv1, m1 = du2 * dv0 - du0 * dv2, m2 = du0 * dv1 - du1 * dv0;
        const double l2 = (m0 * m0 + m1 * m1) + m2 * m2;
        if (!(l2 > 0.0 && l2 < __builtin_inf())) continue;
        const double d0 = P0 - zt * ax, d1 = P1 - zt * ay, d2 = P2 - zt;
        if (!((d0 * d0 + d1 * d1) + d2 * d2 <= a.dist_max * a.dist_max)) continue;
        const double r = sqrt(l2);
        double J[6];
        J[3] = m0 / r; J[4] = m1 / r; J[5] = m2 / r;
        const double e = (J[3] * d0 + J[4] * d1) + J[5] * d2;
        J[0] = P1 * J[5] - P2 * J[4];
        J[1] = P2 * J[3] - P0 * J[5];
        J[2] = P0 * J[4] - P1 * J[3];
        int q = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int l = k; l < 6; ++l) {
                S[q] = S[q] + J[k] * J[l];
                ++q;
            }
#pragma unroll
        for (int k = 0; k < 6; ++k) S[21 + k] = S[21 + k] + J[k] * e;
        S[27] = S[27] + e * e;
        ++n_used;
    }

    // the header's tree; a wave that used no pixel holds +0 in every lane, and so does its sum.  A lane
    // with t + o past the wave gets its own value back from the shuffle; the header's tree never reads
    // such a lane again, and lane 0 is all that is kept.
    const bool any = __any(n_used != 0);
    if (any) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
            for (int q = 0; q < kSum; ++q) S[q] = S[q] + __shfl_down(S[q], o, 64);
            n_used += __shfl_down(n_used, o, 64);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kSum; ++q) wsum[wave][q] = any ? S[q] : 0.0;
        wcnt[wave] = any ? n_used : 0;
    }
    __syncthreads();
    const int64_t row = (int64_t)i * a.nblk + blk;
    if (tid < kSum) a.part[row * kSum + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
    if (tid == kSum) a.pcnt[row] = ((wcnt[0] + wcnt[1]) + wcnt[2]) + wcnt[3];
}

__global__ __launch_bounds__(64) void k_solve(Args a) {
    __shared__ double sums[kSum];
    __shared__ int bad_s;
    const int i = blockIdx.x, lane = threadIdx.x;
    if (a.status[i] == PV_ICP_CONVERGED) return;
    const double nan = __builtin_nan("");
    double *pose = a.pose + (int64_t)i * 12;
    double *stats = a.stats + (int64_t)i * PV_ICP_NSTAT;
    double *neq = a.neq ? a.neq + (int64_t)i * kSum : nullptr;

    if (lane == 0) {
        const double *K = a.K + (int64_t)i * a.K_stride;
        const int img = a.img_id ? a.img_id[i] : i;
        bool ok = img >= 0 && img < a.n_img;
        for (int e = 0; e < 12; ++e) ok = ok && isfinite(pose[e]);
        ok = ok && isfinite(K[0]) && isfinite(K[1]) && isfinite(K[2]) && isfinite(K[4]) && isfinite(K[5]);
        ok = ok && K[0] != 0.0 && K[4] != 0.0;
        bad_s = !ok;
    }
    __syncthreads();
    if (bad_s) {
        if (lane < kSum && neq) neq[lane] = nan;
        if (lane < PV_ICP_NSTAT) stats[lane] = nan;
        if (lane == 0) {
            a.status[i] = PV_ICP_BAD_INPUT;
            a.cnt[i] = 0;
        }
        return;
    }
    const int64_t row = (int64_t)i * a.nblk;
    if (lane < kSum) {
        double s = 0.0;
        for (int k = 0; k < a.nblk; ++k) s = s + a.part[(row + k) * kSum + lane];
        sums[lane] = s;
        if (neq) neq[lane] = s;
    }
    __syncthreads();
    if (lane != 0) return;
    int cnt = 0;
    for (int k = 0; k < a.nblk; ++k) cnt += a.pcnt[row + k];
    a.cnt[i] = cnt;
    const double rms = cnt > 0 ? sqrt(sums[27] / (double)cnt) : nan;
    stats[PV_ICP_STAT_RMS] = rms;
    if (cnt < a.min_count) {
        a.status[i] = PV_ICP_FEW;
        stats[PV_ICP_STAT_ROT] = stats[PV_ICP_STAT_TRANS] = nan;
        return;
    }
    double M[6][6], L[6][6], g[6], z[6], yv[6];
    {
        int q = 0;
        for (int k = 0; k < 6; ++k)
            for (int l = k; l < 6; ++l) {
                M[k][l] = M[l][k] = sums[q];
                ++q;
            }
        for (int k = 0; k < 6; ++k) {
            M[k][k] = M[k][k] + a.lambda * M[k][k];
            g[k] = sums[21 + k];
        }
    }
    // straight-line (every loop unrolls, so L stays in registers): after a bad pivot the rest is
    // computed on NaN and thrown away
    bool pd = true;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            double s = M[r][c];
#pragma unroll
            for (int k = 0; k < c; ++k) s = s - L[r][k] * L[c][k];
            if (r == c) {
                pd = pd && s > 0.0 && s < __builtin_inf();
                L[r][r] = sqrt(s);
            } else {
                L[r][c] = s / L[c][c];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = g[r];
#pragma unroll
        for (int k = 0; k < r; ++k) s = s - L[r][k] * z[k];
        z[r] = s / L[r][r];
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = z[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s = s - L[k][r] * yv[k];
        yv[r] = s / L[r][r];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) pd = pd && isfinite(yv[r]);
    if (!pd) {
        a.status[i] = PV_ICP_NOT_PD;
        stats[PV_ICP_STAT_ROT] = stats[PV_ICP_STAT_TRANS] = nan;
        return;
    }
    const double w0 = -yv[0], w1 = -yv[1], w2 = -yv[2], v0 = -yv[3], v1 = -yv[4], v2 = -yv[5];
    const double rn = sqrt((w0 * w0 + w1 * w1) + w2 * w2), tn = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    double k = 1.0;
    if (rn > a.max_rot) k = a.max_rot / rn;
    if (tn > a.max_trans) {
        const double kt = a.max_trans / tn;
        if (kt < k) k = kt;
    }
    const double a0 = (k * w0) * 0.5, a1 = (k * w1) * 0.5, a2 = (k * w2) * 0.5;
    const double qq = (a0 * a0 + a1 * a1) + a2 * a2, den = 1.0 + qq, om = 1.0 - qq;
    const double b0 = 2.0 * a0, b1 = 2.0 * a1, b2 = 2.0 * a2;
    double C[3][3];
    C[0][0] = (om + b0 * a0) / den; C[0][1] = (b0 * a1 - b2) / den; C[0][2] = (b0 * a2 + b1) / den;
    C[1][0] = (b1 * a0 + b2) / den; C[1][1] = (om + b1 * a1) / den; C[1][2] = (b1 * a2 - b0) / den;
    C[2][0] = (b2 * a0 - b1) / den; C[2][1] = (b2 * a1 + b0) / den; C[2][2] = (om + b2 * a2) / den;
    const double kv[3] = {k * v0, k * v1, k * v2};
    double out[12];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[r * 4 + c] = (C[r][0] * pose[c] + C[r][1] * pose[4 + c]) + C[r][2] * pose[8 + c];
        out[r * 4 + 3] = ((C[r][0] * pose[3] + C[r][1] * pose[7]) + C[r][2] * pose[11]) + kv[r];
    }
    for (int e = 0; e < 12; ++e) pose[e] = out[e];
    a.iters[i] = a.iters[i] + 1;
    stats[PV_ICP_STAT_ROT] = rn;
    stats[PV_ICP_STAT_TRANS] = tn;
    a.status[i] = (rn <= a.eps_rot && tn <= a.eps_trans) ? PV_ICP_CONVERGED : PV_ICP_RUNNING;
}

}  // namespace

extern "C" {

size_t pv_icp_workspace_size(int32_t b, int32_t H, int32_t W) {
    if (b < 1 || H < 1 || W < 1) return 0;
    const int64_t nblk = chunks((int64_t)H * W, kPix);
    return (size_t)align_up((int64_t)b * nblk * (kSum * (int64_t)sizeof(double) + (int64_t)sizeof(int32_t)), 256);
}

int pv_icp_iterate(const pv_icp_batch *bt, const pv_icp_state *st, void *workspace, size_t workspace_bytes,
                   pv_stream_t stream) {
    if (!bt || !st) return PV_EINVAL;
    if (bt->b < 0 || bt->n_img < 0 || bt->min_count < 0 || bt->K_stride < 0 || bt->H < 1 || bt->H > PV_ICP_MAX_DIM ||
        bt->W < 1 || bt->W > PV_ICP_MAX_DIM)
        return PV_EINVAL;
    if (!(bt->dist_max >= 0.0) || !(bt->edge_max >= 0.0) || !(bt->eps_rot >= 0.0) || !(bt->eps_trans >= 0.0) ||
        !(bt->lambda >= 0.0 && bt->lambda < INFINITY) || !(bt->max_rot > 0.0) || !(bt->max_trans > 0.0))
        return PV_EINVAL;
    if (bt->b == 0) return PV_OK;
    if (!st->pose || !st->status || !st->iters || !st->cnt || !st->stats || !bt->depth_est || !bt->K) return PV_EINVAL;
    if (!bt->depth_test && bt->n_img > 0) return PV_EINVAL;
    const int64_t npix = (int64_t)bt->H * bt->W, nblk = chunks(npix, kPix);
    if (nblk * bt->b > INT32_MAX) return PV_EINVAL;
    const size_t need = pv_icp_workspace_size(bt->b, bt->H, bt->W);
    if (!workspace || workspace_bytes < need) return PV_EWORKSPACE;
    if (((uintptr_t)st->pose | (uintptr_t)st->stats | (uintptr_t)st->neq | (uintptr_t)bt->K | (uintptr_t)workspace) & 7)
        return PV_EALIGN;
    if (((uintptr_t)st->status | (uintptr_t)st->iters | (uintptr_t)st->cnt | (uintptr_t)bt->img_id |
         (uintptr_t)bt->depth_test | (uintptr_t)bt->depth_est) & 3)
        return PV_EALIGN;

    Args a{};
    a.depth_test = bt->depth_test; a.depth_est = bt->depth_est; a.img_id = bt->img_id; a.K = bt->K;
    a.pose = st->pose; a.stats = st->stats; a.neq = st->neq;
    a.status = st->status; a.iters = st->iters; a.cnt = st->cnt;
    a.part = (double *)workspace;
    a.pcnt = (int32_t *)((char *)workspace + (int64_t)bt->b * nblk * kSum * (int64_t)sizeof(double));
    a.K_stride = bt->K_stride; a.npix = npix;
    a.dist_max = bt->dist_max; a.edge_max = bt->edge_max; a.lambda = bt->lambda;
    a.max_rot = bt->max_rot; a.max_trans = bt->max_trans; a.eps_rot = bt->eps_rot; a.eps_trans = bt->eps_trans;
    a.b = bt->b; a.n_img = bt->n_img; a.H = bt->H; a.W = bt->W; a.min_count = bt->min_count; a.nblk = (int32_t)nblk;
    hipStream_t s = (hipStream_t)stream;
    k_linearise<<<dim3((unsigned)(nblk * bt->b)), kThreads, 0, s>>>(a);
    const int e = last();
    if (e) return e;
    k_solve<<<bt->b, 64, 0, s>>>(a);
    return last();
}

}  // extern "C"
