// pveval.hip -- libpveval.so (include/pveval.h): nearest reference point and the fused pose
// metrics (ADD, ADD-S, 2-D projection, 5 cm 5 deg) for a batch of poses.  One translation
// unit, no symbol of libpvvote.so's; pv_common.h / pv_host.h are used for their inline helpers.
//
// Both hot loops are the same pair loop: a block of kThreads lanes holds kQPL
// queries per lane in registers and walks the references in LDS tiles of kT points, one
// LDS read (all lanes the same address: a broadcast) per reference feeding kQPL distance
// evaluations of 8 (dim 3) fp32 VALU operations plus one v_min_f32.  There is no fmaf in the
// distance: every operation rounds (-ffp-contract=off), so a float32 numpy restatement
// reproduces every decision.
#include "pv_common.h"
#include "pv_host.h"

#include "../../include/pveval.h"

using namespace pvv;

namespace {

constexpr int kThreads = 128;            // 2 waves per block
// Queries per lane: every reference read feeds 4 distances.  One query per lane for small
// models (4x the waves) was measured and is slower: the LDS reads then bound the loop
// (DESIGN 10b).  The block's size never depends on b, so a pose's result does not change
// with the batch it is scored in.
constexpr int kQPL = 4;
constexpr int kQ = kThreads * kQPL;      // queries per block
constexpr int kT = 512;                 // references per LDS tile (8 KiB as float4)
constexpr int kSub = 64;                 // references per minimum-tracking sub-tile
constexpr int kTPL = kT / kThreads;      // references each thread stages per tile
static_assert(kT % kSub == 0 && kT % kThreads == 0, "tile sizes");

// the distance of include/pveval.h, every operation rounded
template <int DIM>
__device__ __forceinline__ float dist2(float qx, float qy, float qz, float rx, float ry, float rz) {
    const float dx = qx - rx;
    const float dy = qy - ry;
    float d = dx * dx + dy * dy;
    if constexpr (DIM == 3) {
        const float dz = qz - rz;
        d = d + dz * dz;
    }
    return d;
}

// --------------------------------------------------------------------------
// pv_nearest_point_idx
// --------------------------------------------------------------------------
// Block (i, qb): image i, queries [qb * kQ, +kQ).  The per-pair work keeps no index: each
// sub-tile of kSub references keeps its minimum with v_min_f32 (which drops a NaN operand),
// one strict compare per sub-tile records the first sub-tile that lowered the running
// minimum, and the winning sub-tile is scanned once more for the first reference whose d2
// equals the minimum (recomputed from the same operands by the same operations: bit-equal).
// Strictness across sub-tiles plus the first match within one gives the lowest index.
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_nearest_idx(const float *__restrict__ ref,
                                                          const float *__restrict__ que,
                                                          int32_t *__restrict__ idx, int pn1, int pn2, int nqb) {
    __shared__ float4 tile[kT];
    const int i = blockIdx.x / nqb, qb = blockIdx.x - i * nqb;
    const int tid = threadIdx.x;
    const float *r = ref + (int64_t)i * pn1 * DIM;
    const float *q = que + (int64_t)i * pn2 * DIM;

    float qx[kQPL], qy[kQPL], qz[kQPL], best[kQPL];
    int bsub[kQPL];
#pragma unroll
    for (int k = 0; k < kQPL; ++k) {
        const int j = min(qb * kQ + k * kThreads + tid, pn2 - 1);   // a lane past the end repeats the last query
        qx[k] = q[(int64_t)j * DIM];
        qy[k] = q[(int64_t)j * DIM + 1];
        qz[k] = DIM == 3 ? q[(int64_t)j * DIM + 2] : 0.f;
        best[k] = INFINITY;
        bsub[k] = -1;
    }

    for (int t0 = 0; t0 < pn1; t0 += kT) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kTPL; ++s) {
            const int l = s * kThreads + tid, j = t0 + l;
            float4 v = make_float4(NAN, NAN, NAN, 0.f);              // padding never wins
            if (j < pn1) {
                v.x = r[(int64_t)j * DIM];
                v.y = r[(int64_t)j * DIM + 1];
                v.z = DIM == 3 ? r[(int64_t)j * DIM + 2] : 0.f;
            }
            tile[l] = v;
        }
        __syncthreads();
        const int nsub = (min(kT, pn1 - t0) + kSub - 1) / kSub;
        for (int s = 0; s < nsub; ++s) {
            float m[kQPL];
#pragma unroll
            for (int k = 0; k < kQPL; ++k) m[k] = INFINITY;
#pragma unroll 16
            for (int j = 0; j < kSub; ++j) {
                const float4 v = tile[s * kSub + j];
#pragma unroll
                for (int k = 0; k < kQPL; ++k)
                    m[k] = __builtin_fminf(m[k], dist2<DIM>(qx[k], qy[k], qz[k], v.x, v.y, v.z));
            }
#pragma unroll
            for (int k = 0; k < kQPL; ++k)
                if (m[k] < best[k]) {
                    best[k] = m[k];
                    bsub[k] = t0 + s * kSub;
                }
        }
    }

#pragma unroll
    for (int k = 0; k < kQPL; ++k) {
        const int j = qb * kQ + k * kThreads + tid;
        if (j >= pn2) continue;
        int found = 0;                                               // no reference won
        if (bsub[k] >= 0) {
            for (int c = min(bsub[k] + kSub, pn1) - 1; c >= bsub[k]; --c) {
                const float rx = r[(int64_t)c * DIM], ry = r[(int64_t)c * DIM + 1];
                const float rz = DIM == 3 ? r[(int64_t)c * DIM + 2] : 0.f;
                if (dist2<DIM>(qx[k], qy[k], qz[k], rx, ry, rz) == best[k]) found = c;
            }
        }
        idx[(int64_t)i * pn2 + j] = found;
    }
}

// --------------------------------------------------------------------------
// pv_pose_metrics
// --------------------------------------------------------------------------
struct EvalArgs {
    const double *pose_pred, *pose_gt, *K;
    const float *model;
    const int32_t *model_off, *model_id;
    double *partial;        // [b][nblk][4]: ADD, ADDS, PROJ, PROJ_SYM sums of each block
    double *out;
    int64_t K_stride;
    int32_t b, total, nmodels, max_pn, nblk;
    uint32_t metrics;
};

// pose i's model as rows [lo, lo + pn) of the table, every index checked before use;
// false: no such model (the per-point columns are NaN)
__device__ __forceinline__ bool model_rows(const EvalArgs &a, int i, int *lo, int *pn) {
    const int mid = a.model_id ? a.model_id[i] : 0;
    if (mid < 0 || mid >= a.nmodels) return false;
    const int l = a.model_off[mid], h = a.model_off[mid + 1];
    if (l < 0 || h > a.total || h <= l || h - l > a.max_pn) return false;
    *lo = l;
    *pn = h - l;
    return true;
}

struct Pose {
    double Rp[9], Rg[9], dR[9], tp[3], tg[3], dt[3], K[9];
    double cu, cv;          // projection of t_gt: the centre of the 2-D frame
};

__device__ __forceinline__ void mul3(const double *M, double x, double y, double z, double *o) {
    o[0] = M[0] * x + M[1] * y + M[2] * z;
    o[1] = M[3] * x + M[4] * y + M[5] * z;
    o[2] = M[6] * x + M[7] * y + M[8] * z;
}

// Block (i, blk): pose i, the model's points [blk * kQ, +kQ) as queries against all of its
// points as references.  SYM3 / SYM2: the ADD-S / symmetric projection pair loops.
template <bool SYM3, bool SYM2>
__global__ __launch_bounds__(kThreads) void k_pose_partial(EvalArgs a) {
    __shared__ float4 tile3[SYM3 ? kT : 1];
    __shared__ float2 tile2[SYM2 ? kT : 1];
    __shared__ double wsum[kThreads / 64][4];
    const int i = blockIdx.x / a.nblk, blk = blockIdx.x - i * a.nblk;
    const int tid = threadIdx.x;
    int lo, pn;
    if (!model_rows(a, i, &lo, &pn)) return;
    if (blk * kQ >= pn) return;                                       // past this pose's model
    const float *P = a.model + (int64_t)lo * 3;

    Pose s;
    const double *pp = a.pose_pred + (int64_t)i * 12, *pg = a.pose_gt + (int64_t)i * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s.Rp[r * 3 + c] = pp[r * 4 + c];
            s.Rg[r * 3 + c] = pg[r * 4 + c];
            s.dR[r * 3 + c] = pp[r * 4 + c] - pg[r * 4 + c];
        }
        s.tp[r] = pp[r * 4 + 3];
        s.tg[r] = pg[r * 4 + 3];
        s.dt[r] = s.tp[r] - s.tg[r];
    }
    const bool proj = (a.metrics & (PV_EVAL_PROJ | PV_EVAL_PROJ_SYM)) != 0;
    s.cu = s.cv = 0.0;
    if (proj) {
#pragma unroll
        for (int e = 0; e < 9; ++e) s.K[e] = a.K[(int64_t)i * a.K_stride + e];
        double c[3];
        mul3(s.K, s.tg[0], s.tg[1], s.tg[2], c);
        s.cu = c[0] / c[2];
        s.cv = c[1] / c[2];
    }

    float qx[kQPL], qy[kQPL], qz[kQPL], qu[kQPL], qv[kQPL], m3[kQPL], m2[kQPL];
    double sum_add = 0.0, sum_proj = 0.0;
#pragma unroll
    for (int k = 0; k < kQPL; ++k) {
        const int jq = blk * kQ + k * kThreads + tid;
        const int j = min(jq, pn - 1);
        const double x = P[(int64_t)j * 3], y = P[(int64_t)j * 3 + 1], z = P[(int64_t)j * 3 + 2];
        double g[3], d[3];
        mul3(s.Rg, x, y, z, g);                                        // ground-truth cloud, centred on t_gt
        mul3(s.dR, x, y, z, d);                                        // (R_pred - R_gt) p + (t_pred - t_gt):
        d[0] += s.dt[0]; d[1] += s.dt[1]; d[2] += s.dt[2];             // the ADD difference without cancellation
        qx[k] = (float)g[0]; qy[k] = (float)g[1]; qz[k] = (float)g[2];
        m3[k] = m2[k] = INFINITY;
        qu[k] = qv[k] = 0.f;
        if (jq < pn) sum_add += sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (proj) {
            double bg[3], kd[3];
            mul3(s.K, g[0] + s.tg[0], g[1] + s.tg[1], g[2] + s.tg[2], bg);
            mul3(s.K, d[0], d[1], d[2], kd);
            // pi(b + kd) - pi(b) = (kd_xy * b_z - b_xy * kd_z) / ((b_z + kd_z) * b_z)
            const double den = (bg[2] + kd[2]) * bg[2];
            const double du = (kd[0] * bg[2] - bg[0] * kd[2]) / den;
            const double dv = (kd[1] * bg[2] - bg[1] * kd[2]) / den;
            if (jq < pn) sum_proj += sqrt(du * du + dv * dv);
            qu[k] = (float)(bg[0] / bg[2] - s.cu);
            qv[k] = (float)(bg[1] / bg[2] - s.cv);
        }
    }

    if constexpr (SYM3 || SYM2) {
        for (int t0 = 0; t0 < pn; t0 += kT) {
            __syncthreads();
#pragma unroll
            for (int w = 0; w < kTPL; ++w) {
                const int l = w * kThreads + tid, j = t0 + l;
                float4 v3 = make_float4(NAN, NAN, NAN, 0.f);          // padding never wins
                float2 v2 = make_float2(NAN, NAN);
                if (j < pn) {
                    const double x = P[(int64_t)j * 3], y = P[(int64_t)j * 3 + 1], z = P[(int64_t)j * 3 + 2];
                    double rp[3];
                    mul3(s.Rp, x, y, z, rp);
                    if constexpr (SYM3)
                        v3 = make_float4((float)(rp[0] + s.dt[0]), (float)(rp[1] + s.dt[1]),
                                         (float)(rp[2] + s.dt[2]), 0.f);
                    if constexpr (SYM2) {
                        double c[3];
                        mul3(s.K, rp[0] + s.tp[0], rp[1] + s.tp[1], rp[2] + s.tp[2], c);
                        v2 = make_float2((float)(c[0] / c[2] - s.cu), (float)(c[1] / c[2] - s.cv));
                    }
                }
                if constexpr (SYM3) tile3[l] = v3;
                if constexpr (SYM2) tile2[l] = v2;
            }
            __syncthreads();
            const int nsub = (min(kT, pn - t0) + kSub - 1) / kSub;
            for (int sb = 0; sb < nsub; ++sb) {
#pragma unroll 16
                for (int j = 0; j < kSub; ++j) {
                    if constexpr (SYM3) {
                        const float4 v = tile3[sb * kSub + j];
#pragma unroll
                        for (int k = 0; k < kQPL; ++k)
                            m3[k] = __builtin_fminf(m3[k], dist2<3>(qx[k], qy[k], qz[k], v.x, v.y, v.z));
                    }
                    if constexpr (SYM2) {
                        const float2 v = tile2[sb * kSub + j];
#pragma unroll
                        for (int k = 0; k < kQPL; ++k)
                            m2[k] = __builtin_fminf(m2[k], dist2<2>(qu[k], qv[k], 0.f, v.x, v.y, 0.f));
                    }
                }
            }
        }
    }

    double sum_adds = 0.0, sum_psym = 0.0;
#pragma unroll
    for (int k = 0; k < kQPL; ++k) {
        if (blk * kQ + k * kThreads + tid >= pn) continue;
        if constexpr (SYM3) sum_adds += sqrt((double)m3[k]);
        if constexpr (SYM2) sum_psym += sqrt((double)m2[k]);
    }
    // lanes by the xor tree, then the waves in order: one fixed order of additions
    const double v[4] = {wave_sum_d(sum_add), wave_sum_d(sum_adds), wave_sum_d(sum_proj), wave_sum_d(sum_psym)};
    if (lane_id() == 0)
        for (int c = 0; c < 4; ++c) wsum[tid / 64][c] = v[c];
    __syncthreads();
    if (tid < 4) {
        double t = wsum[0][tid];
        for (int w = 1; w < kThreads / 64; ++w) t += wsum[w][tid];
        a.partial[((int64_t)i * a.nblk + blk) * 4 + tid] = t;
    }
}

// One thread per pose: the blocks' partial sums in block order, the means, and the two
// columns that need no model.
__global__ __launch_bounds__(64) void k_pose_finish(EvalArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.b) return;
    const double *pp = a.pose_pred + (int64_t)i * 12, *pg = a.pose_gt + (int64_t)i * 12;
    const double nan = __builtin_nan("");
    bool finite = true;
    for (int e = 0; e < 12; ++e) finite = finite && isfinite(pp[e]) && isfinite(pg[e]);
    bool kfinite = true;
    if (a.metrics & (PV_EVAL_PROJ | PV_EVAL_PROJ_SYM))
        for (int e = 0; e < 9; ++e) kfinite = kfinite && isfinite(a.K[(int64_t)i * a.K_stride + e]);

    double col[4] = {nan, nan, nan, nan};
    int lo, pn;
    if (finite && (a.metrics & 15u) && model_rows(a, i, &lo, &pn)) {
        const int nb = (pn + kQ - 1) / kQ;
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int blk = 0; blk < nb; ++blk)
            for (int c = 0; c < 4; ++c) t[c] += a.partial[((int64_t)i * a.nblk + blk) * 4 + c];
        for (int c = 0; c < 4; ++c) col[c] = t[c] / (double)pn;
        if (!kfinite) col[PV_EVAL_COL_PROJ] = col[PV_EVAL_COL_PROJ_SYM] = nan;
    }
    double *o = a.out + (int64_t)i * PV_EVAL_NCOL;
    if (a.metrics & PV_EVAL_ADD) o[PV_EVAL_COL_ADD] = col[0];
    if (a.metrics & PV_EVAL_ADDS) o[PV_EVAL_COL_ADDS] = col[1];
    if (a.metrics & PV_EVAL_PROJ) o[PV_EVAL_COL_PROJ] = col[2];
    if (a.metrics & PV_EVAL_PROJ_SYM) o[PV_EVAL_COL_PROJ_SYM] = col[3];
    if (a.metrics & PV_EVAL_CMDEG) {
        // trace(R_pred R_gt^T) as an unevaluated sum hi + lo (products exact by fma, sums by
        // two-sum): arccos is ill-conditioned at both ends of its range, and both ends matter
        // (identical poses, and the 180 deg of a symmetric object), so the rounding of a plain
        // fp64 trace would decide the angle there
        double hi = 0.0, lo = 0.0, d2 = 0.0;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) {
                const double x = pp[r * 4 + c], y = pg[r * 4 + c];
                const double p = x * y, pe = fma(x, y, -p);
                const double s = hi + p, bb = s - hi;
                lo += pe + ((hi - (s - bb)) + (p - bb));
                hi = s;
            }
            const double d = pp[r * 4 + 3] - pg[r * 4 + 3];
            d2 += d * d;
        }
        // arccos(clamp((min(tr, 3) - 1) / 2, -1, .)) by its half angle: sin^2 = (3 - tr) / 4,
        // cos^2 = (1 + tr) / 4, the two clamps being the two max(., 0)
        const double sn = fmax((3.0 - hi) - lo, 0.0), cn = fmax((1.0 + hi) + lo, 0.0);
        o[PV_EVAL_COL_TRANS_CM] = finite ? 100.0 * sqrt(d2) : nan;
        o[PV_EVAL_COL_ROT_DEG] = finite ? 2.0 * atan2(sqrt(sn), sqrt(cn)) * (180.0 / 3.14159265358979323846) : nan;
    }
}

int64_t query_blocks(int64_t n) { return (n + kQ - 1) / kQ; }

}  // namespace

extern "C" {

int pv_nearest_point_idx(const float *ref, const float *que, int32_t *idx, int32_t b, int32_t pn1, int32_t pn2,
                         int32_t dim, pv_stream_t stream) {
    if (b < 0 || pn1 < 1 || pn2 < 0 || (dim != 2 && dim != 3)) return PV_EINVAL;
    if (b == 0 || pn2 == 0) return PV_OK;
    if (!ref || !que || !idx) return PV_EINVAL;
    const int64_t nqb = query_blocks(pn2);
    if (nqb * b > INT32_MAX) return PV_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(nqb * b));
    if (dim == 3)
        k_nearest_idx<3><<<grid, kThreads, 0, st>>>(ref, que, idx, pn1, pn2, (int)nqb);
    else
        k_nearest_idx<2><<<grid, kThreads, 0, st>>>(ref, que, idx, pn1, pn2, (int)nqb);
    return last();
}

size_t pv_eval_workspace_size(int32_t b, int32_t max_pn) {
    if (b < 1 || max_pn < 0) return 0;
    return (size_t)align_up((int64_t)b * query_blocks(max_pn) * 4 * (int64_t)sizeof(double), 256);
}

int pv_pose_metrics(const pv_eval_batch *bt, double *out, void *workspace, size_t workspace_bytes,
                    pv_stream_t stream) {
    if (!bt) return PV_EINVAL;
    if (bt->b < 0 || bt->nmodels < 1 || bt->max_pn < 0 || bt->total < 0 || bt->K_stride < 0 ||
        (bt->metrics & ~PV_EVAL_ALL))
        return PV_EINVAL;
    if (bt->b == 0 || bt->metrics == 0) return PV_OK;
    const bool points = (bt->metrics & 15u) != 0;
    const bool proj = (bt->metrics & (PV_EVAL_PROJ | PV_EVAL_PROJ_SYM)) != 0;
    if (!out || !bt->pose_pred || !bt->pose_gt) return PV_EINVAL;
    if (points && (!bt->model_off || (!bt->model && bt->total > 0))) return PV_EINVAL;
    if (proj && !bt->K) return PV_EINVAL;
    const int64_t nblk = query_blocks(bt->max_pn);
    if (nblk * bt->b > INT32_MAX) return PV_EINVAL;
    const size_t need = points ? pv_eval_workspace_size(bt->b, bt->max_pn) : 0;
    if (need && (!workspace || workspace_bytes < need)) return PV_EWORKSPACE;
    if (((uintptr_t)out | (uintptr_t)workspace | (uintptr_t)bt->pose_pred | (uintptr_t)bt->pose_gt |
         (uintptr_t)bt->K) & 7)
        return PV_EALIGN;

    EvalArgs a{};
    a.pose_pred = bt->pose_pred; a.pose_gt = bt->pose_gt; a.K = bt->K;
    a.model = bt->model; a.model_off = bt->model_off; a.model_id = bt->model_id;
    a.partial = (double *)workspace; a.out = out;
    a.K_stride = bt->K_stride;
    a.b = bt->b; a.total = bt->total; a.nmodels = bt->nmodels; a.max_pn = bt->max_pn; a.nblk = (int32_t)nblk;
    a.metrics = bt->metrics;
    hipStream_t st = (hipStream_t)stream;
    if (points && nblk > 0) {
        const dim3 grid((unsigned)(nblk * bt->b));
        const bool s3 = bt->metrics & PV_EVAL_ADDS, s2 = bt->metrics & PV_EVAL_PROJ_SYM;
        if (s3 && s2) k_pose_partial<true, true><<<grid, kThreads, 0, st>>>(a);
        else if (s3) k_pose_partial<true, false><<<grid, kThreads, 0, st>>>(a);
        else if (s2) k_pose_partial<false, true><<<grid, kThreads, 0, st>>>(a);
        else k_pose_partial<false, false><<<grid, kThreads, 0, st>>>(a);
        const int e = last();
        if (e) return e;
    }
    k_pose_finish<<<(bt->b + 63) / 64, 64, 0, st>>>(a);
    return last();
}

}  // extern "C"
