// pvbop.hip -- libpvbop.so (include/pvbop.h): the BOP Challenge's pose errors for a batch of poses:
// MSSD and MSPD over a table of models and their symmetry transformations, and VSD over rendered
// depth maps.  One translation unit that includes no other file of csrc/.
//
// Everything is fp64 VALU with every operation rounded (-ffp-contract=off; no fused multiply-add, no MFMA: the
// definition rounds after each product and each sum), so tests/bop_ref.py's numpy
// float64 restatement reproduces every bit.
//
// k_sym_partial: block (pose, chunk of kChunk vertices).  Each lane keeps kVPL vertices, and for MSPD
// the estimate's projection of each (its two divides are paid once per vertex, not once per
// symmetry), in registers across the symmetry loop.  The symmetries are walked in LDS tiles of
// kTile: one lane per symmetry builds A_s | c_s and G_s once, then every lane reads them by
// broadcast.  Per symmetry the block's maximum (lanes by shuffles, waves through LDS) goes to the
// workspace.  k_sym_finish: one wave per pose takes the maximum over chunks, the minimum over
// symmetries with the lowest index, and the one square root.
// k_vsd: block (pose, kPix pixels).  A pixel neither map covers costs two loads and nothing else;
// the counts are wave ballots, summed per block and added with one integer atomic per counter.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pvbop.h"

namespace {

constexpr int kThreads = 256;             // 4 waves per block, both kernels
constexpr int kWaves = kThreads / 64;
constexpr int kVPL = 4;                   // vertices per lane
constexpr int kChunk = kThreads * kVPL;   // vertices per block: 1024
constexpr int kTile = 32;                 // symmetries per LDS tile
constexpr int kTab = 25;                  // doubles per symmetry in the tile: A 9, c 3, RG 9, tG 3, D_s' start
constexpr int kPPT = 4;                   // pixels per lane
constexpr int kPix = kThreads * kPPT;     // pixels per block: 1024
static_assert(kTile * 2 <= kThreads && kTile <= kThreads, "one lane per (symmetry, column) of a tile");
static_assert(2 + PV_BOP_MAX_TAUS <= kThreads, "one lane per counter");
constexpr double kBig = 0x1p300;          // the header's bound on an entry of A_s | c_s
static_assert(PV_BOP_MAX_ENTRY_EXP == 300, "kBig is 2^PV_BOP_MAX_ENTRY_EXP");

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
inline int last() { return rc(hipGetLastError()); }
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
inline int64_t chunks(int64_t n, int64_t per) { return (n + per - 1) / per; }

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = __builtin_fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// --------------------------------------------------------------------------
// pv_bop_sym_errors
// --------------------------------------------------------------------------
struct SymArgs {
    const double *pose_est, *pose_gt, *syms, *K;
    const float *model;
    const int32_t *model_off, *model_id, *sym_off;
    double *part;           // [b][nchunk][max_ns][2]: each block's maxima of d2, MSSD then MSPD
    double *err;
    int32_t *best;
    int64_t K_stride;
    int32_t b, total, total_s, nmodels, max_pn, max_ns, nchunk;
    uint32_t metrics;
};

// pose i's model as rows [lo, lo + pn) and its symmetries as rows [slo, slo + ns), every index
// checked before use; false: no such model or symmetry range (the pose scores NaN)
__device__ __forceinline__ bool ranges(const SymArgs &a, int i, int *lo, int *pn, int *slo, int *ns) {
    const int mid = a.model_id ? a.model_id[i] : 0;
    if (mid < 0 || mid >= a.nmodels) return false;
    const int l = a.model_off[mid], h = a.model_off[mid + 1];
    if (l < 0 || h > a.total || h <= l || h - l > a.max_pn) return false;
    const int sl = a.sym_off[mid], sh = a.sym_off[mid + 1];
    if (sl < 0 || sh > a.total_s || sh <= sl || sh - sl > a.max_ns) return false;
    *lo = l; *pn = h - l; *slo = sl; *ns = sh - sl;
    return true;
}

// M p + t with the header's parentheses: M row-major [9], t [3]
__device__ __forceinline__ void affine(const double *M, const double *t, double x, double y, double z, double *o) {
    o[0] = ((M[0] * x + M[1] * y) + M[2] * z) + t[0];
    o[1] = ((M[3] * x + M[4] * y) + M[5] * z) + t[1];
    o[2] = ((M[6] * x + M[7] * y) + M[8] * z) + t[2];
}

template <bool SSD, bool SPD>
__global__ __launch_bounds__(kThreads) void k_sym_partial(SymArgs a) {
    __shared__ double tab[kTile][kTab];
    __shared__ double wmax[kWaves][kTile][2];
    const int i = blockIdx.x / a.nchunk, ch = blockIdx.x - i * a.nchunk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int lo, pn, slo, ns;
    if (!ranges(a, i, &lo, &pn, &slo, &ns)) return;
    if ((int64_t)ch * kChunk >= pn) return;                            // past this pose's model
    const float *P = a.model + (int64_t)lo * 3;

    double Re[9], te[3], Rg[9], tg[3];
    const double *pe = a.pose_est + (int64_t)i * 12, *pg = a.pose_gt + (int64_t)i * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Re[r * 3 + c] = pe[r * 4 + c];
            Rg[r * 3 + c] = pg[r * 4 + c];
        }
        te[r] = pe[r * 4 + 3];
        tg[r] = pg[r * 4 + 3];
    }
    double fx = 0.0, sk = 0.0, cx = 0.0, fy = 0.0, cy = 0.0;
    if constexpr (SPD) {
        const double *K = a.K + (int64_t)i * a.K_stride;
        fx = K[0]; sk = K[1]; cx = K[2]; fy = K[4]; cy = K[5];
    }

    double x[kVPL], y[kVPL], z[kVPL], ue[kVPL], ve[kVPL];
#pragma unroll
    for (int k = 0; k < kVPL; ++k) {
        // a lane past the end repeats the last vertex: a maximum does not change
        const int j = min(ch * kChunk + k * kThreads + tid, pn - 1);
        x[k] = P[(int64_t)j * 3];
        y[k] = P[(int64_t)j * 3 + 1];
        z[k] = P[(int64_t)j * 3 + 2];
        ue[k] = ve[k] = 0.0;
        if constexpr (SPD) {
            double c[3];
            affine(Re, te, x[k], y[k], z[k], c);
            ue[k] = (fx * c[0] + sk * c[1]) / c[2] + cx;
            ve[k] = (fy * c[1]) / c[2] + cy;
            if (!(c[2] > 0.0)) ue[k] = __builtin_nan("");              // Z_e <= 0: d2 is not finite for any symmetry
        }
    }

    const double inf = __builtin_inf();
    for (int s0 = 0; s0 < ns; s0 += kTile) {
        const int nt = min(kTile, ns - s0);
        __syncthreads();                                               // the previous tile is consumed
        if (tid < nt) {
            const double *S = a.syms + (int64_t)(slo + s0 + tid) * 12;
            double *T = tab[tid];
            bool over = false;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double g = (Rg[r * 3] * S[c] + Rg[r * 3 + 1] * S[4 + c]) + Rg[r * 3 + 2] * S[8 + c];
                    const double d = Re[r * 3 + c] - g;
                    T[r * 3 + c] = d;
                    T[12 + r * 3 + c] = g;
                    over = over || !(fabs(d) < kBig);
                }
                const double g = ((Rg[r * 3] * S[3] + Rg[r * 3 + 1] * S[7]) + Rg[r * 3 + 2] * S[11]) + tg[r];
                const double d = te[r] - g;
                T[9 + r] = d;
                T[21 + r] = g;
                over = over || !(fabs(d) < kBig);
            }
            T[24] = over ? inf : 0.0;                                  // where D_s starts: +inf stays +inf
        }
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const double *T = tab[t];                                  // every lane the same address: a broadcast
            double m1 = 0.0, m2 = 0.0;
            if constexpr (SSD) {
                double A[9], c[3];
#pragma unroll
                for (int e = 0; e < 9; ++e) A[e] = T[e];
#pragma unroll
                for (int e = 0; e < 3; ++e) c[e] = T[9 + e];
                m1 = T[24];
#pragma unroll
                for (int k = 0; k < kVPL; ++k) {
                    double e[3];
                    affine(A, c, x[k], y[k], z[k], e);
                    m1 = __builtin_fmax(m1, (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
                }
            }
            if constexpr (SPD) {
                double G[9], tG[3];
#pragma unroll
                for (int e = 0; e < 9; ++e) G[e] = T[12 + e];
#pragma unroll
                for (int e = 0; e < 3; ++e) tG[e] = T[21 + e];
#pragma unroll
                for (int k = 0; k < kVPL; ++k) {
                    double c[3];
                    affine(G, tG, x[k], y[k], z[k], c);
                    const double ug = (fx * c[0] + sk * c[1]) / c[2] + cx;
                    const double vg = (fy * c[1]) / c[2] + cy;
                    const double du = ue[k] - ug, dv = ve[k] - vg;
                    double d2 = du * du + dv * dv;
                    if (!(c[2] > 0.0 && d2 < inf)) d2 = inf;           // a NaN d2 is not below +inf
                    m2 = __builtin_fmax(m2, d2);
                }
            }
            if constexpr (SSD) m1 = wave_max(m1);
            if constexpr (SPD) m2 = wave_max(m2);
            if (lane == 0) {
                wmax[wave][t][0] = m1;
                wmax[wave][t][1] = m2;
            }
        }
        __syncthreads();
        if (tid < nt * 2) {
            const int t = tid >> 1, c = tid & 1;
            double m = wmax[0][t][c];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) m = __builtin_fmax(m, wmax[w][t][c]);
            a.part[(((int64_t)i * a.nchunk + ch) * a.max_ns + (s0 + t)) * 2 + c] = m;
        }
    }
}

// One wave per pose: lane l takes symmetries l, l + 64, ...
__global__ __launch_bounds__(64) void k_sym_finish(SymArgs a) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const double inf = __builtin_inf(), nan = __builtin_nan("");
    const bool want[2] = {(a.metrics & PV_BOP_MSSD) != 0, (a.metrics & PV_BOP_MSPD) != 0};
    const double *pe = a.pose_est + (int64_t)i * 12, *pg = a.pose_gt + (int64_t)i * 12;
    bool ok = true;
    for (int e = 0; e < 12; ++e) ok = ok && isfinite(pe[e]) && isfinite(pg[e]);
    bool kok = true;
    if (want[1]) {
        const double *K = a.K + (int64_t)i * a.K_stride;
        kok = isfinite(K[0]) && isfinite(K[1]) && isfinite(K[2]) && isfinite(K[4]) && isfinite(K[5]);
    }
    int lo, pn, slo, ns;
    ok = ok && ranges(a, i, &lo, &pn, &slo, &ns);

    double bv[2] = {inf, inf};
    int bi[2] = {INT32_MAX, INT32_MAX};
    bool bad = false;
    if (ok) {
        const int nch = (pn + kChunk - 1) / kChunk;
        for (int s = lane; s < ns; s += 64) {
            const double *S = a.syms + (int64_t)(slo + s) * 12;
            for (int e = 0; e < 12; ++e) bad = bad || !isfinite(S[e]);
            for (int c = 0; c < 2; ++c) {
                if (!want[c]) continue;
                double m = a.part[(((int64_t)i * a.nchunk) * a.max_ns + s) * 2 + c];
                for (int ch = 1; ch < nch; ++ch) {
                    const double v = a.part[(((int64_t)i * a.nchunk + ch) * a.max_ns + s) * 2 + c];
                    m = v > m ? v : m;
                }
                if (bi[c] == INT32_MAX || m < bv[c]) {                 // strict: the lowest index keeps a tie
                    bv[c] = m;
                    bi[c] = s;
                }
            }
        }
    }
    for (int o = 32; o >= 1; o >>= 1) {
        for (int c = 0; c < 2; ++c) {
            const double ov = __shfl_xor(bv[c], o, 64);
            const int oi = __shfl_xor(bi[c], o, 64);
            if (ov < bv[c] || (ov == bv[c] && oi < bi[c])) {
                bv[c] = ov;
                bi[c] = oi;
            }
        }
    }
    bad = __any(bad);
    if (lane == 0) {
        for (int c = 0; c < 2; ++c) {
            if (!want[c]) continue;
            const bool good = ok && !bad && (c == 0 || kok);
            a.err[(int64_t)i * PV_BOP_NCOL + c] = good ? sqrt(bv[c]) : nan;
            a.best[(int64_t)i * PV_BOP_NCOL + c] = good ? bi[c] : -1;
        }
    }
}

// --------------------------------------------------------------------------
// pv_bop_vsd
// --------------------------------------------------------------------------
struct VsdArgs {
    const float *depth_test, *depth_est, *depth_gt;
    const int32_t *img_id;
    const double *K, *taus;
    int64_t *counts;
    double *err;
    int64_t K_stride, npix;
    double delta;
    int32_t b, n_img, H, W, ntau, nblk;
};

// pose i's image and camera, checked; false: the pose scores NaN
__device__ __forceinline__ bool vsd_pose(const VsdArgs &a, int i, int *img, double *fx, double *fy, double *cx, double *cy) {
    const int j = a.img_id ? a.img_id[i] : i;
    if (j < 0 || j >= a.n_img) return false;
    const double *K = a.K + (int64_t)i * a.K_stride;
    *fx = K[0]; *cx = K[2]; *fy = K[4]; *cy = K[5];
    *img = j;
    return isfinite(*fx) && isfinite(*fy) && isfinite(*cx) && isfinite(*cy);
}

__device__ __forceinline__ bool depth_ok(float z) { return z > 0.f && z < __builtin_inff(); }

__global__ __launch_bounds__(kThreads) void k_vsd(VsdArgs a) {
    __shared__ unsigned cnt[kWaves][2 + PV_BOP_MAX_TAUS];
    const int i = blockIdx.x / a.nblk, blk = blockIdx.x - i * a.nblk;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int img;
    double fx, fy, cx, cy;
    if (!vsd_pose(a, i, &img, &fx, &fy, &cx, &cy)) return;
    const float *zt_ = a.depth_test + (int64_t)img * a.npix;
    const float *ze_ = a.depth_est + (int64_t)i * a.npix;
    const float *zg_ = a.depth_gt + (int64_t)i * a.npix;
    const double *tau = a.taus + (int64_t)i * a.ntau;
    const int ncnt = 2 + a.ntau;
    if (lane == 0)                                                     // each wave owns its row, and only its lane 0 touches it
        for (int t = 0; t < ncnt; ++t) cnt[wave][t] = 0;

    unsigned n_un = 0, n_in = 0;                                       // lane 0's are the wave's
#pragma unroll
    for (int k = 0; k < kPPT; ++k) {
        const int64_t p = (int64_t)blk * kPix + k * kThreads + tid;
        bool un = false, in = false;
        double diff = 0.0;
        if (p < a.npix) {
            const float zef = ze_[p], zgf = zg_[p];
            const bool e_ok = depth_ok(zef), g_ok = depth_ok(zgf);
            if (e_ok || g_ok) {
                const float ztf = zt_[p];
                const bool t_ok = depth_ok(ztf);
                int64_t px, py;
                if (a.npix <= INT32_MAX) {
                    py = (uint32_t)p / (uint32_t)a.W;
                    px = (uint32_t)p - (uint32_t)py * (uint32_t)a.W;
                } else {
                    py = p / a.W;
                    px = p - py * a.W;
                }
                const double ax = ((double)px - cx) / fx, ay = ((double)py - cy) / fy;
                const double r = sqrt((ax * ax + ay * ay) + 1.0);
                const double dt = (double)ztf * r, de = (double)zef * r, dg = (double)zgf * r;
                const bool vis_gt = g_ok && (!t_ok || dg - dt <= a.delta);
                const bool vis_est = e_ok && (!t_ok || de - dt <= a.delta || vis_gt);
                un = vis_gt || vis_est;
                in = vis_gt && vis_est;
                diff = fabs(dg - de);
            }
        }
        n_un += __popcll(__ballot(un));
        const unsigned long long both = __ballot(in);
        n_in += __popcll(both);
        if (both) {                                                    // uniform over the wave
            for (int t = 0; t < a.ntau; ++t) {
                const unsigned c = __popcll(__ballot(in && diff >= tau[t]));
                if (lane == 0) cnt[wave][2 + t] += c;
            }
        }
    }
    if (lane == 0) {
        cnt[wave][0] = n_un;
        cnt[wave][1] = n_in;
    }
    __syncthreads();
    if (tid < ncnt) {
        unsigned long long s = 0;
        for (int w = 0; w < kWaves; ++w) s += cnt[w][tid];
        if (s) atomicAdd((unsigned long long *)(a.counts + (int64_t)i * ncnt + tid), s);
    }
}

// One thread per pose: the errors from the counts, or NaN and -1
__global__ __launch_bounds__(64) void k_vsd_finish(VsdArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.b) return;
    int img;
    double fx, fy, cx, cy;
    const bool ok = vsd_pose(a, i, &img, &fx, &fy, &cx, &cy);
    int64_t *cn = a.counts + (int64_t)i * (2 + a.ntau);
    double *er = a.err + (int64_t)i * a.ntau;
    if (!ok) {
        for (int t = 0; t < 2 + a.ntau; ++t) cn[t] = -1;
        for (int t = 0; t < a.ntau; ++t) er[t] = __builtin_nan("");
        return;
    }
    const int64_t un = cn[0], in = cn[1];
    for (int t = 0; t < a.ntau; ++t) er[t] = un > 0 ? (double)(cn[2 + t] + (un - in)) / (double)un : 1.0;
}

}  // namespace

extern "C" {

size_t pv_bop_workspace_size(int32_t b, int32_t max_pn, int32_t max_ns) {
    if (b < 1 || max_pn < 1 || max_ns < 1) return 0;
    return (size_t)align_up((int64_t)b * chunks(max_pn, kChunk) * max_ns * 2 * (int64_t)sizeof(double), 256);
}

int pv_bop_sym_errors(const pv_bop_batch *bt, double *err, int32_t *best, void *workspace, size_t workspace_bytes,
                      pv_stream_t stream) {
    if (!bt) return PV_EINVAL;
    if (bt->b < 0 || bt->total < 0 || bt->total_s < 0 || bt->max_pn < 0 || bt->max_ns < 0 || bt->K_stride < 0 ||
        bt->nmodels < 1 || (bt->metrics & ~PV_BOP_ALL))
        return PV_EINVAL;
    if (bt->b == 0 || bt->metrics == 0) return PV_OK;
    if (!err || !best || !bt->pose_est || !bt->pose_gt || !bt->model_off || !bt->sym_off) return PV_EINVAL;
    if ((!bt->model && bt->total > 0) || (!bt->syms && bt->total_s > 0)) return PV_EINVAL;
    if ((bt->metrics & PV_BOP_MSPD) && !bt->K) return PV_EINVAL;
    const int64_t nchunk = chunks(bt->max_pn, kChunk);
    if (nchunk * bt->b > INT32_MAX) return PV_EINVAL;
    const size_t need = pv_bop_workspace_size(bt->b, bt->max_pn, bt->max_ns);
    if (need && (!workspace || workspace_bytes < need)) return PV_EWORKSPACE;
    if (((uintptr_t)err | (uintptr_t)workspace | (uintptr_t)bt->pose_est | (uintptr_t)bt->pose_gt | (uintptr_t)bt->syms |
         (uintptr_t)bt->K) & 7)
        return PV_EALIGN;
    if ((uintptr_t)best & 3) return PV_EALIGN;

    SymArgs a{};
    a.pose_est = bt->pose_est; a.pose_gt = bt->pose_gt; a.syms = bt->syms; a.K = bt->K;
    a.model = bt->model; a.model_off = bt->model_off; a.model_id = bt->model_id; a.sym_off = bt->sym_off;
    a.part = (double *)workspace; a.err = err; a.best = best;
    a.K_stride = bt->K_stride;
    a.b = bt->b; a.total = bt->total; a.total_s = bt->total_s; a.nmodels = bt->nmodels;
    a.max_pn = bt->max_pn; a.max_ns = bt->max_ns; a.nchunk = (int32_t)nchunk;
    a.metrics = bt->metrics;
    hipStream_t st = (hipStream_t)stream;
    if (need) {                                     // max_pn or max_ns of 0: no pose has a range, all NaN
        const dim3 grid((unsigned)(nchunk * bt->b));
        const bool ssd = bt->metrics & PV_BOP_MSSD, spd = bt->metrics & PV_BOP_MSPD;
        if (ssd && spd) k_sym_partial<true, true><<<grid, kThreads, 0, st>>>(a);
        else if (ssd) k_sym_partial<true, false><<<grid, kThreads, 0, st>>>(a);
        else k_sym_partial<false, true><<<grid, kThreads, 0, st>>>(a);
        const int e = last();
        if (e) return e;
    }
    k_sym_finish<<<bt->b, 64, 0, st>>>(a);
    return last();
}

int pv_bop_vsd(const pv_bop_vsd_batch *bt, int64_t *counts, double *err, pv_stream_t stream) {
    if (!bt) return PV_EINVAL;
    if (bt->b < 0 || bt->n_img < 0 || bt->K_stride < 0 || bt->H < 1 || bt->H > PV_BOP_MAX_DIM || bt->W < 1 ||
        bt->W > PV_BOP_MAX_DIM || bt->ntau < 1 || bt->ntau > PV_BOP_MAX_TAUS || !(bt->delta >= 0.0 && bt->delta < INFINITY))
        return PV_EINVAL;
    if (bt->b == 0) return PV_OK;
    if (!counts || !err || !bt->depth_est || !bt->depth_gt || !bt->K || !bt->taus) return PV_EINVAL;
    if (!bt->depth_test && bt->n_img > 0) return PV_EINVAL;
    const int64_t npix = (int64_t)bt->H * bt->W, nblk = chunks(npix, kPix);
    if (nblk * bt->b > INT32_MAX) return PV_EINVAL;
    if (((uintptr_t)counts | (uintptr_t)err | (uintptr_t)bt->K | (uintptr_t)bt->taus) & 7) return PV_EALIGN;
    if (((uintptr_t)bt->depth_test | (uintptr_t)bt->depth_est | (uintptr_t)bt->depth_gt | (uintptr_t)bt->img_id) & 3)
        return PV_EALIGN;

    VsdArgs a{};
    a.depth_test = bt->depth_test; a.depth_est = bt->depth_est; a.depth_gt = bt->depth_gt;
    a.img_id = bt->img_id; a.K = bt->K; a.taus = bt->taus;
    a.counts = counts; a.err = err;
    a.K_stride = bt->K_stride; a.npix = npix; a.delta = bt->delta;
    a.b = bt->b; a.n_img = bt->n_img; a.H = bt->H; a.W = bt->W; a.ntau = bt->ntau; a.nblk = (int32_t)nblk;
    hipStream_t st = (hipStream_t)stream;
    int e = rc(hipMemsetAsync(counts, 0, (size_t)bt->b * (2 + bt->ntau) * sizeof(int64_t), st));
    if (e) return e;
    k_vsd<<<dim3((unsigned)(nblk * bt->b)), kThreads, 0, st>>>(a);
    if ((e = last())) return e;
    k_vsd_finish<<<(bt->b + 63) / 64, 64, 0, st>>>(a);
    return last();
}

}  // extern "C"
