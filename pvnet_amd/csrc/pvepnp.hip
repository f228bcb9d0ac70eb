// pvepnp.hip -- MI355X (gfx950) batched EPnP, the plain PnP behind Evaluator.evaluate.
// The only translation unit of libpvpose.so; exported through include/pvpose.h.
//
// Reference (kennege/pvnet): lib/utils/evaluation_utils.py:19-52 pnp(), which is
// cv2.solvePnP(SOLVEPNP_EPNP).  OpenCV's epnp.cpp is restated in pvepnp_core.h.
//
// Layout: one wave (one 64-thread block) per image, lane = model point (pn <= 64), all fp64,
// as k_uncertainty_pnp.  Sums over the points are formed per output entry in point order out of
// LDS (the 78 entries of M^T M over the lanes, and so on), the 12x12 eigenproblem is a
// round-robin cyclic Jacobi with the step's six disjoint rotations applied by the whole wave,
// the three beta candidates run on lanes 0..2.  About 12.5 KB of LDS per block: the kernel is
// latency-bound (a few hundred barriers of short phases), so it wants many blocks per CU.
#include <hip/hip_runtime.h>

#include "../../include/pvpose.h"
#include "pvepnp_core.h"

static_assert(pve::kStatusOk == PV_EPNP_OK && pve::kStatusDegenerate == PV_EPNP_DEGENERATE, "status codes");
static_assert(pve::kMinPts == PV_EPNP_MIN_POINTS && pve::kMaxPts == PV_EPNP_MAX_POINTS, "point limits");

namespace {

inline int last() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PV_OK : (int)e;
}

__global__ __launch_bounds__(64) void k_epnp(pv_epnp_batch bt, double *Rt, double *rt6, pv_epnp_diag dg) {
    __shared__ pve::Epnp S;
    const int64_t img = blockIdx.x;
    const int64_t p2 = img * bt.pn * 2;
    pve::Out o;
    pve::epnp_image(S, bt.pn, bt.pts3d + img * bt.pts3d_stride, bt.K + img * bt.K_stride,
                    bt.pts2d ? bt.pts2d + p2 : nullptr, bt.pts2d64 ? bt.pts2d64 + p2 : nullptr, o);
    if (threadIdx.x == 0) {
        if (Rt)
            for (int k = 0; k < 12; ++k) Rt[img * 12 + k] = o.Rt[k];
        if (rt6)
            for (int k = 0; k < 6; ++k) rt6[img * 6 + k] = o.rt6[k];
        if (dg.status) dg.status[img] = o.status;
        if (dg.n_used) dg.n_used[img] = o.n_used;
        if (dg.cand_err)
            for (int k = 0; k < 3; ++k) dg.cand_err[img * 3 + k] = o.cand_err[k];
    }
}

__global__ __launch_bounds__(64) void k_rt6_to_Rt(const double *rt6, double *Rt, int b) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= b) return;
    double r[6], R[9];
    for (int k = 0; k < 6; ++k) r[k] = rt6[i * 6 + k];
    pve::rodrigues_to_mat(r, R);
    for (int row = 0; row < 3; ++row) {
        for (int c = 0; c < 3; ++c) Rt[i * 12 + row * 4 + c] = R[row * 3 + c];
        Rt[i * 12 + row * 4 + 3] = r[3 + row];
    }
}

}  // namespace

extern "C" {

int pv_epnp(const pv_epnp_batch *batch, double *Rt, double *rt6, const pv_epnp_diag *diag, pv_stream_t stream) {
    if (!batch || batch->b < 0 || batch->pn < PV_EPNP_MIN_POINTS || batch->pn > PV_EPNP_MAX_POINTS) return PV_EINVAL;
    if (batch->pts3d_stride < 0 || batch->K_stride < 0) return PV_EINVAL;
    if (batch->b == 0) return PV_OK;
    if ((!batch->pts2d && !batch->pts2d64) || !batch->pts3d || !batch->K || (!Rt && !rt6)) return PV_EINVAL;
    pv_epnp_batch bt = *batch;
    if (bt.pts2d64) bt.pts2d = nullptr;
    pv_epnp_diag dg{};
    if (diag) dg = *diag;
    k_epnp<<<bt.b, 64, 0, (hipStream_t)stream>>>(bt, Rt, rt6, dg);
    return last();
}

int pv_rt6_to_Rt(const double *rt6, double *Rt, int32_t b, pv_stream_t stream) {
    if (b < 0) return PV_EINVAL;
    if (b == 0) return PV_OK;
    if (!rt6 || !Rt) return PV_EINVAL;
    k_rt6_to_Rt<<<(unsigned)(((int64_t)b + 63) / 64), 64, 0, (hipStream_t)stream>>>(rt6, Rt, b);
    return last();
}

}  // extern "C"
