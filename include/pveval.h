/* pveval.h -- C ABI of libpveval.so: batched pose evaluation on the device.
 *
 * The stage after pv_uncertainty_pnp (include/pvvote.h): scoring poses the way the reference's
 * Evaluator does (lib/utils/evaluation_utils.py:63-225, "EU") -- ADD, ADD-S, 2-D projection error,
 * translation / rotation error -- and the nearest-neighbour kernel ADD-S rests on
 * (extend_utils/src/nearest_neighborhood.cu).  A library of its own: nothing here needs
 * libpvvote.so, and libpvvote.so's export list does not change.
 *
 * Conventions (those of pvvote.h):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below (the values
 *     of pvvote.h's PV_EINVAL / PV_EWORKSPACE / PV_EALIGN); nothing calls exit();
 *   - every bad argument (NULL required pointer, b < 0, dim outside {2, 3}, pn1 < 1, nmodels < 1,
 *     a workspace that is too small, a metric bit out of range) is rejected on the host before
 *     anything is launched; b == 0 or pn2 == 0 is success with no launch.
 */
#ifndef PVEVAL_H_
#define PVEVAL_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The stream type and the return codes: the same block under the same guard in every public header
 * of this project, so they can be included together in any order. */
#ifndef PV_STATUS_
#define PV_STATUS_
typedef void *pv_stream_t; /* hipStream_t */

#define PV_OK 0
#define PV_EINVAL (-1)     /* bad size / pointer / enum */
#define PV_EWORKSPACE (-2) /* workspace missing or too small */
#define PV_EALIGN (-3)     /* pointer not aligned as documented */
#endif

/* ---- 1. nearest reference point ---------------------------------------------------------------
 * Replaces findNearestPoint{2,3}DIdx (extend_utils/src/nearest_neighborhood.cu:48,84; its only
 * caller is ADD-S / projection_2d_sym, EU:54-61,118-129).
 * ref f32 [b][pn1][dim], que f32 [b][pn2][dim], idx i32 [b][pn2]; dim 2 or 3.
 *
 * The semantics below are this project's definition (the reference source is cited, not copied).
 * For query q and reference r, in fp32, every operation rounded, nothing contracted:
 *     dx = qx - rx, dy = qy - ry, dz = qz - rz
 *     d2 = (dx*dx + dy*dy) + dz*dz          (dim 3)
 *     d2 = dx*dx + dy*dy                    (dim 2)
 * idx[q] is the lowest reference index attaining the minimum d2: strict `<` against a running
 * minimum that starts at +inf, so a NaN d2 never wins, and idx = 0 if no reference wins.
 * A numpy float32 restatement of these lines reproduces every index bit for bit. */
int pv_nearest_point_idx(const float *ref, const float *que, int32_t *idx,
                         int32_t b, int32_t pn1, int32_t pn2, int32_t dim, pv_stream_t stream);

/* ---- 2. fused pose metrics ---------------------------------------------------------------------
 * One call scores a batch of poses against their ground truth over a table of models
 * (Evaluator's add_metric, add_metric_sym, projection_2d, projection_2d_sym, cm_degree_5_metric:
 * EU:63-225).  Thresholds (0.1 diameter, 5 px, 5 cm 5 deg) are the caller's. */
#define PV_EVAL_ADD 1u       /* column ADD */
#define PV_EVAL_ADDS 2u      /* column ADDS */
#define PV_EVAL_PROJ 4u      /* column PROJ */
#define PV_EVAL_PROJ_SYM 8u  /* column PROJ_SYM */
#define PV_EVAL_CMDEG 16u    /* columns TRANS_CM and ROT_DEG */
#define PV_EVAL_ALL 31u

#define PV_EVAL_COL_ADD 0
#define PV_EVAL_COL_ADDS 1
#define PV_EVAL_COL_PROJ 2
#define PV_EVAL_COL_PROJ_SYM 3
#define PV_EVAL_COL_TRANS_CM 4
#define PV_EVAL_COL_ROT_DEG 5
#define PV_EVAL_NCOL 6

typedef struct pv_eval_batch {
    int32_t b;                 /* poses (for multi-object frames: the virtual images bi*ncls + c) */
    int32_t total;             /* host: rows of `model`; every offset read on the device is checked against it */
    const double *pose_pred;   /* f64 [b][3][4] = [R | t], e.g. pv_uncertainty_pnp's Rt, in place */
    const double *pose_gt;     /* f64 [b][3][4] */
    const float  *model;       /* f32 [total][3]: the vertices of all models, concatenated */
    const int32_t *model_off;  /* i32 [nmodels + 1] device: model m is rows [off[m], off[m+1]) */
    const int32_t *model_id;   /* i32 [b] device, or NULL = model 0 for every pose */
    int32_t nmodels;
    int32_t max_pn;            /* host: the largest model's vertex count (sizes the grid, no readback) */
    const double *K;           /* f64 [3][3], pose i at K + i*K_stride; K_stride 0 = shared */
    int64_t K_stride;
    uint32_t metrics;          /* PV_EVAL_ADD | PV_EVAL_ADDS | PV_EVAL_PROJ | PV_EVAL_PROJ_SYM | PV_EVAL_CMDEG */
} pv_eval_batch;

/* Columns of out f64 [b][PV_EVAL_NCOL], p running over the pose's model (pn vertices):
 *   ADD       mean_p |(R_pred p + t_pred) - (R_gt p + t_gt)|                      (EU add_metric), fp64
 *   ADDS      mean over the ground-truth-transformed points of the distance to the nearest
 *             pred-transformed point (EU:54-61 add_metric_sym): queries are the ground-truth
 *             cloud, references the predicted cloud, as in pv_nearest_point_idx
 *   PROJ      mean_p |pi(K(R_pred p + t_pred)) - pi(K(R_gt p + t_gt))| in pixels  (EU projection_2d), fp64
 *   PROJ_SYM  the same with the nearest predicted projection for each ground-truth projection (EU:118-129)
 *   TRANS_CM  100 |t_pred - t_gt|
 *   ROT_DEG   degrees(arccos(clamp((min(trace(R_pred R_gt^T), 3) - 1) / 2, -1, .)))  (EU cm_degree_5_metric), fp64,
 *             evaluated by the half angle, 2 atan2(sqrt(max(3 - tr, 0)), sqrt(max(1 + tr, 0))): the same
 *             function, well conditioned at 0 and at 180 degrees
 * ADD and PROJ are evaluated through the difference (R_pred - R_gt) p + (t_pred - t_gt), so nearly
 * equal poses do not cancel and identical poses score exactly 0.
 * The two nearest-neighbour columns: the clouds are transformed in fp64 in a frame centred on the
 * ground truth (3-D: g = R_gt p and q = R_pred p + (t_pred - t_gt); 2-D: both projections minus
 * the projection of t_gt) and only then rounded to fp32; the pair loop is fp32 in exactly the
 * arithmetic of pv_nearest_point_idx; the square root of each query's minimum is taken and summed
 * in fp64.  Absolute error <= 32 * 2^-24 * M, M the largest absolute centred coordinate.
 *
 * A pose whose model is empty, larger than max_pn, outside `total`, or whose model_id is outside
 * [0, nmodels) gets NaN in the four per-point columns (model_id is device data: not an error
 * return).  A pose (or, for the projection columns, a K) with a NaN or infinite entry gets NaN in
 * every requested column.  A column whose metric was not requested is left untouched.
 * No float atomics: per-block partial sums go to the workspace and a second launch adds them in
 * block order, so `out` is bit-identical from run to run.  The workspace need not be cleared: the
 * call writes every partial it reads, and writes nothing but `out` and workspace[0, size). */
size_t pv_eval_workspace_size(int32_t b, int32_t max_pn);   /* host only; 0 for b < 1 or max_pn < 0 */
int pv_pose_metrics(const pv_eval_batch *batch /* host */, double *out, void *workspace, size_t workspace_bytes,
                    pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVEVAL_H_ */
