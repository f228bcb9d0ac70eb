/* pvmodel.h -- C ABI of libpvmodel.so: the per-model constants of the pipeline, on the device.
 *
 * From the points of a model table (a mesh table's vertices, or a ModelTable's points): the
 * bounding box, the centroid and the count of finite points (pv_model_extent), farthest-point
 * keypoints (pv_farthest_points; the reference's extend_utils/src/farthest_point_sampling.cpp,
 * batched over the table and with a deterministic tie rule) and the diameter (pv_model_diameter;
 * the reference reads it from a dataset file).  A library of its own: nothing here needs the other
 * four, and their export lists do not change.  This header defines the semantics;
 * tests/model_ref.py restates them in numpy.
 *
 * Conventions (those of pvvote.h, pveval.h, pvpose.h and pvrender.h):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below; nothing
 *     calls exit();
 *   - every bad argument (a NULL descriptor, a negative size or max_pn, k outside
 *     1..PV_MODEL_MAX_K, an unknown start mode, PV_FPS_START_INDEX without start_idx, a NULL
 *     input or output, a workspace that is NULL, too small or misaligned) is rejected on the host
 *     before any pointer is touched; nmodels == 0 is success;
 *   - every offset and index read from device memory is checked against the bounds the host
 *     vouches for before it is used.
 *
 * Arithmetic.  Coordinates are widened from f32 to f64 and everything below runs in fp64, every
 * operation rounded (nothing is contracted into an FMA, no fast reciprocal, no fast sqrt):
 *     d2(a, b) = ((dx dx + dy dy) + dz dz),  dx = ax - bx, dy = ay - by, dz = az - bz.
 *
 * Points that do not count.  A point with a non-finite coordinate is absent: it is never picked
 * and enters neither the box, the centroid nor the diameter.  A model is skipped if its offset
 * range is not 0 <= lo <= hi <= total or if it has more than max_pn points.  A skipped model, and
 * a model with no finite point, gives count 0, NaN for every f64 output and -1 for every index.
 * The ranges of the models that are not skipped must not overlap: pv_farthest_points keeps the
 * running minimum of a model above PV_MODEL_BLOCK_MAX_PN points in the workspace, one slot per
 * row of `points`, so overlapping large models get unspecified picks (never a fault).
 */
#ifndef PVMODEL_H_
#define PVMODEL_H_

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

#define PV_MODEL_SUM_LANES 256      /* the centroid's summation order, below */
#define PV_MODEL_MAX_K 1024         /* picks per model */
#define PV_MODEL_BLOCK_MAX_PN 12288 /* a model of at most this many points is sampled by one block, from LDS */
#define PV_MODEL_CHUNK 8192         /* points per block of the per-step form (larger models) */
#define PV_MODEL_TILE 256           /* points per side of a diameter block's tile pair */

/* how pick 0 is chosen */
#define PV_FPS_START_CENTROID 0      /* the point farthest from the centroid; the running minimum then
                                      * starts from d2(., pick 0) alone */
#define PV_FPS_START_CENTROID_KEPT 1 /* the same pick 0, but the running minimum starts from
                                      * min(d2(., centroid), d2(., pick 0)): the centre counts as sampled */
#define PV_FPS_START_INDEX 2         /* pick 0 is start_idx[m] (the reference's random first index, as an
                                      * argument) */

typedef struct pv_model_points {
    const float *points;    /* f32 [total][3], all models concatenated */
    const int32_t *off;     /* i32 [nmodels + 1], device: model m is rows [off[m], off[m+1]) */
    int32_t nmodels, total;
    int32_t max_pn;         /* host-vouched: a model with more points is skipped */
    int32_t reserved_;
} pv_model_points;

/* Bytes of workspace for any of the calls below on a table of these sizes; pass k = 1 for a call
 * that takes no k.  0 for bad sizes (negative, or k outside 1..PV_MODEL_MAX_K).  The workspace is
 * 256-byte aligned device memory, owned by the call until it has run.  It need not be cleared: a
 * call initialises every accumulator and slot it reads, and writes nothing but its outputs and
 * workspace[0, size). */
size_t pv_model_workspace_size(int32_t nmodels, int32_t total, int32_t k);

/* ---- 1. pv_model_extent ---------------------------------------------------------------------------
 * bbox[m] = the exact minimum and maximum per coordinate of the model's finite points (order
 * independent); count[m] = their number; centroid[m] = sum / (double)count per coordinate, with the
 * sum taken in a fixed order so that every run gives the same bits: with L = PV_MODEL_SUM_LANES,
 * lane j adds the points i = j (mod L) of the model in increasing i starting from +0.0 (an absent
 * point contributes +0.0), then for s = L/2, L/4, ..., 1: lane[j] += lane[j + s] for j < s; the
 * sum is lane[0].  Any output may be NULL, but not all three. */
int pv_model_extent(const pv_model_points *p /* host */, double *bbox /* f64 [nmodels][2][3]: min, max */,
                    double *centroid /* f64 [nmodels][3] */, int32_t *count /* i32 [nmodels] */, pv_stream_t stream);

/* ---- 2. pv_farthest_points ------------------------------------------------------------------------
 * idx[m][j] is the index within model m of pick j, 0 <= j < k.  Pick 0 by `start` (above; the
 * centroid is pv_model_extent's).  In index mode a start_idx[m] outside [0, the model's point
 * count), or naming an absent point, gives that model -1 / NaN.  With min_d2[i] the running
 * minimum of point i, after each pick  min_d2[i] = min(min_d2[i], d2(p_i, p_pick)),  and pick
 * j >= 1 is the arg-max of min_d2 over the model's finite points; A TIE GOES TO THE LOWEST INDEX
 * (pick 0 of the centroid modes too), so the result does not depend on how the reduction is
 * shaped.  k may exceed the count: picks then repeat, following the same rule.
 * picked[m][j] = the pick's coordinates (widened); pick_d2[m][j] = the value that won pick j: for
 * pick 0 the squared distance to the centroid in the centroid modes and +inf in index mode.
 * A model of at most PV_MODEL_BLOCK_MAX_PN points is sampled by one block that keeps the points
 * and the running minimum on chip for all k steps; a larger one takes one launch per step over
 * blocks of PV_MODEL_CHUNK points; one call may mix both kinds. */
int pv_farthest_points(const pv_model_points *p /* host */, int32_t k, int32_t start,
                       const int32_t *start_idx /* i32 [nmodels], PV_FPS_START_INDEX only */,
                       int32_t *idx /* i32 [nmodels][k] */, double *picked /* optional f64 [nmodels][k][3] */,
                       double *pick_d2 /* optional f64 [nmodels][k] */, void *workspace, size_t workspace_bytes,
                       pv_stream_t stream);

/* ---- 3. pv_model_diameter -------------------------------------------------------------------------
 * diameter[m] = sqrt(max over i <= j of d2(p_i, p_j)) over the model's finite points, with the
 * correctly rounded fp64 sqrt; one finite point gives 0.  The maximum is order independent: blocks
 * of PV_MODEL_TILE x PV_MODEL_TILE pairs combine through one 64-bit integer atomic maximum on the
 * bit pattern of the non-negative double (no floating-point atomics), so every run gives the same
 * bits.  A table whose max_pn needs more than 2^31 - 1 tile pairs (about 16.7 million points in
 * one model) is PV_EINVAL. */
int pv_model_diameter(const pv_model_points *p /* host */, double *diameter /* f64 [nmodels] */, void *workspace,
                      size_t workspace_bytes, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVMODEL_H_ */
