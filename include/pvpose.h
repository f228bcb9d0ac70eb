/* pvpose.h -- C ABI of libpvpose.so: the plain PnP (EPnP) on the device.
 *
 * The pose step of the reference's Evaluator.evaluate (lib/utils/evaluation_utils.py:19-52, "EU":
 * pnp() = cv2.solvePnP(..., flags=cv2.SOLVEPNP_EPNP)) for a batch of images.  A library of its
 * own: nothing here needs libpvvote.so or libpveval.so, and their export lists do not change.
 * pv_epnp's rt6 is what pv_uncertainty_pnp_refine (include/pvvote.h) takes as init_rt, and
 * pv_rt6_to_Rt turns that call's result into [R | t], so EPnP -> Levenberg-Marquardt -> Rt is
 * three launches on one stream with no host trip.
 *
 * Conventions (those of pvvote.h and pveval.h):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below; nothing
 *     calls exit();
 *   - every bad argument (NULL batch, b < 0, pn outside 6..64, both point pointers NULL, a NULL
 *     model or camera, Rt and rt6 both NULL, a negative stride) is rejected on the host before any
 *     pointer is touched; b == 0 is success with no launch.
 */
#ifndef PVPOSE_H_
#define PVPOSE_H_

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

/* ---- 1. EPnP -------------------------------------------------------------------------------------
 * OpenCV's modules/calib3d/src/epnp.cpp (Lepetit, Moreno-Noguer, Fua, "EPnP: An Accurate O(n)
 * Solution to the PnP Problem", IJCV 2009) restated in fp64, one 64-lane block per image.  The
 * steps, which are the definition (tests/epnp_ref.py restates them in numpy):
 *   1. Control points: c0 = the model's centroid, c_i = c0 + sqrt(lambda_i / pn) u_i for the
 *      eigenpairs (lambda_i, u_i) of sum (p - c0)(p - c0)^T in descending lambda.
 *      SIGN CONVENTION (this project's; cv2's comes out of its SVD and is not pinned): each u_i is
 *      signed so that its largest-magnitude component is positive, ties to the lowest index.
 *      Under keypoint noise the pose depends on this sign (1e-4 in the median at 1 px, far more
 *      in rare cases), so parity with
 *      cv2 is algorithmic (exact on exact data), not bitwise.
 *      REPEATED EIGENVALUES (a cube, a box with a square section, a can: the box corners and
 *      farthest points the product uses as keypoints): the axes inside the eigenspace are whatever
 *      the cyclic 3x3 Jacobi solver returns for this covariance, a dependence of the same kind as
 *      the sign.  EPnP is exact for any non-degenerate control basis, so the pose is exact on exact
 *      data; under noise it depends on the basis (another orthonormal basis of the eigenspace
 *      moves it by up to 0.3 at 1 to 3 px and is as close to the truth in the rms).
 *   2. Barycentric coordinates alpha of every model point, from inv([c1-c0 c2-c0 c3-c0]).
 *   3. M [2 pn][12]: point i, control point j gives (alpha_ij fu, 0, alpha_ij (uc - u_i)) and
 *      (0, alpha_ij fv, alpha_ij (vc - v_i)); v1..v4 = the eigenvectors of M^T M with the four
 *      smallest eigenvalues, smallest first (cyclic Jacobi).
 *   4. L [6][10] and rho [6] over the control-point pairs (0,1),(0,2),(0,3),(1,2),(1,3),(2,3),
 *      columns B11 B12 B22 B13 B23 B33 B14 B24 B34 B44 with the factor 2 on the mixed terms.
 *   5. cv2's three beta starts (find_betas_approx_1/2/3) by least squares on columns {0,1,3,6},
 *      {0,1,2}, {0..4}, with cv2's sign and zero rules.
 *   6. Exactly five Gauss-Newton iterations on the 6x4 system for each start (Householder QR).
 *   7. Per candidate: control points in the camera frame sum beta_k v_k, points alpha . ccs,
 *      everything negated if the first point's z < 0; Arun/Horn: R = U V^T from the SVD of
 *      sum (pc - mean)(pw - mean)^T (one-sided Jacobi), third row negated if det R < 0,
 *      t = mean pc - R mean pw; error = the mean Euclidean reprojection distance in px.
 *      A candidate whose camera-frame points are coplanar or collinear (smallest singular value
 *      <= 1e-10 of the largest) has no rotation: its error is +inf.
 *   8. cv2's strict choice: N = 1; N = 2 if err2 < err1; N = 3 if err3 < err_N.  No refinement.
 *   9. Degenerate inputs give a finite answer, never NaN: status PV_EPNP_DEGENERATE,
 *      Rt = [I | 0], rt6 = 0 when the model's smallest PCA eigenvalue is <= 1e-12 of its largest
 *      (planar or collinear model), or when the chosen candidate's error or any value of its
 *      pose is not finite (NaN / Inf keypoints; keypoints that all coincide, as the all-zero
 *      keypoints of an absent class do).
 *      THIN MODELS: on exact projections every candidate is the true cloud, whose Arun matrix has
 *      singular values that scale like the PCA eigenvalues, so step 7's 1e-10 decides before the
 *      1e-12 here: a model whose eigenvalue ratio is below about 1e-10 loses all three candidates
 *      and is DEGENERATE (OK and exact at a ratio >= 1e-9, DEGENERATE at <= 1e-11, either between).
 *      Keypoint noise lifts the candidates off their plane: at a ratio of 1e-11, noise of
 *      0.001 px leaves four images in five DEGENERATE, 0.01 px one in five, 1 px none.  At 1 px
 *      only the 1e-12 planar gate is left: OK at 1e-11, DEGENERATE at 1e-13.  In between (0.003 to
 *      0.3 px) about one image in 400 loses one or two candidates to step 7 and another wins.
 * pn >= 6: with fewer points 2 pn < 12 and M^T M's null space has more than one dimension
 * whatever the data, so the result would depend on the eigen solver's choice of basis.
 * Sums over the points run in index order; two runs on the same input are bit-equal. */
#define PV_EPNP_OK 0
#define PV_EPNP_DEGENERATE 1
#define PV_EPNP_MIN_POINTS 6
#define PV_EPNP_MAX_POINTS 64

typedef struct pv_epnp_batch {
    int32_t b, pn;            /* images; points per image, 6 <= pn <= 64 */
    const float  *pts2d;      /* f32 [b][pn][2], or NULL when pts2d64 is given */
    const double *pts2d64;    /* optional f64 [b][pn][2], used instead of pts2d */
    const double *pts3d;      /* f64 [pn][3], image i at pts3d + i * pts3d_stride (0 = shared) */
    const double *K;          /* f64 [3][3],  image i at K + i * K_stride (0 = shared) */
    int64_t pts3d_stride, K_stride;   /* in doubles */
} pv_epnp_batch;

typedef struct pv_epnp_diag { /* optional device outputs, any may be NULL */
    int32_t *status;          /* [b] PV_EPNP_OK / PV_EPNP_DEGENERATE */
    int32_t *n_used;          /* [b] 1, 2 or 3: which beta approximation won */
    double  *cand_err;        /* [b][3] the three candidates' mean reprojection errors, px */
} pv_epnp_diag;

/* Rt f64 [b][3][4] = [R | t] and / or rt6 f64 [b][6] = (cv2.Rodrigues(R), t); one may be NULL. */
int pv_epnp(const pv_epnp_batch *batch /* host */, double *Rt, double *rt6, const pv_epnp_diag *diag /* host, or NULL */,
            pv_stream_t stream);

/* ---- 2. [rvec | t] -> [Rodrigues(rvec) | t] ---------------------------------------------------
 * rt6 f64 [b][6] (e.g. pv_uncertainty_pnp_refine's result) -> Rt f64 [b][3][4]. */
int pv_rt6_to_Rt(const double *rt6, double *Rt, int32_t b, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVPOSE_H_ */
