/* pvicp.h -- C ABI of libpvicp.so: depth pose refinement on the device, one Gauss-Newton step of a
 * projective point-to-plane ICP per call.
 *
 * pvbop.h reads the sensor's depth map to score a pose (VSD); this header uses it to improve one.  The
 * method is the render-and-compare ICP every RGB-D pipeline ends with (Chen and Medioni, "Object
 * modelling by registration of multiple range images"; the projective data association of Newcombe
 * et al., "KinectFusion"): pv_render_labels (pvrender.h) renders each pose alone into its own depth
 * map, the rendered map at pixel (x, y) and the sensor's map at the same pixel are the correspondence,
 * the normal comes from the rendered map, and pv_icp_iterate linearises, solves and updates the pose.
 * The loop (render, iterate, render, ...) is the caller's (pvnet_amd.icp.refine_depth).  Those sources
 * are cited, not copied: the arithmetic below is this project's definition, and tests/icp_ref.py
 * restates it in numpy float64 with every sum and product written out.  The device equals that
 * restatement bit for bit on every output.  A library of its own: nothing here needs another library
 * of this project, and no other library's export list changes.
 *
 * Conventions (those of pvbop.h and pvrender.h):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host, allocates nothing and
 *     reads nothing back, and issues exactly two launches, so N calls can sit in one hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below; nothing
 *     calls exit();
 *   - every bad argument is rejected on the host before anything is launched; b == 0 is success with
 *     no launch;
 *   - every index read from device memory (img_id) is checked against the bound the host vouches for
 *     (n_img) before it is used; a value outside it gives status PV_ICP_BAD_INPUT, never an error
 *     return;
 *   - all arithmetic is fp64 with every operation rounded: no contraction into FMA and no matrix
 *     instruction; sums run as the parentheses say; the divide and the square root are the correctly
 *     rounded ones; there is no transcendental anywhere (the rotation update is the Cayley map);
 *   - no floating-point atomics and no block that waits on another: the order of every sum (rule 4)
 *     depends on H and W alone, so every output is bit-identical from run to run;
 *   - a call writes nothing but its outputs and workspace[0, size), and the workspace need not be
 *     cleared: the call writes every word of it that it reads.
 */
#ifndef PVICP_H_
#define PVICP_H_

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

/* status[i] */
#define PV_ICP_RUNNING 0   /* a step was taken and was not small: call again */
#define PV_ICP_CONVERGED 1 /* a step was taken and was small: later calls leave this pose alone */
#define PV_ICP_FEW 2       /* fewer than min_count pixels were used: pose untouched */
#define PV_ICP_NOT_PD 3    /* a Cholesky pivot was not finite and > 0, or the step was not finite: pose untouched */
#define PV_ICP_BAD_INPUT 4 /* rule 0: pose untouched */

#define PV_ICP_NSUM 28      /* sums per pose: A's upper triangle (21), g (6), E (1) */
#define PV_ICP_RUN 4        /* consecutive pixels per lane (rule 4) */
#define PV_ICP_LANES 256    /* lanes per block (rule 4) */
#define PV_ICP_BLOCK 1024   /* pixels per block: PV_ICP_RUN * PV_ICP_LANES */
#define PV_ICP_MAX_DIM 1048576 /* largest H or W: 2^20, pvrender.h's */

#define PV_ICP_STAT_RMS 0
#define PV_ICP_STAT_ROT 1
#define PV_ICP_STAT_TRANS 2
#define PV_ICP_NSTAT 3

typedef struct pv_icp_batch {
    int32_t b;                 /* poses */
    int32_t n_img;             /* host: images in depth_test; every img_id is checked against it */
    int32_t H, W;              /* 1 .. PV_ICP_MAX_DIM each */
    int32_t min_count;         /* host: >= 0; a pose with fewer used pixels is PV_ICP_FEW */
    int32_t reserved_;         /* not read */
    const float *depth_test;   /* f32 [n_img][H][W]: the sensor's depth; 0, negative or non-finite = missing */
    const int32_t *img_id;     /* i32 [b], or NULL = image i for pose i */
    const float *depth_est;    /* f32 [b][H][W]: pose i rendered alone at its current value (+inf = background) */
    const double *K;           /* f64 [3][3], pose i at K + i*K_stride; K_stride 0 = shared */
    int64_t K_stride;
    double dist_max;           /* host: correspondences farther apart than this are rejected; >= 0, not NaN (+inf allowed) */
    double edge_max;           /* host: a rendered depth step larger than this is an edge; >= 0, not NaN (+inf allowed) */
    double lambda;             /* host: Levenberg damping, M = A + lambda diag(A); finite and >= 0 */
    double max_rot;            /* host: the largest rotation step |w|, radians to first order; > 0, not NaN (+inf allowed) */
    double max_trans;          /* host: the largest translation step |v|, depth units; > 0, not NaN (+inf allowed) */
    double eps_rot, eps_trans; /* host: a step with |w| <= eps_rot and |v| <= eps_trans converges; >= 0, not NaN */
} pv_icp_batch;

typedef struct pv_icp_state {
    double *pose;              /* f64 [b][3][4] = [R | t], in and out */
    int32_t *status;           /* i32 [b], in and out: the caller writes PV_ICP_RUNNING before the first call */
    int32_t *iters;            /* i32 [b], in and out: the caller writes 0 before the first call; +1 per step taken */
    int32_t *cnt;              /* i32 [b], out: pixels used */
    double *stats;             /* f64 [b][PV_ICP_NSTAT], out */
    double *neq;               /* f64 [b][PV_ICP_NSUM], out, or NULL: the normal equations before damping */
} pv_icp_state;

/* pv_icp_iterate: for pose i with status[i] != PV_ICP_CONVERGED (a pose whose status is
 * PV_ICP_CONVERGED is skipped: none of its outputs is written and its blocks exit after reading the
 * status), image j = img_id[i], ze = depth_est[i][y][x] and zt = depth_test[j][y][x] widened to f64:
 *
 * 0. Bad input.  status[i] = PV_ICP_BAD_INPUT, cnt[i] = 0, NaN in stats[i][.] and neq[i][.], pose and
 *    iters untouched, when: a pose entry is not finite; fx, s, cx, fy or cy is not finite; fx or fy is
 *    0; img_id[i] is outside [0, n_img).  The camera is pvrender.h rule 1's: fx = K00, s = K01,
 *    cx = K02, fy = K11, cy = K12; K's other entries are not read.
 *
 * 1. Back-projection, at any pixel (x, y) with rendered depth z:
 *        ay(y)    = (y - cy) / fy
 *        ax(x, y) = ((x - cx) - s * ay(y)) / fx
 *        P(x, y)  = (z * ax, z * ay, z)
 *    and Q = (zt * ax, zt * ay, zt) with the centre pixel's ax, ay.
 *
 * 2. The normal of the rendered surface:
 *        du = P(x+1, y) - P(x-1, y),  dv = P(x, y+1) - P(x, y-1)      (componentwise)
 *        m  = (du1 dv2 - du2 dv1,  du2 dv0 - du0 dv2,  du0 dv1 - du1 dv0)
 *        l2 = (m0 m0 + m1 m1) + m2 m2,   r = sqrt(l2),   n = (m0 / r, m1 / r, m2 / r)
 *
 * 3. A pixel is used iff 1 <= x <= W-2 and 1 <= y <= H-2; ze and the depths zl, zr, zu, zd of its four
 *    neighbours are finite and > 0 (as f32); |zl - ze|, |zr - ze|, |zu - ze|, |zd - ze| <= edge_max;
 *    zt is finite and > 0; l2 is finite and > 0; and with d = P - Q (componentwise),
 *    (d0 d0 + d1 d1) + d2 d2 <= dist_max * dist_max.  For a used pixel
 *        e = (n0 d0 + n1 d1) + n2 d2
 *        c = (P1 n2 - P2 n1,  P2 n0 - P0 n2,  P0 n1 - P1 n0)
 *        J = (c0, c1, c2, n0, n1, n2)
 *    and its 28 terms are T[q]: J_k J_l for k <= l in the order (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
 *    (q = 0 .. 20), J_k e (q = 21 .. 26) and e e (q = 27).  An unused pixel's terms are +0.
 *
 * 4. The order of the 28 sums.  Pixels are numbered p = y W + x and cut into nblk = ceil(H W / 1024)
 *    blocks of PV_ICP_BLOCK; lane t (0 .. 255) of block k owns the PV_ICP_RUN pixels
 *    p = 1024 k + 4 t + j, j = 0 .. 3 (pixels past H W are unused):
 *        L[t] = (((0 + T_0) + T_1) + T_2) + T_3                        (the lane's run)
 *        for o = 32, 16, 8, 4, 2, 1:  L[t] = L[t] + L[t + o] for every t with t mod 64 < o, at once
 *        S_w  = L[64 w], w = 0 .. 3                                    (a halving tree per 64 lanes)
 *        B_k  = ((S_0 + S_1) + S_2) + S_3                              (the block's partial)
 *        sum  = (..((0 + B_0) + B_1) + ..) + B_{nblk-1}                (increasing k)
 *    cnt is the integer count of used pixels.  neq[i][q] = sum_q.
 *
 * 5. Solve.  A is symmetric with A[k][l] = sum of J_k J_l, g[k] = sum_{21+k}, E = sum_27.
 *        rms = sqrt(E / (double)cnt), NaN when cnt is 0
 *    If cnt < min_count: status PV_ICP_FEW, stats (rms, NaN, NaN), pose and iters untouched.  Else
 *        M[k][k] = A[k][k] + lambda * A[k][k],   M[k][l] = A[k][l] for k != l
 *        for i = 0 .. 5, for j = 0 .. i:  s = M[i][j];  for k = 0 .. j-1: s = s - L[i][k] * L[j][k];
 *            j == i: the pivot s must be finite and > 0, L[i][i] = sqrt(s);  j < i: L[i][j] = s / L[j][j]
 *        for i = 0 .. 5:  s = g[i];  for k = 0 .. i-1: s = s - L[i][k] * z[k];   z[i] = s / L[i][i]
 *        for i = 5 .. 0:  s = z[i];  for k = i+1 .. 5: s = s - L[k][i] * y[k];   y[i] = s / L[i][i]
 *        xi = -y,  w = (xi0, xi1, xi2),  v = (xi3, xi4, xi5)
 *    A bad pivot or a non-finite xi entry: status PV_ICP_NOT_PD, stats (rms, NaN, NaN), pose and iters
 *    untouched.
 *
 * 6. Step limit.  rn = sqrt((w0 w0 + w1 w1) + w2 w2), tn = sqrt((v0 v0 + v1 v1) + v2 v2);  k = 1;
 *    if rn > max_rot: k = max_rot / rn;  if tn > max_trans and max_trans / tn < k: k = max_trans / tn.
 *
 * 7. Update, by the Cayley map of a = ((k w0) 0.5, (k w1) 0.5, (k w2) 0.5):
 *        q = (a0 a0 + a1 a1) + a2 a2,   den = 1 + q,   b = (2 a0, 2 a1, 2 a2)
 *        C[i][i] = ((1 - q) + b_i a_i) / den
 *        C[0][1] = (b0 a1 - b2) / den,  C[0][2] = (b0 a2 + b1) / den,  C[1][0] = (b1 a0 + b2) / den,
 *        C[1][2] = (b1 a2 - b0) / den,  C[2][0] = (b2 a0 - b1) / den,  C[2][1] = (b2 a1 + b0) / den
 *        R'[r][c] = (C[r][0] R[0][c] + C[r][1] R[1][c]) + C[r][2] R[2][c]
 *        t'[r]    = ((C[r][0] t[0] + C[r][1] t[1]) + C[r][2] t[2]) + k v_r
 *    C is a rotation by 2 atan|a| about a, so R' stays orthogonal to rounding.  pose[i] = [R' | t'],
 *    iters[i] += 1, stats (rms, rn, tn), and status PV_ICP_CONVERGED if rn <= eps_rot and
 *    tn <= eps_trans, else PV_ICP_RUNNING.
 *
 * Workspace: f64 [b][nblk][PV_ICP_NSUM] block partials, then i32 [b][nblk] block counts.
 *
 * Rejected on the host, nothing launched:
 *   PV_EINVAL      bt or st NULL; b, n_img, min_count or K_stride negative; H or W outside
 *                  1 .. PV_ICP_MAX_DIM; dist_max, edge_max, eps_rot or eps_trans negative or NaN; lambda
 *                  negative or not finite; max_rot or max_trans not > 0; (with b > 0) pose, status,
 *                  iters, cnt, stats, depth_est or K NULL; depth_test NULL with n_img > 0; b * nblk
 *                  beyond 2^31 - 1
 *   PV_EWORKSPACE  workspace NULL or smaller than pv_icp_workspace_size(b, H, W)
 *   PV_EALIGN      pose, stats, neq, K or workspace not 8-byte aligned; status, iters, cnt, img_id or a
 *                  depth map not 4-byte aligned
 * b == 0 is success with no launch. */
size_t pv_icp_workspace_size(int32_t b, int32_t H, int32_t W); /* host only; 0 if any is < 1 */
int pv_icp_iterate(const pv_icp_batch *batch /* host */, const pv_icp_state *state /* host */, void *workspace,
                   size_t workspace_bytes, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVICP_H_ */
