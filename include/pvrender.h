/* pvrender.h -- C ABI of libpvrender.so: ground truth from a pose, on the device.
 *
 * The direction the other three libraries lack: (meshes, poses, cameras) -> label map, instance
 * map and depth map through a z-buffer (pv_render_labels; the reference's
 * extend_utils/src/mesh_rasterization.cpp is a binary rasteriser for one object on the host),
 * and (label map, projected keypoints) -> the unit vector field (pv_vertex_field; the
 * reference's compute_vertex, tools/demo.py:58-71).  The outputs have the layouts
 * pv_ransac_voting_v3 and pv_estimate_voting_distribution_with_mean take for a multi-object
 * frame (include/pvvote.h: a label map, class c = label c + 1, channels [c vn, (c + 1) vn)).
 * A library of its own: nothing here needs the other three, and their export lists do not change.
 * This header defines the semantics; tests/render_ref.py restates them in numpy.
 *
 * Conventions (those of pvvote.h, pveval.h and pvpose.h):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below; nothing
 *     calls exit();
 *   - every bad argument (a NULL descriptor, a negative size, H or W outside 1..2^20, znear <= 0 or
 *     NaN, no output requested, a NULL input, an unknown kind, a negative stride, a workspace that
 *     is NULL or too small) is rejected on the host before any pointer is touched; b == 0 or zero
 *     instances is success (zero instances still writes the background into the outputs);
 *   - every index read from device memory (model ids, offsets, face indices, instance ranges) is
 *     checked against the bounds the host vouches for before it is used.
 */
#ifndef PVRENDER_H_
#define PVRENDER_H_

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

/* element kind of a label map; the values are PV_MASK_I64 / U8 / I32 of pvvote.h */
#define PV_LABEL_I64 0
#define PV_LABEL_U8 1
#define PV_LABEL_I32 2
/* element kind of the vector field (PV_VERTEX_F32 / F16 of pvvote.h) and of the keypoints */
#define PV_FIELD_F32 0
#define PV_FIELD_F16 1
#define PV_KP_F64 0
#define PV_KP_F32 1

#define PV_RENDER_SUBPIXEL_BITS 8      /* the snap: 1/256 px */
#define PV_RENDER_MAX_SNAP 536870912   /* 2^29: a vertex snapped beyond it drops its triangles */
#define PV_RENDER_MAX_DIM 1048576      /* 2^20: H and W */
#define PV_RENDER_SNAP_INVALID (-2147483647 - 1) /* snap_xy of a vertex that drops its triangles */

/* ---- 1. pv_render_labels ----------------------------------------------------------------------
 * Semantics (the definition):
 *  1. Projection, fp64, every operation rounded (no contraction), in this order:
 *       X = ((R00 x + R01 y) + R02 z) + t0, Y and Z alike with rows 1 and 2 of the pose;
 *       u = (fx X + s Y) / Z + cx,  v = (fy Y) / Z + cy
 *     with fx = K00, s = K01 (the skew is honoured), cx = K02, fy = K11, cy = K12; K's other
 *     entries are not read (row 2 is taken to be 0 0 1).  The pixel in column x, row y has its
 *     sample point at (x, y): keypoint coordinates index pixels directly, as in the reference's
 *     Projector.project / compute_vertex.
 *  2. Snap: sx = rint(256 u), sy = rint(256 v) (ties to even) as int32.
 *  3. A triangle is dropped whole -- there is no clipping -- if any vertex has Z < znear, a
 *     non-finite X, Y, Z, u or v, or |256 u| or |256 v| rounding beyond 2^29 (so every edge
 *     function stays inside int64: differences < 2^30, products < 2^60, sums < 2^61); if its snapped
 *     doubled area (x1-x0)(y2-y0) - (x2-x0)(y1-y0) is zero; or if one of its three indices is
 *     outside [0, the model's vertex count).
 *  4. Coverage is exact: a triangle with negative doubled area has its vertices 1 and 2 swapped
 *     (both windings rasterise; nothing is culled), then for each directed edge a -> b over
 *     (0,1), (1,2), (2,0) with d = b - a the int64 edge function at the sample p = (256 x, 256 y) is
 *     E = dx (py - ay) - dy (px - ax); the sample is covered iff for every edge E > 0, or E == 0
 *     and the edge is a left edge (dy < 0) or a top edge (dy == 0 and dx > 0): the D3D top-left
 *     rule with y down.  Two triangles sharing an edge cover each sample on it exactly once.
 *  5. Depth, perspective-correct in fp64: with w0 = E12, w1 = E20, w2 = E01 (the weights of
 *     vertices 0, 1, 2 after the swap) and q_i = 1.0 / Z_i,
 *       Z = 1.0 / ((((double)w0 q0 + (double)w1 q1) + (double)w2 q2) / (double)(w0 + w1 + w2))
 *     rounded to f32.  The smallest f32 depth wins the pixel.
 *  6. Equal f32 depths go to the lower instance index within the image; within an instance the
 *     winner does not matter (same label, same value).  The z-buffer is one 64-bit integer minimum
 *     per pixel over (f32 depth bits << 32 | instance index): depths are positive, so their bit
 *     patterns order as they do; an integer minimum does not depend on the order it is taken in, so
 *     every run gives the same bits whatever the launch order.  No floating-point atomics.
 *  7. An instance is skipped whole, writing nothing, if its model_id is outside [0, nmodels), its
 *     model's vertex or face range is not 0 <= lo <= hi <= total, its model has more than max_verts
 *     vertices or max_faces faces, its pose has a non-finite entry, or its label is outside 1..255.
 *     An image whose instance range (inst_off) is not 0 <= lo <= hi <= total_inst has no instances.
 *  8. Diagnostics (pv_render_out): the snapped vertices and each instance's won-pixel count. */
typedef struct pv_render_meshes {
    const float *verts;        /* f32 [total_v][3], all models concatenated */
    const int32_t *vert_off;   /* i32 [nmodels + 1]: model m is rows [vert_off[m], vert_off[m+1]) */
    const int32_t *faces;      /* i32 [total_f][3], indices local to the model */
    const int32_t *face_off;   /* i32 [nmodels + 1] */
    int32_t nmodels, total_v, total_f;
    int32_t max_verts, max_faces;   /* host-vouched bounds: a larger model's instances are skipped */
    int32_t reserved_;
} pv_render_meshes;

typedef struct pv_render_batch {
    int32_t b, H, W;
    int32_t ninst;             /* instances per image when inst_off is NULL: image i owns [i ninst, (i+1) ninst) */
    int32_t total_inst;        /* rows of model_id / label / pose; b * ninst when inst_off is NULL */
    int32_t label_kind;        /* PV_LABEL_* of pv_render_out.label */
    const int32_t *inst_off;   /* optional i32 [b + 1]: image i owns instances [inst_off[i], inst_off[i+1]) */
    const int32_t *model_id;   /* i32 [total_inst] */
    const int32_t *label;      /* i32 [total_inst], 1..255: the value written to the label map */
    const double *pose;        /* f64 [total_inst][3][4] = [R | t] */
    const double *K;           /* f64 [3][3], image i at K + i * K_stride (0 = shared) */
    int64_t K_stride;          /* in doubles */
    double znear;              /* > 0 */
} pv_render_batch;

typedef struct pv_render_out { /* any may be NULL, but not all of label, inst and depth */
    void *label;               /* label_kind [b][H][W]; 0 = background */
    int32_t *inst;             /* i32 [b][H][W]: the winner's index within its image; -1 = background */
    float *depth;              /* f32 [b][H][W]; +inf = background */
    int32_t *snap_xy;          /* i32 [total_inst][max_verts][2]: (sx, sy) of vertex v of instance g, or
                                * (PV_RENDER_SNAP_INVALID, same) for a vertex that drops its triangles;
                                * rows past the model's vertex count, and skipped instances, are not written */
    double *snap_z;            /* f64 [total_inst][max_verts]: the camera-frame Z, same rows */
    int32_t *won;              /* i32 [total_inst]: pixels the instance owns in the final maps */
} pv_render_out;

/* total_iv = total_inst * max_verts (the projected vertices' slots); 0 for bad sizes */
size_t pv_render_workspace_size(int32_t b, int32_t H, int32_t W, int64_t total_iv, int32_t total_inst);

/* workspace: 256-byte aligned device memory of at least pv_render_workspace_size(...) bytes,
 * owned by the call until it has run.  It need not be cleared: the call initialises every key,
 * record and count it reads, and writes nothing but its outputs and workspace[0, size). */
int pv_render_labels(const pv_render_meshes *meshes /* host */, const pv_render_batch *batch /* host */,
                     const pv_render_out *out /* host */, void *workspace, size_t workspace_bytes,
                     pv_stream_t stream);

/* ---- 2. pv_vertex_field -------------------------------------------------------------------------
 * For a pixel (x, y) of image i whose label is c + 1 with 0 <= c < ncls, and keypoint k of class
 * c at (kx, ky) = keypoints[i][c][k], in fp64 with every operation rounded:
 *     dx = kx - x, dy = ky - y, n = sqrt(dx dx + dy dy), if (n < 1e-3) n += 1e-3,
 *     vertex[i][y][x][c vn + k] = (dx / n, dy / n) rounded to f32 (for f16: that f32 rounded to f16)
 * which is compute_vertex.  Every other channel of that pixel, and every channel of a pixel whose
 * label is 0, negative or above ncls, is 0.  Every element of vertex is written, in one pass.
 * vertex_strides are element strides of [b][H][W][ncls vn][2], so both the contiguous tensor and
 * the network's [b][2 ncls vn][H][W] are views; overlapping elements are the caller's error. */
typedef struct pv_field_desc {
    const void *label;         /* label_kind [b][H][W] with label_strides (elements) */
    const void *keypoints;     /* kp_kind [b][ncls][vn][2], contiguous, 16-byte aligned */
    void *vertex;              /* vertex_kind, vertex_strides */
    int64_t label_strides[3];
    int64_t vertex_strides[5];
    int32_t label_kind;        /* PV_LABEL_* */
    int32_t kp_kind;           /* PV_KP_F64 / PV_KP_F32 */
    int32_t vertex_kind;       /* PV_FIELD_F32 / PV_FIELD_F16 */
    int32_t b, H, W, ncls, vn; /* 1 <= ncls, 1 <= vn; b == 0 is success */
} pv_field_desc;

int pv_vertex_field(const pv_field_desc *desc /* host */, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVRENDER_H_ */
