/* pvshade.h -- C ABI of libpvshade.so: colour frames from vertex-coloured meshes, on the device.
 *
 * What pvrender.h leaves out: the picture itself.  (meshes with per-vertex colours, poses, cameras,
 * lights) -> u8 RGB frames with Lambert shading, and with them the label, instance, depth and face
 * maps of the same z-buffer (pv_shade_render); smooth vertex normals for a mesh table
 * (pv_shade_normals).  The reference gets its frames from Blender and OpenGL (render_utils.py,
 * opengl_render_backend.py); LINEMOD and YCB models carry per-vertex colours, which is what this
 * library draws.  The image and the label map are a ready bank for pv_compose_apply (pvcompose.h).
 * A library of its own: nothing here needs the other nine, and their export lists do not change.
 * It includes no other header of this project: the projection and coverage rules of pvrender.h are
 * restated below on purpose, so the two libraries stay apart.  This header defines the semantics;
 * tests/shade_ref.py restates them in numpy.
 *
 * Conventions (those of pvrender.h):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below; nothing
 *     calls exit();
 *   - every bad argument (a NULL descriptor, a negative size, H or W outside 1..2^20, znear <= 0 or
 *     NaN, no output requested, a NULL input, NULL lights, an unknown kind, a negative stride,
 *     total_inst * max_faces >= 2^32, a workspace that is NULL or too small) is rejected on the
 *     host before any pointer is touched; b == 0 is success; zero instances is success and still
 *     writes the background into the outputs;
 *   - every index read from device memory (model ids, offsets, face indices, instance ranges, the
 *     z-buffer's own slots) is checked against the bounds the host vouches for before it is used;
 *   - there is no CPU path.
 *
 * OUT OF SCOPE: a specular term (powf cannot be restated bit for bit), textures and materials, and
 * anti-aliasing (pv_compose_finish's blur is the softening step).
 */
#ifndef PVSHADE_H_
#define PVSHADE_H_

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

/* element kind of a label map: the values and the names of pvrender.h (an identical definition) */
#ifndef PV_LABEL_I64
#define PV_LABEL_I64 0
#define PV_LABEL_U8 1
#define PV_LABEL_I32 2
#endif

#define PV_SHADE_SUBPIXEL_BITS 8      /* the snap: 1/256 px */
#define PV_SHADE_MAX_SNAP 536870912   /* 2^29: a vertex snapped beyond it drops its triangles */
#define PV_SHADE_MAX_DIM 1048576      /* 2^20: H and W */
#define PV_SHADE_LIGHT_DOUBLES 9      /* direction (3), ambient rgb (3), diffuse rgb (3) */

/* The meshes: pv_render_meshes' fields, and per vertex a colour and (optionally) a normal. */
typedef struct pv_shade_meshes {
    const float *verts;        /* f32 [total_v][3], all models concatenated */
    const int32_t *vert_off;   /* i32 [nmodels + 1]: model m is rows [vert_off[m], vert_off[m+1]) */
    const int32_t *faces;      /* i32 [total_f][3], indices local to the model */
    const int32_t *face_off;   /* i32 [nmodels + 1] */
    const uint8_t *colors;     /* u8 [total_v][3]: r, g, b of each vertex */
    const double *normals;     /* optional f64 [total_v][3], model frame; NULL = flat shading */
    int32_t nmodels, total_v, total_f;
    int32_t max_verts, max_faces;   /* host-vouched bounds: a larger model's instances are skipped */
    int32_t reserved_;
} pv_shade_meshes;

/* ---- 1. pv_shade_normals ------------------------------------------------------------------------
 * Smooth vertex normals, fp64, every operation rounded (no contraction).  For vertex v of model m:
 *   N = the sum over the model's faces f = (i0, i1, i2) that name v, in ascending face index, of
 *       cross(p1 - p0, p2 - p0)       (area-weighted, not normalised; p the f32 vertices as f64)
 *   with cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx).  A face naming v more than
 *   once counts once; a face with an index outside [0, the model's vertex count) is skipped.
 *   L = sqrt((Nx Nx + Ny Ny) + Nz Nz);  normals_out[vert_off[m] + v] = N / L, or (0, 0, 0) when L is
 *   zero or not finite -- which pv_shade_render reads as "use the face normal".
 * The order of the sum is fixed, so the result does not depend on the launch order; no
 * floating-point atomics.  A model whose vertex or face range is not 0 <= lo <= hi <= total, or that
 * has more than max_verts vertices or max_faces faces, is skipped: its rows are not written.
 * meshes->colors and meshes->normals are not read.  normals_out: 8-byte aligned f64 [total_v][3]. */
int pv_shade_normals(const pv_shade_meshes *meshes /* host */, double *normals_out, pv_stream_t stream);

/* ---- 2. pv_shade_render -------------------------------------------------------------------------
 * Semantics (the definition).  Rules 1 to 5 and 7 are pvrender.h's, word for word:
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
 *  6. The z-buffer is one 64-bit integer minimum per pixel over (f32 depth bits << 32 | slot) with
 *     slot = local instance index * max_faces + face index (the face's index within its model); the
 *     host rejects total_inst * max_faces >= 2^32 with PV_EINVAL.  Equal f32 depths therefore go to
 *     the lower slot: the lower instance, then the lower face.  Depths are positive, so their bit
 *     patterns order as they do; an integer minimum does not depend on the order it is taken in, so
 *     every run gives the same bits whatever the launch order.  No floating-point atomics.  label,
 *     inst, depth and won are bit-identical to pv_render_labels' on the same inputs.
 *  7. An instance is skipped whole, writing nothing, if its model_id is outside [0, nmodels), its
 *     model's vertex or face range is not 0 <= lo <= hi <= total, its model has more than max_verts
 *     vertices or max_faces faces, its pose has a non-finite entry, or its label is outside 1..255.
 *     An image whose instance range (inst_off) is not 0 <= lo <= hi <= total_inst has no instances.
 *  8. Shading is deferred: one pass over the pixels after the z-buffer is final, in fp64, every
 *     operation rounded.  The pass re-reads the winning face's three snapped vertices and their
 *     camera-frame X, Y, Z; vertices 1 and 2 -- with their colours and normals -- are swapped as
 *     in rule 4.  With the edge values w_i at the sample (rule 5) and q_i = 1.0 / Z_i:
 *       a_i = (double)w_i q_i,   s = (a0 + a1) + a2,   beta_i = a_i / s;
 *       colour, per channel k:   c = (beta0 c0 + beta1 c1) + beta2 c2     (c_i the u8 as f64);
 *       face normal:             n_f = cross(P1 - P0, P2 - P0) with P_i = (X_i, Y_i, Z_i) and cross
 *                                as in pv_shade_normals, negated if dot(n_f, P0) > 0, so it faces
 *                                the camera for either winding; dot(a, b) = (ax bx + ay by) + az bz;
 *       with `normals` given:    n_m = (beta0 n0 + beta1 n1) + beta2 n2 per component; if n_m is
 *                                not (0, 0, 0): n = R n_m, each row as (R_0 x + R_1 y) + R_2 z (the
 *                                projection's order), negated if dot(n, n_f) < 0;
 *       otherwise                n = n_f;
 *       cos = dot(n, l) / (|n| |l|),  |a| = sqrt((ax ax + ay ay) + az az),  l = lights[0..3);
 *       d = cos if cos > 0, else 0 (a NaN gives 0); d = 0 if |n| or |l| is zero or not finite;
 *       value = c (ambient_k + diffuse_k d),  ambient = lights[3..6), diffuse = lights[6..9);
 *       image = (u8) rint(value) (ties to even) clamped to 0..255; a NaN gives 0.
 *     A background pixel gets the background image's pixel, or bg_color without one.
 *  9. Diagnostics: the winning face per pixel and each instance's won-pixel count. */
typedef struct pv_shade_batch { /* pv_render_batch's fields */
    int32_t b, H, W;
    int32_t ninst;             /* instances per image when inst_off is NULL: image i owns [i ninst, (i+1) ninst) */
    int32_t total_inst;        /* rows of model_id / label / pose; b * ninst when inst_off is NULL */
    int32_t label_kind;        /* PV_LABEL_* of pv_shade_out.label */
    const int32_t *inst_off;   /* optional i32 [b + 1]: image i owns instances [inst_off[i], inst_off[i+1]) */
    const int32_t *model_id;   /* i32 [total_inst] */
    const int32_t *label;      /* i32 [total_inst], 1..255: the value written to the label map */
    const double *pose;        /* f64 [total_inst][3][4] = [R | t] */
    const double *K;           /* f64 [3][3], image i at K + i * K_stride (0 = shared) */
    int64_t K_stride;          /* in doubles */
    double znear;              /* > 0 */
} pv_shade_batch;

typedef struct pv_shade_lights {
    const double *lights;      /* required: f64 [.][9] = direction towards the light in the camera frame,
                                * ambient rgb, diffuse rgb; image i at lights + i * lights_stride */
    int64_t lights_stride;     /* in doubles; 0 = shared */
    const uint8_t *background; /* optional u8 image with bg_strides; NULL = bg_color everywhere */
    int64_t bg_strides[4];     /* element strides of [b][H][W][3]; bg_strides[0] == 0 = shared */
    uint8_t bg_color[3];
    uint8_t pad_[5];
} pv_shade_lights;

typedef struct pv_shade_out { /* any may be NULL, but not all of image, label, inst, depth and face */
    uint8_t *image;            /* u8, logical [b][H][W][3] with image_strides: a CHW tensor is a view */
    int64_t image_strides[4];  /* element strides, >= 0; overlapping elements are the caller's error */
    void *label;               /* label_kind [b][H][W]; 0 = background */
    int32_t *inst;             /* i32 [b][H][W]: the winner's index within its image; -1 = background */
    float *depth;              /* f32 [b][H][W]; +inf = background */
    int32_t *face;             /* i32 [b][H][W]: the winning face's index within its model; -1 = background */
    int32_t *won;              /* i32 [total_inst]: pixels the instance owns in the final maps */
} pv_shade_out;

/* total_iv = total_inst * max_verts (the projected vertices' slots); 0 for bad sizes */
size_t pv_shade_workspace_size(int32_t b, int32_t H, int32_t W, int64_t total_iv, int32_t total_inst);

/* workspace: 256-byte aligned device memory of at least pv_shade_workspace_size(...) bytes,
 * owned by the call until it has run.  It need not be cleared: the call initialises every key,
 * record and count it reads, and writes nothing but its outputs and workspace[0, size). */
int pv_shade_render(const pv_shade_meshes *meshes /* host */, const pv_shade_batch *batch /* host */,
                    const pv_shade_lights *lights /* host */, const pv_shade_out *out /* host */,
                    void *workspace, size_t workspace_bytes, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVSHADE_H_ */
