/* pvaugment.h -- C ABI of libpvaugment.so: PVNet's training augmentation, on the device.
 *
 * The step between a decoded u8 batch and the network's input that the reference does on the host,
 * image by image (lib/datasets/linemod_dataset.py LineModDatasetRealAug, lib/utils/data_utils.py):
 * rotate_instance (a rotation about the mask's centre), crop_resize_instance_v1 (a random scale and
 * a crop), crop_or_padding_to_fixed_size, torchvision's ColorJitter(0.1, 0.1, 0.05, 0.05), the
 * background replacement of the fuse synthesis, and the normalisation to the network's input.  The
 * reference resamples an image up to three times with cv2 and recomputes the vector field with
 * compute_vertex; here the three geometric steps are ONE affine map per image, applied once to the
 * image (bilinear) and to the label map (nearest), and the vector field is pv_vertex_field of
 * pvrender.h on the augmented label and the transformed keypoints.  A library of its own: nothing
 * here needs the other six, and their export lists do not change.  This header defines the
 * semantics; tests/augment_ref.py restates them in numpy.
 *
 * NOT A REPLAY OF THE REFERENCE.  The map is parametrised differently (angle, scale, the point the
 * foreground centroid lands on) and the draws come from the generator below, not from Python's
 * `random` or numpy's; a run does not reproduce the reference's random stream, only its family of
 * transforms.  The photometric steps run in the FIXED order brightness, contrast, saturation, hue;
 * torchvision's ColorJitter shuffles the order per call.
 *
 * Not in this header: Gaussian blur, additive noise and occlusion pasting, which are pvcompose.h's
 * (a library of its own, whose draw numbers start after PV_AUG_DRAWS).  Not in scope anywhere: flips
 * (they change the handedness of the pose, so the keypoints of a flipped image belong to no rigid
 * pose of the model), and reading or decoding files.
 *
 * Conventions (those of pvvote.h, pveval.h, pvpose.h, pvrender.h, pvmodel.h and pvloss.h):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below; nothing
 *     calls exit();
 *   - every bad argument (a NULL descriptor, a negative size or stride, a size outside
 *     1..PV_AUG_MAX_DIM, ncls outside 1..PV_AUG_MAX_CLASSES, an unknown kind or flag, a range that
 *     is not finite or not ordered, scale <= 0, margin outside [0, 0.5], a jitter outside its
 *     range, fill outside [0, 255], mean / std not finite or std <= 0, one image of the source, the
 *     label map or the background spanning more than 2^31 - 1 elements, a batch whose launch would
 *     reach 2^32 threads (b * ceil(Ho * ceil(Wo / 8) / 256) blocks of pv_augment_apply, b * ceil(H W / 8192)
 *     of pv_label_stats, above 2^24 - 1), a NULL or misaligned pointer, a workspace
 *     that is NULL, too small or misaligned when the contrast step needs it) is rejected on the
 *     host before any pointer is touched; b == 0 is success.
 *
 * Coordinates: x right, y down, a pixel's sample point is its integer coordinate (the renderer's
 * convention: no half-pixel offset).
 *
 * 1. pv_label_stats.  For image i, over the pixels with 1 <= label <= ncls:
 *      stats[i] = (count, sum x, sum y, xmin, ymin, xmax, ymax, 0);
 *    with no such pixel the box is (W, H, -1, -1).  Integers only (LDS integer adds, then global
 *    integer add / min / max): the result does not depend on any order.  All eight elements are
 *    written by the call, their initialisation included.
 *
 * 2. pv_augment_params.  The draws: with mix(z) the splitmix64 finaliser
 *      z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *    and G = 0x9E3779B97F4A7C15, all in uint64 arithmetic modulo 2^64,
 *      u(seed, n, k) = (mix(mix(mix(seed + G) + (n + 1) G) + (k + 1) G) >> 11) * 2^-53   in [0, 1)
 *    for sample n = state[1] + i and draw number k.  state = (seed, first sample index) is read
 *    and never written: a replayed graph gets fresh draws when the caller advances state[1] by b.
 *    Per image, in fp64, every operation rounded, with U(k; lo, hi) = lo + u_k (hi - lo):
 *      theta = U(0; rot_deg) * (pi / 180),  s = U(1; scale),
 *      t = ((margin + u_2 (1 - 2 margin)) (Wo - 1),  (margin + u_3 (1 - 2 margin)) (Ho - 1)),
 *      c = (sum x / count, sum y / count)  or  ((W - 1) / 2, (H - 1) / 2)  with no foreground,
 *      a = s cos(theta),  q = s sin(theta),
 *      fwd = [[a, -q, t_x - (a c_x - q c_y)],      = [sR | t - sR c],  R = [[cos, -sin], [sin, cos]]:
 *             [q,  a, t_y - (q c_x + a c_y)]]        what keypoints undergo; the centroid lands on t;
 *      d = a a + q q,  ia = a / d,  iq = q / d,
 *      inv = [[ ia, iq, -(ia f02 + iq f12)],       its closed-form inverse: what the sampler uses
 *             [-iq, ia,   iq f02 - ia f12 ]];
 *      color = (1 + jb (2 u_4 - 1), 1 + jc (2 u_5 - 1), 1 + js (2 u_6 - 1), jh (2 u_7 - 1))  as f32.
 *    The device's cos and sin may differ from a host libm in the last ulps; the draws do not.
 *
 * 3. pv_augment_apply.  Per output pixel (x, y) of image i, with M = inv[i]:
 *      sx = (M00 x + M01 y) + M02,  sy = (M10 x + M11 y) + M12      in fp64, every operation rounded.
 *    Label: with rx = rint(sx), ry = rint(sy) (ties to even), the source label at (rx, ry) when
 *    0 <= rx <= W - 1 and 0 <= ry <= H - 1, else 0.  EVERY RANGE CHECK IS MADE IN FP64 BEFORE ANY
 *    CONVERSION TO AN INTEGER, and a comparison with a NaN is false: a NaN, infinite or 1e300
 *    matrix reads nothing out of bounds and gives label 0 and colour `fill` everywhere.
 *    Colour, per channel, on the 0..255 scale in f32, every operation rounded: with fx = floor(sx),
 *    fy = floor(sy), wx = (float)(sx - fx), wy = (float)(sy - fy) and v00, v01, v10, v11 the taps
 *    at (fx, fy), (fx + 1, fy), (fx, fy + 1), (fx + 1, fy + 1), a tap outside the source being
 *    `fill`:
 *      top = v00 + wx (v01 - v00),  bot = v10 + wx (v11 - v10),  c = top + wy (bot - top);
 *    when -1 <= fx <= W - 1 and -1 <= fy <= H - 1 does not hold (no tap inside, or not finite)
 *    c = fill.  If a background is given and the output label is 0, c is the background's pixel.
 *    Then c = c * (1.0f / 255.0f) and, each step only if its flag is set, with clamp(v) =
 *    min(max(v, 0), 1), grey(r, g, b) = (0.299f r + 0.587f g) + 0.114f b and
 *    (beta, kappa, sigma, eta) = color[i]:
 *      brightness  c = clamp(beta c);
 *      contrast    c = clamp(kappa c + (1 - kappa) m),  m = (float)(S / (Ho Wo)),  S the f64 sum of
 *                  the f32 values grey(c) over the image's pixels after brightness;
 *      saturation  c = clamp(sigma c + (1 - sigma) grey(c));
 *      hue         (h, s, v) = rgb_to_hsv(c) as Python's colorsys defines it, h = h + eta,
 *                  h = h - floorf(h), c = hsv_to_rgb(h, s, v)   (sector 6 is sector 0).
 *    Output: (c - mean) * (1.0f / std) per channel, rounded to the output's kind.
 *
 *    The contrast mean is a reduction over the output.  S is an f64 sum in an order that depends on
 *    the shapes alone: a lane adds the greys of its PV_AUG_PIXELS consecutive pixels of a row in
 *    increasing x, the PV_AUG_THREADS lanes of a block combine in a halving tree, each block stores
 *    its partial to the workspace, and every block of the second pass adds its image's partials,
 *    lane t taking partials t, t + PV_AUG_THREADS, ... in increasing order and the lanes combining
 *    in the same tree.  No floating-point atomics and no block waits on another: two runs, and two
 *    replays of a captured graph, give the same bits.  Without PV_AUG_CONTRAST there is one pass
 *    and no workspace is needed.
 */
#ifndef PVAUGMENT_H_
#define PVAUGMENT_H_

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

/* element kind of a label map (the values of PV_LABEL_* of pvrender.h) */
#define PV_AUG_LABEL_I64 0
#define PV_AUG_LABEL_U8 1
#define PV_AUG_LABEL_I32 2
/* element kind of the output image (the values of PV_FIELD_* of pvrender.h) */
#define PV_AUG_F32 0
#define PV_AUG_F16 1
/* the photometric steps that run */
#define PV_AUG_BRIGHTNESS 1
#define PV_AUG_CONTRAST 2
#define PV_AUG_SATURATION 4
#define PV_AUG_HUE 8

#define PV_AUG_PIXELS 8          /* consecutive output pixels of a row per lane */
#define PV_AUG_THREADS 256       /* lanes per block */
#define PV_AUG_MAX_DIM 1048576   /* 2^20: H, W, Ho and Wo */
#define PV_AUG_MAX_CLASSES 1024  /* ncls */
#define PV_AUG_DRAWS 8           /* draw numbers 0..7: angle, scale, t_x, t_y, brightness, contrast, saturation, hue */

typedef struct pv_aug_label {
    const void *label;          /* label_kind [b][H][W], label_strides in elements, >= 0 */
    int64_t label_strides[3];
    int32_t label_kind;         /* PV_AUG_LABEL_* */
    int32_t b, H, W;            /* b == 0 is success */
} pv_aug_label;

typedef struct pv_aug_ranges {
    double rot_deg[2];          /* degrees, lo <= hi */
    double scale[2];            /* 0 < lo <= hi */
    double margin;              /* in [0, 0.5] */
    double jitter[4];           /* brightness, contrast, saturation in [0, 1], hue in [0, 0.5] */
    int32_t b, H, W, Ho, Wo;    /* source and output sizes */
    int32_t pad_;
} pv_aug_ranges;

typedef struct pv_aug_desc {
    const void *image;          /* u8, logical [b][H][W][3], image_strides (a CHW tensor is a view) */
    const void *label;          /* label_kind [b][H][W], label_strides */
    const double *inv;          /* f64 [b][2][3], pv_augment_params' */
    const float *color;         /* f32 [b][4] */
    const void *background;     /* optional u8, logical [b][Ho][Wo][3], background_strides; image stride 0: shared */
    void *out_image;            /* out_kind, logical [b][3][Ho][Wo], out_image_strides (channels-last is a view) */
    void *out_label;            /* label_kind [b][Ho][Wo], out_label_strides */
    int64_t image_strides[4];   /* all strides in elements, >= 0 */
    int64_t label_strides[3];
    int64_t background_strides[4];
    int64_t out_image_strides[4];
    int64_t out_label_strides[3];
    float fill[3];              /* on the 0..255 scale, in [0, 255] */
    float mean[3];              /* finite */
    float std[3];               /* finite, > 0 */
    int32_t label_kind;         /* PV_AUG_LABEL_* */
    int32_t out_kind;           /* PV_AUG_F32 / PV_AUG_F16 */
    int32_t flags;              /* PV_AUG_BRIGHTNESS | ... */
    int32_t b, H, W, Ho, Wo;
} pv_aug_desc;

/* Bytes of workspace of pv_augment_apply with PV_AUG_CONTRAST for these sizes; 0 for bad sizes.
 * The workspace is 256-byte aligned device memory, owned by the call until it has run.  It need
 * not be cleared: the first pass writes every partial the second reads, and the call writes nothing
 * but its two outputs and workspace[0, size). */
size_t pv_augment_workspace_size(int32_t b, int32_t Ho, int32_t Wo);

/* stats: i64 [b][8], 8-byte aligned. */
int pv_label_stats(const pv_aug_label *desc /* host */, int32_t ncls, int64_t *stats, pv_stream_t stream);

/* stats: pv_label_stats'; state: u64 [2] = (seed, first sample index), read only;
 * fwd, inv: f64 [b][2][3]; color: f32 [b][4].  One thread per image. */
int pv_augment_params(const pv_aug_ranges *ranges /* host */, const int64_t *stats, const uint64_t *state,
                      double *fwd, double *inv, float *color, pv_stream_t stream);

/* The warp, the background, the photometric chain and the normalisation.  The workspace may be
 * NULL when desc->flags has no PV_AUG_CONTRAST. */
int pv_augment_apply(const pv_aug_desc *desc /* host */, void *workspace, size_t workspace_bytes, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVAUGMENT_H_ */
