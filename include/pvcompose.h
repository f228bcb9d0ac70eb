/* pvcompose.h -- C ABI of libpvcompose.so: multi-object training frames composed on the device.
 *
 * What pvaugment.h leaves out and the reference does on the host: the "fuse" synthesis
 * (lib/datasets/linemod_dataset.py, lib/utils/data_utils.py: the objects of several single-object
 * frames cut out by their masks and pasted over one background, later ones over earlier ones), random
 * erasing inside an object's box, Gaussian blur and additive noise.  From a bank of single-object
 * frames to a batch of multi-object, occluded, blurred, noisy u8 frames with a label map: the form
 * pv_augment_apply, pv_vertex_field, pv_loss_forward and the multi-object voting take.  A library of
 * its own: nothing here needs the other seven, and their export lists do not change.  This header
 * defines the semantics; tests/compose_ref.py restates them in numpy.
 *
 * NOT A REPLAY OF THE REFERENCE.  The placement is parametrised differently (an integer shift that puts
 * the box's centre on a drawn target) and the draws come from pvaugment.h's generator, not from
 * Python's `random` or numpy's; a run does not reproduce the reference's random stream, only its family
 * of operations.  Flips stay out (a flipped image belongs to no rigid pose), and so does reading files.
 *
 * Conventions (pvaugment.h's):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph; no entry needs a workspace;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below;
 *   - every bad argument (a NULL descriptor, a negative size or stride, H, W, Ho or Wo outside
 *     1..PV_CMP_MAX_DIM, N < 1, S outside 1..PV_CMP_MAX_SLOTS, E outside 0..PV_CMP_MAX_ERASE, ncls
 *     outside 1..PV_CMP_MAX_CLASSES or above 255 with u8 labels, an unknown kind, fill outside 0..255,
 *     a range listed under pv_compose_params, a half-kernel that is not finite or negative, one frame of
 *     any operand spanning more than 2^31 - 1 elements, a batch whose launch would reach 2^32 threads
 *     (b * ceil(Ho * ceil(Wo / 8) / 256) blocks of pv_compose_apply, b * ceil(H / T) * ceil(W / T) of
 *     pv_compose_finish with T = PV_CMP_TILE, above 2^24 - 1), a NULL or misaligned pointer, E > 0
 *     without `erase`, the output of pv_compose_finish at its input's address) is rejected on the host
 *     before any pointer is touched; b == 0 is success;
 *   - strides are in elements and >= 0; x right, y down, a pixel's sample point is its integer
 *     coordinate.
 * Everything below is integer or fixed-order f32 arithmetic, and fp64 in pv_compose_params, with no
 * transcendental on the device: numpy reproduces every output bit for bit.
 *
 * 1. pv_compose_apply.  pick[f][s] = (src, src_label, cls, x0, y0, x1, y1, 0), the box inclusive, in
 *    the source frame; shift[f][s] = (dx, dy); erase[f][e] = (x0, y0, x1, y1), inclusive, in output
 *    coordinates.  Slot s of frame f is LIVE iff 0 <= src < N and 1 <= cls <= ncls.  Its box is the
 *    given box clipped to the source frame, (max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1));
 *    a live slot whose clipped box is empty (x1 < x0 or y1 < y0 after clipping) paints nothing.
 *    Output pixel (x, y) BELONGS TO slot s iff s is live, (x - dx, y - dy) lies in the clipped box and
 *    the source label of frame src there equals src_label (compared as 64-bit integers).
 *      - The pixel goes to the belonging slot of highest s (later slots on top): that source pixel's
 *        colour, label cls, instance s + 1.
 *      - With no belonging slot: the background's pixel, or `fill` without a background; label 0,
 *        instance 0.
 *      - A pixel inside any eraser box (x0 <= x <= x1 and y0 <= y <= y1; x1 < x0 or y1 < y0 is the
 *        empty box) is then `fill`, label 0, instance 0.
 *    visible[f][s] = the number of output pixels of frame f whose final instance is s + 1: LDS integer
 *    adds, then global integer adds, exact whatever the order; the call initialises it.
 *    pick, shift and erase are device data the host cannot validate.  EVERY RANGE CHECK IS MADE BEFORE
 *    ANY ADDRESS IS FORMED, in 64-bit integer arithmetic that cannot overflow: the shifted box
 *    (x0 + dx .. x1 + dx) is clipped to the output frame first, and only a pixel inside it forms
 *    x - dx.  An INT32_MIN or INT32_MAX shift, src = N, an inverted box, an eraser with x1 < x0 read
 *    and write nothing out of bounds and give background, or nothing.
 *
 * 2. pv_compose_params.  One thread per frame.  u(seed, n, k) is pvaugment.h's (the same mix and G,
 *    sample n = state[1] + f); state = (seed, first sample index) is read and never written.  Draw
 *    numbers start at PV_CMP_DRAW0 = 64, so they are disjoint from PV_AUG_DRAWS: one state can drive
 *    both libraries.  In fp64, every operation rounded, rint to nearest even, U(k; lo, hi) =
 *    lo + u_k (hi - lo).  A slot that is live with a non-empty clipped box (x0..x1, y0..y1), draws
 *    u_j = u(seed, n, 64 + 8 s + j):
 *      tx = (margin + u_0 (1 - 2 margin)) (Wo - 1),  dx = (int) rint(tx - (x0 + x1) / 2),
 *      ty = (margin + u_1 (1 - 2 margin)) (Ho - 1),  dy = (int) rint(ty - (y0 + y1) / 2):
 *    the box's centre lands on the drawn target.  Any other slot gets (0, 0).
 *    Eraser e, draws u_j = u(seed, n, 192 + 8 e + j), targets slot e mod S.  If that slot got no shift
 *    by the rule above it is the empty box (0, 0, -1, -1).  Else with bw = x1 - x0 + 1, bh = y1 - y0 + 1:
 *      w = max(1, (int) rint(U(0; erase_frac) bw)),  h = max(1, (int) rint(U(1; erase_frac) bh)),
 *      left = x0 + dx + (int) floor(u_2 (bw - w + 1)),  top = y0 + dy + (int) floor(u_3 (bh - h + 1)),
 *      erase = (left, top, left + w - 1, top + h - 1):   inside the slot's shifted box.
 *    The finish, draws u_j = u(seed, n, 256 + j):
 *      ksel = u_0 < p_blur ? 1 + min(3, (int) floor(4 u_1)) : 0,
 *      amp = (float)(noise[0] + u_2 (noise[1] - noise[0])).
 *    Rejected on the host: margin outside [0, 0.5]; erase_frac not 0 < lo <= hi <= 1; p_blur outside
 *    [0, 1]; noise not 0 <= lo <= hi, or not finite.
 *
 * 3. pv_compose_finish.  Per frame f the blur's size is k = 2 j + 1 with j = ksel[f] for ksel[f] in
 *    0..4; any other ksel[f] is treated as 0.  w[j][0..j] are the half-kernel's f32 weights, made on
 *    the host (the device evaluates no exp).  r(i) is the reflect-101 index map of a length n: with
 *    p = 2 (n - 1) and m = i mod p in 0..p - 1, r(i) = m < n ? m : p - m; n = 1 maps everything to 0.
 *    Per channel, in f32, every operation rounded, v the input:
 *      horizontal  a = v(x, y) for j = 0; else a = w[j][0] v(x, y), then for t = 1..j in this order
 *                  a = a + w[j][t] (v(r(x - t), y) + v(r(x + t), y));
 *      vertical    the same over y on the horizontal result;
 *      noise       key = mix(mix(seed + G) + (n + 1) G),  n = state[1] + f,  p = y W + x,
 *                  z = mix(key + (2^40 + 3 p + ch + 1) G),  s = the sum of z's four 16-bit fields,
 *                  t = (float)(s - 131070) * 2^-16   (exact; standard deviation 0.577),
 *                  c = a + amp[f] * t;
 *      output      (uint8) rint(fmin(fmax(c, 0), 255))   (ties to even; fmax drops a NaN).
 *    With ksel = 0 and amp = 0 the output equals the input exactly.  A block takes a PV_CMP_TILE x
 *    PV_CMP_TILE tile of one frame: the tile with a 4-pixel halo as u8 into LDS once, the horizontal
 *    pass to LDS as f32, the vertical pass from there.
 */
#ifndef PVCOMPOSE_H_
#define PVCOMPOSE_H_

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

/* element kind of a label map (the values of PV_AUG_LABEL_* of pvaugment.h) */
#define PV_CMP_LABEL_I64 0
#define PV_CMP_LABEL_U8 1
#define PV_CMP_LABEL_I32 2

#define PV_CMP_PIXELS 8          /* consecutive output pixels of a row per lane of pv_compose_apply */
#define PV_CMP_THREADS 256       /* lanes per block */
#define PV_CMP_TILE 32           /* pv_compose_finish: a block's tile is PV_CMP_TILE x PV_CMP_TILE pixels */
#define PV_CMP_HALO 4            /* the widest half-kernel */
#define PV_CMP_MAX_SLOTS 16      /* S */
#define PV_CMP_MAX_ERASE 8       /* E */
#define PV_CMP_MAX_DIM 32768     /* 2^15: H, W, Ho and Wo */
#define PV_CMP_MAX_CLASSES 1024  /* ncls */
#define PV_CMP_DRAW0 64          /* first draw number: slots 64 + 8 s + j, erasers 192 + 8 e + j, finish 256 + j */

typedef struct pv_cmp_desc {
    const void *image;          /* u8, logical [N][H][W][3], image_strides (a CHW tensor is a view) */
    const void *label;          /* label_kind [N][H][W], label_strides */
    const int32_t *pick;        /* i32 [b][S][8] */
    const int32_t *shift;       /* i32 [b][S][2] */
    const int32_t *erase;       /* i32 [b][E][4]; may be NULL when E == 0 */
    const void *background;     /* optional u8, logical [b][Ho][Wo][3], background_strides; frame stride 0: shared */
    void *out_image;            /* u8, logical [b][Ho][Wo][3], out_image_strides */
    void *out_label;            /* label_kind [b][Ho][Wo], out_label_strides */
    void *out_instance;         /* optional label_kind [b][Ho][Wo], out_instance_strides */
    int32_t *visible;           /* i32 [b][S] */
    int64_t image_strides[4];   /* all strides in elements, >= 0 */
    int64_t label_strides[3];
    int64_t background_strides[4];
    int64_t out_image_strides[4];
    int64_t out_label_strides[3];
    int64_t out_instance_strides[3];
    int32_t label_kind;         /* PV_CMP_LABEL_* */
    int32_t N, H, W;            /* the bank */
    int32_t b, Ho, Wo;          /* the output; b == 0 is success */
    int32_t S, E, ncls;
    int32_t fill[3];            /* 0..255 */
    int32_t pad_;
} pv_cmp_desc;

typedef struct pv_cmp_ranges {
    double margin;              /* in [0, 0.5] */
    double erase_frac[2];       /* 0 < lo <= hi <= 1 */
    double p_blur;              /* in [0, 1] */
    double noise[2];            /* 0 <= lo <= hi, finite */
    int32_t b, N, H, W, Ho, Wo, S, E, ncls;
    int32_t pad_;
} pv_cmp_ranges;

typedef struct pv_cmp_finish {
    const void *image;          /* u8, logical [b][H][W][3], image_strides */
    void *out;                  /* u8, logical [b][H][W][3], out_strides; must not alias image */
    const int32_t *ksel;        /* i32 [b] */
    const float *amp;           /* f32 [b] */
    const uint64_t *state;      /* u64 [2] = (seed, first sample index), read only */
    int64_t image_strides[4];
    int64_t out_strides[4];
    float w[5][5];              /* host data: w[j][t], t <= j, finite and >= 0; the rest is not read */
    int32_t b, H, W;
    int32_t pad_;
} pv_cmp_finish;

int pv_compose_apply(const pv_cmp_desc *desc /* host */, pv_stream_t stream);

/* pick: i32 [b][S][8]; state: u64 [2], read only; shift: i32 [b][S][2]; erase: i32 [b][E][4], may be
 * NULL when E == 0; ksel: i32 [b]; amp: f32 [b]. */
int pv_compose_params(const pv_cmp_ranges *ranges /* host */, const int32_t *pick, const uint64_t *state,
                      int32_t *shift, int32_t *erase, int32_t *ksel, float *amp, pv_stream_t stream);

int pv_compose_finish(const pv_cmp_finish *desc /* host */, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVCOMPOSE_H_ */
