/* pvloss.h -- C ABI of libpvloss.so: PVNet's training objective and its gradient, on the device.
 *
 * The comparison of the network's two outputs with the two ground-truth maps of pvrender.h: the
 * cross-entropy of the segmentation logits (the reference's nn.CrossEntropyLoss(reduce=False) and its
 * per-image mean, tools/train_linemod.py), the mask-weighted smooth-L1 of the vector field (the
 * reference's lib/utils/net_utils.py smooth_l1_loss(..., normalize=True, reduce=False)) and the
 * counts behind lib/utils/net_utils.py compute_precision_recall, generalised from one object to a
 * label map of ncls classes (class c = label c + 1, channels [c vn, (c + 1) vn), as pvvote.h and
 * pvrender.h lay a multi-object frame out).  pv_loss_forward gives the per-image losses and counts;
 * pv_loss_backward recomputes from the same inputs and writes the gradients of the two predictions.
 * A library of its own: nothing here needs the other five, and their export lists do not change.
 * This header defines the semantics; tests/loss_ref.py restates them in numpy f64.
 *
 * Conventions (those of pvvote.h, pveval.h, pvpose.h, pvrender.h and pvmodel.h):
 *   - pointers are device pointers unless a comment says host;
 *   - every call is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below; nothing
 *     calls exit();
 *   - every bad argument (a NULL descriptor, both terms absent, a negative size or stride, H or W
 *     outside 1..PV_LOSS_MAX_DIM, ncls outside 1..PV_LOSS_MAX_CLASSES, vn < 1, an unknown kind,
 *     sigma <= 0 or NaN, a NULL input or output of a term that is present, a misaligned pointer, a
 *     workspace that is NULL, too small or misaligned) is rejected on the host before any pointer
 *     is touched; b == 0 is success.
 *
 * Semantics, for image i and pixel p = (y, x), with L = label[i][p]:
 *
 *  1. loss_seg[i] = (1 / (H W)) sum_p ce(p).  For 0 <= L <= ncls,
 *       ce(p) = (m + logf(sum_c expf(seg[i][c][p] - m))) - seg[i][L][p],  m = max_c seg[i][c][p];
 *     for any other L (an ignored pixel) ce(p) = 0, and the mean still divides by H W.
 *  2. loss_vertex[i] = S_i / (2 vn fg_i + 1e-3).  A pixel is foreground if 1 <= L <= ncls, fg_i
 *     counts them, and with c = L - 1
 *       S_i = sum_{p foreground} sum_{k < vn} sum_{j < 2} sl1(vertex[i][p][c vn + k][j] - target[i][p][c vn + k][j]),
 *       sl1(d) = 0.5 sigma^2 d^2  if |d| < 1 / sigma^2 (strict),  |d| - 0.5 / sigma^2  otherwise.
 *     THE DIFFERENCE FROM THE REFERENCE: an element whose weight is 0 (the background, another class's
 *     channels, an ignored label) contributes exactly 0 and gets gradient exactly 0 whatever it holds,
 *     NaN and inf included, where the reference's multiplication by the weight would spread a NaN.
 *     No zero-weight element enters any arithmetic.  In the vector form (below) a 16- or 32-byte
 *     group of 8 consecutive pixels is loaded whole when one of its pixels is weighted and the
 *     others are discarded by a select; a group without a weighted pixel, and in the scalar form
 *     every zero-weight element, is not loaded at all.
 *  3. fg[i] = fg_i.
 *  4. counts[i][c] = (tp, fp, fn) with pred(p) the arg-max over the ncls + 1 logits, A TIE GOING TO THE
 *     LOWEST INDEX: tp = #(pred = c + 1 and L = c + 1), fp = #(pred = c + 1 and L != c + 1),
 *     fn = #(pred != c + 1 and L = c + 1).  Ignored pixels count like any other pixel here.
 *
 *  Gradients (pv_loss_backward), with g_seg[i], g_vertex[i] the upstream gradients of the per-image
 *  losses, read on the device:
 *       grad_seg[i][c][p] = g_seg[i] (softmax_c - [c = L]) / (H W),  0 at ignored pixels;
 *       grad_vertex[i][p][ch][j] = g_vertex[i] (sigma^2 d  if |d| < 1 / sigma^2,  sign(d) otherwise)
 *                                  / (2 vn fg_i + 1e-3)  on the weighted elements, 0 elsewhere.
 *  Every element of both gradients is written.  They are computed in f32 and rounded to the
 *  prediction's kind: an f16 gradient of a mean over H W pixels is subnormal at full frames, so the
 *  caller scales the loss as in any f16 training.
 *
 * Arithmetic.  Per-pixel arithmetic is f32, every operation rounded (nothing is contracted, expf and
 * logf are the accurate forms).  Every sum over pixels is an f64 sum of those f32 terms in an order
 * that depends on the shapes alone: a lane adds the terms of its PV_LOSS_PIXELS consecutive pixels
 * of a row in increasing (class, k, j, x) order -- for the vector field over its block's share of the
 * 2 vn planes (k, j) of a class, which are dealt to at most PV_LOSS_MAX_CHUNKS blocks in runs of
 * consecutive planes --, the PV_LOSS_THREADS lanes of a block combine in a halving tree, each block
 * stores its partial to the workspace, and one final block per image adds the partials, lane t
 * taking partials t, t + PV_LOSS_THREADS, ... in increasing order and the lanes combining in the
 * same tree.  Counts are integer sums.  No floating-point atomics and no block waits on another:
 * two runs give the same bits.
 *
 * Speed.  When the pixel stride of a field is 1 (the network's [b][channels][H][W]) and a lane's
 * group of 8 pixels lies inside the row and is 16-byte aligned, the group is loaded and stored with
 * 16-byte accesses, channel after channel (the vector form); any other strides take scalar accesses
 * (the scalar form), which are correct, not fast.
 */
#ifndef PVLOSS_H_
#define PVLOSS_H_

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

/* element kind of the label map (the values of PV_LABEL_* of pvrender.h) */
#define PV_LOSS_LABEL_I64 0
#define PV_LOSS_LABEL_U8 1
#define PV_LOSS_LABEL_I32 2
/* element kind of seg, vertex and target (the values of PV_FIELD_* of pvrender.h) */
#define PV_LOSS_F32 0
#define PV_LOSS_F16 1

#define PV_LOSS_PIXELS 8          /* consecutive pixels of a row per lane */
#define PV_LOSS_THREADS 256       /* lanes per block */
#define PV_LOSS_MAX_DIM 1048576   /* 2^20: H and W */
#define PV_LOSS_MAX_CLASSES 1024  /* ncls */
#define PV_LOSS_MAX_CHUNKS 8      /* blocks that share the planes of a pixel group in the forward */

typedef struct pv_loss_desc {
    const void *seg;            /* seg_kind, logical [b][ncls + 1][H][W], seg_strides; NULL: no segmentation term */
    const void *vertex;         /* vertex_kind, logical [b][H][W][ncls vn][2], vertex_strides; NULL: no vector-field term */
    const void *target;         /* target_kind, the same logical shape, target_strides; needed with vertex */
    const void *label;          /* label_kind [b][H][W], label_strides */
    int64_t seg_strides[4];     /* all strides in elements, >= 0 */
    int64_t vertex_strides[5];
    int64_t target_strides[5];
    int64_t label_strides[3];
    int32_t seg_kind;           /* PV_LOSS_F32 / PV_LOSS_F16 */
    int32_t vertex_kind;
    int32_t target_kind;
    int32_t label_kind;         /* PV_LOSS_LABEL_* */
    int32_t b, H, W, ncls, vn;  /* 1 <= ncls <= PV_LOSS_MAX_CLASSES, 1 <= vn; b == 0 is success */
    float sigma;                /* > 0 */
} pv_loss_desc;

typedef struct pv_loss_out {
    float *loss_seg;            /* f32 [b]; needed with seg */
    float *loss_vertex;         /* f32 [b]; needed with vertex */
    int64_t *fg;                /* optional i64 [b] */
    int64_t *counts;            /* optional i64 [b][ncls][3] = (tp, fp, fn); written with seg only */
} pv_loss_out;

typedef struct pv_loss_grad {
    const float *g_seg;         /* f32 [b]; needed with seg */
    const float *g_vertex;      /* f32 [b]; needed with vertex */
    const int64_t *fg;          /* i64 [b], pv_loss_forward's; needed with vertex */
    void *grad_seg;             /* seg_kind, seg's logical shape, grad_seg_strides */
    void *grad_vertex;          /* vertex_kind, vertex's logical shape, grad_vertex_strides */
    int64_t grad_seg_strides[4];
    int64_t grad_vertex_strides[5];
} pv_loss_grad;

/* Bytes of workspace of pv_loss_forward for these sizes; 0 for bad sizes.  The workspace is 256-byte
 * aligned device memory, owned by the call until it has run.  pv_loss_backward reduces nothing and
 * takes none.  The workspace need not be cleared: the forward writes every partial it reads, and
 * writes nothing but its outputs and workspace[0, size). */
size_t pv_loss_workspace_size(int32_t b, int32_t H, int32_t W, int32_t ncls);

/* At least one of desc->seg and desc->vertex.  With seg absent loss_seg and counts are not written,
 * with vertex absent loss_vertex is not written; fg, when asked for, is written either way. */
int pv_loss_forward(const pv_loss_desc *desc /* host */, const pv_loss_out *out /* host */, void *workspace,
                    size_t workspace_bytes, pv_stream_t stream);

/* The gradients of the terms that desc names, recomputed from the same inputs: nothing is kept from
 * the forward but fg.  A term the caller wants no gradient of is left out of desc (its pointer NULL). */
int pv_loss_backward(const pv_loss_desc *desc /* host */, const pv_loss_grad *grad /* host */, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVLOSS_H_ */
