/* pvoptim.h -- C ABI of libpvoptim.so: the mixed-precision parameter update, on the device.
 *
 * What follows pv_loss_backward and autograd in a training step: the non-finite check over every
 * gradient, the unscaling of a scaled loss's gradients, the global-norm clip
 * (torch.nn.utils.clip_grad_norm_), the update itself (torch.optim.Adam, AdamW or SGD with momentum),
 * the f16 copy of the f32 master weights, the zeroing of the gradients and the adaptive loss scale
 * (torch._amp_update_scale_), as ONE call that decides on the device whether the step happens.  No
 * value is read back, so a training step that contains it can be captured into a hipGraph.
 * A library of its own: nothing here needs the other eight, and their export lists do not change.
 * This header defines the semantics; tests/optim_ref.py restates them in numpy.
 *
 * Conventions (those of pvloss.h):
 *   - pointers are device pointers unless a comment says host;
 *   - pv_optim_step is asynchronous on `stream`, synchronises nothing on the host and allocates
 *     nothing, so it can be captured into a hipGraph;
 *   - the return value is 0, a positive hipError_t, or one of the negative codes below; nothing
 *     calls exit();
 *   - every bad argument (a NULL descriptor, table, chunk list or state, a negative count, an unknown
 *     algorithm, beta1 or beta2 outside [0, 1), eps <= 0, a negative weight_decay or momentum,
 *     growth_factor < 1, backoff_factor outside (0, 1], a negative growth_interval, zero_grads other
 *     than 0 / 1, any NaN or infinite hyper-parameter other than max_norm = +inf, a misaligned
 *     pointer, a workspace that is NULL, too small or misaligned) is rejected on the host before any
 *     pointer is touched; a table of no tensors or no chunks is success: nothing is launched and the
 *     state is left as it is.
 *   - pv_optim_plan checks the tensors on the host (a negative n, an unknown kind, a pointer not
 *     aligned to its element and, in a tensor with n > 0, a NULL master, grad or m, or a NULL v when
 *     the algorithm reads it; a tensor without elements may have no address).  The
 *     table and the chunk list that pv_optim_step reads are device memory, which it cannot check; its
 *     kernels skip a chunk whose tensor index, first element or tensor entry is out of range.
 *
 * The tensor table.  One pv_optim_tensor per parameter: the f32 master weights, the f16 model copy
 * (NULL when the parameter itself is f32), the gradient (f32 or f16), the two f32 moments, n elements
 * (0 allowed).  One pv_optim_chunk per block: PV_OPT_CHUNK consecutive elements of one tensor from a
 * first element that is a multiple of PV_OPT_CHUNK.  pv_optim_plan lists the chunks tensor after
 * tensor, first element increasing, none for n = 0: the order is a function of the n's alone.
 *
 * One step, three launches (S = *state, d = *desc):
 *
 *  1. k_optim_stats, a block per chunk: cnt = the number of non-finite gradient elements of the chunk,
 *     sum = the f64 sum of (double)g (double)g over its FINITE elements (a product of two f32 values is
 *     exact in f64; a non-finite element adds nothing, so the norm of a skipped step is that of the
 *     finite elements and a fixed value).  Element e of the chunk belongs to lane (e / 8) mod
 *     PV_OPT_THREADS; a lane adds its elements in increasing order, the lanes combine in a halving
 *     tree (lane t += lane t + s, s = PV_OPT_THREADS / 2 ... 1).
 *  2. k_optim_decide, one block: lane t adds partials t, t + PV_OPT_THREADS, ... in increasing order,
 *     the same tree.  Then, in f64 unless f32 is named:
 *       found_inf = any cnt != 0
 *       inv = 1 / (double)S.scale,  norm = sqrt(sum) inv
 *       c = d.max_norm > 0 ? min(1, (double)d.max_norm / (norm + 1e-6)) : 1
 *       k = (float)(inv c)
 *       if !found_inf:  S.step += 1,  S.b1pow *= (double)d.beta1,  S.b2pow *= (double)d.beta2
 *       bc1 = (float)(1 - S.b1pow),  bc2 = (float)(1 - S.b2pow)
 *       f32:  step_size = S.lr / bc1,  sq2 = sqrtf(bc2),  lr_wd = S.lr * d.weight_decay
 *       the scale (f32, only when d.growth_interval > 0; with 0 scale and tracker never change):
 *         found_inf:  S.scale = S.scale * d.backoff_factor,  S.growth_tracker = 0
 *         otherwise:  t = S.growth_tracker + 1;  if t == d.growth_interval
 *                       { s = S.scale * d.growth_factor;  if s is finite S.scale = s;  t = 0 }
 *                     S.growth_tracker = t          (a tracker that is already past the interval
 *                                                    counts on, as torch's does)
 *       S.grad_norm = (float)norm,  S.found_inf = S.skipped = found_inf
 *     and the decision (k, step_size, sq2, lr, lr_wd, skipped) goes to the workspace.
 *  3. k_optim_apply, a block per chunk.  On a skipped step nothing is stored but, with d.zero_grads,
 *     +0 to every gradient element (an overflow does not live into the next accumulation).
 *     Otherwise per element, in f32 with every operation rounded (nothing contracted, sqrtf and /
 *     correctly rounded, subnormals kept), p = master, wd = d.weight_decay:
 *       g = (float)grad * k
 *       PV_OPT_ADAM    if wd != 0: g = g + wd * p
 *                      m = d.beta1 * m + (1 - d.beta1) * g           (1 - beta in f32, on the host)
 *                      v = d.beta2 * v + ((1 - d.beta2) * g) * g
 *                      p = p - step_size * (m / (sqrtf(v) / sq2 + d.eps))
 *       PV_OPT_ADAMW   if wd != 0: p = p - lr_wd * p;  then m, v, p as PV_OPT_ADAM without its first line
 *       PV_OPT_SGD     if wd != 0: g = g + wd * p
 *                      m = d.momentum * m + g;  p = p - lr * m         (v is neither read nor written)
 *     and master = p, m, v are stored, model = (f16)p rounded to nearest even when present, and +0 to
 *     the gradient with d.zero_grads.
 *     A chunk whose present pointers are all 16-byte aligned at its first element moves its whole
 *     groups of 8 elements with 16-byte accesses (the vector form: one access for an f16 group, two
 *     for an f32 group); its last, partial group and every chunk of a tensor with a misaligned
 *     pointer take scalar accesses.  Both forms compute the same bits.
 *
 * No floating-point atomics and no block waits on another: two runs give the same bits.
 */
#ifndef PVOPTIM_H_
#define PVOPTIM_H_

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

/* element kind of a gradient (the values of PV_LOSS_F32 / PV_LOSS_F16 of pvloss.h) */
#define PV_OPT_F32 0
#define PV_OPT_F16 1

#define PV_OPT_ADAM 0   /* weight decay added to the gradient, as torch.optim.Adam */
#define PV_OPT_ADAMW 1  /* decoupled weight decay, as torch.optim.AdamW */
#define PV_OPT_SGD 2    /* momentum, dampening 0, no Nesterov, L2 decay, as torch.optim.SGD */

#define PV_OPT_CHUNK 8192   /* elements of a chunk: one block's */
#define PV_OPT_THREADS 256  /* lanes per block */
#define PV_OPT_GROUP 8      /* consecutive elements a lane takes at a time */

typedef struct pv_optim_tensor {
    float *master;       /* f32 [n] */
    void *model;         /* f16 [n], or NULL: the parameter is the master */
    void *grad;          /* grad_kind [n] */
    float *m;            /* f32 [n]: first moment / momentum buffer */
    float *v;            /* f32 [n]: second moment; PV_OPT_SGD never touches it, NULL allowed there */
    int64_t n;           /* >= 0 */
    int32_t grad_kind;   /* PV_OPT_F32 / PV_OPT_F16 */
    int32_t pad_;
} pv_optim_tensor;

typedef struct pv_optim_chunk {
    int64_t first;       /* first element, a multiple of PV_OPT_CHUNK */
    int32_t tensor;      /* index into the table */
    int32_t pad_;
} pv_optim_chunk;

/* What changes from step to step: device memory, so a captured step needs no new arguments. */
typedef struct pv_optim_state {
    double b1pow, b2pow;     /* beta1^step, beta2^step as running products; start at 1 */
    int64_t step;            /* steps taken (skipped ones not counted); start at 0 */
    float lr;
    float scale;             /* the loss scale; 1 for none */
    int32_t growth_tracker;  /* unskipped steps since the scale last changed */
    float grad_norm;         /* out: the unscaled global norm of the last step's gradients, before the clip */
    int32_t found_inf;       /* out: 1 if a gradient element of the last step was NaN or +-inf */
    int32_t skipped;         /* out: 1 if the last step changed no parameter */
} pv_optim_state;

typedef struct pv_optim_desc {   /* host */
    int32_t algorithm;       /* PV_OPT_ADAM / PV_OPT_ADAMW / PV_OPT_SGD */
    float beta1, beta2;      /* [0, 1) */
    float eps;               /* > 0 */
    float weight_decay;      /* >= 0 */
    float momentum;          /* >= 0 */
    float max_norm;          /* <= 0: no clip */
    float growth_factor;     /* >= 1 */
    float backoff_factor;    /* (0, 1] */
    int32_t growth_interval; /* >= 0; 0: the scale is static */
    int32_t zero_grads;      /* 0 / 1 */
    int32_t pad_;
} pv_optim_desc;

/* The chunk list of `count` tensors, all host memory: writes at most `capacity` chunks to `chunks`
 * (NULL with capacity 0 only counts) and returns how many the tensors need, or a negative code for a
 * bad tensor (above; v may be NULL only with PV_OPT_SGD) or for more than 2^31 - 1 chunks. */
int64_t pv_optim_plan(const pv_optim_tensor *tensors /* host */, int32_t count, int32_t algorithm,
                      pv_optim_chunk *chunks /* host, out */, int64_t capacity);

/* Bytes of workspace of pv_optim_step for this many chunks; 0 for a negative count or one beyond
 * 2^31 - 1.  The workspace is 256-byte aligned device memory, owned by the call until it has run.  It
 * need not be cleared: every byte a kernel reads was written by the one before it, and nothing is
 * written but workspace[0, size), the state and the tensors' arrays. */
size_t pv_optim_workspace_size(int64_t n_chunks);

/* table and chunks are 8-byte aligned device arrays, state is 8-byte aligned device memory. */
int pv_optim_step(const pv_optim_desc *desc /* host */, const pv_optim_tensor *table, int32_t n_tensors,
                  const pv_optim_chunk *chunks, int64_t n_chunks, pv_optim_state *state, void *workspace,
                  size_t workspace_bytes, pv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PVOPTIM_H_ */
