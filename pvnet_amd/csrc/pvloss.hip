// pvloss.hip -- libpvloss.so (include/pvloss.h): the per-image cross-entropy of the segmentation, the
// mask-weighted smooth-L1 of the vector field, the precision / recall counts, and the gradients of
// the two predictions.  One translation unit that includes no other csrc/ file, so the other five
// libraries' sources do not rebuild it.
//
// Every kernel gives one lane kPx = 8 consecutive pixels of a row and a block kThreads lanes; the
// grid is (blocks per image) x b, flattened, and for the two vector-field kernels blockIdx.y deals
// the channel planes out in runs:
//   k_seg_fwd   logits -> ce per pixel, arg-max -> (tp, fp, fn); block partials to the workspace
//   k_vtx_fwd   foreground count; vertex / target of the labelled class's channels -> smooth-L1
//   k_final     one block per image: partials -> loss_seg, loss_vertex, fg, counts
//   k_seg_bwd   logits -> (softmax - one-hot) g / (H W), every element stored
//   k_vtx_bwd   the labelled class's channels -> the smooth-L1 slope, zeros everywhere else
// The forward is up to three launches, the backward up to two; nothing waits on anything but the
// stream's order.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pvloss.h"

namespace {

constexpr int kThreads = PV_LOSS_THREADS;
constexpr int kPx = PV_LOSS_PIXELS;
static_assert(kPx == 8 && (kThreads & (kThreads - 1)) == 0, "the group loads below are written for 8 pixels");
// The vector-field kernels split the channel planes over blockIdx.y: a lane that walked all 2 vn
// planes of its pixels alone made the few foreground waves a serial chain of loads the rest of the
// grid waited for.
constexpr int kMaxChunks = PV_LOSS_MAX_CHUNKS;   // of the forward: its partials are sized by it
constexpr int kChunkPlanes = 6;                  // planes a block aims at

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
inline int last() { return rc(hipGetLastError()); }
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct Work {
    double *part_seg;    // [b][nblk]
    double *part_vtx;    // [b][nblk][chunks]
    uint32_t *part_fg;   // [b][nblk]
    uint32_t *part_cnt;  // [b][nblk][ncls][3]
    size_t bytes;
};

inline Work carve(void *base, int64_t blocks, int64_t ncls) {
    Work w{};
    int64_t off = 0;
    char *p = (char *)base;
    w.part_seg = (double *)(p + off);   off = align_up(off + blocks * 8, 256);
    w.part_vtx = (double *)(p + off);   off = align_up(off + blocks * kMaxChunks * 8, 256);
    w.part_fg = (uint32_t *)(p + off);  off = align_up(off + blocks * 4, 256);
    w.part_cnt = (uint32_t *)(p + off); off = align_up(off + blocks * ncls * 12, 256);
    w.bytes = (size_t)off;
    return w;
}

struct LossArgs {
    pv_loss_desc d;
    pv_loss_out out;
    pv_loss_grad gr;
    Work w;
    int32_t nblk;        // blocks per image
    int32_t gw;          // groups of kPx pixels per row
    int32_t chunk;       // planes per blockIdx.y of a vector-field kernel
    float s2, inv_s2;    // sigma^2, 1 / sigma^2
    float half_s2, half_inv_s2;
};

// ---- the lane's group of pixels ---------------------------------------------------------------------
struct Group {
    int i, y, x, n;      // image, row, first column, pixels inside the row (0: no group)
};

__device__ __forceinline__ Group my_group(const LossArgs &a) {
    Group g;
    g.i = (int)(blockIdx.x / (uint32_t)a.nblk);
    const uint32_t blk = blockIdx.x - (uint32_t)g.i * (uint32_t)a.nblk;
    const int64_t t = (int64_t)blk * kThreads + threadIdx.x;
    g.y = (int)(t / a.gw);
    g.x = (int)(t - (int64_t)g.y * a.gw) * kPx;
    g.n = g.y < a.d.H ? min(kPx, a.d.W - g.x) : 0;
    return g;
}

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// labels of the group as int: the label itself in 0..ncls, -1 for any other value (ignored) and for
// the pixels past the row's end
__device__ __forceinline__ void load_labels(const LossArgs &a, const Group &g, int (&lab)[kPx]) {
    const int64_t *s = a.d.label_strides;
    const int64_t o = (int64_t)g.i * s[0] + (int64_t)g.y * s[1] + (int64_t)g.x * s[2];
    int64_t v[kPx];
    if (a.d.label_kind == PV_LOSS_LABEL_U8) {
        const uint8_t *p = (const uint8_t *)a.d.label + o;
        if (s[2] == 1 && g.n == kPx && ((uintptr_t)p & 7) == 0) {
            const uint2 w = *(const uint2 *)p;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = (w.x >> (8 * e)) & 255u;
                v[e + 4] = (w.y >> (8 * e)) & 255u;
            }
        } else {
#pragma unroll
            for (int e = 0; e < kPx; ++e) v[e] = e < g.n ? (int64_t)p[e * s[2]] : -1;
        }
    } else if (a.d.label_kind == PV_LOSS_LABEL_I32) {
        const int32_t *p = (const int32_t *)a.d.label + o;
#pragma unroll
        for (int e = 0; e < kPx; ++e) v[e] = e < g.n ? (int64_t)p[e * s[2]] : -1;
    } else {
        const int64_t *p = (const int64_t *)a.d.label + o;
#pragma unroll
        for (int e = 0; e < kPx; ++e) v[e] = e < g.n ? p[e * s[2]] : -1;
    }
#pragma unroll
    for (int e = 0; e < kPx; ++e) lab[e] = (e < g.n && v[e] >= 0 && v[e] <= a.d.ncls) ? (int)v[e] : -1;
}

__device__ __forceinline__ float h2f(uint32_t bits16) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits16);
}
__device__ __forceinline__ uint32_t f2h(float v) {     // round to nearest even, as __float2half_rn
    return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v);
}

// eight elements sx apart -> f32.  The vector form (16-byte loads) when they are consecutive, inside
// the row and aligned; otherwise only the elements of `need` are loaded, the others read as 0.
template <typename T>
__device__ __forceinline__ void load8(const T *p, int64_t sx, bool full, uint32_t need, float (&v)[kPx]);

template <>
__device__ __forceinline__ void load8<float>(const float *p, int64_t sx, bool full, uint32_t need, float (&v)[kPx]) {
    if (sx == 1 && full && aligned16(p)) {
        const float4 lo = *(const float4 *)p, hi = *(const float4 *)(p + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
        v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
    } else {
#pragma unroll
        for (int e = 0; e < kPx; ++e) v[e] = (need >> e) & 1u ? p[e * sx] : 0.f;
    }
}

template <>
__device__ __forceinline__ void load8<__half>(const __half *p, int64_t sx, bool full, uint32_t need, float (&v)[kPx]) {
    if (sx == 1 && full && aligned16(p)) {
        const uint4 w = *(const uint4 *)p;
        v[0] = h2f(w.x & 0xffffu); v[1] = h2f(w.x >> 16);
        v[2] = h2f(w.y & 0xffffu); v[3] = h2f(w.y >> 16);
        v[4] = h2f(w.z & 0xffffu); v[5] = h2f(w.z >> 16);
        v[6] = h2f(w.w & 0xffffu); v[7] = h2f(w.w >> 16);
    } else {
#pragma unroll
        for (int e = 0; e < kPx; ++e) v[e] = (need >> e) & 1u ? __half2float(p[e * sx]) : 0.f;
    }
}

// the first n of eight values, rounded to T, to elements sx apart: full-width stores in the vector form
template <typename T>
__device__ __forceinline__ void store8(T *p, int64_t sx, int n, const float (&v)[kPx]);

template <>
__device__ __forceinline__ void store8<float>(float *p, int64_t sx, int n, const float (&v)[kPx]) {
    if (sx == 1 && n == kPx && aligned16(p)) {
        *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
        *(float4 *)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int e = 0; e < kPx; ++e)
            if (e < n) p[e * sx] = v[e];
    }
}

template <>
__device__ __forceinline__ void store8<__half>(__half *p, int64_t sx, int n, const float (&v)[kPx]) {
    if (sx == 1 && n == kPx && aligned16(p)) {
        *(uint4 *)p = make_uint4(f2h(v[0]) | (f2h(v[1]) << 16), f2h(v[2]) | (f2h(v[3]) << 16),
                                 f2h(v[4]) | (f2h(v[5]) << 16), f2h(v[6]) | (f2h(v[7]) << 16));
    } else {
#pragma unroll
        for (int e = 0; e < kPx; ++e)
            if (e < n) p[e * sx] = __float2half_rn(v[e]);
    }
}

// the block's f64 sum in a halving tree over red[kThreads]; the result is red[0] after the call
__device__ __forceinline__ void block_sum(double *red, double v) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = kThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
}

// the dynamic LDS of a forward block: red[kThreads] f64, then the block's integer counters
__device__ __forceinline__ double *lds_red(unsigned char *lds) { return (double *)lds; }
__device__ __forceinline__ uint32_t *lds_cnt(unsigned char *lds) { return (uint32_t *)(lds + kThreads * sizeof(double)); }

// ---- the segmentation term ---------------------------------------------------------------------------
// m = the maximum, am = its lowest index, s = sum_c expf(v_c - m), vl = the label's logit
template <typename T>
__device__ __forceinline__ void softmax_stats(const LossArgs &a, const Group &g, const int (&lab)[kPx], float (&m)[kPx],
                                              int (&am)[kPx], float (&s)[kPx], float (&vl)[kPx]) {
    const int64_t *st = a.d.seg_strides;
    const T *base = (const T *)a.d.seg + (int64_t)g.i * st[0] + (int64_t)g.y * st[2] + (int64_t)g.x * st[3];
    const uint32_t valid = (1u << g.n) - 1u;
    const bool full = g.n == kPx;
    float v[kPx];
#pragma unroll
    for (int e = 0; e < kPx; ++e) { m[e] = 0.f; am[e] = 0; s[e] = 0.f; vl[e] = 0.f; }
    for (int c = 0; c <= a.d.ncls; ++c) {
        load8<T>(base + (int64_t)c * st[1], st[3], full, valid, v);
#pragma unroll
        for (int e = 0; e < kPx; ++e) {
            if (c == 0 || v[e] > m[e]) { m[e] = v[e]; am[e] = c; }
            if (c == lab[e]) vl[e] = v[e];
        }
    }
    for (int c = 0; c <= a.d.ncls; ++c) {
        load8<T>(base + (int64_t)c * st[1], st[3], full, valid, v);
#pragma unroll
        for (int e = 0; e < kPx; ++e) s[e] = s[e] + expf(v[e] - m[e]);
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_seg_fwd(LossArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double *red = lds_red(lds);
    uint32_t *cnt = lds_cnt(lds);
    const int ncnt = 3 * a.d.ncls;
    for (int q = threadIdx.x; q < ncnt; q += kThreads) cnt[q] = 0;
    __syncthreads();
    const Group g = my_group(a);
    double acc = 0.0;
    if (g.n > 0) {
        int lab[kPx], am[kPx];
        float m[kPx], s[kPx], vl[kPx];
        load_labels(a, g, lab);
        softmax_stats<T>(a, g, lab, m, am, s, vl);
        // runs of equal events of the lane's pixels go to the block's counters as one integer add
        int pend = -1, pn = 0;
        auto event = [&](int idx) {
            if (idx == pend) { ++pn; return; }
            if (pn) atomicAdd(&cnt[pend], (uint32_t)pn);
            pend = idx; pn = 1;
        };
        // the raw label decides the counts: an ignored pixel is "not class c" for every c
#pragma unroll
        for (int e = 0; e < kPx; ++e) {
            if (e < g.n) {
                if (lab[e] >= 0) acc += (double)((m[e] + logf(s[e])) - vl[e]);
                const int pr = am[e], lb = lab[e];
                if (pr >= 1) event(3 * (pr - 1) + (lb == pr ? 0 : 1));
                if (lb >= 1 && lb != pr) event(3 * (lb - 1) + 2);
            }
        }
        if (pn) atomicAdd(&cnt[pend], (uint32_t)pn);
    }
    block_sum(red, acc);
    if (threadIdx.x == 0) a.w.part_seg[blockIdx.x] = red[0];
    uint32_t *o = a.w.part_cnt + (int64_t)blockIdx.x * ncnt;
    for (int q = threadIdx.x; q < ncnt; q += kThreads) o[q] = cnt[q];
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_seg_bwd(LossArgs a) {
    const Group g = my_group(a);
    if (g.n == 0) return;
    int lab[kPx], am[kPx];
    float m[kPx], s[kPx], vl[kPx], v[kPx], o[kPx];
    load_labels(a, g, lab);
    softmax_stats<T>(a, g, lab, m, am, s, vl);
    const float gs = a.gr.g_seg[g.i] / (float)((int64_t)a.d.H * a.d.W);
    const int64_t *st = a.d.seg_strides, *gt = a.gr.grad_seg_strides;
    const T *base = (const T *)a.d.seg + (int64_t)g.i * st[0] + (int64_t)g.y * st[2] + (int64_t)g.x * st[3];
    T *out = (T *)a.gr.grad_seg + (int64_t)g.i * gt[0] + (int64_t)g.y * gt[2] + (int64_t)g.x * gt[3];
    const uint32_t valid = (1u << g.n) - 1u;
    for (int c = 0; c <= a.d.ncls; ++c) {
        load8<T>(base + (int64_t)c * st[1], st[3], g.n == kPx, valid, v);
#pragma unroll
        for (int e = 0; e < kPx; ++e) {
            const float p = expf(v[e] - m[e]) / s[e];
            o[e] = lab[e] >= 0 ? (p - (c == lab[e] ? 1.f : 0.f)) * gs : 0.f;
        }
        store8<T>(out + (int64_t)c * gt[1], gt[3], g.n, o);
    }
}

// ---- the vector-field term ---------------------------------------------------------------------------
// cls[e] = label - 1 of a foreground pixel, -1 otherwise; returns the foreground count
__device__ __forceinline__ int classes(const LossArgs &a, const Group &g, int (&cls)[kPx], int *cmin, int *cmax) {
    int lab[kPx];
    load_labels(a, g, lab);
    int n = 0, lo = INT32_MAX, hi = -1;
#pragma unroll
    for (int e = 0; e < kPx; ++e) {
        cls[e] = lab[e] >= 1 ? lab[e] - 1 : -1;
        if (cls[e] >= 0) { ++n; lo = min(lo, cls[e]); hi = max(hi, cls[e]); }
    }
    *cmin = lo; *cmax = hi;
    return n;
}

__device__ __forceinline__ uint32_t class_mask(const int (&cls)[kPx], int c) {
    uint32_t mk = 0;
#pragma unroll
    for (int e = 0; e < kPx; ++e) mk |= (cls[e] == c ? 1u : 0u) << e;
    return mk;
}

template <typename TV, typename TT>
__global__ __launch_bounds__(kThreads) void k_vtx_fwd(LossArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    double *red = lds_red(lds);
    uint32_t *cnt = lds_cnt(lds);
    if (threadIdx.x == 0) cnt[0] = 0;
    __syncthreads();
    const Group g = my_group(a);
    double acc = 0.0;
    if (g.n > 0) {
        int cls[kPx], cmin, cmax;
        const int nfg = classes(a, g, cls, &cmin, &cmax);
        if (nfg > 0) {
            if (blockIdx.y == 0) atomicAdd(&cnt[0], (uint32_t)nfg);
            if (a.d.vertex) {
                // this block's planes q = 2 k + j of every class: [q0, q1) of the 2 vn
                const int q0 = blockIdx.y * a.chunk, q1 = min(2 * a.d.vn, q0 + a.chunk);
                const int64_t *sv = a.d.vertex_strides, *tv = a.d.target_strides;
                const TV *pv = (const TV *)a.d.vertex + (int64_t)g.i * sv[0] + (int64_t)g.y * sv[1] + (int64_t)g.x * sv[2];
                const TT *pt = (const TT *)a.d.target + (int64_t)g.i * tv[0] + (int64_t)g.y * tv[1] + (int64_t)g.x * tv[2];
                const bool full = g.n == kPx;
                float p[kPx], t[kPx];
                for (int c = cmin; c <= cmax; ++c) {
                    const uint32_t mk = class_mask(cls, c);
                    if (!mk) continue;
                    for (int q = q0; q < q1; ++q) {
                        const int64_t ch = (int64_t)c * a.d.vn + (q >> 1);
                        const int j = q & 1;
                        load8<TV>(pv + ch * sv[3] + j * sv[4], sv[2], full, mk, p);
                        load8<TT>(pt + ch * tv[3] + j * tv[4], tv[2], full, mk, t);
#pragma unroll
                        for (int e = 0; e < kPx; ++e) {
                            if ((mk >> e) & 1u) {
                                const float d = p[e] - t[e], ad = fabsf(d);
                                const float term = ad < a.inv_s2 ? (a.half_s2 * d) * d : ad - a.half_inv_s2;
                                acc += (double)term;
                            }
                        }
                    }
                }
            }
        }
    }
    block_sum(red, acc);
    if (threadIdx.x == 0) {
        a.w.part_vtx[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = red[0];
        if (blockIdx.y == 0) a.w.part_fg[blockIdx.x] = cnt[0];
    }
}

template <typename TV, typename TT>
__global__ __launch_bounds__(kThreads) void k_vtx_bwd(LossArgs a) {
    const Group g = my_group(a);
    if (g.n == 0) return;
    int cls[kPx], cmin, cmax;
    classes(a, g, cls, &cmin, &cmax);
    const float den = (float)(2.0 * (double)a.d.vn * (double)a.gr.fg[g.i] + 1e-3);
    const float scale = a.gr.g_vertex[g.i] / den;
    const int64_t *sv = a.d.vertex_strides, *tv = a.d.target_strides, *gv = a.gr.grad_vertex_strides;
    const TV *pv = (const TV *)a.d.vertex + (int64_t)g.i * sv[0] + (int64_t)g.y * sv[1] + (int64_t)g.x * sv[2];
    const TT *pt = (const TT *)a.d.target + (int64_t)g.i * tv[0] + (int64_t)g.y * tv[1] + (int64_t)g.x * tv[2];
    TV *po = (TV *)a.gr.grad_vertex + (int64_t)g.i * gv[0] + (int64_t)g.y * gv[1] + (int64_t)g.x * gv[2];
    const bool full = g.n == kPx;
    float p[kPx], t[kPx], o[kPx];
    // this block's planes Q = 2 ch + j of all 2 ncls vn: [Q0, Q1)
    const int Q0 = blockIdx.y * a.chunk, Q1 = min(2 * a.d.ncls * a.d.vn, Q0 + a.chunk);
    for (int Q = Q0; Q < Q1; ++Q) {
        const int64_t ch = Q >> 1;
        const int j = Q & 1;
        const uint32_t mk = class_mask(cls, (int)(ch / a.d.vn));
#pragma unroll
        for (int e = 0; e < kPx; ++e) o[e] = 0.f;
        if (mk) {
            load8<TV>(pv + ch * sv[3] + j * sv[4], sv[2], full, mk, p);
            load8<TT>(pt + ch * tv[3] + j * tv[4], tv[2], full, mk, t);
#pragma unroll
            for (int e = 0; e < kPx; ++e) {
                if ((mk >> e) & 1u) {
                    const float d = p[e] - t[e];
                    const float slope = fabsf(d) < a.inv_s2 ? a.s2 * d : (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
                    o[e] = scale * slope;
                }
            }
        }
        store8<TV>(po + ch * gv[3] + j * gv[4], gv[2], g.n, o);
    }
}

// ---- one block per image: the partials, in a fixed order ----------------------------------------------
__global__ __launch_bounds__(kThreads) void k_final(LossArgs a, int with_vtx, int chunks) {
    __shared__ double red[kThreads];
    __shared__ unsigned long long fg_s;
    __shared__ unsigned long long cnt_s[3 * PV_LOSS_MAX_CLASSES];
    const int i = blockIdx.x, t = threadIdx.x;
    const int64_t p0 = (int64_t)i * a.nblk;
    if (a.d.seg) {
        double acc = 0.0;
        for (int q = t; q < a.nblk; q += kThreads) acc += a.w.part_seg[p0 + q];
        block_sum(red, acc);
        if (t == 0) a.out.loss_seg[i] = (float)(red[0] / (double)((int64_t)a.d.H * a.d.W));
        __syncthreads();
        if (a.out.counts) {
            // the image's [nblk][3 ncls] partials are one contiguous run: coalesced reads, integer adds
            const int ncnt = 3 * a.d.ncls;
            for (int q = t; q < ncnt; q += kThreads) cnt_s[q] = 0;
            __syncthreads();
            const uint32_t *pc = a.w.part_cnt + p0 * ncnt;
            const int64_t n = (int64_t)a.nblk * ncnt;
            for (int64_t q = t; q < n; q += kThreads) {
                const uint32_t v = pc[q];
                if (v) atomicAdd(&cnt_s[q % ncnt], (unsigned long long)v);
            }
            __syncthreads();
            for (int q = t; q < ncnt; q += kThreads) a.out.counts[(int64_t)i * ncnt + q] = (int64_t)cnt_s[q];
        }
    }
    if (with_vtx) {
        if (t == 0) fg_s = 0;
        __syncthreads();
        unsigned long long n = 0;
        double acc = 0.0;
        for (int q = t; q < a.nblk; q += kThreads) n += a.w.part_fg[p0 + q];
        const int64_t np = (int64_t)a.nblk * chunks;
        for (int64_t q = t; q < np; q += kThreads) acc += a.w.part_vtx[p0 * chunks + q];
        if (n) atomicAdd(&fg_s, n);
        block_sum(red, acc);
        if (t == 0) {
            if (a.out.fg) a.out.fg[i] = (int64_t)fg_s;
            if (a.d.vertex) a.out.loss_vertex[i] = (float)(red[0] / (2.0 * (double)a.d.vn * (double)fg_s + 1e-3));
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------
bool kind_ok(int32_t k) { return k == PV_LOSS_F32 || k == PV_LOSS_F16; }
bool label_kind_ok(int32_t k) { return k == PV_LOSS_LABEL_I64 || k == PV_LOSS_LABEL_U8 || k == PV_LOSS_LABEL_I32; }
uintptr_t kind_mask(int32_t k) { return k == PV_LOSS_F32 ? 3 : 1; }

bool sizes_ok(int32_t b, int32_t H, int32_t W, int32_t ncls) {
    return b >= 0 && H >= 1 && W >= 1 && H <= PV_LOSS_MAX_DIM && W <= PV_LOSS_MAX_DIM && ncls >= 1 &&
           ncls <= PV_LOSS_MAX_CLASSES;
}

int32_t groups_per_row(int32_t W) { return (W + kPx - 1) / kPx; }
// blocks per image; 0 if the flattened grid would not fit
int64_t blocks_per_image(int32_t b, int32_t H, int32_t W) {
    const int64_t nblk = ((int64_t)H * groups_per_row(W) + kThreads - 1) / kThreads;
    return nblk * std::max<int64_t>(b, 1) <= INT32_MAX ? nblk : 0;
}

// everything both entries check of the descriptor; PV_OK with *empty set for b == 0
int check_desc(const pv_loss_desc *d, bool *empty) {
    *empty = false;
    if (!d) return PV_EINVAL;
    if (!sizes_ok(d->b, d->H, d->W, d->ncls) || d->vn < 1 || (int64_t)d->ncls * d->vn > (1 << 20)) return PV_EINVAL;
    if (!(d->sigma > 0.f) || !(d->sigma <= 3.0e38f)) return PV_EINVAL;   // also rejects NaN and inf
    if (!kind_ok(d->seg_kind) || !kind_ok(d->vertex_kind) || !kind_ok(d->target_kind) || !label_kind_ok(d->label_kind))
        return PV_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (d->seg_strides[i] < 0) return PV_EINVAL;
    for (int i = 0; i < 5; ++i)
        if (d->vertex_strides[i] < 0 || d->target_strides[i] < 0) return PV_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->label_strides[i] < 0) return PV_EINVAL;
    if (blocks_per_image(d->b, d->H, d->W) == 0) return PV_EINVAL;
    if (d->b == 0) { *empty = true; return PV_OK; }
    if (!d->seg && !d->vertex) return PV_EINVAL;
    if (!d->label || (d->vertex && !d->target)) return PV_EINVAL;
    const uintptr_t l_al = d->label_kind == PV_LOSS_LABEL_I64 ? 7 : d->label_kind == PV_LOSS_LABEL_I32 ? 3 : 0;
    if (((uintptr_t)d->seg & kind_mask(d->seg_kind)) || ((uintptr_t)d->vertex & kind_mask(d->vertex_kind)) ||
        ((uintptr_t)d->target & kind_mask(d->target_kind)) || ((uintptr_t)d->label & l_al))
        return PV_EALIGN;
    return PV_OK;
}

LossArgs make_args(const pv_loss_desc *d) {
    LossArgs a{};
    a.d = *d;
    a.nblk = (int32_t)blocks_per_image(d->b, d->H, d->W);
    a.gw = groups_per_row(d->W);
    a.s2 = d->sigma * d->sigma;
    a.inv_s2 = 1.0f / a.s2;
    a.half_s2 = 0.5f * a.s2;
    a.half_inv_s2 = 0.5f / a.s2;
    return a;
}

}  // namespace

extern "C" {

size_t pv_loss_workspace_size(int32_t b, int32_t H, int32_t W, int32_t ncls) {
    if (!sizes_ok(b, H, W, ncls)) return 0;
    const int64_t nblk = blocks_per_image(b, H, W);
    if (nblk == 0) return 0;
    return carve(nullptr, nblk * b, ncls).bytes + 256;
}

int pv_loss_forward(const pv_loss_desc *d, const pv_loss_out *out, void *workspace, size_t workspace_bytes,
                    pv_stream_t stream) {
    bool empty;
    const int e0 = check_desc(d, &empty);
    if (e0 != PV_OK) return e0;
    if (!out) return PV_EINVAL;
    if (empty) return PV_OK;
    if ((d->seg && !out->loss_seg) || (d->vertex && !out->loss_vertex)) return PV_EINVAL;
    const size_t need = pv_loss_workspace_size(d->b, d->H, d->W, d->ncls);
    if (need == 0) return PV_EINVAL;
    if (!workspace || workspace_bytes < need) return PV_EWORKSPACE;
    if (((uintptr_t)workspace & 255) || (((uintptr_t)out->loss_seg | (uintptr_t)out->loss_vertex) & 3) ||
        (((uintptr_t)out->fg | (uintptr_t)out->counts) & 7))
        return PV_EALIGN;

    LossArgs a = make_args(d);
    a.out = *out;
    const int64_t blocks = (int64_t)a.nblk * d->b;
    a.w = carve(workspace, blocks, d->ncls);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks);
    int e;
    if (d->seg) {
        const size_t lds = kThreads * sizeof(double) + (size_t)3 * d->ncls * sizeof(uint32_t);
        if (d->seg_kind == PV_LOSS_F32) k_seg_fwd<float><<<grid, kThreads, lds, st>>>(a);
        else k_seg_fwd<__half><<<grid, kThreads, lds, st>>>(a);
        if ((e = last())) return e;
    }
    const int with_vtx = d->vertex || out->fg;
    // the 2 vn planes of a class in at most kMaxChunks chunks of about kChunkPlanes
    const int planes = d->vertex ? 2 * d->vn : 1;
    const int chunks = std::min(kMaxChunks, (planes + kChunkPlanes - 1) / kChunkPlanes);
    a.chunk = (planes + chunks - 1) / chunks;
    if (with_vtx) {
        const size_t lds = kThreads * sizeof(double) + sizeof(uint32_t);
        const dim3 grid((unsigned)blocks, (unsigned)chunks);
        const bool v32 = d->vertex_kind == PV_LOSS_F32, t32 = d->target_kind == PV_LOSS_F32;
        if (v32 && t32) k_vtx_fwd<float, float><<<grid, kThreads, lds, st>>>(a);
        else if (v32) k_vtx_fwd<float, __half><<<grid, kThreads, lds, st>>>(a);
        else if (t32) k_vtx_fwd<__half, float><<<grid, kThreads, lds, st>>>(a);
        else k_vtx_fwd<__half, __half><<<grid, kThreads, lds, st>>>(a);
        if ((e = last())) return e;
    }
    k_final<<<dim3((unsigned)d->b), kThreads, 0, st>>>(a, with_vtx, chunks);
    return last();
}

int pv_loss_backward(const pv_loss_desc *d, const pv_loss_grad *gr, pv_stream_t stream) {
    bool empty;
    const int e0 = check_desc(d, &empty);
    if (e0 != PV_OK) return e0;
    if (!gr) return PV_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (gr->grad_seg_strides[i] < 0) return PV_EINVAL;
    for (int i = 0; i < 5; ++i)
        if (gr->grad_vertex_strides[i] < 0) return PV_EINVAL;
    if (empty) return PV_OK;
    if (d->seg && (!gr->g_seg || !gr->grad_seg)) return PV_EINVAL;
    if (d->vertex && (!gr->g_vertex || !gr->grad_vertex || !gr->fg)) return PV_EINVAL;
    if ((((uintptr_t)gr->g_seg | (uintptr_t)gr->g_vertex) & 3) || ((uintptr_t)gr->fg & 7) ||
        ((uintptr_t)gr->grad_seg & kind_mask(d->seg_kind)) || ((uintptr_t)gr->grad_vertex & kind_mask(d->vertex_kind)))
        return PV_EALIGN;

    LossArgs a = make_args(d);
    a.gr = *gr;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((int64_t)a.nblk * d->b);
    const dim3 grid(blocks);
    int e;
    if (d->seg) {
        if (d->seg_kind == PV_LOSS_F32) k_seg_bwd<float><<<grid, kThreads, 0, st>>>(a);
        else k_seg_bwd<__half><<<grid, kThreads, 0, st>>>(a);
        if ((e = last())) return e;
    }
    if (d->vertex) {
        // all 2 ncls vn planes in chunks of kChunkPlanes (more when blockIdx.y would not hold them)
        const int64_t planes = (int64_t)2 * d->ncls * d->vn;
        a.chunk = (int)std::max<int64_t>(kChunkPlanes, (planes + 65534) / 65535);
        const dim3 grid(blocks, (unsigned)((planes + a.chunk - 1) / a.chunk));
        const bool v32 = d->vertex_kind == PV_LOSS_F32, t32 = d->target_kind == PV_LOSS_F32;
        if (v32 && t32) k_vtx_bwd<float, float><<<grid, kThreads, 0, st>>>(a);
        else if (v32) k_vtx_bwd<float, __half><<<grid, kThreads, 0, st>>>(a);
        else if (t32) k_vtx_bwd<__half, float><<<grid, kThreads, 0, st>>>(a);
        else k_vtx_bwd<__half, __half><<<grid, kThreads, 0, st>>>(a);
        if ((e = last())) return e;
    }
    return PV_OK;
}

}  // extern "C"
