// pvaugment.hip -- libpvaugment.so (include/pvaugment.h): the foreground statistics of a label map,
// the draw of one affine map and one colour jitter per image, and the warp + background +
// photometric chain + normalisation of a u8 batch.  One translation unit that includes no other
// csrc/ file, so the other six libraries' sources do not rebuild it.
//
//   k_stats_init  stats[i] = (0, 0, 0, W, H, -1, -1, 0)
//   k_stats       a block's pixels -> LDS integer add / min / max -> global integer add / min / max
//   k_params      one thread per image: the draws, fwd, inv, color
//   k_apply<MODE> a lane owns kPx = 8 consecutive output pixels of a row, a block kThreads lanes, the
//                 grid is (blocks per image) x b, flattened; the eight source coordinates
//                 first, then the eight label loads together, then each pixel's twelve taps together,
//                 every load at clamped coordinates with a select after it:
//                   MODE 0  no contrast: the whole chain, one launch
//                   MODE 1  warp, background, brightness -> the block's f64 sum of greys to the workspace
//                   MODE 2  the image's partials summed by every block in a fixed order, then the whole
//                           chain with the warp recomputed (the u8 source stays in L2; an f32
//                           intermediate would cost 24 bytes a pixel more than reading it again)
// Nothing waits on anything but the stream's order.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pvaugment.h"

namespace {

constexpr int kThreads = PV_AUG_THREADS;
constexpr int kPx = PV_AUG_PIXELS;
static_assert(kPx == 8 && (kThreads & (kThreads - 1)) == 0, "the group stores below are written for 8 pixels");

constexpr int kStatPx = 32;   // pixels per lane of k_stats: a block's 8,192 pixels end in seven global integer atomics

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
inline int last() { return rc(hipGetLastError()); }
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// ---- labels ------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t load_label(const void *base, int kind, int64_t off) {
    if (kind == PV_AUG_LABEL_U8) return (int64_t)((const uint8_t *)base)[off];
    if (kind == PV_AUG_LABEL_I32) return (int64_t)((const int32_t *)base)[off];
    return ((const int64_t *)base)[off];
}

// ---- pv_label_stats ------------------------------------------------------------------------------------
struct StatsArgs {
    pv_aug_label d;
    int64_t *stats;
    int32_t ncls;
    int32_t nblk;   // blocks per image
};

__global__ void k_stats_init(int64_t *stats, int32_t b, int32_t H, int32_t W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b) return;
    int64_t *o = stats + (int64_t)i * 8;
    o[0] = 0; o[1] = 0; o[2] = 0; o[3] = W; o[4] = H; o[5] = -1; o[6] = -1; o[7] = 0;
}

__global__ __launch_bounds__(kThreads) void k_stats(StatsArgs a) {
    __shared__ unsigned long long s_add[3];
    __shared__ int s_box[4];
    const int t = threadIdx.x;
    if (t < 3) s_add[t] = 0;
    if (t == 0) { s_box[0] = a.d.W; s_box[1] = a.d.H; s_box[2] = -1; s_box[3] = -1; }
    __syncthreads();
    const int i = (int)(blockIdx.x / (uint32_t)a.nblk);
    const uint32_t blk = blockIdx.x - (uint32_t)i * (uint32_t)a.nblk;
    const int64_t npix = (int64_t)a.d.H * a.d.W;
    const int64_t *s = a.d.label_strides;
    unsigned long long n = 0, sx = 0, sy = 0;
    int x0 = a.d.W, y0 = a.d.H, x1 = -1, y1 = -1;
    // consecutive lanes on consecutive pixels
    for (int j = 0; j < kStatPx; ++j) {
        const int64_t p = ((int64_t)blk * kStatPx + j) * kThreads + t;
        if (p >= npix) break;
        const int y = (int)(p / a.d.W), x = (int)(p - (int64_t)y * a.d.W);
        const int64_t v = load_label(a.d.label, a.d.label_kind, (int64_t)i * s[0] + (int64_t)y * s[1] + (int64_t)x * s[2]);
        if (v >= 1 && v <= a.ncls) {
            ++n; sx += (unsigned)x; sy += (unsigned)y;
            x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
        }
    }
    if (n) {
        atomicAdd(&s_add[0], n); atomicAdd(&s_add[1], sx); atomicAdd(&s_add[2], sy);
        atomicMin(&s_box[0], x0); atomicMin(&s_box[1], y0); atomicMax(&s_box[2], x1); atomicMax(&s_box[3], y1);
    }
    __syncthreads();
    if (s_add[0] == 0) return;
    int64_t *o = a.stats + (int64_t)i * 8;
    if (t < 3) atomicAdd((unsigned long long *)&o[t], s_add[t]);
    else if (t < 5) atomicMin((long long *)&o[t], (long long)s_box[t - 3]);
    else if (t < 7) atomicMax((long long *)&o[t], (long long)s_box[t - 3]);
}

// ---- pv_augment_params -----------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

struct ParamArgs {
    pv_aug_ranges r;
    const int64_t *stats;
    const uint64_t *state;
    double *fwd, *inv;
    float *color;
};

__global__ void k_params(ParamArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.r.b) return;
    constexpr uint64_t G = 0x9E3779B97F4A7C15ull;
    const uint64_t seed = a.state[0], n = a.state[1] + (uint64_t)i;
    const uint64_t base = mix64(mix64(seed + G) + (n + 1) * G);
    double u[PV_AUG_DRAWS];
#pragma unroll
    for (int k = 0; k < PV_AUG_DRAWS; ++k)
        u[k] = (double)(mix64(base + (uint64_t)(k + 1) * G) >> 11) * (1.0 / 9007199254740992.0);
    const double theta = (a.r.rot_deg[0] + u[0] * (a.r.rot_deg[1] - a.r.rot_deg[0])) * (3.141592653589793 / 180.0);
    const double s = a.r.scale[0] + u[1] * (a.r.scale[1] - a.r.scale[0]);
    const double span = 1.0 - 2.0 * a.r.margin;
    const double tx = (a.r.margin + u[2] * span) * (double)(a.r.Wo - 1);
    const double ty = (a.r.margin + u[3] * span) * (double)(a.r.Ho - 1);
    const int64_t *st = a.stats + (int64_t)i * 8;
    double cx, cy;
    if (st[0] > 0) {
        cx = (double)st[1] / (double)st[0];
        cy = (double)st[2] / (double)st[0];
    } else {
        cx = (double)(a.r.W - 1) / 2.0;
        cy = (double)(a.r.H - 1) / 2.0;
    }
    const double ca = s * cos(theta), q = s * sin(theta);
    const double f02 = tx - (ca * cx - q * cy), f12 = ty - (q * cx + ca * cy);
    double *f = a.fwd + (int64_t)i * 6, *m = a.inv + (int64_t)i * 6;
    f[0] = ca; f[1] = -q; f[2] = f02;
    f[3] = q;  f[4] = ca; f[5] = f12;
    const double d = ca * ca + q * q, ia = ca / d, iq = q / d;
    m[0] = ia;  m[1] = iq; m[2] = -(ia * f02 + iq * f12);
    m[3] = -iq; m[4] = ia; m[5] = iq * f02 - ia * f12;
    float *c = a.color + (int64_t)i * 4;
    c[0] = (float)(1.0 + a.r.jitter[0] * (2.0 * u[4] - 1.0));
    c[1] = (float)(1.0 + a.r.jitter[1] * (2.0 * u[5] - 1.0));
    c[2] = (float)(1.0 + a.r.jitter[2] * (2.0 * u[6] - 1.0));
    c[3] = (float)(a.r.jitter[3] * (2.0 * u[7] - 1.0));
}

// ---- pv_augment_apply --------------------------------------------------------------------------------------
struct ApplyArgs {
    pv_aug_desc d;
    double *part;        // [b][nblk]
    int32_t nblk;        // blocks per image
    int32_t gw;          // groups of kPx pixels per output row
    float rstd[3];       // 1.0f / std
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float grey(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }

// colorsys.rgb_to_hsv, the shift, colorsys.hsv_to_rgb, in f32.  Selects, no branches: on an image with
// colour every sector occurs in every wave, and a branch per sector ran them all one after another.
__device__ __forceinline__ void hue_shift(float &r, float &g, float &b, float eta) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool flat = minc == maxc;               // h = 0, s = 0: hsv_to_rgb gives (v, v, v) back
    const float rng = maxc - minc, v = maxc;
    const float den = flat ? 1.0f : rng;          // a flat pixel divides by 1 and is dropped at the end
    const float s = rng / (flat ? 1.0f : maxc);
    const float rc_ = (maxc - r) / den, gc = (maxc - g) / den, bc = (maxc - b) / den;
    float h = r == maxc ? bc - gc : (g == maxc ? (2.0f + rc_) - bc : (4.0f + gc) - rc_);
    h = h / 6.0f;
    h = h - floorf(h);
    h = h + eta;
    h = h - floorf(h);
    const float h6 = h * 6.0f;
    const float fi = floorf(h6);
    const float f = h6 - fi;
    const float p = v * (1.0f - s), q = v * (1.0f - s * f), t = v * (1.0f - s * (1.0f - f));
    const int sec = (int)fi;                      // 0..6; 6 (h rounded up to 1) is sector 0
    // sector:        0  1  2  3  4  5
    //   r            v  q  p  p  t  v
    //   g            t  v  v  q  p  p
    //   b            p  p  t  v  v  q
    const float nr = sec == 1 ? q : ((sec == 2 || sec == 3) ? p : (sec == 4 ? t : v));
    const float ng = (sec == 1 || sec == 2) ? v : (sec == 3 ? q : ((sec == 4 || sec == 5) ? p : t));
    const float nb = sec == 2 ? t : ((sec == 3 || sec == 4) ? v : (sec == 5 ? q : p));
    r = flat ? r : nr;
    g = flat ? g : ng;
    b = flat ? b : nb;
}

template <typename TO>
__device__ __forceinline__ void store8(TO *p, int64_t sx, int n, const float (&v)[kPx]);

template <>
__device__ __forceinline__ void store8<float>(float *p, int64_t sx, int n, const float (&v)[kPx]) {
    if (sx == 1 && n == kPx && ((uintptr_t)p & 15) == 0) {
        *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
        *(float4 *)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int e = 0; e < kPx; ++e)
            if (e < n) p[e * sx] = v[e];
    }
}

__device__ __forceinline__ uint32_t f2h(float v) {     // round to nearest even, as __float2half_rn
    return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)v);
}

template <>
__device__ __forceinline__ void store8<__half>(__half *p, int64_t sx, int n, const float (&v)[kPx]) {
    if (sx == 1 && n == kPx && ((uintptr_t)p & 15) == 0) {
        *(uint4 *)p = make_uint4(f2h(v[0]) | (f2h(v[1]) << 16), f2h(v[2]) | (f2h(v[3]) << 16),
                                 f2h(v[4]) | (f2h(v[5]) << 16), f2h(v[6]) | (f2h(v[7]) << 16));
    } else {
#pragma unroll
        for (int e = 0; e < kPx; ++e)
            if (e < n) p[e * sx] = __float2half_rn(v[e]);
    }
}

__device__ __forceinline__ void store_labels(const ApplyArgs &a, int i, int y, int x, int n, const int64_t (&lab)[kPx]) {
    const int64_t *s = a.d.out_label_strides;
    const int64_t o = (int64_t)i * s[0] + (int64_t)y * s[1] + (int64_t)x * s[2];
    if (a.d.label_kind == PV_AUG_LABEL_U8) {
        uint8_t *p = (uint8_t *)a.d.out_label + o;
        if (s[2] == 1 && n == kPx && ((uintptr_t)p & 7) == 0) {
            uint2 w = make_uint2(0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                w.x |= ((uint32_t)lab[e] & 255u) << (8 * e);
                w.y |= ((uint32_t)lab[e + 4] & 255u) << (8 * e);
            }
            *(uint2 *)p = w;
        } else {
#pragma unroll
            for (int e = 0; e < kPx; ++e)
                if (e < n) p[e * s[2]] = (uint8_t)lab[e];
        }
    } else if (a.d.label_kind == PV_AUG_LABEL_I32) {
        int32_t *p = (int32_t *)a.d.out_label + o;
#pragma unroll
        for (int e = 0; e < kPx; ++e)
            if (e < n) p[e * s[2]] = (int32_t)lab[e];
    } else {
        int64_t *p = (int64_t *)a.d.out_label + o;
#pragma unroll
        for (int e = 0; e < kPx; ++e)
            if (e < n) p[e * s[2]] = lab[e];
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

// The offsets inside one image are 32-bit (the host vouches that every image spans at most 2^31 - 1
// elements); only the image's base is 64-bit.
struct Strides32 {
    int32_t is1, is2, is3;   // image: row, pixel, channel
    int32_t ls1, ls2;        // label
    int32_t bs1, bs2, bs3;   // background
};

// Phase A: the source coordinates of the lane's pixels and their labels.  Every load is issued whatever
// the range check says, at coordinates clamped into the source, and a select drops what the check
// rejects: eight independent loads in flight, none behind a branch.  The range is checked in fp64 before
// any conversion to an integer.
template <typename TL>
__device__ __forceinline__ void labels8(const TL *lab_i, const Strides32 &q, int W, int H, const double (&sx)[kPx],
                                        const double (&sy)[kPx], int64_t (&lab)[kPx]) {
    TL v[kPx];
    bool in[kPx];
#pragma unroll
    for (int e = 0; e < kPx; ++e) {
        const double rx = rint(sx[e]), ry = rint(sy[e]);
        in[e] = rx >= 0.0 && rx <= (double)(W - 1) && ry >= 0.0 && ry <= (double)(H - 1);
        const int cx = (int)(in[e] ? rx : 0.0), cy = (int)(in[e] ? ry : 0.0);
        v[e] = lab_i[cy * q.ls1 + cx * q.ls2];
    }
#pragma unroll
    for (int e = 0; e < kPx; ++e) lab[e] = in[e] ? (int64_t)v[e] : 0;
}

// Phase B: one pixel's colour on the 0..255 scale.  The four taps are loaded at clamped coordinates,
// unconditionally, and a tap outside the source is replaced by the fill afterwards.
__device__ __forceinline__ void bilinear(const uint8_t *img_i, const Strides32 &q, int W, int H, const float (&fill)[3],
                                         double sx, double sy, float (&c)[3]) {
    const double fx = floor(sx), fy = floor(sy);
    const bool any = fx >= -1.0 && fx <= (double)(W - 1) && fy >= -1.0 && fy <= (double)(H - 1);
    const int ix = (int)(any ? fx : 0.0), iy = (int)(any ? fy : 0.0);      // in [-1, W - 1] x [-1, H - 1]
    const float wx = (float)(sx - fx), wy = (float)(sy - fy);
    const bool x0 = ix >= 0, x1 = ix + 1 <= W - 1, y0 = iy >= 0, y1 = iy + 1 <= H - 1;
    const int r0 = max(iy, 0) * q.is1, r1 = min(iy + 1, H - 1) * q.is1;
    const int c0 = max(ix, 0) * q.is2, c1 = min(ix + 1, W - 1) * q.is2;
    uint8_t t[3][4];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const uint8_t *p = img_i + ch * q.is3;
        t[ch][0] = p[r0 + c0]; t[ch][1] = p[r0 + c1]; t[ch][2] = p[r1 + c0]; t[ch][3] = p[r1 + c1];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float f = fill[ch];
        const float v00 = (y0 && x0) ? (float)t[ch][0] : f, v01 = (y0 && x1) ? (float)t[ch][1] : f;
        const float v10 = (y1 && x0) ? (float)t[ch][2] : f, v11 = (y1 && x1) ? (float)t[ch][3] : f;
        const float top = v00 + wx * (v01 - v00), bot = v10 + wx * (v11 - v10);
        c[ch] = any ? top + wy * (bot - top) : f;
    }
}

template <typename TO, int MODE>
__global__ __launch_bounds__(kThreads) void k_apply(ApplyArgs a, Strides32 q) {
    __shared__ double red[MODE == 0 ? 1 : kThreads];
    (void)red;
    const pv_aug_desc &d = a.d;
    const int i = (int)(blockIdx.x / (uint32_t)a.nblk);
    const uint32_t blk = blockIdx.x - (uint32_t)i * (uint32_t)a.nblk;
    const int64_t t = (int64_t)blk * kThreads + threadIdx.x;
    const int y = (int)(t / a.gw);
    const int x = (int)(t - (int64_t)y * a.gw) * kPx;
    const int n = y < d.Ho ? min(kPx, d.Wo - x) : 0;

    float mterm = 0.f;
    const float beta = d.color[i * 4 + 0], kappa = d.color[i * 4 + 1], sigma = d.color[i * 4 + 2], eta = d.color[i * 4 + 3];
    if (MODE == 2) {
        double acc = 0.0;
        const double *pp = a.part + (int64_t)i * a.nblk;
        for (int k = threadIdx.x; k < a.nblk; k += kThreads) acc += pp[k];
        block_sum(red, acc);
        const float m = (float)(red[0] / (double)((int64_t)d.Ho * d.Wo));
        mterm = (1.0f - kappa) * m;
    }
    if (MODE != 1 && n == 0) return;

    // a lane past the image's last row (n == 0, MODE 1 only) works on row 0 and adds nothing
    const int yy = n ? y : 0, xx = n ? x : 0;
    const double *M = d.inv + (int64_t)i * 6;
    const double ay0 = M[1] * (double)yy, ay1 = M[4] * (double)yy;
    double sx[kPx], sy[kPx];
#pragma unroll
    for (int e = 0; e < kPx; ++e) {
        sx[e] = (M[0] * (double)(xx + e) + ay0) + M[2];
        sy[e] = (M[3] * (double)(xx + e) + ay1) + M[5];
    }
    int64_t lab[kPx];
    const int64_t lbase = (int64_t)i * d.label_strides[0];
    if (d.label_kind == PV_AUG_LABEL_U8) labels8((const uint8_t *)d.label + lbase, q, d.W, d.H, sx, sy, lab);
    else if (d.label_kind == PV_AUG_LABEL_I32) labels8((const int32_t *)d.label + lbase, q, d.W, d.H, sx, sy, lab);
    else labels8((const int64_t *)d.label + lbase, q, d.W, d.H, sx, sy, lab);

    const uint8_t *img_i = (const uint8_t *)d.image + (int64_t)i * d.image_strides[0];
    const uint8_t *bg_row = d.background
        ? (const uint8_t *)d.background + (int64_t)i * d.background_strides[0] + yy * q.bs1 : nullptr;
    float o[3][kPx];
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < kPx; ++e) {
        float c[3];
        if (bg_row && lab[e] == 0) {
            const uint8_t *p = bg_row + min(xx + e, d.Wo - 1) * q.bs2;      // clamped: a pixel past the row's end reads its last
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] = (float)p[ch * q.bs3];
        } else {
            bilinear(img_i, q, d.W, d.H, d.fill, sx[e], sy[e], c);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            c[ch] = c[ch] * (1.0f / 255.0f);
            if (d.flags & PV_AUG_BRIGHTNESS) c[ch] = clamp01(beta * c[ch]);
        }
        if (MODE == 1) {
            if (e < n) acc += (double)grey(c[0], c[1], c[2]);
        } else {
            if (MODE == 2) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch] = clamp01(kappa * c[ch] + mterm);
            }
            if (d.flags & PV_AUG_SATURATION) {
                const float g = (1.0f - sigma) * grey(c[0], c[1], c[2]);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) c[ch] = clamp01(sigma * c[ch] + g);
            }
            if (d.flags & PV_AUG_HUE) hue_shift(c[0], c[1], c[2], eta);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[ch][e] = (c[ch] - d.mean[ch]) * a.rstd[ch];
        }
    }
    if (MODE == 1) {
        block_sum(red, acc);
        if (threadIdx.x == 0) a.part[blockIdx.x] = red[0];
        return;
    }
    const int64_t *s = d.out_image_strides;
    TO *po = (TO *)d.out_image + (int64_t)i * s[0] + (int64_t)y * s[2] + (int64_t)x * s[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) store8<TO>(po + ch * s[1], s[3], n, o[ch]);
    store_labels(a, i, y, x, n, lab);
}

// ---- host ----------------------------------------------------------------------------------------------
bool dim_ok(int32_t v) { return v >= 1 && v <= PV_AUG_MAX_DIM; }
bool label_kind_ok(int32_t k) { return k == PV_AUG_LABEL_I64 || k == PV_AUG_LABEL_U8 || k == PV_AUG_LABEL_I32; }
uintptr_t label_mask(int32_t k) { return k == PV_AUG_LABEL_I64 ? 7 : k == PV_AUG_LABEL_I32 ? 3 : 0; }
bool is_finite(double v) { return v - v == 0.0; }

// a launch stays below 2^32 threads, which is what the runtime accepts: at most 2^24 - 1 blocks of kThreads lanes
constexpr int64_t kMaxBlocks = ((int64_t)1 << 32) / kThreads - 1;

int32_t groups_per_row(int32_t W) { return (W + kPx - 1) / kPx; }
// blocks per image of k_apply (a lane: kPx pixels of a row); 0 if the flattened grid would exceed kMaxBlocks
int64_t apply_blocks(int32_t b, int32_t Ho, int32_t Wo) {
    const int64_t nblk = ((int64_t)Ho * groups_per_row(Wo) + kThreads - 1) / kThreads;
    return nblk * std::max<int64_t>(b, 1) <= kMaxBlocks ? nblk : 0;
}
// blocks per image of k_stats (a block: kStatPx * kThreads pixels)
int64_t stats_blocks(int32_t b, int32_t H, int32_t W) {
    const int64_t nblk = ((int64_t)H * W + (int64_t)kStatPx * kThreads - 1) / ((int64_t)kStatPx * kThreads);
    return nblk * std::max<int64_t>(b, 1) <= kMaxBlocks ? nblk : 0;
}

// elements from the first to the last of an [n0][n1][n2] array with these strides (n2 == 1: two dimensions)
int64_t span(const int64_t *s, int64_t n0, int64_t n1, int64_t n2) {
    return (n0 - 1) * s[0] + (n1 - 1) * s[1] + (n2 > 1 ? (n2 - 1) * s[2] : 0);
}

}  // namespace

extern "C" {

size_t pv_augment_workspace_size(int32_t b, int32_t Ho, int32_t Wo) {
    if (b < 0 || !dim_ok(Ho) || !dim_ok(Wo)) return 0;
    const int64_t nblk = apply_blocks(b, Ho, Wo);
    if (nblk == 0) return 0;
    return (size_t)align_up(nblk * b * 8, 256) + 256;
}

int pv_label_stats(const pv_aug_label *d, int32_t ncls, int64_t *stats, pv_stream_t stream) {
    if (!d) return PV_EINVAL;
    if (d->b < 0 || !dim_ok(d->H) || !dim_ok(d->W) || ncls < 1 || ncls > PV_AUG_MAX_CLASSES) return PV_EINVAL;
    if (!label_kind_ok(d->label_kind)) return PV_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->label_strides[i] < 0) return PV_EINVAL;
    const int64_t nblk = stats_blocks(d->b, d->H, d->W);
    if (nblk == 0) return PV_EINVAL;
    if (d->b == 0) return PV_OK;
    if (!d->label || !stats) return PV_EINVAL;
    if (((uintptr_t)d->label & label_mask(d->label_kind)) || ((uintptr_t)stats & 7)) return PV_EALIGN;
    hipStream_t st = (hipStream_t)stream;
    k_stats_init<<<dim3((unsigned)((d->b + kThreads - 1) / kThreads)), kThreads, 0, st>>>(stats, d->b, d->H, d->W);
    int e;
    if ((e = last())) return e;
    StatsArgs a{*d, stats, ncls, (int32_t)nblk};
    k_stats<<<dim3((unsigned)(nblk * d->b)), kThreads, 0, st>>>(a);
    return last();
}

int pv_augment_params(const pv_aug_ranges *r, const int64_t *stats, const uint64_t *state, double *fwd, double *inv,
                      float *color, pv_stream_t stream) {
    if (!r) return PV_EINVAL;
    if (r->b < 0 || !dim_ok(r->H) || !dim_ok(r->W) || !dim_ok(r->Ho) || !dim_ok(r->Wo)) return PV_EINVAL;
    if (!is_finite(r->rot_deg[0]) || !is_finite(r->rot_deg[1]) || !(r->rot_deg[0] <= r->rot_deg[1])) return PV_EINVAL;
    if (!is_finite(r->scale[0]) || !is_finite(r->scale[1]) || !(r->scale[0] > 0.0) || !(r->scale[0] <= r->scale[1])) return PV_EINVAL;
    if (!(r->margin >= 0.0) || !(r->margin <= 0.5)) return PV_EINVAL;
    for (int k = 0; k < 4; ++k)
        if (!(r->jitter[k] >= 0.0) || !(r->jitter[k] <= (k == 3 ? 0.5 : 1.0))) return PV_EINVAL;
    if (r->b == 0) return PV_OK;
    if (!stats || !state || !fwd || !inv || !color) return PV_EINVAL;
    if ((((uintptr_t)stats | (uintptr_t)state | (uintptr_t)fwd | (uintptr_t)inv) & 7) || ((uintptr_t)color & 3)) return PV_EALIGN;
    ParamArgs a{*r, stats, state, fwd, inv, color};
    k_params<<<dim3((unsigned)((r->b + 63) / 64)), 64, 0, (hipStream_t)stream>>>(a);
    return last();
}

int pv_augment_apply(const pv_aug_desc *d, void *workspace, size_t workspace_bytes, pv_stream_t stream) {
    if (!d) return PV_EINVAL;
    if (d->b < 0 || !dim_ok(d->H) || !dim_ok(d->W) || !dim_ok(d->Ho) || !dim_ok(d->Wo)) return PV_EINVAL;
    if (!label_kind_ok(d->label_kind) || (d->out_kind != PV_AUG_F32 && d->out_kind != PV_AUG_F16)) return PV_EINVAL;
    if (d->flags < 0 || d->flags > (PV_AUG_BRIGHTNESS | PV_AUG_CONTRAST | PV_AUG_SATURATION | PV_AUG_HUE)) return PV_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (d->image_strides[i] < 0 || d->background_strides[i] < 0 || d->out_image_strides[i] < 0) return PV_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->label_strides[i] < 0 || d->out_label_strides[i] < 0) return PV_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (!(d->fill[i] >= 0.f) || !(d->fill[i] <= 255.f) || !is_finite(d->mean[i]) || !is_finite(d->std[i]) || !(d->std[i] > 0.f))
            return PV_EINVAL;
    // an image, a label map and a background each span at most 2^31 - 1 elements: the kernel's offsets inside one are 32-bit
    if (span(d->image_strides + 1, d->H, d->W, 3) > INT32_MAX || span(d->label_strides + 1, d->H, d->W, 1) > INT32_MAX ||
        (d->background && span(d->background_strides + 1, d->Ho, d->Wo, 3) > INT32_MAX))
        return PV_EINVAL;
    const int64_t nblk = apply_blocks(d->b, d->Ho, d->Wo);
    if (nblk == 0) return PV_EINVAL;
    if (d->b == 0) return PV_OK;
    if (!d->image || !d->label || !d->inv || !d->color || !d->out_image || !d->out_label) return PV_EINVAL;
    const bool contrast = (d->flags & PV_AUG_CONTRAST) != 0;
    if (contrast) {
        const size_t need = pv_augment_workspace_size(d->b, d->Ho, d->Wo);
        if (!workspace || workspace_bytes < need) return PV_EWORKSPACE;
        if ((uintptr_t)workspace & 255) return PV_EALIGN;
    }
    const uintptr_t lm = label_mask(d->label_kind), om = d->out_kind == PV_AUG_F32 ? 3 : 1;
    if (((uintptr_t)d->label & lm) || ((uintptr_t)d->out_label & lm) || ((uintptr_t)d->out_image & om) ||
        ((uintptr_t)d->inv & 7) || ((uintptr_t)d->color & 3))
        return PV_EALIGN;

    ApplyArgs a{};
    a.d = *d;
    a.part = (double *)workspace;
    a.nblk = (int32_t)nblk;
    a.gw = groups_per_row(d->Wo);
    for (int i = 0; i < 3; ++i) a.rstd[i] = 1.0f / d->std[i];
    const Strides32 q{(int32_t)d->image_strides[1], (int32_t)d->image_strides[2], (int32_t)d->image_strides[3],
                      (int32_t)d->label_strides[1], (int32_t)d->label_strides[2],
                      (int32_t)d->background_strides[1], (int32_t)d->background_strides[2], (int32_t)d->background_strides[3]};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(nblk * d->b));
    const bool f32 = d->out_kind == PV_AUG_F32;
    if (contrast) {
        k_apply<float, 1><<<grid, kThreads, 0, st>>>(a, q);
        int e;
        if ((e = last())) return e;
        if (f32) k_apply<float, 2><<<grid, kThreads, 0, st>>>(a, q);
        else k_apply<__half, 2><<<grid, kThreads, 0, st>>>(a, q);
    } else {
        if (f32) k_apply<float, 0><<<grid, kThreads, 0, st>>>(a, q);
        else k_apply<__half, 0><<<grid, kThreads, 0, st>>>(a, q);
    }
    return last();
}

}  // extern "C"
