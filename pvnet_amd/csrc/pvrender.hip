// pvrender.hip -- libpvrender.so (include/pvrender.h): label / instance / depth maps from meshes and
// poses through a z-buffer, and the unit vector field from a label map and keypoints.  One
// translation unit that includes no other csrc/ file, so the other three libraries' sources do
// not rebuild it.
//
// pv_render_labels is five launches on the caller's stream:
//   k_clear    keys <- all ones, instance records and won counts <- 0
//   k_inst     one thread per image: its instance range, each instance validated into a record
//   k_project  one thread per (instance, vertex): fp64 transform, snap to 1/256 px
//   k_raster   one lane per triangle for setup; a triangle whose clipped box holds at most
//              kSmallPx samples is walked by its own lane, a larger one is handed to the whole
//              wave, which strides over 8x8 sample blocks of its box (blockIdx.y slices those
//              blocks further, so a 12-triangle box still fills the device).  Coverage is int64 edge
//              functions; a covered sample does one 64-bit integer atomicMin on
//              (f32 depth bits << 32 | instance index), which is order-independent.
//   k_resolve  key -> label / inst / depth, and the won-pixel counts (integer atomicAdd)
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pvrender.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSmallPx = 32;             // samples in a clipped box a single lane walks
constexpr int kMaxSlices = 256;
constexpr uint64_t kEmpty = ~0ull;
constexpr int32_t kInvalid = PV_RENDER_SNAP_INVALID;

inline int rc(hipError_t e) { return e == hipSuccess ? PV_OK : (int)e; }
inline int last() { return rc(hipGetLastError()); }
inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

inline int cu_count() {
    static const int n = [] {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 0;
        return cus > 0 ? cus : 256;
    }();
    return n;
}

// one instance, validated by k_inst; nf == 0: skipped
struct InstRec {
    int32_t vlo, nv, flo, nf, img, local, label, pad;
};

struct Work {
    uint64_t *keys;     // [b][H][W]
    double *pz;         // [total_inst][max_verts]
    int32_t *pxy;       // [total_inst][max_verts][2]
    InstRec *rec;       // [total_inst]
    int32_t *img_base;  // [b]
    size_t bytes;
};

inline Work carve(void *base, int64_t npix, int64_t total_iv, int64_t total_inst, int64_t b) {
    Work w{};
    int64_t off = 0;
    char *p = (char *)base;
    w.keys = (uint64_t *)(p + off);  off = align_up(off + npix * 8, 256);
    w.pz = (double *)(p + off);      off = align_up(off + total_iv * 8, 256);
    w.pxy = (int32_t *)(p + off);    off = align_up(off + total_iv * 8, 256);
    w.rec = (InstRec *)(p + off);    off = align_up(off + total_inst * (int64_t)sizeof(InstRec), 256);
    w.img_base = (int32_t *)(p + off); off = align_up(off + b * 4, 256);
    w.bytes = (size_t)off;
    return w;
}

struct RenderArgs {
    Work w;
    pv_render_meshes m;
    pv_render_batch bt;
    pv_render_out out;
    int64_t npix;       // b * H * W
    int32_t vchunks, fchunks;
};

// --------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_clear(RenderArgs a) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (2 * t + 1 < a.npix)
        *(ulonglong2 *)(a.w.keys + 2 * t) = make_ulonglong2(kEmpty, kEmpty);
    else if (2 * t < a.npix)
        a.w.keys[2 * t] = kEmpty;
    if (t < a.bt.total_inst) {
        a.w.rec[t] = InstRec{0, 0, 0, 0, 0, 0, 0, 0};
        if (a.out.won) a.out.won[t] = 0;
    }
    if (t < a.bt.b) a.w.img_base[t] = 0;
}

__global__ __launch_bounds__(64) void k_inst(RenderArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.bt.b) return;
    int64_t lo, hi;
    if (a.bt.inst_off) {
        lo = a.bt.inst_off[i];
        hi = a.bt.inst_off[i + 1];
    } else {
        lo = (int64_t)i * a.bt.ninst;
        hi = lo + a.bt.ninst;
    }
    if (lo < 0 || hi < lo || hi > a.bt.total_inst) return;            // no instances
    a.w.img_base[i] = (int32_t)lo;
    for (int64_t g = lo; g < hi; ++g) {
        const int mid = a.bt.model_id[g], lab = a.bt.label[g];
        if (mid < 0 || mid >= a.m.nmodels || lab < 1 || lab > 255) continue;
        const int vl = a.m.vert_off[mid], vh = a.m.vert_off[mid + 1];
        const int fl = a.m.face_off[mid], fh = a.m.face_off[mid + 1];
        if (vl < 0 || vh < vl || vh > a.m.total_v || vh - vl > a.m.max_verts) continue;
        if (fl < 0 || fh < fl || fh > a.m.total_f || fh - fl > a.m.max_faces) continue;
        bool finite = true;
        for (int e = 0; e < 12; ++e) finite = finite && isfinite(a.bt.pose[g * 12 + e]);
        if (!finite) continue;
        a.w.rec[g] = InstRec{vl, vh - vl, fl, fh - fl, i, (int32_t)(g - lo), lab, 0};
    }
}

__global__ __launch_bounds__(kThreads) void k_project(RenderArgs a) {
    const int g = blockIdx.x / a.vchunks, chunk = blockIdx.x - g * a.vchunks;
    const InstRec r = a.w.rec[g];
    const int v = chunk * kThreads + threadIdx.x;
    if (r.nf == 0 || v >= r.nv) return;
    const float *p = a.m.verts + (int64_t)(r.vlo + v) * 3;
    const double x = p[0], y = p[1], z = p[2];
    const double *P = a.bt.pose + (int64_t)g * 12;
    const double *K = a.bt.K + (int64_t)r.img * a.bt.K_stride;
    const double X = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const double Y = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const double Z = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    const double u = (K[0] * X + K[1] * Y) / Z + K[2];
    const double vv = (K[4] * Y) / Z + K[5];
    const double su = rint(u * 256.0), sv = rint(vv * 256.0);
    const double lim = (double)PV_RENDER_MAX_SNAP;
    // NaN fails every comparison, so a non-finite u or v lands in the else branch
    const bool ok = isfinite(X) && isfinite(Y) && isfinite(Z) && Z >= a.bt.znear && fabs(su) <= lim && fabs(sv) <= lim;
    const int32_t sx = ok ? (int32_t)su : kInvalid, sy = ok ? (int32_t)sv : kInvalid;
    const int64_t slot = (int64_t)g * a.m.max_verts + v;
    *(int2 *)(a.w.pxy + slot * 2) = make_int2(sx, sy);
    a.w.pz[slot] = Z;
    if (a.out.snap_xy) *(int2 *)(a.out.snap_xy + slot * 2) = make_int2(sx, sy);
    if (a.out.snap_z) a.out.snap_z[slot] = Z;
}

// a triangle oriented to positive doubled area, with its box clipped to the image
struct Tri {
    int32_t x0, y0, x1, y1, x2, y2;
    int32_t bx0, by0, bx1, by1;
    double q0, q1, q2;                   // 1 / Z of the three vertices
};

// directed edge a -> b at the sample (X, Y), all in 1/256 px; every difference fits int32
// (|coordinates| <= 2^29, samples in [0, 2^28]), every product int64
__device__ __forceinline__ bool edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t X, int32_t Y, int64_t *E) {
    const int32_t dx = bx - ax, dy = by - ay;
    const int64_t e = (int64_t)dx * (int64_t)(Y - ay) - (int64_t)dy * (int64_t)(X - ax);
    *E = e;
    return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));      // top-left rule, y down
}

__device__ __forceinline__ void shade(const Tri &t, int px, int py, uint64_t *img_keys, int W, uint32_t local) {
    const int32_t X = px << PV_RENDER_SUBPIXEL_BITS, Y = py << PV_RENDER_SUBPIXEL_BITS;
    int64_t w0, w1, w2;
    const bool c2 = edge(t.x0, t.y0, t.x1, t.y1, X, Y, &w2);
    const bool c0 = edge(t.x1, t.y1, t.x2, t.y2, X, Y, &w0);
    const bool c1 = edge(t.x2, t.y2, t.x0, t.y0, X, Y, &w1);
    if (!(c0 && c1 && c2)) return;
    const double num = ((double)w0 * t.q0 + (double)w1 * t.q1) + (double)w2 * t.q2;
    const double Z = 1.0 / (num / (double)(w0 + w1 + w2));
    const uint64_t key = ((uint64_t)__float_as_uint((float)Z) << 32) | local;
    uint64_t *k = img_keys + (int64_t)py * W + px;
    // the plain read may be stale, never too small: the minimum only falls
    if (key < *(volatile uint64_t *)k) atomicMin((unsigned long long *)k, (unsigned long long)key);
}

__device__ __forceinline__ int rl(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double rld(double v, int src) {
    const int lo = rl(__double2loint(v), src), hi = rl(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kThreads) void k_raster(RenderArgs a) {
    const int g = blockIdx.x / a.fchunks, chunk = blockIdx.x - g * a.fchunks;
    const int slice = blockIdx.y, nslices = gridDim.y;
    const InstRec r = a.w.rec[g];
    if (chunk * kThreads >= r.nf) return;                              // whole block past the model (or skipped)
    const int f = chunk * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int W = a.bt.W, H = a.bt.H;
    uint64_t *img_keys = a.w.keys + (int64_t)r.img * H * W;

    Tri t{};
    bool ok = f < r.nf;
    if (ok) {
        const int32_t *F = a.m.faces + (int64_t)(r.flo + f) * 3;
        const int i0 = F[0], i1 = F[1], i2 = F[2];
        ok = (unsigned)i0 < (unsigned)r.nv && (unsigned)i1 < (unsigned)r.nv && (unsigned)i2 < (unsigned)r.nv;
        if (ok) {
            const int64_t base = (int64_t)g * a.m.max_verts;
            const int2 p0 = *(const int2 *)(a.w.pxy + (base + i0) * 2);
            int2 p1 = *(const int2 *)(a.w.pxy + (base + i1) * 2);
            int2 p2 = *(const int2 *)(a.w.pxy + (base + i2) * 2);
            ok = p0.x != kInvalid && p1.x != kInvalid && p2.x != kInvalid;
            if (ok) {
                double z0 = a.w.pz[base + i0], z1 = a.w.pz[base + i1], z2 = a.w.pz[base + i2];
                const int64_t area = (int64_t)(p1.x - p0.x) * (int64_t)(p2.y - p0.y) -
                                     (int64_t)(p2.x - p0.x) * (int64_t)(p1.y - p0.y);
                if (area < 0) {
                    const int2 tp = p1; p1 = p2; p2 = tp;
                    const double tz = z1; z1 = z2; z2 = tz;
                }
                t.x0 = p0.x; t.y0 = p0.y; t.x1 = p1.x; t.y1 = p1.y; t.x2 = p2.x; t.y2 = p2.y;
                t.q0 = 1.0 / z0; t.q1 = 1.0 / z1; t.q2 = 1.0 / z2;
                const int mnx = min(p0.x, min(p1.x, p2.x)), mxx = max(p0.x, max(p1.x, p2.x));
                const int mny = min(p0.y, min(p1.y, p2.y)), mxy = max(p0.y, max(p1.y, p2.y));
                // samples x with 256 x in [mnx, mxx]: ceil and floor by arithmetic shifts
                t.bx0 = max(0, (mnx + 255) >> 8); t.bx1 = min(W - 1, mxx >> 8);
                t.by0 = max(0, (mny + 255) >> 8); t.by1 = min(H - 1, mxy >> 8);
                ok = area != 0 && t.bx0 <= t.bx1 && t.by0 <= t.by1;
            }
        }
    }
    const int bw = ok ? t.bx1 - t.bx0 + 1 : 0, bh = ok ? t.by1 - t.by0 + 1 : 0;
    const int64_t npx = (int64_t)bw * bh;
    const bool small = ok && npx <= kSmallPx;

    if (slice == 0 && small) {
        int x = t.bx0, y = t.by0;
        for (int k = 0; k < (int)npx; ++k) {
            shade(t, x, y, img_keys, W, (uint32_t)r.local);
            if (++x > t.bx1) { x = t.bx0; ++y; }
        }
    }

    uint64_t big = __ballot(ok && !small);
    while (big) {
        const int src = __ffsll((unsigned long long)big) - 1;
        big &= big - 1;
        Tri s;
        s.x0 = rl(t.x0, src); s.y0 = rl(t.y0, src); s.x1 = rl(t.x1, src); s.y1 = rl(t.y1, src);
        s.x2 = rl(t.x2, src); s.y2 = rl(t.y2, src);
        s.bx0 = rl(t.bx0, src); s.by0 = rl(t.by0, src); s.bx1 = rl(t.bx1, src); s.by1 = rl(t.by1, src);
        s.q0 = rld(t.q0, src); s.q1 = rld(t.q1, src); s.q2 = rld(t.q2, src);
        const int nbx = (s.bx1 - s.bx0 + 8) >> 3, nby = (s.by1 - s.by0 + 8) >> 3;
        const int64_t nblk = (int64_t)nbx * nby;
        for (int64_t blk = slice; blk < nblk; blk += nslices) {
            const int byi = (int)(blk / nbx), bxi = (int)(blk - (int64_t)byi * nbx);
            const int px = s.bx0 + bxi * 8 + (lane & 7), py = s.by0 + byi * 8 + (lane >> 3);
            if (px <= s.bx1 && py <= s.by1) shade(s, px, py, img_keys, W, (uint32_t)r.local);
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_resolve(RenderArgs a) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool in = p < a.npix;
    int g = -1;
    if (in) {
        const uint64_t key = a.w.keys[p];
        int lab = 0, local = -1;
        float depth = INFINITY;
        if (key != kEmpty) {
            const int64_t hw = (int64_t)a.bt.H * a.bt.W;
            const int img = (int)(p / hw);
            local = (int)(uint32_t)key;
            depth = __uint_as_float((uint32_t)(key >> 32));
            g = a.w.img_base[img] + local;
            // instance ranges that overlap (inst_off is the caller's) can leave a record of mixed
            // origin: such a pixel is background, never an index outside the records
            if ((unsigned)g < (unsigned)a.bt.total_inst) {
                lab = a.w.rec[g].label;
            } else {
                g = -1; local = -1; depth = INFINITY;
            }
        }
        if (a.out.label) {
            if (a.bt.label_kind == PV_LABEL_U8) ((uint8_t *)a.out.label)[p] = (uint8_t)lab;
            else if (a.bt.label_kind == PV_LABEL_I32) ((int32_t *)a.out.label)[p] = lab;
            else ((int64_t *)a.out.label)[p] = lab;
        }
        if (a.out.inst) a.out.inst[p] = local;
        if (a.out.depth) a.out.depth[p] = depth;
    }
    if (a.out.won) {
        // one atomicAdd per (wave, instance): the lanes of one instance elect a leader
        uint64_t m = __ballot(g >= 0);
        while (m) {
            const int src = __ffsll((unsigned long long)m) - 1;
            const int gs = rl(g, src);
            const uint64_t same = __ballot(g == gs);
            if ((int)(threadIdx.x & 63) == src) atomicAdd(a.out.won + gs, __popcll(same));
            m &= ~same;
        }
    }
}

// --------------------------------------------------------------------------
// pv_vertex_field
// --------------------------------------------------------------------------
struct FieldArgs {
    pv_field_desc d;
    int64_t total;      // threads of the launch; below 2^31 the kernels decompose it in 32 bits
    int32_t C;          // ncls * vn
};

__device__ __forceinline__ int label_class(const FieldArgs &a, int i, int y, int x) {
    const int64_t o = (int64_t)i * a.d.label_strides[0] + (int64_t)y * a.d.label_strides[1] + (int64_t)x * a.d.label_strides[2];
    int64_t lab;
    if (a.d.label_kind == PV_LABEL_U8) lab = ((const uint8_t *)a.d.label)[o];
    else if (a.d.label_kind == PV_LABEL_I32) lab = ((const int32_t *)a.d.label)[o];
    else lab = ((const int64_t *)a.d.label)[o];
    return lab >= 1 && lab <= a.d.ncls ? (int)(lab - 1) : -1;
}

// keypoint ch = c vn + k of image i
__device__ __forceinline__ void load_kp(const FieldArgs &a, int i, int ch, double *kx, double *ky) {
    const int64_t o = ((int64_t)i * a.C + ch) * 2;
    if (a.d.kp_kind == PV_KP_F64) {
        const double2 v = *(const double2 *)((const double *)a.d.keypoints + o);
        *kx = v.x; *ky = v.y;
    } else {
        const float2 v = *(const float2 *)((const float *)a.d.keypoints + o);
        *kx = v.x; *ky = v.y;
    }
}

// compute_vertex for one (pixel, keypoint), rounded to f32
__device__ __forceinline__ float2 unit_to(double kx, double ky, int x, int y) {
    const double dx = kx - (double)x, dy = ky - (double)y;
    double n = sqrt(dx * dx + dy * dy);
    if (n < 1e-3) n += 1e-3;
    return make_float2((float)(dx / n), (float)(dy / n));
}

template <typename T> struct Vec;
template <> struct Vec<float> {
    using V4 = float4;
    static __device__ __forceinline__ float cv(float v) { return v; }
    static __device__ __forceinline__ V4 pack(float a, float b, float c, float d) { return make_float4(a, b, c, d); }
};
template <> struct Vec<__half> {
    using V4 = uint2;
    static __device__ __forceinline__ __half cv(float v) { return __float2half_rn(v); }
    static __device__ __forceinline__ V4 pack(float a, float b, float c, float d) {
        const __half2 lo = __floats2half2_rn(a, b), hi = __floats2half2_rn(c, d);
        return make_uint2(*(const uint32_t *)&lo, *(const uint32_t *)&hi);
    }
};

// Any strides: one thread per (pixel, channel), two scalar stores.  XFAST: threads run along x
// within a channel plane (the network layout), otherwise along the channels of a pixel.
template <typename T, typename I, bool XFAST>
__global__ __launch_bounds__(kThreads) void k_field_any(FieldArgs a) {
    const I t = (I)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (I)a.total) return;
    int i, y, x, ch;
    if (XFAST) {
        x = (int)(t % (I)a.d.W); I r = t / (I)a.d.W;
        y = (int)(r % (I)a.d.H); r /= (I)a.d.H;
        ch = (int)(r % (I)a.C); i = (int)(r / (I)a.C);
    } else {
        ch = (int)(t % (I)a.C); I r = t / (I)a.C;
        x = (int)(r % (I)a.d.W); r /= (I)a.d.W;
        y = (int)(r % (I)a.d.H); i = (int)(r / (I)a.d.H);
    }
    float2 v = make_float2(0.f, 0.f);
    const int c = label_class(a, i, y, x);
    if (c >= 0 && ch / a.d.vn == c) {
        double kx, ky;
        load_kp(a, i, ch, &kx, &ky);
        v = unit_to(kx, ky, x, y);
    }
    const int64_t *s = a.d.vertex_strides;
    T *o = (T *)a.d.vertex + (int64_t)i * s[0] + (int64_t)y * s[1] + (int64_t)x * s[2] + (int64_t)ch * s[3];
    o[0] = Vec<T>::cv(v.x);
    o[s[4]] = Vec<T>::cv(v.y);
}

// [.., C, 2] innermost and contiguous, C even: one (pixel, channel pair) is one store of four
// elements (16 B in f32, 8 B in f16)
template <typename T>
__device__ __forceinline__ void field_pair(const FieldArgs &a, int i, int y, int x, int j) {
    float2 v0 = make_float2(0.f, 0.f), v1 = v0;
    const int c = label_class(a, i, y, x);
    if (c >= 0) {
        double kx, ky;
        if ((2 * j) / a.d.vn == c) { load_kp(a, i, 2 * j, &kx, &ky); v0 = unit_to(kx, ky, x, y); }
        if ((2 * j + 1) / a.d.vn == c) { load_kp(a, i, 2 * j + 1, &kx, &ky); v1 = unit_to(kx, ky, x, y); }
    }
    const int64_t *s = a.d.vertex_strides;
    T *o = (T *)a.d.vertex + (int64_t)i * s[0] + (int64_t)y * s[1] + (int64_t)x * s[2] + (int64_t)j * 4;
    *(typename Vec<T>::V4 *)o = Vec<T>::pack(v0.x, v0.y, v1.x, v1.y);
}

// The grid is (chunks of a row's W C / 2 pairs, rows, images): one 32-bit division per pair, and
// kPairsPerThread pairs, a block apart, per thread -- with one store per thread the launch of
// 1.4 million waves, not the stores, set the time.
constexpr int kPairsPerThread = 4;
template <typename T>
__global__ __launch_bounds__(kThreads) void k_field_pixel_rows(FieldArgs a) {
    const uint32_t half = (uint32_t)(a.C >> 1), n = (uint32_t)a.total;
    const uint32_t e0 = blockIdx.x * (kThreads * kPairsPerThread) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < kPairsPerThread; ++u) {
        const uint32_t e = e0 + u * kThreads;
        if (e < n) {
            const uint32_t x = e / half;
            field_pair<T>(a, blockIdx.z, blockIdx.y, (int)x, (int)(e - x * half));
        }
    }
}

// H or b beyond a grid dimension's 65,535: a linear launch, one pair per thread, three divisions
template <typename T, typename I>
__global__ __launch_bounds__(kThreads) void k_field_pixel(FieldArgs a) {
    const I t = (I)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (I)a.total) return;
    const I half = (I)(a.C >> 1);
    const int j = (int)(t % half); I r = t / half;
    const int x = (int)(r % (I)a.d.W); r /= (I)a.d.W;
    const int y = (int)(r % (I)a.d.H);
    field_pair<T>(a, (int)(r / (I)a.d.H), y, x, j);
}

// x innermost and contiguous (the network's [b, 2 C, H, W]), W a multiple of 4: one thread per
// (image, channel, row, four pixels), one store of four elements into each component's plane
template <typename T, typename I>
__global__ __launch_bounds__(kThreads) void k_field_plane(FieldArgs a) {
    const I t = (I)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (I)a.total) return;
    const I w4 = (I)(a.d.W >> 2);
    const int x = (int)(t % w4) * 4; I r = t / w4;
    const int y = (int)(r % (I)a.d.H); r /= (I)a.d.H;
    const int ch = (int)(r % (I)a.C);
    const int i = (int)(r / (I)a.C);
    const int c = ch / a.d.vn;
    float vx[4], vy[4];
    double kx = 0.0, ky = 0.0;
    bool have = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        vx[e] = vy[e] = 0.f;
        if (label_class(a, i, y, x + e) == c) {
            if (!have) { load_kp(a, i, ch, &kx, &ky); have = true; }
            const float2 v = unit_to(kx, ky, x + e, y);
            vx[e] = v.x; vy[e] = v.y;
        }
    }
    const int64_t *s = a.d.vertex_strides;
    T *o = (T *)a.d.vertex + (int64_t)i * s[0] + (int64_t)y * s[1] + (int64_t)x + (int64_t)ch * s[3];
    *(typename Vec<T>::V4 *)o = Vec<T>::pack(vx[0], vx[1], vx[2], vx[3]);
    *(typename Vec<T>::V4 *)(o + s[4]) = Vec<T>::pack(vy[0], vy[1], vy[2], vy[3]);
}

template <typename T>
int launch_field(const FieldArgs &a0, hipStream_t st) {
    FieldArgs a = a0;
    const pv_field_desc &d = a.d;
    const int64_t *s = d.vertex_strides;
    const int64_t pix = (int64_t)d.b * d.H * d.W;
    const uintptr_t vec_bytes = 4 * sizeof(T);
    const bool base_ok = ((uintptr_t)d.vertex & (vec_bytes - 1)) == 0;
    auto m4 = [](int64_t v) { return (v & 3) == 0; };
    enum { ANY, ANY_X, PIXEL, PLANE } path = ANY;
    if (s[4] == 1 && s[3] == 2 && (a.C & 1) == 0 && base_ok && m4(s[0]) && m4(s[1]) && m4(s[2])) {
        path = PIXEL;
        a.total = pix * (a.C >> 1);
    } else if (s[2] == 1 && (d.W & 3) == 0 && base_ok && m4(s[0]) && m4(s[1]) && m4(s[3]) && m4(s[4])) {
        path = PLANE;
        a.total = pix / 4 * a.C;
    } else {
        path = s[2] < s[3] ? ANY_X : ANY;
        a.total = pix * a.C;
    }
    const int64_t blocks = (a.total + kThreads - 1) / kThreads;
    if (blocks > INT32_MAX) return PV_EINVAL;
    const dim3 grid((unsigned)blocks);
    // 64-bit integer division costs the pixel kernel more than its store: 32 bits when they do
    const bool narrow = blocks * kThreads <= (int64_t)INT32_MAX;
    switch (path) {
    case PIXEL:
        if (d.H <= 65535 && d.b <= 65535 && (int64_t)d.W * (a.C >> 1) <= INT32_MAX / 2) {
            a.total = (int64_t)d.W * (a.C >> 1);                       // per row
            const int per_block = kThreads * kPairsPerThread;
            const dim3 rows((unsigned)((a.total + per_block - 1) / per_block), (unsigned)d.H, (unsigned)d.b);
            k_field_pixel_rows<T><<<rows, kThreads, 0, st>>>(a);
        } else if (narrow) {
            k_field_pixel<T, uint32_t><<<grid, kThreads, 0, st>>>(a);
        } else {
            k_field_pixel<T, int64_t><<<grid, kThreads, 0, st>>>(a);
        }
        break;
    case PLANE:
        if (narrow) k_field_plane<T, uint32_t><<<grid, kThreads, 0, st>>>(a);
        else k_field_plane<T, int64_t><<<grid, kThreads, 0, st>>>(a);
        break;
    case ANY_X:
        if (narrow) k_field_any<T, uint32_t, true><<<grid, kThreads, 0, st>>>(a);
        else k_field_any<T, int64_t, true><<<grid, kThreads, 0, st>>>(a);
        break;
    default:
        if (narrow) k_field_any<T, uint32_t, false><<<grid, kThreads, 0, st>>>(a);
        else k_field_any<T, int64_t, false><<<grid, kThreads, 0, st>>>(a);
        break;
    }
    return last();
}

bool dims_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && H <= PV_RENDER_MAX_DIM && W <= PV_RENDER_MAX_DIM; }

}  // namespace

extern "C" {

size_t pv_render_workspace_size(int32_t b, int32_t H, int32_t W, int64_t total_iv, int32_t total_inst) {
    if (b < 1 || !dims_ok(H, W) || total_iv < 0 || total_inst < 0 || total_iv > ((int64_t)1 << 40)) return 0;
    return carve(nullptr, (int64_t)b * H * W, total_iv, total_inst, b).bytes;
}

int pv_render_labels(const pv_render_meshes *m, const pv_render_batch *bt, const pv_render_out *out, void *workspace,
                     size_t workspace_bytes, pv_stream_t stream) {
    if (!m || !bt || !out) return PV_EINVAL;
    if (bt->b < 0 || bt->ninst < 0 || bt->total_inst < 0 || bt->K_stride < 0 || !dims_ok(bt->H, bt->W)) return PV_EINVAL;
    if (m->nmodels < 0 || m->total_v < 0 || m->total_f < 0 || m->max_verts < 0 || m->max_faces < 0) return PV_EINVAL;
    if (!(bt->znear > 0.0)) return PV_EINVAL;                          // also rejects NaN
    if (bt->label_kind != PV_LABEL_I64 && bt->label_kind != PV_LABEL_U8 && bt->label_kind != PV_LABEL_I32)
        return PV_EINVAL;
    if (!bt->inst_off && (int64_t)bt->b * bt->ninst != bt->total_inst) return PV_EINVAL;
    if (bt->b == 0) return PV_OK;
    if (!out->label && !out->inst && !out->depth) return PV_EINVAL;
    const int32_t n = bt->total_inst;
    if (n > 0) {
        if (!bt->model_id || !bt->label || !bt->pose || !bt->K) return PV_EINVAL;
        if (m->nmodels < 1 || !m->vert_off || !m->face_off) return PV_EINVAL;
        if ((m->total_v > 0 && !m->verts) || (m->total_f > 0 && !m->faces)) return PV_EINVAL;
    }
    const int64_t npix = (int64_t)bt->b * bt->H * bt->W, total_iv = (int64_t)n * m->max_verts;
    const size_t need = pv_render_workspace_size(bt->b, bt->H, bt->W, total_iv, n);
    if (need == 0) return PV_EINVAL;
    if (!workspace || workspace_bytes < need) return PV_EWORKSPACE;
    if (((uintptr_t)workspace & 255) || (((uintptr_t)bt->pose | (uintptr_t)bt->K | (uintptr_t)out->snap_z) & 7) ||
        (((uintptr_t)out->snap_xy) & 7) || ((uintptr_t)out->label & (bt->label_kind == PV_LABEL_I64 ? 7 : bt->label_kind == PV_LABEL_I32 ? 3 : 0)))
        return PV_EALIGN;

    RenderArgs a{};
    a.w = carve(workspace, npix, total_iv, n, bt->b);
    a.m = *m; a.bt = *bt; a.out = *out;
    a.npix = npix;
    a.vchunks = (m->max_verts + kThreads - 1) / kThreads;
    a.fchunks = (m->max_faces + kThreads - 1) / kThreads;
    const int64_t clear_blocks = (std::max<int64_t>((npix + 1) / 2, std::max<int64_t>(n, bt->b)) + kThreads - 1) / kThreads;
    const int64_t res_blocks = (npix + kThreads - 1) / kThreads;
    const int64_t vblocks = (int64_t)n * a.vchunks, fblocks = (int64_t)n * a.fchunks;
    if (res_blocks > INT32_MAX || vblocks > INT32_MAX || fblocks > INT32_MAX) return PV_EINVAL;

    hipStream_t st = (hipStream_t)stream;
    k_clear<<<dim3((unsigned)clear_blocks), kThreads, 0, st>>>(a);
    int e = last();
    if (e) return e;
    if (n > 0) {
        k_inst<<<dim3((unsigned)((bt->b + 63) / 64)), 64, 0, st>>>(a);
        if ((e = last())) return e;
        if (vblocks > 0) {
            k_project<<<dim3((unsigned)vblocks), kThreads, 0, st>>>(a);
            if ((e = last())) return e;
        }
        if (fblocks > 0) {
            // slices of a large triangle's sample blocks: enough waves for 8 per CU when the
            // meshes are small (counting the waves that hold a triangle: a 12-triangle model
            // fills one of its block's four), one slice when the triangles alone fill the device
            const int64_t waves = (int64_t)n * ((m->max_faces + 63) / 64);
            const int64_t want = (int64_t)cu_count() * 8 / waves;
            const int slices = (int)std::min<int64_t>(kMaxSlices, std::max<int64_t>(1, want));
            k_raster<<<dim3((unsigned)fblocks, (unsigned)slices), kThreads, 0, st>>>(a);
            if ((e = last())) return e;
        }
    }
    k_resolve<<<dim3((unsigned)res_blocks), kThreads, 0, st>>>(a);
    return last();
}

int pv_vertex_field(const pv_field_desc *d, pv_stream_t stream) {
    if (!d) return PV_EINVAL;
    if (d->b < 0 || !dims_ok(d->H, d->W) || d->ncls < 1 || d->vn < 1 || (int64_t)d->ncls * d->vn > (1 << 20))
        return PV_EINVAL;
    if (d->label_kind != PV_LABEL_I64 && d->label_kind != PV_LABEL_U8 && d->label_kind != PV_LABEL_I32) return PV_EINVAL;
    if (d->kp_kind != PV_KP_F64 && d->kp_kind != PV_KP_F32) return PV_EINVAL;
    if (d->vertex_kind != PV_FIELD_F32 && d->vertex_kind != PV_FIELD_F16) return PV_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->label_strides[i] < 0) return PV_EINVAL;
    for (int i = 0; i < 5; ++i)
        if (d->vertex_strides[i] < 0) return PV_EINVAL;
    if (d->b == 0) return PV_OK;
    if (!d->label || !d->keypoints || !d->vertex) return PV_EINVAL;
    const uintptr_t kp_al = d->kp_kind == PV_KP_F64 ? 15 : 7, v_al = d->vertex_kind == PV_FIELD_F32 ? 3 : 1;
    const uintptr_t l_al = d->label_kind == PV_LABEL_I64 ? 7 : d->label_kind == PV_LABEL_I32 ? 3 : 0;
    if (((uintptr_t)d->keypoints & kp_al) || ((uintptr_t)d->vertex & v_al) || ((uintptr_t)d->label & l_al)) return PV_EALIGN;
    FieldArgs a{};
    a.d = *d;
    a.C = d->ncls * d->vn;
    hipStream_t st = (hipStream_t)stream;
    return d->vertex_kind == PV_FIELD_F32 ? launch_field<float>(a, st) : launch_field<__half>(a, st);
}

}  // extern "C"
