// pvshade.hip -- libpvshade.so (include/pvshade.h): u8 RGB frames with Lambert shading from
// vertex-coloured meshes and poses, with the label / instance / depth / face maps of the same
// z-buffer, and smooth vertex normals.  One translation unit that includes no other csrc/ file and
// no other public header: the projection, snap and coverage code restates pvrender.hip's on purpose
// (tests/test_render_abi.py holds that library to its own two files), so neither rebuilds the other.
//
// pv_shade_render is five launches on the caller's stream, pvrender.hip's structure:
//   k_clear    keys <- all ones, instance records and won counts <- 0
//   k_inst     one thread per image: its instance range, each instance validated into a record
//   k_project  one thread per (instance, vertex): fp64 transform, snap to 1/256 px; keeps X, Y, Z
//   k_raster   one lane per triangle for setup; a triangle whose clipped box holds at most
//              kSmallPx samples is walked by its own lane, a larger one is handed to the whole
//              wave, which strides over 8x8 sample blocks of its box.  A covered sample does one
//              64-bit integer atomicMin on (f32 depth bits << 32 | instance * max_faces + face),
//              behind a plain read that filters the samples that cannot win.
//   k_resolve  key -> label / inst / depth / face, the won-pixel counts (integer atomicAdd, one
//              per wave and instance), and the deferred shading: the winning face's three vertices
//              are read again, the sample's barycentric weights rebuilt, colour and normal
//              interpolated and lit, all in fp64 with every operation rounded.
// pv_shade_normals is one launch: a block per (model, 256 vertices), the model's faces tiled through
// LDS with their cross products, each thread summing the faces that name its vertex in face order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/pvshade.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSmallPx = 32;             // samples in a clipped box a single lane walks
constexpr int kMaxSlices = 256;
constexpr uint64_t kEmpty = ~0ull;
constexpr int32_t kInvalid = -2147483647 - 1;   // snap of a vertex that drops its triangles

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
    double *pz;         // [total_inst][max_verts]: camera-frame Z
    int32_t *pxy;       // [total_inst][max_verts][2]: the snap
    double *pcam;       // [total_inst][max_verts][2]: camera-frame X, Y
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
    w.pcam = (double *)(p + off);    off = align_up(off + total_iv * 16, 256);
    w.rec = (InstRec *)(p + off);    off = align_up(off + total_inst * (int64_t)sizeof(InstRec), 256);
    w.img_base = (int32_t *)(p + off); off = align_up(off + b * 4, 256);
    w.bytes = (size_t)off;
    return w;
}

struct ShadeArgs {
    Work w;
    pv_shade_meshes m;
    pv_shade_batch bt;
    pv_shade_lights lt;
    pv_shade_out out;
    int64_t npix;       // b * H * W
    int32_t vchunks, fchunks;
};

// --------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_clear(ShadeArgs a) {
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

__global__ __launch_bounds__(64) void k_inst(ShadeArgs a) {
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

__global__ __launch_bounds__(kThreads) void k_project(ShadeArgs a) {
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
    const double lim = (double)PV_SHADE_MAX_SNAP;
    // NaN fails every comparison, so a non-finite u or v lands in the else branch
    const bool ok = isfinite(X) && isfinite(Y) && isfinite(Z) && Z >= a.bt.znear && fabs(su) <= lim && fabs(sv) <= lim;
    const int32_t sx = ok ? (int32_t)su : kInvalid, sy = ok ? (int32_t)sv : kInvalid;
    const int64_t slot = (int64_t)g * a.m.max_verts + v;
    *(int2 *)(a.w.pxy + slot * 2) = make_int2(sx, sy);
    a.w.pz[slot] = Z;
    *(double2 *)(a.w.pcam + slot * 2) = make_double2(X, Y);
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

__device__ __forceinline__ void sample(const Tri &t, int px, int py, uint64_t *img_keys, int W, uint32_t slot) {
    const int32_t X = px << PV_SHADE_SUBPIXEL_BITS, Y = py << PV_SHADE_SUBPIXEL_BITS;
    int64_t w0, w1, w2;
    const bool c2 = edge(t.x0, t.y0, t.x1, t.y1, X, Y, &w2);
    const bool c0 = edge(t.x1, t.y1, t.x2, t.y2, X, Y, &w0);
    const bool c1 = edge(t.x2, t.y2, t.x0, t.y0, X, Y, &w1);
    if (!(c0 && c1 && c2)) return;
    const double num = ((double)w0 * t.q0 + (double)w1 * t.q1) + (double)w2 * t.q2;
    const double Z = 1.0 / (num / (double)(w0 + w1 + w2));
    const uint64_t key = ((uint64_t)__float_as_uint((float)Z) << 32) | slot;
    uint64_t *k = img_keys + (int64_t)py * W + px;
    // the plain read may be stale, never too small: the minimum only falls
    if (key < *(volatile uint64_t *)k) atomicMin((unsigned long long *)k, (unsigned long long)key);
}

__device__ __forceinline__ int rl(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double rld(double v, int src) {
    const int lo = rl(__double2loint(v), src), hi = rl(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kThreads) void k_raster(ShadeArgs a) {
    const int g = blockIdx.x / a.fchunks, chunk = blockIdx.x - g * a.fchunks;
    const int slice = blockIdx.y, nslices = gridDim.y;
    const InstRec r = a.w.rec[g];
    if (chunk * kThreads >= r.nf) return;                              // whole block past the model (or skipped)
    const int f = chunk * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int W = a.bt.W, H = a.bt.H;
    uint64_t *img_keys = a.w.keys + (int64_t)r.img * H * W;
    // local < total_inst and f < max_faces, and the host vouches total_inst * max_faces < 2^32
    const uint32_t slot = (uint32_t)r.local * (uint32_t)a.m.max_faces + (uint32_t)f;

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
            sample(t, x, y, img_keys, W, slot);
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
        const uint32_t sslot = (uint32_t)rl((int)slot, src);
        const int nbx = (s.bx1 - s.bx0 + 8) >> 3, nby = (s.by1 - s.by0 + 8) >> 3;
        const int64_t nblk = (int64_t)nbx * nby;
        for (int64_t blk = slice; blk < nblk; blk += nslices) {
            const int byi = (int)(blk / nbx), bxi = (int)(blk - (int64_t)byi * nbx);
            const int px = s.bx0 + bxi * 8 + (lane & 7), py = s.by0 + byi * 8 + (lane >> 3);
            if (px <= s.bx1 && py <= s.by1) sample(s, px, py, img_keys, W, sslot);
        }
    }
}

// ---- the deferred shading (rule 8) ----------------------------------------------------------------
struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 sub(const V3 &a, const V3 &b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross(const V3 &a, const V3 &b) {
    return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot(const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double length(const V3 &a) { return sqrt(dot(a, a)); }
__device__ __forceinline__ V3 neg(const V3 &a) { return V3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ double mix3(double b0, double c0, double b1, double c1, double b2, double c2) {
    return (b0 * c0 + b1 * c1) + b2 * c2;
}

// the colour of sample (x, y) of image img on face f of instance g; false when the face's indices
// do not hold (only a record of mixed origin can do that): the pixel is then background
__device__ __forceinline__ bool shade_pixel(const ShadeArgs &a, const InstRec &r, int img, int g, int f, int x, int y, uint8_t rgb[3]) {
    const int32_t *F = a.m.faces + (int64_t)(r.flo + f) * 3;
    const int i0 = F[0];
    int i1 = F[1], i2 = F[2];
    if (!((unsigned)i0 < (unsigned)r.nv && (unsigned)i1 < (unsigned)r.nv && (unsigned)i2 < (unsigned)r.nv)) return false;
    const int64_t base = (int64_t)g * a.m.max_verts;
    const int2 p0 = *(const int2 *)(a.w.pxy + (base + i0) * 2);
    int2 p1 = *(const int2 *)(a.w.pxy + (base + i1) * 2);
    int2 p2 = *(const int2 *)(a.w.pxy + (base + i2) * 2);
    if (p0.x == kInvalid || p1.x == kInvalid || p2.x == kInvalid) return false;
    const int64_t area = (int64_t)(p1.x - p0.x) * (int64_t)(p2.y - p0.y) - (int64_t)(p2.x - p0.x) * (int64_t)(p1.y - p0.y);
    if (area < 0) {
        const int2 tp = p1; p1 = p2; p2 = tp;
        const int ti = i1; i1 = i2; i2 = ti;
    }
    const int32_t X = x << PV_SHADE_SUBPIXEL_BITS, Y = y << PV_SHADE_SUBPIXEL_BITS;
    int64_t w0, w1, w2;
    edge(p0.x, p0.y, p1.x, p1.y, X, Y, &w2);
    edge(p1.x, p1.y, p2.x, p2.y, X, Y, &w0);
    edge(p2.x, p2.y, p0.x, p0.y, X, Y, &w1);
    const double2 c0 = *(const double2 *)(a.w.pcam + (base + i0) * 2);
    const double2 c1 = *(const double2 *)(a.w.pcam + (base + i1) * 2);
    const double2 c2 = *(const double2 *)(a.w.pcam + (base + i2) * 2);
    const V3 P0{c0.x, c0.y, a.w.pz[base + i0]}, P1{c1.x, c1.y, a.w.pz[base + i1]}, P2{c2.x, c2.y, a.w.pz[base + i2]};
    const double a0 = (double)w0 * (1.0 / P0.z), a1 = (double)w1 * (1.0 / P1.z), a2 = (double)w2 * (1.0 / P2.z);
    const double s = (a0 + a1) + a2;
    const double b0 = a0 / s, b1 = a1 / s, b2 = a2 / s;

    V3 nf = cross(sub(P1, P0), sub(P2, P0));
    if (dot(nf, P0) > 0.0) nf = neg(nf);
    V3 n = nf;
    if (a.m.normals) {
        const double *n0 = a.m.normals + (int64_t)(r.vlo + i0) * 3;
        const double *n1 = a.m.normals + (int64_t)(r.vlo + i1) * 3;
        const double *n2 = a.m.normals + (int64_t)(r.vlo + i2) * 3;
        const V3 nm{mix3(b0, n0[0], b1, n1[0], b2, n2[0]), mix3(b0, n0[1], b1, n1[1], b2, n2[1]),
                    mix3(b0, n0[2], b1, n1[2], b2, n2[2])};
        if (!(nm.x == 0.0 && nm.y == 0.0 && nm.z == 0.0)) {
            const double *P = a.bt.pose + (int64_t)g * 12;
            n = V3{(P[0] * nm.x + P[1] * nm.y) + P[2] * nm.z, (P[4] * nm.x + P[5] * nm.y) + P[6] * nm.z,
                   (P[8] * nm.x + P[9] * nm.y) + P[10] * nm.z};
            if (dot(n, nf) < 0.0) n = neg(n);
        }
    }
    const double *L = a.lt.lights + (int64_t)img * a.lt.lights_stride;
    const V3 l{L[0], L[1], L[2]};
    const double ln = length(n), ll = length(l);
    double d = 0.0;
    if (ln > 0.0 && ll > 0.0 && isfinite(ln) && isfinite(ll)) {
        const double c = dot(n, l) / (ln * ll);
        d = c > 0.0 ? c : 0.0;                                         // a NaN compares false
    }
    const uint8_t *k0 = a.m.colors + (int64_t)(r.vlo + i0) * 3;
    const uint8_t *k1 = a.m.colors + (int64_t)(r.vlo + i1) * 3;
    const uint8_t *k2 = a.m.colors + (int64_t)(r.vlo + i2) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = mix3(b0, (double)k0[k], b1, (double)k1[k], b2, (double)k2[k]);
        const double v = rint(c * (L[3 + k] + L[6 + k] * d));
        rgb[k] = !(v >= 0.0) ? (uint8_t)0 : v > 255.0 ? (uint8_t)255 : (uint8_t)v;   // a NaN gives 0
    }
    return true;
}

__global__ __launch_bounds__(kThreads) void k_resolve(ShadeArgs a) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bool in = p < a.npix;
    int g = -1;
    if (in) {
        const uint64_t key = a.w.keys[p];
        const int64_t hw = (int64_t)a.bt.H * a.bt.W;
        const int img = (int)(p / hw);
        const int64_t rem = p - (int64_t)img * hw;
        const int y = (int)(rem / a.bt.W), x = (int)(rem - (int64_t)y * a.bt.W);
        int lab = 0, local = -1, face = -1;
        float depth = INFINITY;
        uint8_t rgb[3] = {0, 0, 0};
        bool lit = false;
        if (key != kEmpty) {
            const uint32_t slot = (uint32_t)key, mf = (uint32_t)max(a.m.max_faces, 1);
            local = (int)(slot / mf);
            face = (int)(slot - (uint32_t)local * mf);
            depth = __uint_as_float((uint32_t)(key >> 32));
            g = a.w.img_base[img] + local;
            // instance ranges that overlap (inst_off is the caller's) can leave a record of mixed
            // origin: such a pixel is background, never an index outside the records or the faces
            if ((unsigned)g < (unsigned)a.bt.total_inst) {
                const InstRec r = a.w.rec[g];
                lab = r.label;
                if (a.out.image) lit = face < r.nf && shade_pixel(a, r, img, g, face, x, y, rgb);
            } else {
                g = -1; local = -1; face = -1; depth = INFINITY;
            }
        }
        if (a.out.image) {
            if (!lit) {
                if (a.lt.background) {
                    const int64_t *s = a.lt.bg_strides;
                    const uint8_t *q = a.lt.background + (int64_t)img * s[0] + (int64_t)y * s[1] + (int64_t)x * s[2];
                    rgb[0] = q[0]; rgb[1] = q[s[3]]; rgb[2] = q[2 * s[3]];
                } else {
                    rgb[0] = a.lt.bg_color[0]; rgb[1] = a.lt.bg_color[1]; rgb[2] = a.lt.bg_color[2];
                }
            }
            const int64_t *s = a.out.image_strides;
            uint8_t *o = a.out.image + (int64_t)img * s[0] + (int64_t)y * s[1] + (int64_t)x * s[2];
            o[0] = rgb[0]; o[s[3]] = rgb[1]; o[2 * s[3]] = rgb[2];
        }
        if (a.out.label) {
            if (a.bt.label_kind == PV_LABEL_U8) ((uint8_t *)a.out.label)[p] = (uint8_t)lab;
            else if (a.bt.label_kind == PV_LABEL_I32) ((int32_t *)a.out.label)[p] = lab;
            else ((int64_t *)a.out.label)[p] = lab;
        }
        if (a.out.inst) a.out.inst[p] = local;
        if (a.out.depth) a.out.depth[p] = depth;
        if (a.out.face) a.out.face[p] = face;
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
// pv_shade_normals
// --------------------------------------------------------------------------
struct NormArgs {
    pv_shade_meshes m;
    double *out;
    int32_t vchunks;
};

__global__ __launch_bounds__(kThreads) void k_normals(NormArgs a) {
    __shared__ int32_t s_idx[kThreads][3];
    __shared__ double s_n[kThreads][3];
    const int mdl = blockIdx.x / a.vchunks, chunk = blockIdx.x - mdl * a.vchunks;
    const int vl = a.m.vert_off[mdl], vh = a.m.vert_off[mdl + 1];
    const int fl = a.m.face_off[mdl], fh = a.m.face_off[mdl + 1];
    // uniform over the block, so the barriers below are reached by all of it or by none
    if (vl < 0 || vh < vl || vh > a.m.total_v || vh - vl > a.m.max_verts) return;
    if (fl < 0 || fh < fl || fh > a.m.total_f || fh - fl > a.m.max_faces) return;
    const int nv = vh - vl, nf = fh - fl;
    if (chunk * kThreads >= nv) return;
    const int t = threadIdx.x, v = chunk * kThreads + t;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    for (int f0 = 0; f0 < nf; f0 += kThreads) {
        int i0 = -1, i1 = -1, i2 = -1;
        V3 c{0.0, 0.0, 0.0};
        if (f0 + t < nf) {
            const int32_t *F = a.m.faces + (int64_t)(fl + f0 + t) * 3;
            const int j0 = F[0], j1 = F[1], j2 = F[2];
            if ((unsigned)j0 < (unsigned)nv && (unsigned)j1 < (unsigned)nv && (unsigned)j2 < (unsigned)nv) {
                const float *q0 = a.m.verts + (int64_t)(vl + j0) * 3;
                const float *q1 = a.m.verts + (int64_t)(vl + j1) * 3;
                const float *q2 = a.m.verts + (int64_t)(vl + j2) * 3;
                const V3 p0{(double)q0[0], (double)q0[1], (double)q0[2]}, p1{(double)q1[0], (double)q1[1], (double)q1[2]},
                    p2{(double)q2[0], (double)q2[1], (double)q2[2]};
                c = cross(sub(p1, p0), sub(p2, p0));
                i0 = j0; i1 = j1; i2 = j2;
            }
        }
        s_idx[t][0] = i0; s_idx[t][1] = i1; s_idx[t][2] = i2;          // -1 matches no vertex
        s_n[t][0] = c.x; s_n[t][1] = c.y; s_n[t][2] = c.z;
        __syncthreads();
        const int cnt = min(kThreads, nf - f0);
        if (v < nv) {
            for (int j = 0; j < cnt; ++j) {                            // every lane reads one address: a broadcast
                if (s_idx[j][0] == v || s_idx[j][1] == v || s_idx[j][2] == v) {
                    nx = nx + s_n[j][0]; ny = ny + s_n[j][1]; nz = nz + s_n[j][2];
                }
            }
        }
        __syncthreads();
    }
    if (v < nv) {
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        double *o = a.out + (int64_t)(vl + v) * 3;
        if (len > 0.0 && isfinite(len)) {
            o[0] = nx / len; o[1] = ny / len; o[2] = nz / len;
        } else {
            o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
        }
    }
}

bool dims_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && H <= PV_SHADE_MAX_DIM && W <= PV_SHADE_MAX_DIM; }

bool sizes_ok(const pv_shade_meshes *m) {
    return m->nmodels >= 0 && m->total_v >= 0 && m->total_f >= 0 && m->max_verts >= 0 && m->max_faces >= 0;
}

bool tables_ok(const pv_shade_meshes *m) {
    if (m->nmodels < 1 || !m->vert_off || !m->face_off) return false;
    return !(m->total_v > 0 && !m->verts) && !(m->total_f > 0 && !m->faces);
}

}  // namespace

extern "C" {

int pv_shade_normals(const pv_shade_meshes *m, double *normals_out, pv_stream_t stream) {
    if (!m || !sizes_ok(m)) return PV_EINVAL;
    if (m->nmodels == 0 || m->total_v == 0 || m->max_verts == 0) return PV_OK;
    if (!normals_out || !tables_ok(m)) return PV_EINVAL;
    if ((uintptr_t)normals_out & 7) return PV_EALIGN;
    NormArgs a{};
    a.m = *m;
    a.out = normals_out;
    a.vchunks = (m->max_verts + kThreads - 1) / kThreads;
    const int64_t blocks = (int64_t)m->nmodels * a.vchunks;
    if (blocks > INT32_MAX) return PV_EINVAL;
    k_normals<<<dim3((unsigned)blocks), kThreads, 0, (hipStream_t)stream>>>(a);
    return last();
}

size_t pv_shade_workspace_size(int32_t b, int32_t H, int32_t W, int64_t total_iv, int32_t total_inst) {
    if (b < 1 || !dims_ok(H, W) || total_iv < 0 || total_inst < 0 || total_iv > ((int64_t)1 << 40)) return 0;
    return carve(nullptr, (int64_t)b * H * W, total_iv, total_inst, b).bytes;
}

int pv_shade_render(const pv_shade_meshes *m, const pv_shade_batch *bt, const pv_shade_lights *lt, const pv_shade_out *out,
                    void *workspace, size_t workspace_bytes, pv_stream_t stream) {
    if (!m || !bt || !lt || !out) return PV_EINVAL;
    if (bt->b < 0 || bt->ninst < 0 || bt->total_inst < 0 || bt->K_stride < 0 || !dims_ok(bt->H, bt->W)) return PV_EINVAL;
    if (!sizes_ok(m)) return PV_EINVAL;
    if (!(bt->znear > 0.0)) return PV_EINVAL;                          // also rejects NaN
    if (bt->label_kind != PV_LABEL_I64 && bt->label_kind != PV_LABEL_U8 && bt->label_kind != PV_LABEL_I32)
        return PV_EINVAL;
    if (!bt->inst_off && (int64_t)bt->b * bt->ninst != bt->total_inst) return PV_EINVAL;
    if (lt->lights_stride < 0) return PV_EINVAL;
    for (int i = 0; i < 4; ++i)
        if (lt->bg_strides[i] < 0 || out->image_strides[i] < 0) return PV_EINVAL;
    // the z-buffer's slot, instance * max_faces + face, has to fit the key's low 32 bits
    if ((int64_t)bt->total_inst * m->max_faces >= ((int64_t)1 << 32)) return PV_EINVAL;
    if (bt->b == 0) return PV_OK;
    if (!out->image && !out->label && !out->inst && !out->depth && !out->face) return PV_EINVAL;
    if (!lt->lights) return PV_EINVAL;
    const int32_t n = bt->total_inst;
    if (n > 0) {
        if (!bt->model_id || !bt->label || !bt->pose || !bt->K) return PV_EINVAL;
        if (!tables_ok(m) || (m->total_v > 0 && !m->colors)) return PV_EINVAL;
    }
    const int64_t npix = (int64_t)bt->b * bt->H * bt->W, total_iv = (int64_t)n * m->max_verts;
    const size_t need = pv_shade_workspace_size(bt->b, bt->H, bt->W, total_iv, n);
    if (need == 0) return PV_EINVAL;
    if (!workspace || workspace_bytes < need) return PV_EWORKSPACE;
    const uintptr_t lab_al = bt->label_kind == PV_LABEL_I64 ? 7 : bt->label_kind == PV_LABEL_I32 ? 3 : 0;
    if (((uintptr_t)workspace & 255) || (((uintptr_t)bt->pose | (uintptr_t)bt->K | (uintptr_t)lt->lights | (uintptr_t)m->normals) & 7) ||
        ((uintptr_t)out->label & lab_al) ||
        (((uintptr_t)out->inst | (uintptr_t)out->depth | (uintptr_t)out->face | (uintptr_t)out->won) & 3))
        return PV_EALIGN;

    ShadeArgs a{};
    a.w = carve(workspace, npix, total_iv, n, bt->b);
    a.m = *m; a.bt = *bt; a.lt = *lt; a.out = *out;
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
            // meshes are small, one slice when the triangles alone fill the device
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

}  // extern "C"
